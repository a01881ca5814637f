#!/usr/bin/env python3
"""Regenerate tests/golden/bcount/random_vectors.json.gz: 20 seeded random read sets (every CIGAR
operation, letters inside and outside the BAM alphabet, three quality thresholds) with the result
of the reference's own compiled count.bcount (oracle/_ref) for each.  Needs oracle/_ref, so it runs
only where the reference's sources are present; tests/test_oracle.py reads the stored file.

    python tests/golden/make_random_vectors.py
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))


def trials(seed: int = 5, n: int = 20):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        L = int(rng.integers(50, 400))
        reads, quals, starts, ctuples = [], [], [], []
        for _ in range(int(rng.integers(0, 60))):
            ops = [(0, int(rng.integers(1, 20)))]
            for _ in range(int(rng.integers(0, 4))):
                ops.append((int(rng.choice([0, 1, 2, 3, 6, 7, 8, 9])), int(rng.integers(1, 6))))
            ops.append((0, int(rng.integers(1, 20))))
            span = sum(n for o, n in ops if o in (0, 2, 3, 7, 8))
            q = sum(n for o, n in ops if o in (0, 1, 7, 8))
            if span >= L:
                continue
            reads.append("".join(rng.choice(list("ACGTN=RYacgt"), q)))
            quals.append(rng.integers(0, 45, q).tolist())
            starts.append(int(rng.integers(0, L - span)))
            ctuples.append(ops)
        yield L, int(rng.choice([0, 10, 30])), reads, quals, starts, ctuples


def main():
    from oracle import ref_bcount

    bcount = ref_bcount()
    if bcount is None:
        sys.exit("oracle/_ref is not built: the reference's sources are needed")
    vec = [dict(ref_len=L, mbq=mbq, reads=reads, qualities=quals, starts=starts, ctuples=ctuples,
                expected=bcount(L, mbq, reads, quals, starts, ctuples))
           for L, mbq, reads, quals, starts, ctuples in trials()]
    with gzip.GzipFile(os.path.join(HERE, "bcount", "random_vectors.json.gz"), "wb", mtime=0) as fh:
        fh.write(json.dumps(vec).encode())
    print("random bcount vectors:", len(vec))


if __name__ == "__main__":
    main()
