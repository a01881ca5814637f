"""Device BGZF inflate against the host's, on the BAMs synth writes ("Device inflate"):
    python scripts/inflate_bench.py [--configs c2,c3] [--levels 1,9] [--passes 3] [--out DIR] [--no-cli]

Per file, in ONE process, one untimed pass and then `passes` alternating passes of
  kernel   bc_bgzf_inflate with the compressed bytes resident, by event pair: GB/s of inflated bytes
  device   bc_bgzf_inflate_host, wall time: upload, kernel, download and the synchronise
  host     bcio_inflate_blocks (the streams' inflater, the default path) on the same blocks, 16 threads
each checked against the host's bytes; then `python -m basecount_amd FILE > out` wall time with
BASECOUNT_DEVICE_INFLATE off and on, alternating, outputs compared.  One JSON line per file."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from basecount_amd import _native as N  # noqa: E402
from basecount_amd import device as D  # noqa: E402
from basecount_amd import synth  # noqa: E402

THREADS = 16


def scan(blob: np.ndarray) -> np.ndarray:
    """bc_zblock descriptors of a well-formed BGZF file, outputs packed back to back."""
    raw, off, uoff, rows = blob.tobytes(), 0, 0, []
    while off < len(raw):
        xlen, = struct.unpack_from("<H", raw, off + 10)
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        isize, = struct.unpack_from("<I", raw, off + bsize - 4)
        rows.append((off + 12 + xlen, bsize - xlen - 20, isize, uoff))
        uoff += isize
        off += bsize
    return np.array(rows, D.ZBLOCK_DTYPE)


def bench_file(ctx, path, passes):
    comp = np.fromfile(path, np.uint8)
    blocks = scan(comp)
    total = int(blocks["isize"].sum())
    want = np.zeros(total, np.uint8)
    lib = N.bcio()

    def host():
        t = time.perf_counter()
        N.bcio_check(lib.bcio_inflate_blocks(comp.ctypes.data, comp.size, blocks.ctypes.data, blocks.size,
                                             want.ctypes.data, want.size, THREADS))
        return (time.perf_counter() - t) * 1e3

    d_comp = ctx.alloc(comp.size).upload(comp)
    d_blocks = ctx.alloc(blocks.nbytes).upload(blocks)
    d_out, d_status = ctx.alloc(total), ctx.alloc(blocks.size)
    ctx.sync()

    def kernel():
        ctx.event_record(0)
        ctx.bgzf_inflate(d_comp.ptr, comp.size, d_blocks.ptr, blocks.size, d_out.ptr, total, d_status.ptr)
        ctx.event_record(1)
        return ctx.event_elapsed_ms(0, 1)

    got = np.zeros(total, np.uint8)

    def device():
        t = time.perf_counter()
        st = ctx.bgzf_inflate_host(comp, blocks, got)
        ms = (time.perf_counter() - t) * 1e3
        assert not st.any(), "device refused %d blocks" % np.count_nonzero(st)
        return ms

    host(), kernel(), device()  # untimed
    assert not d_status.download(np.uint8, blocks.size).any()
    assert np.array_equal(d_out.download(np.uint8, total), want) and np.array_equal(got, want)
    t0 = ctx.bgzf_inflate_times()
    res = {"kernel_ms": [], "device_ms": [], "host_ms": []}
    for _ in range(passes):
        res["kernel_ms"].append(kernel())
        res["device_ms"].append(device())
        res["host_ms"].append(host())
    t1 = ctx.bgzf_inflate_times()
    for b in (d_comp, d_blocks, d_out, d_status):
        b.free()
    split = {k: (t1[k] - t0[k]) / passes for k in ("upload_ms", "kernel_ms", "download_ms")}
    return {"file": os.path.basename(path), "blocks": int(blocks.size), "comp_MB": comp.size / 1e6,
            "inflated_MB": total / 1e6, **{k: [round(x, 3) for x in v] for k, v in res.items()},
            "kernel_GBps": round(total / 1e6 / min(res["kernel_ms"]), 2),
            "device_split_ms": {k: round(v, 3) for k, v in split.items()},
            "host_GBps": round(total / 1e6 / min(res["host_ms"]), 2)}


def cli_wall(path, passes, tmp):
    """Wall time of the CLI, option off and on, alternating; the outputs must be equal."""
    out = {"0": [], "1": []}
    files = {}
    for i in range(passes + 1):  # the first pair is untimed
        for opt in ("0", "1"):
            env = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0", BASECOUNT_DEVICE_INFLATE=opt)
            files[opt] = os.path.join(tmp, "cli_%s.out" % opt)
            with open(files[opt], "wb") as fh:
                t = time.perf_counter()
                subprocess.run([sys.executable, "-m", "basecount_amd", path], env=env, stdout=fh, check=True,
                               timeout=600)
                if i:
                    out[opt].append(round((time.perf_counter() - t) * 1e3, 1))
        with open(files["0"], "rb") as a, open(files["1"], "rb") as b:
            assert a.read() == b.read(), "CLI output differs with the option on"
    # the phase split of one run each way (stderr of BASECOUNT_HIP_TIMING=1; "wall" is run()'s, without
    # the interpreter's start-up and imports that the timings above include)
    phases = {}
    for opt in ("0", "1"):
        env = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0", BASECOUNT_DEVICE_INFLATE=opt,
                   BASECOUNT_HIP_TIMING="1")
        with open(os.devnull, "wb") as fh:
            p = subprocess.run([sys.executable, "-m", "basecount_amd", path], env=env, stdout=fh,
                               stderr=subprocess.PIPE, check=True, timeout=600)
        phases[opt] = [ln.split("] ", 1)[1] for ln in p.stderr.decode().splitlines()
                       if "] host " in ln or "] device inflate" in ln or "] wall " in ln]
    return {"cli_off_ms": out["0"], "cli_on_ms": out["1"], "cli_off_phases": phases["0"], "cli_on_phases": phases["1"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--levels", default="1,9", help="C3 rewritten at these deflate levels")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON lines (inflate_bench.jsonl)")
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    ctx = D.Context(0)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for name in a.configs.split(","):
            rs = synth.make_config(name)
            p = os.path.join(tmp, name + ".bam")
            synth.write_bam(rs, p)  # as bench.py writes it
            jobs.append((p, name == a.configs.split(",")[-1]))
            if name == "c3":
                for lvl in (int(x) for x in a.levels.split(",") if x):
                    p = os.path.join(tmp, "c3_l%d.bam" % lvl)
                    synth.write_bam(rs, p, level=lvl)
                    jobs.append((p, False))
        for p, cli in jobs:
            r = bench_file(ctx, p, a.passes)
            if cli and not a.no_cli:
                r.update(cli_wall(p, a.passes, tmp))
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "inflate_bench.jsonl"), "w") as fh:
                    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
