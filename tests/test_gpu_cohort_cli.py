"""`python -m basecount_amd.cohort ... --out-dir DIR BAM ...` as a subprocess under PYTHONHASHSEED=0:
every DIR/X.tsv holds the bytes `python -m basecount_amd X.bam <flags>` prints -- the reference's
committed golden wherever tests/golden/manifest.json or tests/golden/ont/manifest.json has that
file with those arguments, the single-file run() output (one helper process, same hash seed)
otherwise.  err_range.bam fails: its output is empty, stderr names it with the golden's IndexError,
the exit status is 1, and every other file is complete."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

CASES = {
    "default": [],
    "bed": ["--summarise-with-bed", "scheme.bed"],
    "q20_m30": ["--min-base-quality", "20", "--min-mapping-quality", "30"],
    "shown_long": ["--show-n-bases", "--long-format"],
    "summary": ["--summarise"],
}
# the golden cases the table of the change names: each must be found in a manifest
NAMED = {"default": ["c1_default", "mixed_default", "ont_default"], "bed": ["c1_bed", "mixed_bed"],
         "q20_m30": ["c1_q20_m30", "mixed_q20_m30", "ont_q20_m30"], "shown_long": ["mixed_shown_long", "ont_shown_long"],
         "summary": ["c1_summary", "ont_summary"]}

_HELPER = r"""
import contextlib, io, json, sys
from basecount_amd.main import run
for out, argv in json.load(open(sys.argv[1])):
    with open(out, "wb") as raw:
        txt = io.TextIOWrapper(raw, encoding="utf-8", write_through=True)
        with contextlib.redirect_stdout(txt):
            try:
                run(argv)
            except BaseException as e:  # what it printed before stays; the failure goes beside it
                with open(out + ".err", "w") as fh:
                    fh.write(f"{type(e).__name__}: {e}")
            txt.flush()
        txt.detach()
"""


def _env(**kw):
    env = dict(os.environ, PYTHONPATH=REPO, PYTHONHASHSEED="0")
    for v in ("BASECOUNT_DEVICE_FORMAT", "BASECOUNT_GROUP_MAX", "BASECOUNT_GROUP_REFS", "BASECOUNT_LONG_READS",
              "BASECOUNT_BATCH_RECORDS", "BASECOUNT_COHORT_BYTES", "BASECOUNT_HIP_TIMING", "WORLD_SIZE"):
        env.pop(v, None)
    env.update(kw)
    return env


def _goldens():
    """{(golden file's basename, args): (case name, expected stdout bytes)} of the hash-seed-0 cases that succeed."""
    out = {}
    for root in (GOLDEN, os.path.join(GOLDEN, "ont")):
        with open(os.path.join(root, "manifest.json")) as fh:
            man = json.load(fh)
        for name, c in man.items():
            if c.get("hashseed", "0") != "0" or c.get("returncode", 0) != 0 or "stdout" not in c:
                continue
            with open(os.path.join(root, c["stdout"]), "rb") as fh:
                out[(os.path.basename(c["bam"]), tuple(c["args"]))] = (name, gzip.decompress(fh.read()))
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The inputs, and every expected output: the goldens, and one helper process for the rest."""
    tmp = tmp_path_factory.mktemp("cohort_cli")
    again = str(tmp / "c1_again.bam")
    shutil.copyfile(os.path.join(GOLDEN, "c1.bam"), again)
    bams = [os.path.join(GOLDEN, "c1.bam"), os.path.join(GOLDEN, "mixed.bam"), again,
            os.path.join(GOLDEN, "ont", "ont.bam"), os.path.join(GOLDEN, "edge.bam"),
            os.path.join(GOLDEN, "err_range.bam")]
    gold = _goldens()
    expected, jobs, used = {}, [], {}
    for case, args in CASES.items():
        for b in bams:
            stem = os.path.splitext(os.path.basename(b))[0]
            key = ("c1.bam" if stem == "c1_again" else os.path.basename(b), tuple(args))
            if key in gold:
                expected[(case, stem)] = gold[key][1]
                used.setdefault(case, set()).add(gold[key][0])
            else:
                out = str(tmp / f"exp_{case}_{stem}.out")
                jobs.append((out, [b] + args))
                expected[(case, stem)] = out
    for case, names in NAMED.items():
        assert set(names) <= used.get(case, set()), (case, names, used.get(case))
    job_file = str(tmp / "jobs.json")
    with open(job_file, "w") as fh:
        json.dump(jobs, fh)
    p = subprocess.run([sys.executable, "-c", _HELPER, job_file], cwd=GOLDEN, env=_env(), capture_output=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    failures = {}
    for key, v in expected.items():
        if isinstance(v, str):
            with open(v, "rb") as fh:
                expected[key] = fh.read()
            if os.path.exists(v + ".err"):
                with open(v + ".err") as fh:
                    failures[key] = fh.read()
    with open(os.path.join(GOLDEN, "manifest.json")) as fh:
        err = json.load(fh)["err_range"]["error"]
    # err_range fails with the golden's IndexError wherever base quality 0 is counted; at 20 the
    # overhanging base is below the bar and the single-file command succeeds (golden err_range_q20)
    assert failures == {(case, "err_range"): err for case in CASES if case != "q20_m30"}
    return dict(tmp=tmp, bams=bams, expected=expected, failures=failures)


def _cohort(world, case, out_name, **env):
    out = str(world["tmp"] / out_name)
    p = subprocess.run([sys.executable, "-m", "basecount_amd.cohort"] + CASES[case] + ["--out-dir", out] + world["bams"],
                       cwd=GOLDEN, env=_env(**env), capture_output=True, timeout=300)
    return out, p


def _check(world, case, out, p):
    err = p.stderr.decode()
    failed = {stem: msg for (c, stem), msg in world["failures"].items() if c == case}
    assert p.returncode == (1 if failed else 0), err
    listed = [ln for ln in err.splitlines() if ".bam: " in ln]
    assert listed == [f"{b}: {failed[os.path.splitext(os.path.basename(b))[0]]}" for b in world["bams"]
                      if os.path.splitext(os.path.basename(b))[0] in failed], err
    assert p.stdout == b""
    assert sorted(os.listdir(out)) == sorted(os.path.splitext(os.path.basename(b))[0] + ".tsv" for b in world["bams"])
    for b in world["bams"]:
        stem = os.path.splitext(os.path.basename(b))[0]
        with open(os.path.join(out, stem + ".tsv"), "rb") as fh:
            got = fh.read()
        assert got == world["expected"][(case, stem)], (case, stem)
        assert (len(got) == 0) == (stem in failed), stem  # empty up to the failure, complete otherwise


@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_equal_the_goldens_and_the_single_file_runs(world, case):
    out, p = _cohort(world, case, "out_" + case)
    _check(world, case, out, p)


def test_device_formatted_rows_and_the_timing_line(world):
    out, p = _cohort(world, "default", "out_devfmt", BASECOUNT_DEVICE_FORMAT="1", BASECOUNT_HIP_TIMING="1")
    _check(world, "default", out, p)
    line = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("basecount cohort:")]
    assert len(line) == 1 and "6 files, 2 groups, 2 singles" in line[0]
    for word in ("decode", "upload", "kernels + download", "format + write"):
        assert word in line[0]


def test_bam_list_and_refusals(world, tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(world["bams"][:2]) + "\n")
    out = str(tmp_path / "o")
    p = subprocess.run([sys.executable, "-m", "basecount_amd.cohort", "--summarise", "--out-dir", out, "--bam-list",
                        str(lst)], cwd=GOLDEN, env=_env(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode()
    for stem in ("c1", "mixed"):
        with open(os.path.join(out, stem + ".tsv"), "rb") as fh:
            assert fh.read() == world["expected"][("summary", stem)]
    p = subprocess.run([sys.executable, "-m", "basecount_amd.cohort", "--out-dir", out] + world["bams"][:1],
                       cwd=GOLDEN, env=_env(WORLD_SIZE="2"), capture_output=True, timeout=300)
    assert p.returncode == 2 and b"WORLD_SIZE" in p.stderr
