"""The BGZF block writer (basecount_amd/csrc/bc_deflate.h) on its host machine, compiled with
AddressSanitizer and UBSan as a stand-alone program (tests/native/deflate_check.cpp) and linked with
zlib: every block of every case inflates to its input with zlib's inflate and with the project's own
decoder, carries zlib's CRC-32 and the right BSIZE / ISIZE and fits 65,536 bytes.  On the four real
texts the output must be smaller than the text (a fixed-code coder that finds no match cannot be, so
the matcher works and the stored fallback is not what passes), and its size is pinned against zlib at
level 1 with Z_FIXED on the same cuts."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
# text -> (plain bytes, zlib level 1 Z_FIXED raw deflate on 65,280-byte cuts + 26 bytes of framing per
# block, measured once; the ratio of this writer's bytes to that, measured on the host twin)
TEXTS = {
    "cli/c1_default.out.gz": (625_778, 221_728, 0.9981),
    "cli/mixed_default.out.gz": (2_128_924, 745_943, 0.9833),
    "cli/c1_long.out.gz": (1_670_855, 387_795, 0.9140),
    "ont/cli/ont_default.out.gz": (393_349, 130_050, 0.9984),
}


@pytest.fixture(scope="module")
def output():
    src = os.path.join(REPO, "tests", "native", "deflate_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "deflate_check")
        try:
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe, "-lz"],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("deflate_check.cpp does not compile:\n" + e.stderr)
        return subprocess.run([exe] + [os.path.join(GOLDEN, t) for t in TEXTS], capture_output=True, text=True,
                              timeout=300)


def test_every_case_round_trips_under_the_sanitizers(output):
    # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
    assert output.returncode == 0 and output.stderr == "", output.stdout + output.stderr
    last = output.stdout.split("\n")[-2].split()
    assert last[0] == "ok" and int(last[1]) > 10_000, output.stdout


def sizes(output):
    out = {}
    for line in output.stdout.splitlines():
        w = line.split()
        if w and w[0] == "text":
            out[os.path.relpath(w[1], GOLDEN)] = (int(w[2]), int(w[3]), int(w[4]))
    return out


@pytest.mark.parametrize("text", list(TEXTS))
def test_real_texts_compress(output, text):
    plain, ours, _ = sizes(output)[text]
    assert plain == TEXTS[text][0]
    print(f"{text}: {plain} bytes of text, {ours} compressed")
    assert ours < plain


@pytest.mark.parametrize("text", list(TEXTS))
def test_size_against_zlib_level_1_fixed(output, text):
    """The measured ratio to the zlib reference plus 2 % (the bytes are deterministic; the margin is
    room for a later change to the schedule)."""
    _, ours, zlib_here = sizes(output)[text]
    _, ref, ratio = TEXTS[text]
    print(f"{text}: {ours} bytes, {ours / ref:.4f} of the reference's {ref} (this machine's zlib: {zlib_here})")
    assert ours <= ref * ratio * 1.02
