"""Static VALU counts per basic block of one kernel, from the compiler's assembly listing:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Iinclude \
          -S --cuda-device-only -o pileup.s basecount_amd/csrc/bc_pileup.hip
    python scripts/valu_blocks.py pileup.s 'k_pileup<false, 5, true, int>' [min_valu]
Blocks begin at .LBB labels, at the compiler's fall-through block comments (`; %bb.N`) and after
every branch, so a straight path is the sum of the blocks it runs through.  One line per block with
at least min_valu (default 8) VALU instructions: label (`+n`: the n-th piece after that label),
VALU, of which DPP, v_bitop3, v_alignbit, LDS reads, and the block's last branch target, if any."""
import re
import subprocess
import sys

path, want = sys.argv[1], sys.argv[2]
min_valu = int(sys.argv[3]) if len(sys.argv) > 3 else 8
lines = open(path).read().splitlines()
start = None
for i, ln in enumerate(lines):
    m = re.match(r"^(_Z\w+):", ln)
    if m:
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if want in name.replace("(anonymous namespace)::", ""):
            start = i
            break
if start is None:
    sys.exit("kernel not found: " + want)
blocks, cur = [], {"label": "entry", "ins": []}
base, piece = "entry", 0
for ln in lines[start + 1:]:
    if ln.startswith(".Lfunc_end"):
        break
    m = re.match(r"^(\.LBB\d+_\d+):", ln)
    if m:
        blocks.append(cur)
        cur = {"label": m.group(1), "ins": []}
        base, piece = m.group(1), 0
        continue
    t = ln.strip()
    if re.match(r"^; %bb\.\d+", t) and cur["ins"]:
        blocks.append(cur)
        piece += 1
        cur = {"label": f"{base}+{piece}", "ins": []}
        continue
    if t and not t.startswith((";", ".")):
        cur["ins"].append(t)
        if t.startswith(("s_cbranch", "s_branch")):
            blocks.append(cur)
            piece += 1
            cur = {"label": f"{base}+{piece}", "ins": []}
blocks.append(cur)
total = 0
for b in blocks:
    v = [x for x in b["ins"] if x.startswith("v_")]
    total += len(v)
    if len(v) < min_valu:
        continue
    last = b["ins"][-1] if b["ins"] else ""
    to = last.split()[-1] if last.startswith(("s_cbranch", "s_branch")) else ""
    print(f"{b['label']:>14} valu {len(v):4d} dpp {sum('dpp' in x for x in v):3d} bitop3 {sum(x.startswith('v_bitop3') for x in v):3d}"
          f" alignbit {sum(x.startswith('v_alignbit') for x in v):2d} ds_read {sum(x.startswith('ds_read') for x in b['ins']):2d}"
          f" ins {len(b['ins']):4d}  {('-> ' + to) if to else ''}")
print("kernel VALU (static)", total)
