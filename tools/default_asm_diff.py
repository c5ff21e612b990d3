#!/usr/bin/env python3
"""Instruction diff of kernels between two device-assembly listings of one kernel source of the library (no GPU needed).

A change that must not move a kernel -- the default test configuration of posepaf_kernels.hip keeps launching the instances with
the literals, the halo convolution of posepaf_conv_own.hip keeps its hand-placed main loop -- is shown instruction for instruction.
Emit the listing of each revision of the source with the library's own flags

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -fvisibility=hidden -ffp-contract=off -fno-fast-math -DPP_BUILDING \
          --cuda-device-only -S improved-body-parts_amd/csrc/<source>.hip -o <rev>.s

and run `default_asm_diff.py parent.s new.s [name-substring ...]` (e.g. `k_conv3x3_halo`).  For every kernel present in both listings
whose symbol contains one of the substrings (default: the Python-rule and full-resolution kernels of posepaf_kernels.hip; pass ''
for every kernel of the listing) the instruction streams are compared
after dropping comments, labels' numbering and assembler directives, and the resource lines (.vgpr_count, .sgpr_count, LDS, scratch)
are printed.  Exit status 1 when any compared kernel differs."""
import re
import sys


def kernels(path):
    out, name, body, meta = {}, None, [], {}
    res = {}
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):\s*; @", line)
        if m:
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            if line.startswith(".Lfunc_end"):
                name = None
            continue
        s = line.split(";", 1)[0].rstrip()
        if not s or s.lstrip().startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                body.append("LABEL")
            continue
        body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s.strip()))
    for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", open(path, errors="replace").read()):
        res[m.group(1)] = (int(m.group(3)), int(m.group(2)))
    return out, res


def main():
    a, ra = kernels(sys.argv[1])
    b, rb = kernels(sys.argv[2])
    subs = sys.argv[3:] or ["_py", "fullres"]
    bad = 0
    for name in sorted(a):
        if name not in b or not any(s in name for s in subs):
            continue
        same = a[name] == b[name]
        bad += not same
        print(f"{'same' if same else 'DIFFERENT':9s} {len(a[name]):6d} / {len(b[name]):6d} instructions  vgpr,sgpr {ra.get(name)} / {rb.get(name)}  {name}")
    for name in sorted(set(b) - set(a)):
        if any(s in name for s in subs):
            print(f"{'new':9s} {len(b[name]):6d} instructions  vgpr,sgpr {rb.get(name)}  {name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
