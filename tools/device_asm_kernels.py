#!/usr/bin/env python3
"""Compare two gfx950 assembly files of ONE unit kernel by kernel (for a change that ADDS kernels to a unit, where
tools/device_asm_diff.sh -- which compares whole files -- can only say "differs"):

    tools/device_asm_diff.sh <rev-a> WORKTREE /tmp/asm          # leaves /tmp/asm/{a,b}/asm/<unit>.s
    tools/device_asm_kernels.py /tmp/asm/a/asm/conv_p2.s /tmp/asm/b/asm/conv_p2.s

Per kernel of the first file: the text of the function (label to .Lfunc_end, comments included, nothing normalised) and its
.amdhsa_kernel descriptor block (register counts, LDS, scratch) must be the same in the second; kernels only the second file
has are listed with their descriptor's register counts.  Exit status 0 iff every kernel of the first file is identical."""
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
        if cur:
            out[cur].append(line)
            if re.match(r"^\.Lfunc_end\d+:", line):
                cur = None
    return out


def descriptors(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        if cur:
            out[cur].append(line)
            if ".end_amdhsa_kernel" in line:
                cur = None
    return out


def main(a_path, b_path):
    fa, fb, da, db = functions(a_path), functions(b_path), descriptors(a_path), descriptors(b_path)
    bad = 0
    for k in sorted(fa):
        same = fa[k] == fb.get(k) and da.get(k) == db.get(k)
        bad += not same
        print(f"{'identical' if same else 'DIFFERS  '}  {k}  ({len(fa[k])} lines)")
    for k in sorted(set(fb) - set(fa)):
        regs = " ".join(l.strip() for l in db.get(k, []) if re.search(r"next_free_[vs]gpr|accum_offset|group_segment|private_segment_fixed", l))
        print(f"new        {k}  ({len(fb[k])} lines)  {regs}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
