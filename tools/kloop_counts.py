"""Instruction mix of a GEMM kernel's K loop, read from hipcc's assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc -I include --cuda-device-only -S boxdreamer_amd/csrc/gemm_f16c8.hip -o f16c8.s
    python tools/kloop_counts.py f16c8.s 'gemm_kernel_pc_f16c8ILi3ELi1ELi0ELb1ELi4ELi2ELi4ELb1ELb0EE' [...]

For every kernel whose mangled name contains one of the given substrings: VGPRs, scratch and LDS bytes from the kernel descriptor
comments, then every loop (a backward branch to a label) that contains MFMAs, with its instruction counts by kind.  A loop unrolled
over the ring period holds several slabs; the counts are printed per loop AND per slab (= per s_barrier).
"""
from __future__ import annotations

import collections
import re
import sys


def kind(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_"):
        return "ds_other"
    if op.startswith("v_cvt_scalef32_pk_fp8"):
        return "cvt_fp8"
    if op in ("s_waitcnt", "s_barrier", "s_nop"):
        return op
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("v_"):
        return "valu:" + op
    if op.startswith("s_"):
        return "salu"
    return "other:" + op


def functions(lines):
    name, start = None, 0
    for n, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, start = m.group(1), n
        elif name and l.startswith(".Lfunc_end"):
            yield name, start, n
            name = None


def loops(body):
    """(first, last) line indices of every innermost backward-branch loop."""
    labels = {}
    out = []
    for n, l in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            labels[m.group(1)] = n
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in labels:
            out.append((labels[m.group(1)], n))
    inner = [a for a in out if not any(b != a and a[0] <= b[0] and b[1] <= a[1] for b in out)]
    return inner


def main():
    lines = open(sys.argv[1]).read().splitlines()
    pats = sys.argv[2:]
    meta = {}
    cur = None
    for l in lines:
        m = re.match(r"^\s+\.amdhsa_kernel (\S+)", l)
        if m:
            cur = m.group(1)
            meta[cur] = {}
        m = re.match(r"^\s+\.amdhsa_(next_free_vgpr|group_segment_fixed_size|private_segment_fixed_size|accum_offset) (\d+)", l)
        if m and cur:
            meta[cur][m.group(1)] = int(m.group(2))
    for name, a, b in functions(lines):
        if pats and not any(p in name for p in pats):
            continue
        body = lines[a:b]
        md = meta.get(name, {})
        print(f"== {name}\n   vgprs(+agprs) {md.get('next_free_vgpr')}  scratch {md.get('private_segment_fixed_size')}  lds {md.get('group_segment_fixed_size')}")
        for lo, hi in loops(body):
            c = collections.Counter()
            for l in body[lo:hi + 1]:
                m = re.match(r"^\s+([a-z]\w+)", l)
                if m:
                    c[kind(m.group(1))] += 1
            slabs = max(c["s_barrier"], 1)
            # (not a K loop; or a tile loop around head / remainder slabs and part of the epilogue: its counts are not whole per slab)
            if c["mfma"] < 6 or c["mfma"] % slabs or c["ds_read"] % slabs:
                continue
            valu = sum(v for k, v in c.items() if k.startswith("valu:"))
            total = sum(c.values())
            print(f"   loop of {total} instructions, {slabs} slab(s): per slab {total / slabs:.1f}; mfma {c['mfma'] / slabs:g}  ds_read {c['ds_read'] / slabs:g}  "
                  f"cvt_fp8 {c['cvt_fp8'] / slabs:g}  other VALU {valu / slabs:g}  s_waitcnt {c['s_waitcnt'] / slabs:g}  s_barrier {c['s_barrier'] / slabs:g}  "
                  f"salu {c['salu'] / slabs:g}  branch {c['branch'] / slabs:g}")
            for k, v in sorted(c.items()):
                if k.startswith("valu:") or k.startswith("other:") or k == "ds_other":
                    print(f"      {k}: {v}")


if __name__ == "__main__":
    main()
