"""Record which kernel instances a revision's GEMM dispatchers launch -> tests/golden/gemm_forms.json.

    python tools/make_golden_gemm_forms.py REVISION [OUT.json]

The fixture is the output of the dispatchers of REVISION (a git revision of this repository that still launches from inside its
dispatch chains), never of the working tree: tests/test_gemm_plan_host.py holds bd_gemm_plan against it.  Host only, no GPU:

  1. `git show REVISION:...` extracts csrc/ and the C header into a scratch directory; cu_count() there returns a variable.
  2. A prelude forced in front of gemm.hip and gemm_f16c8.hip re-defines hipLaunchKernelGGL: instead of launching it prints the
     kernel's address (resolved afterwards with nm + c++filt to the instance's name, template arguments included), the grid, the
     block and the argument struct's A, M and sk_split.
  3. A driver reads one case per line (prec, cus, concurrent launches, every integer / pointer field of bd_gemm_args), calls bd_gemm
     and the two predicates, and prints what was "launched".  Pointers are made-up aligned addresses that nothing dereferences.
  4. hipcc --cuda-host-only compiles the three files; this script walks the grid below and normalises the output.

Fixture layout (everything a test needs to rebuild a case is in the file):
  base       every bd_gemm_args field that is not derived, pointers as integers
  derived    lda = ldw = K, ldo = ldr = ln_op_ld = N
  variants   name -> fields that differ from base
  devices    the (cus, concurrent_launches) pairs, in the order of an entry's outcomes
  shapes     name -> {N: [...], K: [...], M: [...]}; a group walks N (outer), K, M (inner)
  kernels    unique instances [family, key...] (key: the template arguments as integers, include/boxdreamer_hip.h: bd_gemm_launch.key)
  outcomes   unique results: a negative return code, or a list of launches [kernel index, grid, block, row0, rows, split_k]
  entries    unique [takes_ln_fold, fuses_qk_rmsnorm, [outcome index per device]]
  groups     [prec, variant, shapes name, [entry index per shape]]; in that list a negative number -n repeats the index before it n more times
"""
from __future__ import annotations

import itertools
import json
import os
import sys
import tempfile

from golden_forms import ROOT, build_host_only, extract, kernel_names, sh, template_args

FILES = ["gemm.hip", "gemm_f16c8.hip", "gemm_common.h", "bd_common.h"]

# bd_gemm_args, in declaration order: (name, kind) with kind p = pointer, l = int64, i = int, f = float (not varied: never read by a dispatcher)
FIELDS = [("A", "p"), ("lda", "l"), ("a_plane", "l"), ("W", "p"), ("ldw", "l"), ("w_plane", "l"), ("bias", "p"), ("wscale", "p"),
          ("resid", "p"), ("ldr", "l"), ("addtab", "p"), ("tab_rows", "i"), ("out", "p"), ("ldo", "l"), ("out_plane", "l"),
          ("out_f32", "i"), ("M", "i"), ("N", "i"), ("K", "i"), ("act", "i"), ("rpg_in", "i"), ("rpg_out", "i"), ("row_off", "i"),
          ("w_qexp", "i"), ("rms_wq", "p"), ("rms_wk", "p"), ("rms_parts", "i"), ("ln_stats_out", "p"), ("ln_op_out", "p"),
          ("ln_op_plane", "l"), ("ln_op_ld", "l"), ("ln_stats_in", "p"), ("ln_colsum", "p"), ("ln_resid_in_op", "i"), ("sk_ws", "p"),
          ("sk_split", "i")]

PRECS = [0, 1, 2, 14, 4, 8]          # BD_PREC_BF16, F16, BF16X3, F16X3, FP8, F16C8: every prec bd_gemm accepts
DEVICES = [[256, 1], [256, 2], [256, 4], [80, 1], [80, 2], [80, 4]]
P = 0x7F0000000000                   # made-up device addresses, 4 KiB apart, 256-byte aligned
A_, W_, OUT, BIAS, RESID, TAB, WSC, RQ, RK, LST, LOP, LSI, LCS, SKW = (P + 0x1000 * k for k in range(1, 15))
BASE = {"A": A_, "a_plane": 1 << 28, "W": W_, "w_plane": 1 << 26, "bias": BIAS, "wscale": 0, "resid": 0, "addtab": 0, "tab_rows": 0,
        "out": OUT, "out_plane": 1 << 28, "out_f32": 0, "act": 0, "rpg_in": 0, "rpg_out": 0, "row_off": 0, "w_qexp": 3, "rms_wq": 0,
        "rms_wk": 0, "rms_parts": 0, "ln_stats_out": 0, "ln_op_out": 0, "ln_op_plane": 1 << 28, "ln_stats_in": 0, "ln_colsum": 0,
        "ln_resid_in_op": 0, "sk_ws": 0, "sk_split": 0}
RMS = {"rms_wq": RQ, "rms_wk": RK}
LNP = {"out_f32": 1, "resid": RESID, "ln_stats_out": LST, "ln_op_out": LOP}
LNP5 = {"ln_stats_out": LST, "ln_op_out": LOP, "ln_resid_in_op": 1}
LNC = {"ln_stats_in": LSI, "ln_colsum": LCS}
F32R = {"out_f32": 1, "resid": RESID}
# epilogue combinations; the first group walks the full shape grid, the second a thinner one that still reaches every table row
VARIANTS_FULL = {
    "f32_resid": F32R,
}
VARIANTS_THIN = {
    "operand": {},
    "gelu": {"act": 1}, "rms": RMS, "ln_producer": LNP, "ln_producer_op": {**LNP5, "out_f32": 0},
    "ln_consumer_gelu": {**LNC, "act": 1}, "splitk": {**F32R, "sk_ws": SKW},
    "no_bias": {"bias": 0},
    "f32": {"out_f32": 1},
    "out_f16": {"out_f32": 2}, "out_bf16": {"out_f32": 3}, "out_bf16x2": {"out_f32": 4}, "out_f16x2": {"out_f32": 5},
    "gelu_f32": {"act": 1, "out_f32": 1},
    "rms_parts2": {**RMS, "rms_parts": 2}, "rms_parts3": {**RMS, "rms_parts": 3},
    "rms_f16": {**RMS, "out_f32": 2}, "rms_bf16": {**RMS, "out_f32": 3}, "rms_bf16x2": {**RMS, "out_f32": 4},
    "addtab": {"addtab": TAB, "tab_rows": 64},
    "row_groups": {"rpg_in": 128, "rpg_out": 256, "row_off": 8},
    "wscale": {"wscale": WSC},
    "bias_4byte": {"bias": BIAS + 4},
    "ln_producer_f32rows": {**LNP5, "out_f32": 1},
    "ln_consumer_f16": {**LNC, "out_f32": 2}, "ln_consumer_bf16x2": {**LNC, "out_f32": 4},
    "ln_consumer_rms_f16": {**LNC, **RMS, "out_f32": 2}, "ln_consumer_rms": {**LNC, **RMS},
    "splitk2": {**F32R, "sk_ws": SKW, "sk_split": 2}, "splitk3": {**F32R, "sk_ws": SKW, "sk_split": 3},
    "splitk4": {**F32R, "sk_ws": SKW, "sk_split": 4}, "splitk_misaligned": {**F32R, "sk_ws": SKW + 16},
    "splitk_ln_producer": {**LNP, "sk_ws": SKW}, "splitk_ln_producer_op": {**LNP5, "out_f32": 0, "sk_ws": SKW, "sk_split": 2},
    "splitk_ln_producer_f32rows": {**LNP5, "out_f32": 1, "sk_ws": SKW},
}
SHAPES = {
    "full": {"N": [192, 768, 1536, 1568, 2304, 3072], "K": [64, 128, 192, 768, 2112, 3072],
             "M": [128, 300, 1024, 1536, 4000, 4096, 8400, 16500, 49152, 50112]},
    "thin": {"N": [768, 1568, 2304], "K": [128, 768, 3072], "M": [300, 1536, 4096, 50112]},
}

PRELUDE = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
extern int g_cus;
template <class ARGS> void bd_rec(const void* kernel, dim3 g, dim3 b, const ARGS& a) {
    std::printf("|%llx;%u;%u;%llu;%d;%d", (unsigned long long)(uintptr_t)kernel, g.x, b.x, (unsigned long long)(uintptr_t)a.A, a.M, a.sk_split);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) bd_rec((const void*)kernel, grid, block, __VA_ARGS__)
"""

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include "boxdreamer_hip.h"
int g_cus = 256;
int& bd_concurrent_launches();
int bd_trace_open(hipStream_t, int, int, int, int) { return -1; }
void bd_trace_close(hipStream_t, int) {}
int main() {
    static char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        long long v[64];
        int n = 0;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) v[n++] = std::atoll(t);
        bd_gemm_args a;
        std::memset(&a, 0, sizeof a);
        const int prec = (int)v[0];
        g_cus = (int)v[1];
        bd_concurrent_launches() = (int)v[2];
        int k = 3;
%s
        a.rms_eps = 1e-6f; a.ln_eps = 1e-6f;
        const int ln = bd_gemm_takes_ln_fold(&a, prec), rms = bd_gemm_fuses_qk_rmsnorm(&a, prec);
        std::printf("%%d %%d ", ln, rms);
        const int rc = bd_gemm(&a, prec, nullptr);
        std::printf("|rc=%%d\n", rc);
    }
    return 0;
}
"""


def build_recorder(rev: str, tmp: str) -> str:
    def edit(f, src):
        if f != "gemm_common.h":
            return src
        assert src.count("inline int cu_count() {") == 1
        return src.replace("inline int cu_count() {", "inline int cu_count() { return ::g_cus; }\ninline int cu_count_of_device() {")

    csrc = extract(rev, tmp, FILES, edit)
    cast = {"p": "(decltype(a.%s))(uintptr_t)", "l": "(int64_t)", "i": "(int)"}
    reads = "\n".join(f"        a.{n} = {cast[t] % n if t == 'p' else cast[t]}v[k++];" for n, t in FIELDS)
    return build_host_only(tmp, [os.path.join(csrc, "gemm.hip"), os.path.join(csrc, "gemm_f16c8.hip")], PRELUDE, DRIVER % reads)


FAMILIES = {"gemm_kernel_pc": 1, "gemm_kernel_glds": 2, "gemm_kernel_pc_f16c8": 3}
KEY_LEN = 13


def parse_kernel(mangled: str):
    """A mangled instance name -> (family, template arguments as integers, zero-padded)."""
    name, key = template_args(mangled, r"gemm_kernel_[a-z0-9_]+?")
    assert len(key) <= KEY_LEN
    return FAMILIES[name], key + [0] * (KEY_LEN - len(key))


def case_fields(variant: dict, N: int, K: int, M: int) -> dict:
    f = {**BASE, **variant, "M": M, "N": N, "K": K}
    f.update(lda=K, ldw=K, ldo=N, ldr=N, ln_op_ld=N)
    return f


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    rev = sh(["git", "-C", ROOT, "rev-parse", sys.argv[1]]).strip()
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "gemm_forms.json")
    groups_in = [(p, v, "full") for v in VARIANTS_FULL for p in PRECS] + [(p, v, "thin") for v in VARIANTS_THIN for p in PRECS]
    variants = {**VARIANTS_FULL, **VARIANTS_THIN}
    lines = []
    for prec, v, sname in groups_in:
        s = SHAPES[sname]
        for N, K, M in itertools.product(s["N"], s["K"], s["M"]):
            f = case_fields(variants[v], N, K, M)
            for cus, conc in DEVICES:
                lines.append(" ".join(str(x) for x in [prec, cus, conc] + [f[n] for n, _ in FIELDS]))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_recorder(rev, tmp)
        res = sh([exe], input="\n".join(lines) + "\n").splitlines()
        names = kernel_names(exe, "gemm_kernel_")
    assert len(res) == len(lines), (len(res), len(lines))
    kernels, outcomes, entries, groups = {}, {}, {}, []
    it = iter(res)
    n_shapes = 0
    for prec, v, sname in groups_in:
        s = SHAPES[sname]
        esz = 1 if prec == 4 else 2
        idx = []
        for N, K, M in itertools.product(s["N"], s["K"], s["M"]):
            per_dev, preds = [], None
            for _ in DEVICES:
                parts = next(it).split("|")
                ln, rms = (int(x) for x in parts[0].split())
                assert preds in (None, (ln, rms)), "a predicate's answer depends on the device parameters"
                preds = (ln, rms)
                rc = int(parts[-1][3:])
                if rc < 0:
                    assert len(parts) == 2, "a refused call launched something"
                    oc = rc
                else:                                    # (0, or the no-device error of hipGetLastError)
                    oc = []
                    for rec in parts[1:-1]:
                        name, g, b, aptr, m, sk = rec.rsplit(";", 5)
                        fam, key = parse_kernel(names[name])
                        row0 = (int(aptr) - A_) // (K * esz)
                        assert (int(aptr) - A_) % (K * esz) == 0
                        kern = kernels.setdefault(json.dumps([fam, *key]), len(kernels))
                        oc.append([kern, int(g), int(b), row0, int(m), int(sk) if key[8] and fam == 3 else 1])
                    assert oc, "an accepted call launched nothing"
                oc_key = json.dumps(oc)
                per_dev.append(outcomes.setdefault(oc_key, len(outcomes)))
            e_key = json.dumps([preds[0], preds[1], per_dev])
            idx.append(entries.setdefault(e_key, len(entries)))
        rle = []
        for e in idx:
            if rle and rle[-1] < 0 and last == e:
                rle[-1] -= 1
            elif rle and last == e:
                rle.append(-1)
            else:
                rle.append(e)
            last = e
        groups.append([prec, v, sname, rle])
        n_shapes += len(idx)
    n_cases = n_shapes * len(DEVICES)
    doc = {"revision": rev, "cases": n_cases, "base": BASE, "derived": "lda = ldw = K; ldo = ldr = ln_op_ld = N",
           "fields": [n for n, _ in FIELDS], "variants": variants, "devices": DEVICES, "shapes": SHAPES,
           "kernels": [json.loads(k) for k in kernels],
           "outcomes": [json.loads(k) for k in outcomes], "entries": [json.loads(k) for k in entries], "groups": groups}
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")
    print(f"{out_path}: {n_cases} cases, {len(outcomes)} outcomes, {os.path.getsize(out_path)} bytes, revision {rev[:12]}")


if __name__ == "__main__":
    main()
