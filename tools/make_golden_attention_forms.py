"""Record which kernel instance a revision's attention entry points launch -> tests/golden/attention_forms.json.

    python tools/make_golden_attention_forms.py REVISION [OUT.json]

The fixture is the output of the entry points of REVISION (a git revision of this repository that still launches from inside its
dispatch templates), never of the working tree: tests/test_attention_plan_host.py holds bd_attention_plan against it.  Host only, no
GPU, by the method of make_golden_gemm_forms.py (golden_forms.py holds what the two share): a prelude forced in front of attention.hip
re-defines hipLaunchKernelGGL to print the kernel's address, grid, block and the argument struct's q_len, q_off and out_rows; a driver
reads one call per line and makes it through bd_attention, bd_attention_q (bd_attention_q_forms with latency_forms 1: no public entry
point takes that flag), bd_attention_prefix or bd_attention_varlen.  Pointers are made-up addresses that nothing dereferences.

Fixture layout (everything a test needs to rebuild a call is in the file):
  fields     the integer fields of a call (include/boxdreamer_hip.h: bd_attn_call), prec and latency_forms apart
  defaults   their values where a group's shape does not name them
  pointers   name -> [qkv, out, view_start, q_view] as integers (q_view: used where the shape has has_q_view)
  precs      the `prec` values every group walks
  kernels    unique instances [family, key...] (bd_attn_launch.key)
  outcomes   unique results: a negative return code, or [kernel index, grid, block, q_len, q_off, out_rows]
  groups     [shape, pointers name, [latency_forms...], [outcome index per (prec, latency_forms), prec outer]]
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

from golden_forms import ROOT, build_host_only, extract, kernel_names, sh, template_args

FILES = ["attention.hip", "bd_common.h"]
FIELDS = ["entry", "batch", "seq", "heads", "head_dim", "has_q_view", "q_len", "n_prefix", "prefix_queries", "n_views", "max_views",
          "tokens_per_view"]
DEFAULTS = {"entry": 0, "batch": 2, "seq": 0, "heads": 8, "head_dim": 96, "has_q_view": 0, "q_len": 0, "n_prefix": 0, "prefix_queries": 0,
            "n_views": 0, "max_views": 0, "tokens_per_view": 0}
PLAIN, Q, PREFIX, VARLEN = 0, 1, 2, 3                # BD_ATTN_ENTRY_*
PRECS = [0, 1, 2, 3, 5, 9, 10, 16, 17, 4, 8, 14]     # the nine classes of attention, then the GEMM-only BD_PREC_FP8, F16C8, F16X3
P = 0x7F0000000000                                   # made-up device addresses
QKV, OUT, VS, QV = (P + 0x1000 * k for k in range(1, 5))
POINTERS = {
    "ok": [QKV, OUT, VS, QV], "out_8": [QKV, OUT + 8, VS, QV],
    "qkv_null": [0, OUT, VS, QV], "out_null": [QKV, 0, VS, QV], "view_start_null": [QKV, OUT, 0, QV],
    "qkv_8": [QKV + 8, OUT, VS, QV], "out_4": [QKV, OUT + 4, VS, QV], "qkv_null_out_4": [0, OUT + 4, VS, QV],
}


def shapes():
    """(shape, latency_forms values): both sides of every threshold of the dispatch rules and of every refusal."""
    out = []
    uniform = []                                     # (entry fields) of the forms that take all `seq` rows as queries
    for seq in (250, 256, 261, 288, 384, 96, 192, 64, 1, 1536, 2048, 2304):          # waste3 < waste4 (ties included); whole ping-pong blocks
        for hd in (96, 64):
            for batch in (1, 2):
                uniform.append({"seq": seq, "head_dim": hd, "batch": batch})
    for bad in ({"seq": 261, "head_dim": 80}, {"seq": 261, "head_dim": 0}, {"seq": 1536, "head_dim": 80}, {"seq": 0}, {"seq": 256, "batch": 0},
                {"seq": 256, "heads": 0}, {"seq": 256, "heads": -1},
                # the 2 GiB of one sample's rows: seq * 3 * heads * head_dim * 2 bytes, just under and just over
                {"seq": 466033}, {"seq": 466034}, {"seq": 699050, "head_dim": 64}, {"seq": 699051, "head_dim": 64},
                {"seq": 261, "heads": 12, "head_dim": 64, "batch": 10}):             # (DINOv2)
        uniform.append(bad)
    for u in uniform:
        out.append(({"entry": PLAIN, **u}, [0]))
        out.append(({"entry": Q, **u, "q_len": u["seq"]}, [0, 1]))
        out.append(({"entry": PREFIX, **u, "n_prefix": 5, "prefix_queries": 1}, [0]))
        out.append(({"entry": PREFIX, **u, "n_prefix": 5, "prefix_queries": 0}, [0]))      # (seq 261: 256 queries, ragged last key tile)
    for extra in ({"seq": 320, "n_prefix": 64}, {"seq": 320, "n_prefix": 64, "head_dim": 64}, {"seq": 1600, "n_prefix": 64},
                  {"seq": 261, "n_prefix": 0}, {"seq": 261, "n_prefix": 261}, {"seq": 261, "n_prefix": 260}, {"seq": 261, "n_prefix": -1}):
        for pq in (0, 1):
            out.append(({"entry": PREFIX, **extra, "prefix_queries": pq}, [0]))
    # bd_attention_q with q_view; "few": 4 * ceil(q_len / 256) * heads * batch <= 256
    for seq, q_len in ((1536, 256), (1536, 512), (1536, 768), (2048, 256), (1536, 1536), (2048, 2048), (2304, 2304), (4608, 2304), (522, 261),
                       (768, 192), (768, 96), (1536, 0), (1536, -256), (256, 512), (1536, 1000), (1536, 1024)):
        for batch in (1, 2):
            for hd in (96, 64) if q_len in (256, 261) else (96,):
                out.append(({"entry": Q, "seq": seq, "q_len": q_len, "has_q_view": 1, "batch": batch, "head_dim": hd}, [0, 1]))
    for batch, heads in ((4, 8), (8, 8), (9, 8), (16, 4), (17, 4), (1, 64), (1, 65)):
        out.append(({"entry": Q, "seq": 1536, "q_len": 256, "has_q_view": 1, "batch": batch, "heads": heads}, [0, 1]))
    out.append(({"entry": Q, "seq": 1536, "q_len": 1536, "has_q_view": 0, "batch": 1}, [0, 1]))      # (few without q_view)
    out.append(({"entry": Q, "seq": 1536, "q_len": 256, "has_q_view": 0}, [0, 1]))                   # q_len != seq without q_view
    # bd_attention_varlen
    rag = {"entry": VARLEN, "n_views": 5, "max_views": 3}
    for tpv in (128, 256, 192, 384, 512, 64, 0, -128):
        for qv in (0, 1):
            out.append(({**rag, "tokens_per_view": tpv, "has_q_view": qv}, [0]))
    for more in ({"max_views": 4}, {"max_views": 5}, {"max_views": 0}, {"n_views": 1}, {"n_views": 2, "max_views": 1}, {"batch": 0}, {"heads": 0},
                 {"head_dim": 64}, {"head_dim": 80}, {"head_dim": 0}, {"batch": 1, "n_views": 1, "max_views": 1},
                 {"batch": 1, "n_views": 3, "max_views": 3, "has_q_view": 1}, {"seq": 1536},
                 # one sample's 2 GiB (max_views * tokens_per_view rows), its row count as an int, and the grid as an int
                 {"n_views": 4000, "max_views": 3640}, {"n_views": 4000, "max_views": 3641},
                 {"n_views": (1 << 24) + 1, "max_views": 1 << 24}, {"n_views": 1 << 24, "max_views": (1 << 24) - 1},
                 {"n_views": (1 << 28) - 1}, {"n_views": 1 << 28}, {"n_views": (1 << 28) - 1, "has_q_view": 1}, {"n_views": 1 << 28, "has_q_view": 1}):
        out.append(({**rag, "tokens_per_view": 128, **more}, [0]))
    for nv in ((1 << 27) - 1, 1 << 27):
        out.append(({**rag, "tokens_per_view": 256, "n_views": nv}, [0]))
    return out


def pointer_cases():
    """Refusals of the pointers, alone and on calls that are wrong in a second way (which refusal wins)."""
    out = []
    calls = [{"entry": PLAIN, "seq": 261, "head_dim": 64}, {"entry": PLAIN, "seq": 261, "head_dim": 80}, {"entry": PLAIN, "seq": 0},
             {"entry": PLAIN, "seq": 466034},
             {"entry": Q, "seq": 1536, "q_len": 256, "has_q_view": 1}, {"entry": Q, "seq": 1536, "q_len": 1000, "has_q_view": 1},
             {"entry": PREFIX, "seq": 261, "n_prefix": 5, "prefix_queries": 0, "head_dim": 64},
             {"entry": PREFIX, "seq": 261, "n_prefix": 5, "prefix_queries": 1, "head_dim": 64},
             {"entry": PREFIX, "seq": 261, "n_prefix": 0, "prefix_queries": 1}, {"entry": PREFIX, "seq": 261, "n_prefix": 5, "prefix_queries": 0, "head_dim": 80},
             {"entry": PREFIX, "seq": 261, "n_prefix": 5, "prefix_queries": 1, "head_dim": 80},
             {"entry": VARLEN, "n_views": 5, "max_views": 3, "tokens_per_view": 256},
             {"entry": VARLEN, "n_views": 5, "max_views": 3, "tokens_per_view": 192},
             {"entry": VARLEN, "n_views": 5, "max_views": 3, "tokens_per_view": 256, "head_dim": 64}]
    for name in POINTERS:
        if name != "ok":
            out += [(c, name) for c in calls]
    return out


PRELUDE = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
template <class ARGS> void bd_rec(const void* kernel, dim3 g, dim3 b, const ARGS& a) {
    std::printf("%llx;%u;%u;%d;%d;%d|", (unsigned long long)(uintptr_t)kernel, g.x, b.x, a.q_len, a.q_off, a.out_rows);
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
int bd_trace_open(hipStream_t, int, int, int, int) { return -1; }
void bd_trace_close(hipStream_t, int) {}
int bd_attention_q_forms(const void* qkv, int64_t qkv_plane, void* out, int64_t out_plane, int batch, int seq, int heads, int head_dim,
                         float scale, const int32_t* q_view, int q_len, int prec, int latency_forms, void* stream);
int main() {
    static char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        long long v[32];
        int n = 0;
        for (char* t = std::strtok(line, " \n"); t; t = std::strtok(nullptr, " \n")) v[n++] = std::atoll(t);
        const int entry = (int)v[0], batch = (int)v[1], seq = (int)v[2], heads = (int)v[3], head_dim = (int)v[4], has_q_view = (int)v[5],
                  q_len = (int)v[6], n_prefix = (int)v[7], prefix_queries = (int)v[8], n_views = (int)v[9], max_views = (int)v[10],
                  tpv = (int)v[11], prec = (int)v[12], lat = (int)v[13];
        const void* qkv = (const void*)(uintptr_t)v[14];
        void* out = (void*)(uintptr_t)v[15];
        const int32_t* vs = (const int32_t*)(uintptr_t)v[16];
        const int32_t* qv = has_q_view ? (const int32_t*)(uintptr_t)v[17] : nullptr;
        const int64_t qp = 1 << 28, op = 1 << 26;
        int rc = -99;
        if (entry == 0 && !lat) rc = bd_attention(qkv, qp, out, op, batch, seq, heads, head_dim, 0.125f, prec, nullptr);
        if (entry == 1 && !lat) rc = bd_attention_q(qkv, qp, out, op, batch, seq, heads, head_dim, 0.125f, qv, q_len, prec, nullptr);
        if (entry == 1 && lat) rc = bd_attention_q_forms(qkv, qp, out, op, batch, seq, heads, head_dim, 0.125f, qv, q_len, prec, lat, nullptr);
        if (entry == 2 && !lat) rc = bd_attention_prefix(qkv, qp, out, op, batch, seq, heads, head_dim, 0.125f, n_prefix, prefix_queries, prec, nullptr);
        if (entry == 3 && !lat) rc = bd_attention_varlen(qkv, qp, out, op, vs, batch, n_views, max_views, tpv, heads, head_dim, 0.125f, qv, prec, nullptr);
        std::printf("rc=%d\n", rc);
    }
    return 0;
}
"""

FAMILIES = {"attn_kernel": 1, "attn_kernel_pp": 2}   # BD_ATTN_FAMILY_*
KEY_LEN = 6


def parse_kernel(mangled: str):
    name, key = template_args(mangled, r"attn_kernel(?:_pp)?")
    return [FAMILIES[name], *key, *[0] * (KEY_LEN - len(key))]


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    rev = sh(["git", "-C", ROOT, "rev-parse", sys.argv[1]]).strip()
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "attention_forms.json")
    groups_in = [(s, "ok", lats) for s, lats in shapes()] + [(s, "out_8", [0]) for s, _ in shapes()[:4]] + [(s, p, [0]) for s, p in pointer_cases()]
    lines = []
    for shape, ptrs, lats in groups_in:
        f = {**DEFAULTS, **shape}
        for prec in PRECS:
            for lat in lats:
                lines.append(" ".join(str(x) for x in [*(f[n] for n in FIELDS), prec, lat, *POINTERS[ptrs]]))
    with tempfile.TemporaryDirectory() as tmp:
        csrc = extract(rev, tmp, FILES)
        exe = build_host_only(tmp, [os.path.join(csrc, "attention.hip")], PRELUDE, DRIVER)
        res = sh([exe], input="\n".join(lines) + "\n").splitlines()
        names = kernel_names(exe, "attn_kernel")
    assert len(res) == len(lines), (len(res), len(lines))
    kernels, outcomes, groups = {}, {}, []
    it = iter(res)
    for shape, ptrs, lats in groups_in:
        idx = []
        for _ in range(len(PRECS) * len(lats)):
            parts = next(it).split("|")
            rc = int(parts[-1][3:])
            assert rc != -99, "no entry point was called"
            if rc < 0:
                assert len(parts) == 1, "a refused call launched something"
                oc = rc
            else:                                    # (0, or the no-device error of hipGetLastError)
                assert len(parts) == 2, "an accepted call makes one launch"
                addr, *nums = parts[0].split(";")
                oc = [kernels.setdefault(json.dumps(parse_kernel(names[addr])), len(kernels)), *(int(x) for x in nums)]
            idx.append(outcomes.setdefault(json.dumps(oc), len(outcomes)))
        groups.append([shape, ptrs, lats, idx])
    doc = {"revision": rev, "cases": len(lines), "fields": FIELDS, "defaults": DEFAULTS, "pointers": POINTERS, "precs": PRECS,
           "kernels": [json.loads(k) for k in kernels], "outcomes": [json.loads(k) for k in outcomes], "groups": groups}
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")
    print(f"{out_path}: {len(lines)} cases, {len(outcomes)} outcomes, {len(kernels)} kernels, {os.path.getsize(out_path)} bytes, revision {rev[:12]}")


if __name__ == "__main__":
    main()
