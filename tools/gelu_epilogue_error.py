"""Measured error of the three GELU forms of the GEMM epilogues (csrc/bd_common.h: gelu_erf2, gelu_fast, gelu_poly2) against fp64
0.5 x erfc(-x / sqrt 2), per decade of |x| and sign, far beyond the forms' clamps.  Prints the Markdown of profiles/gelu_epilogue_error.md.

    python tools/gelu_epilogue_error.py > profiles/gelu_epilogue_error.md

The pre-activation is exact: bd_gemm with an all-zero A operand and bias = the sweep (as tests/test_gpu_range.py does).  The erf form is
read as fp32; the fitted forms exist only in front of a 16/8-bit store, so their rows show the stored value's error and, next to it, what
is left after half a unit in the last place of the stored class is taken off."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from boxdreamer_amd import hip_ops, operand  # noqa: E402

DECADES = [(-3, -2), (-2, -1), (-1, 0), (0, 1), (1, 2), (2, 3), (3, 4)]
PER = 512
# form -> (operand class, fp32 output, relative half unit of the stored class, half its subnormal quantum)
FORMS = {"gelu_erf2 (fp32 result)": ("bf16x3", True, 0.0, 0.0), "gelu_fast (fp16 result)": ("fp16", False, 2.0 ** -11, 2.0 ** -25),
         "gelu_poly2 (bf16 result)": ("bf16", False, 2.0 ** -8, 0.0), "gelu_poly2 (e4m3 result)": ("fp8", False, 2.0 ** -4, 2.0 ** -10)}


def main():
    mags = np.concatenate([np.logspace(a, b, PER, endpoint=(b == 4)) for a, b in DECADES])
    x = np.concatenate([mags, -mags]).astype(np.float32)
    n = -(-len(x) // 192) * 192
    x = torch.from_numpy(np.concatenate([x, np.zeros(n - len(x), dtype=np.float32)]))
    xd = x.double()
    ref = 0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))
    print("# GELU epilogue forms: measured error against fp64\n")
    print("Command: `python tools/gelu_epilogue_error.py` on one MI355X.  Reference: `0.5 x erfc(-x / sqrt 2)` in fp64; 512 log-spaced points per")
    print("decade of |x| and sign; the pre-activation is exact (all-zero A operand, bias = the sweep).  `abs` / `rel`: largest absolute / relative")
    print("error of the stored value; `abs - u`: the largest absolute error left after half a unit in the last place of the stored class")
    print("(relative half unit, at least half its subnormal quantum; e4m3 results saturate at 448: compared with the saturated reference).\n")
    for form, (prec, f32, eps, floor) in FORMS.items():
        K = 128 if prec == "fp8" else 64
        a = operand.empty(prec, 192, K, "cuda", zero=True)
        w = hip_ops.to_operand(torch.randn(n, K, device="cuda") * 0.05, prec)
        out = hip_ops.gemm(a, w, x.cuda(), prec=prec, act=1, out_f32=f32)
        torch.cuda.synchronize()
        got = out[0].float().double().cpu()
        want = ref.clamp(-448.0, 448.0) if prec == "fp8" else ref
        err = (got - want).abs()
        left = (err - torch.clamp(eps * want.abs(), min=floor)).clamp_min(0.0)
        print(f"## {form}\n")
        print("| x | abs | rel | abs - u |")
        print("|---|---|---|---|")
        for sign in (1.0, -1.0):
            for lo, hi in DECADES:
                m = (xd * sign >= 10.0 ** lo) & ((xd * sign < 10.0 ** hi) | ((hi == 4) & (xd * sign <= 10.0 ** hi)))
                rel = (err[m] / want[m].abs().clamp_min(1e-300)).max().item() if bool((want[m] != 0).all()) else float("nan")
                name = f"{'-' if sign < 0 else ''}[1e{lo}, 1e{hi})"
                print(f"| {name} | {err[m].max().item():.3e} | {rel:.3e} | {left[m].max().item():.3e} |")
        print()


if __name__ == "__main__":
    main()
