"""Every row of the GEMM instance tables launches the kernel its key names.

tests/test_gemm_plan_host.py holds bd_gemm_plan against the recorded dispatch on the CPU; what it cannot see is whether the kernel pointer
of a table row is the instance of the row's key.  Here every row (bd_gemm_instance) is launched once: the host searches the smallest launch
whose plan names the row -- an epilogue recipe, N in {192, 576 (the fused q/k RMSNorm: 3 x 2 heads x 96), 768} (wider only where no such N
reaches the row), K = 192 (six slabs: one period of a three-stage ring) or 128 (two-stage), 768 for the LayerNorm-fold consumer, 2112
(2176 for e4m3) where the form needs deep K, and the fewest rows M = 128 j + 44 (a ragged last tile); split-K rows: M = 300 with a forced
factor -- asserts on the launch's very arguments that the plan names the row, and compares the result with the fp64 product of the
decoded operands.  Rows that differ in output kind, GELU or epilogue write different bytes, so a wrong pointer cannot pass.
Tolerances: tests/test_gpu_gemm_kloop.py for F16C8 (2e-5 sqrt(K) on fp32 rows), tests/test_gpu_gemm_views.py otherwise."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from boxdreamer_amd import _lib, hip_ops
from test_gpu_gemm_views import (EPS, _Problem, _gemm, _out_cls, _randn, _rms_ref, _rms_w, _tol_16, _tol_f32, _tol_rms, _value, blank, lift,
                                 place, untouched)

pytestmark = pytest.mark.gpu

PC, GLDS, C8 = _lib.GEMM_FAMILY_PC, _lib.GEMM_FAMILY_GLDS, _lib.GEMM_FAMILY_PC_F16C8
ROWS = {PC: 39, GLDS: 28, C8: 50}                    # (tests/test_gemm_plan_host.py: the tables list every kernel once)
CLASSES = {(0, 1): "bf16", (1, 1): "fp16", (0, 2): "bf16x3", (1, 2): "f16x3", (2, 1): "fp8"}       # (T, NS) of a key -> prec
# EP 3 without the operand ring outside the one-plane 16-bit classes: instantiated, never selected (test_every_table_row_is_reached)
UNREACHABLE = {(PC, tc, ns, bk, 4, 2, 2, 3, 4, 3, 1, 0, 0, 0) for tc, ns, bk in ((0, 2, 32), (1, 2, 32), (2, 1, 128))}
# epilogue recipes: name -> fields of the launch beyond A, W, bias, out (a pointer: True)
RECIPES = {
    "operand": {}, "gelu": {"act": 1}, "f32": {"out_f32": 1}, "f32_resid": {"out_f32": 1, "resid": True}, "gelu_f32": {"out_f32": 1, "act": 1},
    "f16": {"out_f32": 2}, "bf16": {"out_f32": 3}, "bf16x2": {"out_f32": 4},
    "rms": {"rms_wq": True, "rms_wk": True}, "rms_f16": {"rms_wq": True, "rms_wk": True, "out_f32": 2},
    "rms_bf16": {"rms_wq": True, "rms_wk": True, "out_f32": 3}, "rms_bf16x2": {"rms_wq": True, "rms_wk": True, "out_f32": 4},
    "narrow_f32": {"out_f32": 1, "ldo_pad": 4},      # ldo % 8 != 0: no 16-byte epilogue, so no persistent kernel in gemm.hip
    "emit": {"out_f32": 1, "resid": True, "ln_stats_out": True, "ln_op_out": True},
    "emit_op": {"out_f32": 0, "ln_stats_out": True, "ln_op_out": True, "ln_resid_in_op": 1},
    "emit_op_f32": {"out_f32": 1, "ln_stats_out": True, "ln_op_out": True, "ln_resid_in_op": 1},
    "fold_gelu": {"act": 1, "ln_stats_in": True, "ln_colsum": True}, "fold_f16": {"out_f32": 2, "ln_stats_in": True, "ln_colsum": True},
    "fold_bf16x2": {"out_f32": 4, "ln_stats_in": True, "ln_colsum": True},
    "fold_rms_f16": {"out_f32": 2, "rms_wq": True, "rms_wk": True, "ln_stats_in": True, "ln_colsum": True},
    "fold_rms": {"rms_wq": True, "rms_wk": True, "ln_stats_in": True, "ln_colsum": True},
}
SPLIT = ("f32_resid", "emit", "emit_op", "emit_op_f32")


def _key(lib, family, index):
    key = (C.c_int * _lib.GEMM_KEY_LEN)()
    assert lib.bd_gemm_instance(family, index, key), (family, index)
    return tuple(key)


def _args(prec, rec, M, N, K, split=0):
    f = dict(RECIPES[rec])
    pad = f.pop("ldo_pad", 32)
    if prec == "fp8":
        f["wscale"] = True
    if split:
        f.update(sk_ws=True, sk_split=split)
    g = hip_ops.gemm_shape_args(M, N, K, **f)
    g.lda = g.ldw = K + 32                              # the arenas of _Problem.A / W and of the output below
    g.ldo = g.ldr = g.ln_op_ld = N + pad
    return g


@functools.lru_cache(maxsize=None)
def _candidates(prec):
    """launches to try, cheapest first: (recipe, N, K, split, args with every field but M set), M"""
    deep = 2176 if prec == "fp8" else 2112
    rows = [128 * j + 44 for j in list(range(64)) + list(range(64, 520, 8))]
    shapes = [(rec, N, K, 0) for N in (192, 576, 768, 1024, 1536, 2048) for K in (192, 128, 768, deep) for rec in RECIPES
              if K % (128 if prec == "fp8" else 64) == 0]
    cands = [(c, _args(prec, c[0], 44, c[1], c[2]), M) for c in shapes for M in rows]
    cands += [((rec, 768, K, s), _args(prec, rec, 300, 768, K, s), 300) for rec in SPLIT for K in (192, 768) for s in (2, 3, 4)]
    return sorted(cands, key=lambda c: (c[0][1] > 768, c[2] * c[0][1] * c[0][2], c[0]))


@functools.lru_cache(maxsize=None)
def _find(family, key):
    """(prec, recipe, N, K, M, split) of the smallest launch whose plan on this device names the row, or None"""
    lib = _lib.load()
    plan = _lib.GemmPlan()
    prec = "f16c8" if family == C8 else CLASSES[key[0], key[1]]
    pid = _lib.prec_id(prec)
    for (rec, N, K, split), g, M in _candidates(prec):
        g.M = M
        if lib.bd_gemm_plan(C.byref(g), pid, 0, 1, C.byref(plan)) == 0 and any(
                l.family == family and tuple(l.key) == key for l in plan.launch[:plan.n_launches]):
            return prec, rec, N, K, M, split
    return None


def _fold_stats(M):
    """row statistics of a LayerNorm-fold consumer (tests/test_gpu_gemm_kloop.py): eight equal (mean, M2) pairs per row"""
    mean = ((torch.arange(M, dtype=torch.float32) % 11) - 5) * 0.0625
    var = 1.0 + (torch.arange(M, dtype=torch.float32) % 9) * 0.25
    st = torch.stack([mean, var * 96.0], -1)[:, None, :].expand(M, 8, 2).contiguous().cuda()
    return st, mean.cuda().double(), var.cuda().double()


@pytest.mark.parametrize("family,index", [(f, i) for f in (PC, GLDS, C8) for i in range(ROWS[f])])
def test_table_row_launches_the_kernel_of_its_key(hip, family, index):
    lib = _lib.load()
    key = _key(lib, family, index)
    found = _find(family, key)
    if (family, *key) in UNREACHABLE:
        assert found is None, "a row listed as unreachable is reached: give it a launch"
        return
    assert found is not None, f"no launch reaches row {index} of family {family}: {key}"
    prec, rec, N, K, M, split = found
    f = RECIPES[rec]
    kind, act, eps = f.get("out_f32", 0), f.get("act", 0), 1e-6
    cls = _out_cls(prec, kind)
    P = _Problem(prec, M, N, K, w_std=0.03)
    A, W = P.A(True), P.W(True)
    ldo = N + f.get("ldo_pad", 32)
    res = _randn((M, N), 1.0, 31) if (f.get("resid") or f.get("ln_resid_in_op")) else None
    rms = (*_rms_w(), 3) if f.get("rms_wq") else None
    kw, ref = {}, P.lin
    if f.get("ln_stats_in"):                                  # consumer: rstd (acc - mean s) + b
        st, mean, var = _fold_stats(M)
        s = _randn((N,), 0.2, 33)
        rstd = torch.rsqrt(var + eps)[:, None]
        ref = rstd * P.acc - (mean[:, None] * rstd) * s.double() + P.b.double()
        kw["ln_apply"] = (st, s, eps)
    if act:
        ref = F.gelu(ref)
    if rms:
        ref = _rms_ref(ref, 3, rms[0], rms[1])
    op = stats = None
    if f.get("ln_stats_out"):                                 # producer: the rows' operand copy and statistics next to / instead of fp32 rows
        r5 = bool(f.get("ln_resid_in_op"))
        x0 = hip_ops.f16c8_encode(res, 0, False) if r5 else blank("f16c8", M, N, "cuda")
        if r5:
            res = hip_ops.from_operand(x0, "f16c8").float()
        op = place(x0, "f16c8", ldo, poison="out")
        stats = torch.full((M, 8, 2), float("nan"), dtype=torch.float32, device="cuda")
        kw.update(ln_emit=(stats, op), resid_in_op=r5)
    if res is not None:
        ref = ref + res.double()
    in_place = bool(f.get("resid"))
    out = place(res if in_place else blank(cls, M, N, "cuda"), cls, ldo, poison="out")
    ws = hip_ops.splitk_workspace(M, N) if split else None

    def names_the_row(g):                                     # on the arguments bd_gemm is about to get
        launches = hip_ops.gemm_plan(g, prec)
        assert any(l["family"] == hip_ops._FAMILY[family] and tuple(l["key"]) == key for l in launches), (key, launches)
        if split:
            assert launches[0]["split_k"] == split

    _gemm(prec, A, W, out, M, N, K, kind, bias=P.b, wscale=P.ws, resid=out if in_place else None, act=act, w_qexp=P.e, rms=rms,
          split_k=(ws, split) if split else None, edit=names_the_row, **kw)
    torch.cuda.synchronize()
    for name, ar in (("A", A), ("W", W), ("out", out), ("operand copy", op)):
        if ar is not None:
            untouched(ar, name)
    m = max(1.0, ref.abs().max().item())
    if op is not None and kind == 0:                          # EP 5 without fp32 rows: the copy is the result, `out` is ignored
        assert torch.equal(out.buf, out.pristine)
        val, bound = _value(lift(op), "f16c8"), 2e-5 * K ** 0.5 + 1e-5 + 2.0 ** -15 * m
    else:
        val = _value(lift(out), cls)
        g113 = 1.13 if act else 1.0                           # |GELU'| <= 1.13
        if prec == "f16c8":
            # fp32 rows: test_gpu_gemm_kloop (+ 1e-6 on a residual); 16-bit kinds: test_f16c8_operand_class_outputs, test_f16c8_v_columns_..;
            # with the fused q/k RMSNorm test_gemm_fused_qk_rmsnorm's 2 eps m + 1e-4; with the fold test_consumer_f16c8_applies_row_statistics
            fold = bool(f.get("ln_stats_in"))
            e16 = {"f16c8": 2.0 ** -15, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "bf16x3": 2.0 ** -15, "f16x3": 2.0 ** -20}.get(cls)
            if cls == "f32":
                bound = 2e-5 * K ** 0.5 * g113 + (1e-6 if res is not None or act else 0.0)
            elif cls == "fp16":
                bound = 2.0 ** -10 * m + (2e-4 if fold else (1e-4 if rms else 0.0))
            elif rms:
                bound = _tol_rms(e16)(m)
            else:
                bound = (4e-4 * m * 2.0 ** -4 + 2e-5) if cls == "f16c8" else (2.0 ** -14 * m + 2e-4 if fold else e16 * m + 2e-5 * K ** 0.5)
        elif kind == 1:
            bound = ((4e-4 if prec == "bf16x3" else 2e-4) * K ** 0.5 if res is not None else _tol_f32(prec, K)(m)) * g113
        else:
            e16 = EPS[prec] if kind == 0 else {2: 2.0 ** -11, 3: 2.0 ** -8, 4: 2.0 ** -15}[kind]
            bound = (_tol_rms(e16) if rms else _tol_16(prec, K, e16))(m)
    assert bool(torch.isfinite(val).all())
    err = (val - ref).abs().max().item()
    print(f"[forms] family {family} row {index} {key}: {prec} {rec} {M}x{N}x{K} split {split}: err {err:.3e} bound {bound:.3e}")
    assert err < bound, (key, found, err, bound)
    if stats is not None and kind == 1:                       # the statistics of the fp32 rows (tests/test_gpu_lnfold.py)
        xg = lift(out).double().reshape(M, 8, 96)
        mean = xg.mean(-1)
        m2 = ((xg - mean[..., None]) ** 2).sum(-1)
        assert (stats[..., 0].double() - mean).abs().max().item() <= 2e-6 * float(xg.abs().max())
        assert ((stats[..., 1].double() - m2).abs() / m2.clamp_min(1e-3)).max().item() <= 2e-5
