"""GPU: the RANGE contract (csrc/bd_common.h, above bd_saturating_conversions) at every kernel that stores a 16/8-bit operand.

    f32 -> f16 stores clamp to +-65504, the e4m3 images to +-448, every store rounds to nearest even, and an F16C8 operand is
    hi = f16(x), lo8 = e4m3(clamp((x - hi) 2^11, +-448)).

None of it is plain C++: it rests on MODE.FP16_OVFL, which every kernel sets for itself, and on the fence that makes hi and lo round the
same fp32 number.  Here every producer gets launches in which the fp32 value in front of the store is KNOWN exactly (an all-zero A
operand and bias = a table of steered values; gamma = 0 and beta = the table; a copy), and the stored planes are compared bit for bit
with the reference packer hip_ops.to_operand, which tests/test_operand_host.py pins against an integer restatement of the rounding on
the same tables.  Producers that compute (RMSNorm, attention, im2col) are compared with the packer on their fp64 result, bit for bit away
from rounding boundaries.  The GELU epilogues are checked element by element against fp64 over a sweep far beyond their clamps.
Nothing here falls back to PyTorch compute."""
import functools
import math

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, operand, synth
from test_gpu_gemm_views import _CLS, _gemm, _needs_256_cus, _out_cls, _plane_bytes, blank, lift, place, untouched
from test_gpu_ops import _PREFIX_VARIANTS                     # name -> (input class, attention code, how to read the result)
from test_operand_host import BASE_FORMAT, FORMATS, RANGE_CLASSES, steered_count, steered_table

pytestmark = pytest.mark.gpu

LIN = ["bf16", "fp16", "bf16x3", "f16x3", "fp8"]            # the classes of gemm.hip (F16C8 has its own launcher, gemm_f16c8.hip)
MODES = (0, 1, 2, 3, 4, 5)                                  # bd_gemm_args.out_f32: operand class, fp32, f16, bf16, split-bf16, split-f16
# half a unit in the last place of a stored class, relative (tests/test_gpu_ops.py: EPS; e4m3 and F16C8 as in tests/test_gpu_gemm_views.py)
# and its floor, half the class's subnormal quantum (F16C8: lo8's quantum is 2^-9 2^-11)
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -15, "f16x3": 2.0 ** -20, "fp8": 2.0 ** -4, "f16c8": 2.0 ** -15, "f32": 0.0}
HALF_QUANTUM = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25, "bf16x3": 2.0 ** -134, "f16x3": 2.0 ** -25, "fp8": 2.0 ** -10, "f16c8": 2.0 ** -21, "f32": 0.0}
CLASS_MAX = {"bf16": FORMATS["bf16"][2], "bf16x3": FORMATS["bf16"][2], "fp16": 65504.0, "f16x3": 65504.0, "f16c8": 65504.0, "fp8": 448.0,
             "f32": float(np.finfo(np.float32).max)}


# ------------------------------------------------------------------------------------------------------------------ helpers
class _Flat:
    """a contiguous operand tensor with the fields tests/test_gpu_gemm_views.py::_gemm reads from an arena"""

    def __init__(self, t, cls):
        self.t, self.cls, self.ptr, self.ld = t, cls, t.data_ptr(), t.shape[-1]
        self.plane = t[0].numel() if t.dim() == 3 else 0


def _randn(shape, std=1.0, seed=3):
    return torch.from_numpy(synth.bell_np("range", shape, std, 0.0, seed).astype(np.float32)).cuda()


@functools.lru_cache(maxsize=2)
def _zero_a(prec, M, K):
    """an all-zero A operand: every plane of every class is zero bytes, so the accumulators are exactly 0"""
    return _Flat(operand.empty(prec, M, K, "cuda", zero=True), prec)


@functools.lru_cache(maxsize=4)
def _weights(prec, N, K):
    w = _randn((N, K), 0.05, seed=5)
    if prec == "f16c8":
        e = hip_ops.f16c8_qexp(w)
        return _Flat(hip_ops.f16c8_encode(w, e, True), "f16c8_w"), e
    return _Flat(hip_ops.to_operand(w, prec), prec), 0


def _misaligned(v):
    """the same fp32 vector at an address 4 bytes off a 16-byte boundary: no kernel form with the wide (16-byte) epilogue takes it"""
    buf = torch.zeros(v.numel() + 4, dtype=torch.float32, device="cuda")
    off = 1 if buf.data_ptr() % 16 == 0 else (16 - buf.data_ptr() % 16) // 4 + 1
    buf[off:off + v.numel()] = v
    out = buf[off:off + v.numel()]
    assert out.data_ptr() % 16 == 4
    return out


def _expect(pre, cls):
    """the planes (as [rows, bytes]) the packer gives for the fp32 rows `pre` in output class `cls`"""
    if cls == "f32":
        return [pre.contiguous().view(torch.uint8).reshape(pre.shape[0], -1)]
    t = hip_ops.to_operand(pre, cls)
    for p in ([t] if len(_CLS[cls][1]) == 1 else [t[0]]):
        assert torch.isfinite(p.float()).all()
    return [_plane_bytes(t, cls, p) for p in range(len(_CLS[cls][1]))]


def _planes(t, cls):
    return [_plane_bytes(t, cls, p) for p in range(len(_CLS[cls][1]))]


def _where(a, b):
    bad = (a != b).nonzero()
    return f"{bad.shape[0]} bytes differ, the first at (row, byte) {tuple(bad[0].tolist())}"


def _launch(prec, M, N, K, mode, *, bias, act=0, out_rows=None, **kw):
    """bd_gemm with an all-zero A operand into an output arena (leading dimension N + 32, guard rows, planes further apart than rows x ld):
    returns the payload as a contiguous tensor and its class, after checking that nothing outside the payload changed."""
    W, e = _weights(prec, N, K)
    cls = _out_cls(prec, mode)
    out = place(blank(cls, out_rows or M, N, "cuda"), cls, N + 32, poison="out")
    _gemm(prec, _zero_a(prec, M, K), W, out, M, N, K, mode, bias=bias, act=act, w_qexp=e, **kw)
    torch.cuda.synchronize()
    untouched(out, f"output of {prec} mode {mode} {M} x {N} x {K}")
    return lift(out), cls


def _check_bias_only(prec, M, N, K, modes, *, aligned=True, cols=None, **kw):
    """bias = the steered table of the OUTPUT class: every row has the bits of row 0 (compared on the device), row 0 has the packer's bits.
    cols: the column range that carries the table (the v third of a fused q/k RMSNorm launch)."""
    for mode in modes:
        cls = _out_cls(prec, mode)
        c0, c1 = cols or (0, N)
        bias = _randn((N,), 0.3, seed=9)
        bias[c0:c1] = steered_table(cls if cls != "f32" else prec, c1 - c0).cuda()
        got, _ = _launch(prec, M, N, K, mode, bias=bias if aligned else _misaligned(bias), **kw)
        pre = (torch.zeros(1, c1 - c0) + bias[c0:c1].cpu()[None, :])             # 0 * wscale + b, as the kernel adds it (-0 becomes +0)
        bpe = [b for b in _CLS[cls][1]]
        for p, (g, w) in enumerate(zip(_planes(got, cls), _expect(pre, cls))):
            # (a column range that starts and ends on 32-element blocks: F16C8's lo8 bytes are permuted inside a block only)
            g = g[:, c0 * bpe[p]:c1 * bpe[p]]
            assert torch.equal(g, g[:1].expand_as(g)), f"{prec} mode {mode} plane {p}: a row differs from row 0 ({_where(g, g[:1].expand_as(g))})"
            g0 = g[0].cpu()
            assert torch.equal(g0, w[0]), f"{prec} mode {mode} plane {p}: row 0 differs from to_operand ({_where(g0[None], w[:1])}; table of {cls})"


# ------------------------------------------------------------------------------------------------------------------ part 2: GEMM epilogues
# The one-tile kernels of gemm.hip (gemm_kernel_glds) on 256 CUs.  name -> (M, N, K, aligned bias, modes, the form hip_ops.gemm_plan must
# name: asserted in front of every launch).  K = 64 (one slab; 128 for e4m3) except where K >= 2048 selects the form.
def _glds(tm, tn, stages=2, **kw):
    return {"family": "glds", "tile": (tm, tn), "stages": stages, **kw}


GLDS = {
    # 12 tiles of 128 x 128 beat 36 of 64 x 64 and fit the CUs at once: the four-stage ring; wide epilogue
    "128x128_ring4": (192, 768, 64, True, MODES, _glds(128, 128, 4)),
    # 24 tiles of 64 x 64 beat 6 of 128 x 128 and fit the slots at once
    "64x64_ring4": (128, 768, 64, True, MODES, _glds(64, 64, 4)),
    # 576 tiles of 64 x 64: more than the slots; 48 tiles of 256 x 192 fill too little of a round for the persistent kernel
    "64x64": (3072, 768, 64, True, MODES, _glds(64, 64)),
    # 288 tiles of 128 x 128: more than the CUs, better than 64 x 64; 96 tiles of 256 x 192: still no persistent kernel
    "128x128": (6144, 768, 64, True, MODES, _glds(128, 128)),
    # N >= 1536 and 256 tiles = one whole round; N % 192 != 0 keeps the persistent kernel out
    "256x256": (8192, 2048, 64, True, MODES, _glds(256, 256)),
    # hybrid row split (N % 256 == 0, N < 1536, K >= 2048): 256 x 256 tiles on 32768 rows, 128 x 128 on the last 128
    "hybrid": (32896, 512, 2048, True, (0, 1), [_glds(256, 256, rows=32768), _glds(128, 128, row0=32768, rows=128)]),
    # the scalar epilogue gemm_epilogue (operand class / fp32 only): bias 4 bytes off a 16-byte boundary, 128 x 128 ring form
    "narrow_128x128": (192, 768, 64, False, (0, 1), _glds(128, 128, 4)),
    # 256 x 192 one-tile form (one-plane classes, K >= 2048); reachable only where the persistent kernel is not, i.e. with the scalar
    # epilogue; the two-plane classes take 128 x 128 tiles here
    "narrow_256x192": (16384, 768, 2048, False, (0, 1), _glds(256, 192)),
}


@pytest.mark.parametrize("form", sorted(GLDS))
@pytest.mark.parametrize("prec", LIN)
def test_gemm_one_tile_stores_the_table_bit_for_bit(hip, prec, form):
    _needs_256_cus()
    M, N, K, aligned, modes, want = GLDS[form]
    if prec == "fp8":
        K = max(K, 128)
        if not aligned:
            modes = (1,)                                    # e4m3 results exist only in the wide epilogue (bd_gemm: needs_wide)
    if form == "narrow_256x192" and prec in ("bf16x3", "f16x3"):
        want = _glds(128, 128)
    _check_bias_only(prec, M, N, K, modes, aligned=aligned, form=want)


def _rms():
    return (_randn((96,), 0.1, seed=21) + 1).contiguous(), (_randn((96,), 0.1, seed=22) + 1).contiguous(), 0


# The persistent 256 x 192 kernel (gemm_kernel_pc).  M = 7424: 29 x 4 = 116 tiles fill 0.453 >= 0.45 of a round of 256 CUs.
#   mode 0 -> pc_epilogue EP 1 (the one-plane 16-bit classes: the paired-row store), mode 1 -> EP 3, the class's non-native kinds (f16 from
#   the split classes, bf16 from e4m3, split-bf16 from split-f16) -> EP 1 with store8; every other mode -> EP 0 = gemm_epilogue_lds<.., LEAN>.
# "rms": the fused q/k RMSNorm geometry pins this kernel at any M: EP 2 or, for the other kinds, the LEAN generic epilogue's rms branch;
#   the v third of the columns is stored untouched and carries the table.
_PC_KINDS = {"bf16": (0,), "fp16": (0,), "bf16x3": (0, 2), "f16x3": (0, 2, 4), "fp8": (0, 3)}       # 16-bit kinds with an EP 1 / EP 2 instance


def _pc_form(prec, mode, rms):
    ep = 3 if mode == 1 and not rms else ((2 if rms else 1) if mode in _PC_KINDS[prec] else 0)
    return {"family": "pc", "tile": (256, 192), "ep": ep}


@pytest.mark.parametrize("form", ["plain", "rms"])
@pytest.mark.parametrize("prec", LIN)
def test_gemm_persistent_192_stores_the_table_bit_for_bit(hip, prec, form):
    _needs_256_cus()
    K = 128 if prec == "fp8" else 64
    for mode in (MODES if form == "plain" else (0, 2, 3, 4, 5)):
        if form == "plain":
            _check_bias_only(prec, 7424, 768, K, (mode,), form=_pc_form(prec, mode, False))
        else:
            _check_bias_only(prec, 300, 2304, K, (mode,), rms=_rms(), cols=(1536, 2304), form=_pc_form(prec, mode, True))


# gemm_kernel_pc_f16c8 on 256 CUs.  name -> (M, N, K, modes, tile, ring stages).  Where K >= 128, modes 0, 2, 4 take pc_epilogue EP 1, 1 EP 3,
# 3 and 5 the generic epilogue (EP 0); the form is asserted in front of every launch.
C8 = {
    # 4 x 33 = 132 large tiles: 2 x 132 > CUs -> the large form, three-stage ring (K / 32 = 6)
    "large": (8448, 768, 192, MODES, (256, 192), 3),
    # 2 x 4 = 8 tiles, 16 <= CUs -> the small form (128 x 192 tiles)
    "small": (300, 768, 192, MODES, (128, 192), 3),
    # the 128 x 96 form: fp32 results, small, K >= 2048 (K / 32 = 66, a multiple of 3), 4 x 8 <= CUs
    "128x96": (300, 768, 2112, (1,), (128, 96), 3),
    # K < 128: generic epilogue for every kind, two-stage ring (K / 32 = 2), small form
    "generic_small_2stage": (300, 768, 64, MODES, (128, 192), 2),
    # K < 128: generic epilogue, two-stage ring, large form (the three-stage generic forms are what kinds 3 and 5 of "small" and "large"
    # above take)
    "generic_large_2stage": (8448, 768, 64, MODES, (256, 192), 2),
}


def _c8_ep(mode, K):
    return 0 if K < 128 or mode in (3, 5) else (3 if mode == 1 else 1)


@pytest.mark.parametrize("form", sorted(C8))
def test_gemm_f16c8_stores_the_table_bit_for_bit(hip, form):
    _needs_256_cus()
    M, N, K, modes, tile, stages = C8[form]
    for mode in modes:
        _check_bias_only("f16c8", M, N, K, (mode,), form={"tile": tile, "stages": stages, "ep": _c8_ep(mode, K)})


@pytest.mark.parametrize("M", [300, 8448])
def test_gemm_f16c8_fused_rms_keeps_the_v_columns(hip, M):
    """EP 2 of both forms: operand class, f16 plane, split-bf16 planes; the v third carries the table."""
    _needs_256_cus()
    _check_bias_only("f16c8", M, 2304, 192, (0, 2, 4), rms=_rms(), cols=(1536, 2304),
                     form={"tile": (128, 192) if M == 300 else (256, 192), "stages": 3, "ep": 2})


def _any_stats(M):
    """arbitrary finite (mean, M2) pairs per 96-column group: with column sums of zero they cancel out of rstd * acc - mean rstd s + b"""
    st = _randn((M, 8, 2), 1.0, seed=31)
    st[..., 1] = st[..., 1].abs() * 96 + 1.0
    return st.contiguous()


@pytest.mark.parametrize("kind", ["gemm_f16c8_operand_f16_bf16x2", "gemm_f16c8_rms_f16", "gemm_f16_rms"])
@pytest.mark.parametrize("M", [300, 8448])
def test_gemm_layernorm_fold_consumer_stores_the_table(hip, kind, M):
    """The consumer side of the LayerNorm fold (K = 768) with ln_colsum = 0: the value in front of the store is bias[n] exactly.
    F16C8: EP 1 with LNF (the GELU form is in the GELU sweep below), EP 2 with LNF, small and large forms.  f16: the q / k / v launch
    (persistent kernel, EP 2 with LNF)."""
    _needs_256_cus()
    N = 2304
    ln = (_any_stats(M), torch.zeros(N, device="cuda"), 1e-6)
    c8 = {"tile": (128, 192) if M == 300 else (256, 192), "stages": 3, "lnf": True}
    if kind == "gemm_f16c8_operand_f16_bf16x2":
        _check_bias_only("f16c8", M, 768, 768, (2, 4), ln_apply=(ln[0], torch.zeros(768, device="cuda"), 1e-6), form={**c8, "ep": 1})
    elif kind == "gemm_f16c8_rms_f16":
        _check_bias_only("f16c8", M, N, 768, (2,), rms=_rms(), ln_apply=ln, cols=(1536, 2304), form={**c8, "ep": 2})
    else:
        _check_bias_only("fp16", M, N, 768, (0,), rms=_rms(), ln_apply=ln, cols=(1536, 2304), form={"family": "pc", "tile": (256, 192), "ep": 2, "lnf": True})


# ---- the value split over two of bias / addtab / resid, different in every row, through the row map
def _per_row_case(cls, M, N, combo):
    """(bias, addtab, resid, pre): fp32 host tensors whose sum in the kernel's order, ((0 + bias) + addtab) + resid, is `pre` [M, N] exactly.
    Row r holds the table rotated by 7 r columns.  tab+resid: an exact split of every value (high and low mantissa halves).  With a
    per-column bias c the other addend is fp32(V - c) and the value in front of the store is what fp32 arithmetic makes of the sum; the
    steered value itself survives wherever c = 0 or the subtraction is exact."""
    table = steered_table(cls if cls != "f32" else "f16c8", N)
    idx = (torch.arange(N)[None, :] + 7 * torch.arange(M)[:, None]) % N
    V = table[idx].contiguous()
    if combo == "tab+resid":
        a = (V.view(torch.int32) & ~0xFFF).view(torch.float32)
        b = V - a
        assert torch.equal(a + b, V)
        return None, a, b, (0.0 + a) + b
    n = torch.arange(N)
    c = torch.where(n % 2 == 0, torch.zeros(N), 0.25 * ((n % 5).float() - 2.0))
    other = V - c[None, :]
    pre = (0.0 + c[None, :]) + other
    kept = (pre == V)[:, :steered_count(cls if cls != "f32" else "f16c8")].float().mean().item()
    assert kept >= 0.5, kept                               # the steered values themselves still reach the store in a large share of the rows
    return (c, other, None, pre) if combo == "bias+tab" else (c, None, other, pre)


# name -> (prec list, M, N, K, row map (rows per group in, out, offset), form): launches with a table / row map take the generic epilogue
# everywhere (EP 0 of the persistent kernels: gemm_epilogue_lds LEAN)
PER_ROW = {
    "glds_128x128_ring4": (LIN, 192, 768, 64, (64, 70, 3), _glds(128, 128, 4)),
    "glds_64x64_ring4": (LIN, 128, 768, 64, (32, 33, 1), _glds(64, 64, 4)),
    "persistent_192_generic": (LIN, 7424, 768, 64, (256, 261, 5), {"family": "pc", "tile": (256, 192), "ep": 0}),
    "f16c8_small_generic": (["f16c8"], 300, 768, 192, (50, 57, 2), {"tile": (128, 192), "stages": 3, "ep": 0}),
    "f16c8_large_generic": (["f16c8"], 8448, 768, 192, (256, 261, 5), {"tile": (256, 192), "stages": 3, "ep": 0}),
}


@pytest.mark.parametrize("combo", ["tab+resid", "bias+tab", "bias+resid"])
@pytest.mark.parametrize("form,prec", [(f, p) for f in sorted(PER_ROW) for p in PER_ROW[f][0]])
def test_gemm_per_row_values_through_table_residual_and_row_map(hip, prec, form, combo):
    _needs_256_cus()
    _, M, N, K, rpg, want = PER_ROW[form]
    if prec == "fp8":
        K = 128
    rows = torch.arange(M)
    orow = (rows // rpg[0]) * rpg[1] + rows % rpg[0] + rpg[2]
    out_rows = (M + rpg[0] - 1) // rpg[0] * rpg[1] + rpg[2]
    hole = torch.ones(out_rows, dtype=torch.bool)
    hole[orow] = False
    for mode in MODES:
        cls = _out_cls(prec, mode)
        bias, tab, res, pre = _per_row_case(cls, M, N, combo)
        kw = {}
        if tab is not None:
            kw["addtab"] = tab.cuda()
        if res is not None:                                 # the residual is read at the OUTPUT row
            full = torch.zeros(out_rows, N)
            full[orow] = res
            kw["resid"] = _Flat(full.cuda(), "f32")
        got, _ = _launch(prec, M, N, K, mode, bias=bias.cuda() if bias is not None else None, out_rows=out_rows, rpg=rpg, form=want, **kw)
        fill = blank(cls, out_rows, N, "cuda")
        for p, (g, w, f) in enumerate(zip(_planes(got, cls), _expect(pre, cls), _planes(fill, cls))):
            g, f = g.cpu(), f.cpu()
            assert torch.equal(g[orow], w), f"{prec} mode {mode} plane {p}: {_where(g[orow], w)}"
            assert torch.equal(g[hole], f[hole]), f"{prec} mode {mode} plane {p}: a row outside the map changed"


# ---- F16C8: the LayerNorm-fold producer, the 3-byte residual, split-K
C8_PRODUCER = {"small": (300, 192, (128, 192)), "large": (8448, 192, (256, 192)), "128x96": (300, 2112, (128, 96))}      # M, K, tile


def _producer(M, K, *, r5, f32, split=None, tile=None):
    """One producer launch with a zero accumulator.  r5: the residual is the F16C8 copy at ln_op_out (EP 5), else none (EP 4).
    Returns (fp32 rows or None, operand copy, statistics, pre)."""
    N = 768
    table = steered_table("f16c8", N)
    if r5:
        # residual values exact in f16 (lo8 = 0), zero in every ninth element of a row: there bias = the steered value reaches the store
        r = ((torch.arange(M)[:, None] + torch.arange(N)[None, :]) % 9 - 4).float() * 0.25
        pre = (0.0 + table[None, :]) + r
        op = place(hip_ops.f16c8_encode(r.cuda(), 0, False), "f16c8", N + 32, poison="out")
    else:
        pre = (0.0 + table[None, :]).expand(M, N).contiguous()
        op = place(blank("f16c8", M, N, "cuda"), "f16c8", N + 32, poison="out")
    W, e = _weights("f16c8", N, K)
    ocls = "f32" if f32 else "f16c8"
    out = place(blank(ocls, M, N, "cuda"), ocls, N + 32, poison="out")
    st = torch.full((M, 8, 2), float("nan"), dtype=torch.float32, device="cuda")
    kw = {}
    if split:
        kw["split_k"] = (hip_ops.splitk_workspace(M, N), split)
    form = {"ep": 5 if r5 else 4, "outk": int(f32), "split_k": split or 1, "tile": (128, 96) if split else tile}
    _gemm("f16c8", _zero_a("f16c8", M, K), W, out, M, N, K, int(f32), bias=table.cuda(), w_qexp=e, ln_emit=(st, op), resid_in_op=r5, form=form, **kw)
    torch.cuda.synchronize()
    untouched(out, "fp32 rows")
    untouched(op, "operand copy")
    if not f32:
        assert torch.equal(out.buf, out.pristine), "`out` is ignored when no fp32 rows are asked for"
    if split:
        assert int(kw["split_k"][0][:16384].view(torch.int32).abs().max()) == 0, "split-K flags must be left zero"
    return (lift(out) if f32 else None), lift(op), st, pre


def _check_producer(o32, opc, st, pre, what):
    if o32 is not None:
        assert torch.equal(o32.cpu(), pre), f"{what}: the fp32 rows are not the steered values"
    for p, (g, w) in enumerate(zip(_planes(opc, "f16c8"), _expect(pre, "f16c8"))):
        assert torch.equal(g.cpu(), w), f"{what}: plane {p} of the operand copy differs from f16c8_encode ({_where(g.cpu(), w)})"
    # (mean, M2) of a 96-column group must be finite wherever they are representable: a group that holds fp32's largest value has an M2
    # beyond fp32 in exact arithmetic
    g = pre.double().reshape(pre.shape[0], 8, 96)
    fits = ((g - g.mean(-1, keepdim=True)) ** 2).sum(-1) < 1e37
    assert fits.float().mean().item() >= 0.7 and torch.isfinite(st.cpu()[fits]).all(), f"{what}: row statistics"


@pytest.mark.parametrize("form", sorted(C8_PRODUCER))
@pytest.mark.parametrize("ep", ["4", "5", "5_f32"])
def test_gemm_f16c8_producer_copy_is_the_packing_of_the_table(hip, form, ep):
    """pc_epilogue EP 4 (fp32 rows + the operand copy at ln_op_out) and EP 5 (ln_resid_in_op) with out_f32 0 and 1, in the three kernel
    forms."""
    _needs_256_cus()
    M, K, tile = C8_PRODUCER[form]
    _check_producer(*_producer(M, K, r5=ep != "4", f32=ep != "5", tile=tile), f"EP {ep} {form}")


@pytest.mark.parametrize("split", [2, 3, 4])
@pytest.mark.parametrize("ep", ["3", "4", "5", "5_f32"])
def test_gemm_f16c8_split_k_of_a_zero_accumulator_is_bit_identical(hip, ep, split):
    """Split-K sums partial accumulators in a fixed order; all of them are zero here, so the stores must see the very
    same values as the unsplit launch."""
    M, K, N = 300, 192, 768               # (a forced factor: the form does not depend on the device)
    if ep == "3":
        ws = hip_ops.splitk_workspace(M, N)
        W, e = _weights("f16c8", N, K)
        table = steered_table("f16c8", N)
        out = place(blank("f32", M, N, "cuda"), "f32", N + 32, poison="out")
        _gemm("f16c8", _zero_a("f16c8", M, K), W, out, M, N, K, 1, bias=table.cuda(), w_qexp=e, split_k=(ws, split),
              form={"tile": (128, 96), "ep": 3, "split_k": split})
        torch.cuda.synchronize()
        untouched(out)
        assert torch.equal(lift(out).cpu(), (0.0 + table[None, :]).expand(M, N))
        assert int(ws[:16384].view(torch.int32).abs().max()) == 0
        return
    _check_producer(*_producer(M, K, r5=ep != "4", f32=ep != "5", split=split), f"EP {ep} split {split}")


# ------------------------------------------------------------------------------------------------------------------ part 3: GELU
def gelu_sweep():
    """fp32 [4224] (22 x 192 columns): 4097 points uniform on [-12, 12], +-{16, 32, 100, 300, 1000, 1e4}, +-0, +-1e-30, padded with a
    second, coarser pass over [-3, 3]"""
    big = [16.0, 32.0, 100.0, 300.0, 1000.0, 1e4]
    pts = np.concatenate([np.linspace(-12.0, 12.0, 4097), big, [-b for b in big], [0.0, -0.0, 1e-30, -1e-30]])
    pad = np.linspace(-3.0, 3.0, 4224 - len(pts))
    return torch.from_numpy(np.concatenate([pts, pad]).astype(np.float32))


def gelu_ref(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def half_unit(v, cls):
    """half a unit in the last place of class `cls` at the value v (fp64): EPS |v|, at least half the subnormal quantum; beyond 512 an
    F16C8 value is partially saturated (csrc/bd_common.h: RANGE) and keeps the f16 plane's half ulp"""
    v = v.abs()
    u = torch.clamp(EPS[cls] * v, min=HALF_QUANTUM[cls])
    if cls == "f16c8":
        u = torch.where(v >= 512.0, 2.0 ** -11 * v, u)
    return u


GELU_FORM = {"bf16": "poly", "fp8": "poly", "fp16": "fast"}          # csrc/bd_common.h: GeluKind; every other result takes the erf form
# form -> (|x| up to which its comment states a bound, the bound)
GELU_STATED = {"fast": (9.0, 5.4e-5), "poly": (4.0, 1.6e-4)}


def check_gelu(x, value, form, cls, what):
    """x: fp32 sweep (host), value: what the launch stored, as fp64 (host).  Asserts:
    erf form -- from the formula (A&S 7.1.26: 1.5e-7 on erfc = 0.75e-7 |x| on the result; ~ten fp32 operations with v_rcp / v_exp at 1 ulp):
        |err| <= 1e-7 |x| + 2^-20 |gelu(x)| + half a unit of the stored class;
    fitted forms -- inside the interval their comments name, the stated bound + half a unit; outside it only what every caller needs:
        x below: finite and |result| <= 2e-6 |x|;  x above: within 2e-6 |x| + half a unit of x (of the class's MAX where x saturates);
    both signs of zero give a zero."""
    xd = x.double()
    y = gelu_ref(x)
    assert torch.isfinite(value).all(), what
    err = (value - y).abs()
    zero = xd == 0
    assert (value[zero] == 0).all(), f"{what}: gelu(+-0) must be a zero"
    if form == "erf":
        sat = y.clamp(-CLASS_MAX[cls], CLASS_MAX[cls])
        err = (value - sat).abs()
        bound = 1e-7 * xd.abs() + 2.0 ** -20 * y.abs() + half_unit(sat, cls)
        bad = err > bound
        assert not bad.any(), f"{what}: {int(bad.sum())} points beyond the erf form's bound, worst x = {float(x[(err - bound).argmax()])!r}: err {float(err[(err - bound).argmax()]):.3e}"
        return
    lim, stated = GELU_STATED[form]
    inside = xd.abs() <= lim
    bound = stated + half_unit(y, cls)
    bad = inside & (err > bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} points inside [-{lim}, {lim}] beyond the stated {stated}: worst x = {float(x[(err - bound).where(inside, torch.tensor(-1.0, dtype=torch.float64)).argmax()])!r}"
    below, above = xd < -lim, xd > lim
    worst = (value.abs() / xd.abs().clamp_min(1.0))[below].max().item()
    assert worst <= 2e-6, f"{what}: |gelu(x)| / |x| reaches {worst:.3e} below -{lim} (a clamped Phi that is not 0)"
    xs = xd.clamp(-CLASS_MAX[cls], CLASS_MAX[cls])
    over = ((value - xs).abs() - half_unit(xs, cls)) / xd.abs().clamp_min(1.0)
    assert over[above].max().item() <= 2e-6, f"{what}: gelu(x) is {over[above].max().item():.3e} |x| + half a unit from x above {lim}"


def _value_of(t, cls):
    if cls == "f16c8":
        hi, lo, _ = hip_ops.f16c8_decode(t)
        return (hi.double() + lo.double()).cpu()
    return (t.double() if len(_CLS[cls][1]) == 1 else t[0].double() + t[1].double()).cpu()


# name -> (classes, M, K, aligned, mode -> GELU form or None for "the class's own", mode -> kernel form).  N = 4224 = 22 x 192 everywhere.
_C8S, _C8L = {"tile": (128, 192), "stages": 3}, {"tile": (256, 192), "stages": 3}
GELU_LAUNCHES = {
    # wide epilogue of the one-tile kernels: 16/8-bit results take gelu_n<GeluKind<T, NS>>, fp32 results gelu_erf
    "glds_wide": (LIN, 192, 64, True, {0: None, 1: "erf"}, {0: {"family": "glds"}, 1: {"family": "glds"}}),
    # scalar epilogue: gelu_erf for every result
    "glds_narrow": (["bf16", "fp16", "bf16x3", "f16x3"], 192, 64, False, {0: "erf", 1: "erf"}, {0: {"family": "glds"}, 1: {"family": "glds"}}),
    # persistent kernel EP 1 with GELU (paired-row store; store8 for the two-plane classes and e4m3); fp32 + GELU takes its generic epilogue
    "persistent_192": (LIN, 7424, 64, True, {0: None, 1: "erf"},
                       {0: {"family": "pc", "ep": 1, "gelu": True}, 1: {"family": "pc", "ep": 0}}),
    # EP 1 with GELU, small and large forms; kinds 1 and 5 with GELU take the generic epilogue
    "f16c8_small": (["f16c8"], 300, 192, True, {0: "erf", 1: "erf", 5: "erf"},
                    {0: {**_C8S, "ep": 1, "gelu": True}, 1: {**_C8S, "ep": 0}, 5: {**_C8S, "ep": 0}}),
    "f16c8_large": (["f16c8"], 8448, 192, True, {0: "erf"}, {0: {**_C8L, "ep": 1, "gelu": True}}),
    # K < 128, generic epilogue
    "f16c8_generic": (["f16c8"], 300, 64, True, {0: "erf"}, {0: {"tile": (128, 192), "stages": 2, "ep": 0}}),
}


@pytest.mark.parametrize("launch,prec", [(f, p) for f in sorted(GELU_LAUNCHES) for p in GELU_LAUNCHES[f][0]])
def test_gelu_epilogue_element_by_element(hip, launch, prec):
    _needs_256_cus()
    _, M, K, aligned, modes, kforms = GELU_LAUNCHES[launch]
    if prec == "fp8":
        K = 128
    x = gelu_sweep()
    N = x.numel()
    rows = {}
    for mode, form in modes.items():
        if prec == "fp8" and mode == 0 and not aligned:
            continue
        cls = _out_cls(prec, mode)
        form = form or GELU_FORM.get(prec, "erf")
        bias = x.cuda() if aligned else _misaligned(x.cuda())
        got, _ = _launch(prec, M, N, K, mode, bias=bias, act=1, form=kforms[mode])
        for g in _planes(got, cls):
            assert torch.equal(g, g[:1].expand_as(g)), f"{launch} {prec} mode {mode}: a row differs from row 0"
        row0 = got[:, :1].contiguous() if got.dim() == 3 else got[:1].contiguous()
        check_gelu(x, _value_of(row0, cls)[0], form, cls, f"{launch} {prec} mode {mode} ({form} form)")
        rows[mode] = (row0.cpu(), cls, form)
    # The erf form is the same arithmetic wherever it runs (gelu_erf2(x).x == gelu_erf(x.x), csrc/bd_common.h), and the rounding to the
    # stored class is a step of its own: a 16-bit erf-form result is the packing of the fp32 result of the same launch, bit for bit --
    # hi and lo of a two-plane class rounded against the same fp32 number (the fence in split_hi_lo / f16c8_split).
    for mode, (row0, cls, form) in rows.items():
        if mode != 1 and form == "erf" and 1 in rows:
            f32 = rows[1][0]
            live = f32 != 0                                 # (a -0 result becomes +0 in the fp32 rows: they leave through v + table + residual)
            for p, (g, w) in enumerate(zip(_elements(row0, cls), _elements(hip_ops.to_operand(f32, cls), cls))):
                bad = ((g != w) & live).nonzero()
                assert bad.numel() == 0, f"{launch} {prec} mode {mode} plane {p}: not the packing of the fp32 result at x = {x[bad[0, 1]].item()!r}"


@pytest.mark.parametrize("M", [300, 8448])
def test_gelu_f16c8_layernorm_fold_consumer(hip, M):
    """EP 1 with GELU and the LayerNorm fold's consumer side (K = 768), ln_colsum = 0, small and large form."""
    _needs_256_cus()
    x = gelu_sweep()
    N = x.numel()
    got, _ = _launch("f16c8", M, N, 768, 0, bias=x.cuda(), act=1, ln_apply=(_any_stats(M), torch.zeros(N, device="cuda"), 1e-6),
                     form={**(_C8S if M == 300 else _C8L), "ep": 1, "gelu": True, "lnf": True})
    for g in _planes(got, "f16c8"):
        assert torch.equal(g, g[:1].expand_as(g))
    check_gelu(x, _value_of(got[:, :1].contiguous(), "f16c8")[0], "erf", "f16c8", f"fold consumer + GELU, M = {M}")


# ------------------------------------------------------------------------------------------------------------------ part 4: bd_layernorm
@pytest.mark.parametrize("cols", [768, 96])
@pytest.mark.parametrize("prec", RANGE_CLASSES)
def test_layernorm_gamma_zero_stores_beta_bit_for_bit(hip, prec, cols):
    """gamma = 0: the normalised row drops out and the result is beta = the steered table (96 columns: its first two 96-column pieces,
    which hold every steered value).  3 rows, and 257 rows through the gather map.  The 16-bit planes are the packing of the fp32 copy,
    and the fp32 copy equals beta (a -0 in beta becomes +0: 0 * xhat + beta)."""
    table = steered_table(prec)
    for piece in range(1 if cols == 768 else 2):
        beta = table[piece * cols:(piece + 1) * cols].contiguous()
        x = (_randn((300, cols), 2.0, seed=41) + 0.3).contiguous()
        for rows, rpg in ((3, (0, 0, 0)), (257, (64, 70, 3))):
            o16, o32 = hip_ops.layernorm(x, torch.zeros(cols, device="cuda"), beta.cuda(), 1e-6, prec=prec, want32=True, rows=rows, rpg=rpg)
            torch.cuda.synchronize()
            o32 = o32.cpu()
            assert torch.equal(o32, beta[None, :].expand(rows, cols)), f"{prec}: the fp32 copy is not beta"
            for p, (g, w) in enumerate(zip(_planes(o16, prec), _expect(o32, prec))):
                assert torch.equal(g.cpu(), w), f"{prec} {cols} columns, {rows} rows, plane {p}: {_where(g.cpu(), w)}"


@pytest.mark.parametrize("cols", [768, 96])
@pytest.mark.parametrize("prec", RANGE_CLASSES)
def test_layernorm_large_gain_rounds_the_fp32_value_it_writes(hip, prec, cols):
    """gamma = 3000, beta = 0: results in the thousands (beyond e4m3's range and in F16C8's partially saturated band).  The fp32 copy is
    within the 2e-5 of tests/test_gpu_ops.py::test_layernorm (per unit of gain) of fp64 LayerNorm; the planes are finite, the packing of
    that fp32 copy bit for bit, and saturated where it exceeds the class's range."""
    x = (_randn((257, cols), 2.0, seed=43) + 0.3).contiguous()
    gamma = torch.full((cols,), 3000.0, device="cuda")
    o16, o32 = hip_ops.layernorm(x, gamma, torch.zeros(cols, device="cuda"), 1e-6, prec=prec, want32=True)
    torch.cuda.synchronize()
    o32 = o32.cpu()
    ref = torch.nn.functional.layer_norm(x.cpu().double(), (cols,), None, None, 1e-6) * 3000.0
    assert (o32.double() - ref).abs().max().item() <= 2e-5 * 3000.0
    for p, (g, w) in enumerate(zip(_planes(o16, prec), _expect(o32, prec))):
        assert torch.equal(g.cpu(), w), f"{prec} plane {p}: {_where(g.cpu(), w)}"
    hi = (o16[0] if o16.dim() == 3 else o16).float().cpu()
    over = o32.abs() > CLASS_MAX[prec]
    assert torch.isfinite(hi).all() and (hi[over].abs() == CLASS_MAX[prec]).all()
    assert over.any() == (prec == "fp8") and (o32.abs() > 512).any()


# ------------------------------------------------------------------------------------------------------------------ producers that compute
def _elements(t, cls):
    """the planes of an operand tensor as integer tensors [rows, cols], element i of every plane at position i (F16C8: lo8 un-permuted)"""
    if len(_CLS[cls][1]) == 1:
        return [t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16)]
    rows, cols = t.shape[-2:]
    if cls == "f16c8":
        inv = torch.empty(cols, dtype=torch.long, device=t.device)
        inv[hip_ops._f16c8_perm(cols, t.device)] = torch.arange(cols, device=t.device)
        lo8 = t[1].contiguous().view(torch.uint8).reshape(-1)[:rows * cols].reshape(rows, cols)[:, inv]
        return [t[0].contiguous().view(torch.int16), lo8]
    return [t[0].contiguous().view(torch.int16), t[1].contiguous().view(torch.int16)]


def _step_ulps(x, k):
    """fp32 tensor moved by k fp32 ulps in magnitude (k < 0: towards zero, never across it)"""
    bits = x.contiguous().view(torch.int32)
    mag = (bits & 0x7FFFFFFF) + k
    mag = mag.clamp(0, 0x7F7FFFFF)
    return (mag | (bits & -0x80000000)).view(torch.float32)


def check_near(ref64, got, cls, what, max_near=0.05):
    """A producer that COMPUTES its fp32 value (a few roundings away from the fp64 reference), against the packer: every element's planes
    must be the packing of ONE fp32 number within 2 fp32 ulps of the reference.  Away from the class's rounding boundaries all five
    candidates pack to the same bits, so this is bit equality; next to a boundary the neighbouring value is accepted, which is at most one
    unit of the class; where the reference exceeds the class's range every candidate is the saturated MAX.  The share of elements whose
    plane 0 lies next to a boundary must stay below max_near, so that the comparison IS bit equality nearly everywhere (a two-plane class's
    lo plane has a last place of a few fp32 ulps: its candidates differ on most elements, and each is still held to one of them).
    ref64: [rows, cols] fp64 (host); got: operand tensor of class cls (host)."""
    ref32 = ref64.float()
    planes = _elements(got, cls)
    ok = torch.zeros(ref32.shape, dtype=torch.bool)
    first, same0 = None, torch.ones(ref32.shape, dtype=torch.bool)
    for k in (0, -1, 1, -2, 2):
        cand = _elements(hip_ops.to_operand(_step_ulps(ref32, k), cls), cls)
        hit = torch.ones(ref32.shape, dtype=torch.bool)
        for g, c in zip(planes, cand):
            hit &= g == c
        ok |= hit
        if first is None:
            first = cand
        same0 &= cand[0] == first[0]
    hi = (got[0] if len(_CLS[cls][1]) == 2 else got).float()
    assert torch.isfinite(hi).all(), what
    bad = (~ok).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} elements are not the packing of any fp32 value within 2 ulps of the reference, the first at "
                              f"{tuple(bad[0].tolist())}: reference {ref64[tuple(bad[0].tolist())].item()!r}, plane 0 holds {hi[tuple(bad[0].tolist())].item()!r}")
    live = ref64 != 0
    near = (~same0 & live).float().sum().item() / max(1.0, live.float().sum().item())
    assert near < max_near, f"{what}: {near:.3f} of the elements lie next to a rounding boundary of plane 0"
    over = ref64.abs() > CLASS_MAX[cls] * (1 + 2.0 ** -20) + (0.5 * 2.0 ** (int(math.floor(math.log2(CLASS_MAX[cls]))) - FORMATS[BASE_FORMAT[cls]][0]))
    assert (hi[over].abs() == CLASS_MAX[cls]).all(), f"{what}: a result beyond the class's range is not the saturated MAX"
    return near, int(over.sum())


# ---- bd_qk_rmsnorm: norm.hip launch_rms -- heads == 8 and head_dim == 96 take qk_rmsnorm_row_kernel (one wave per row), everything else
# qk_rmsnorm_kernel (one thread per vector)
@pytest.mark.parametrize("hd,heads", [(96, 8), (96, 3), (64, 12)])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "bf16x3", "f16x3"])
def test_qk_rmsnorm_results_across_and_beyond_the_range(hip, prec, hd, heads):
    """One non-zero element per q / k head, weights from {1, 300, 1e5}: results w a / sqrt(a^2 / hd + eps) of about 8 w -- inside the
    range, beyond 448 and beyond 65504 -- against the packer on the fp64 result; v (the class's steered table) untouched bit for bit."""
    rows = 37
    rng = np.random.default_rng(1000 * hd + heads)
    x = torch.zeros(rows, 3, heads, hd)
    pos = torch.from_numpy(rng.integers(0, hd, (rows, 2, heads)))
    a = torch.from_numpy((rng.uniform(0.002, 4.0, (rows, 2, heads)) * rng.choice([-1.0, 1.0], (rows, 2, heads))).astype(np.float32))
    x[:, :2].scatter_(-1, pos[..., None], a[..., None])
    x[:, 2] = steered_table(prec, rows * heads * hd).reshape(rows, heads, hd)
    wq, wk = (torch.from_numpy(rng.choice([1.0, 300.0, 1e5], hd).astype(np.float32)) for _ in range(2))
    t = hip_ops.to_operand(x.reshape(rows, -1).cuda(), prec)
    src = hip_ops.from_operand(t, prec).cpu().double().reshape(rows, 3, heads, hd)          # the values as stored
    before = [e.cpu().clone() for e in _elements(t, prec)]
    hip_ops.qk_rmsnorm_(t, wq.cuda(), wk.cuda(), 1e-6, heads, hd, prec=prec)
    torch.cuda.synchronize()
    ref = src.clone()
    for i, w in ((0, wq), (1, wk)):
        ref[:, i] = w.double() * (src[:, i] * torch.rsqrt(src[:, i].pow(2).mean(-1, keepdim=True) + 1e-6))
    got = t.cpu()
    qk = 2 * heads * hd
    sub = got[..., :qk].contiguous()
    _, over = check_near(ref.reshape(rows, -1)[:, :qk], sub, prec, f"q/k RMSNorm {prec} head_dim {hd} heads {heads}")
    r = ref[:, :2].abs()
    assert (r > 65504).any() and ((r > 448) & (r < 65504)).any() and ((r > 0) & (r < 448)).any()
    assert (over > 0) == (prec in ("fp16", "f16x3"))
    for p, (g, b) in enumerate(zip(_elements(got, prec), before)):
        assert torch.equal(g[:, qk:], b[:, qk:]), f"{prec}: plane {p} of v changed"


def _padding_is_zero(out, cls, real):
    """the columns from `real` on hold zero bytes in every plane (F16C8's lo8 bytes are permuted inside 32-element blocks: from the next block on)"""
    for p, (g, b) in enumerate(zip(_planes(out, cls), _CLS[cls][1])):
        start = -(-real // 32) * 32 if (cls == "f16c8" and p == 1) else real * b
        assert not bool(g[:, start:].any()), f"{cls} plane {p}: padding columns must be zero bytes"


# ---- layout.hip: bd_patchify_heatmaps / bd_im2col_images.  patch == 14 with an even image width takes patchify_pair_kernel /
# im2col_strip_kernel (layout.hip:437, 457), any other patch size patchify_kernel / im2col_kernel
@pytest.mark.parametrize("form,patch", [("pair", 14), ("chunk", 7)])
@pytest.mark.parametrize("prec", RANGE_CLASSES)
def test_patchify_copies_the_table_bit_for_bit(hip, prec, form, patch):
    """Patchify is a copy: heat maps filled with the tiled table come out as the packer's planes; the zero padding columns are zero."""
    from oracle import boxdreamer_oracle as orc
    for size in (28, 224):
        for dt in (torch.float32, torch.bfloat16):
            n, grid = 2 if size == 28 else 1, size // patch
            real = 8 * patch * patch
            kpad = -(-real // 32) * 32 + 32
            # (bf16 input: fp32's largest values would round to Inf in bf16 -- non-finite inputs are no part of the contract)
            heat = steered_table(prec, n * 8 * size * size).reshape(n, 8, size, size).clamp(-CLASS_MAX["bf16"], CLASS_MAX["bf16"]).to(dt)
            out = hip_ops.patchify_heatmaps(heat.cuda(), patch=patch, kpad=kpad, prec=prec)
            torch.cuda.synchronize()
            want = torch.zeros(n * grid * grid, kpad)
            want[:, :real] = orc.patchify(heat.float(), patch, 8).reshape(n * grid * grid, real)
            for p, (g, w) in enumerate(zip(_planes(out, prec), _expect(want, prec))):
                assert torch.equal(g.cpu(), w), f"patchify ({form}) {prec} {dt} size {size} plane {p}: {_where(g.cpu(), w)}"
            _padding_is_zero(out, prec, real)


@pytest.mark.parametrize("form,patch", [("strip", 14), ("chunk", 7)])
@pytest.mark.parametrize("prec", RANGE_CLASSES)
def test_im2col_normalises_pixels_far_outside_the_range(hip, prec, form, patch):
    """im2col computes (x - mean) / std: pixels of +-1e3, +-1e6 and +-3e9 next to ordinary ones, against the packer on the fp64 result (with the
    kernel's fp32 constants)."""
    import torch.nn.functional as F
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).double().view(1, 3, 1, 1)
    for size in (28, 224):
        for dt in (torch.float32, torch.bfloat16):
            n, grid = 2 if size == 28 else 1, size // patch
            real = 3 * patch * patch
            kpad = -(-real // 32) * 32 + 32
            rng = np.random.default_rng(size + patch)
            img = torch.from_numpy(rng.uniform(0.0, 1.0, (n, 3, size, size)).astype(np.float32))
            wild = torch.from_numpy(rng.choice([1e3, -1e3, 1e6, -1e6, 3e9, -3e9], (n, 3, size, size)).astype(np.float32))
            img = torch.where(torch.from_numpy(rng.uniform(size=(n, 3, size, size)) < 0.1), wild, img).to(dt)
            out = hip_ops.im2col_images(img.cuda(), patch=patch, kpad=kpad, prec=prec)
            torch.cuda.synchronize()
            xn = (img.double() - mean) / std
            ref = torch.zeros(n * grid * grid, kpad, dtype=torch.float64)
            ref[:, :real] = F.unfold(xn, patch, stride=patch).transpose(1, 2).reshape(n * grid * grid, real)
            check_near(ref, out.cpu(), prec, f"im2col ({form}) {prec} {dt} size {size}")
            _padding_is_zero(out, prec, real)


# ------------------------------------------------------------------------------------------------------------------ part 5: the consuming side
# name -> (M, split-K factor, tile): large (132 tiles), small, the 128 x 96 form (at K = 768 through split-K)
C8_CONSUMER = {"large": (8448, 0, (256, 192)), "small": (300, 0, (128, 192)), "128x96": (300, 2, (128, 96))}


@pytest.mark.parametrize("form", sorted(C8_CONSUMER))
def test_gemm_f16c8_a_elements_beyond_448(hip, form):
    """The q8 image of A is derived in the K loop and saturates at +-448 (csrc/bd_common.h: RANGE): 32 rows carry a quarter of their elements
    from {449, 1000, 30000, 65504}, W has one column at 1e-4.  Against fp64 on the three decoded planes (f16c8_decode models the clamp) with
    the dot-product bound 2 K 2^-24 (|A_hi| |W|^T) + 1e-6; everything finite; the other rows have the bits they have without the outliers."""
    _needs_256_cus()
    M, split, tile = C8_CONSUMER[form]
    N = K = 768
    rng = np.random.default_rng(77)
    a0 = _randn((M, K), 1.0, seed=51)
    hot = torch.from_numpy(np.sort(rng.choice(M, 32, replace=False)))
    big = torch.from_numpy((rng.choice([449.0, 1000.0, 30000.0, 65504.0], (32, K)) * rng.choice([-1.0, 1.0], (32, K))).astype(np.float32))
    a1 = a0.clone()
    a1[hot.cuda()] = torch.where(torch.from_numpy(rng.uniform(size=(32, K)) < 0.25), big, a0[hot.cuda()].cpu()).cuda()
    w = _randn((N, K), 0.04, seed=52)
    w[:, 100] = _randn((N,), 1e-4, seed=53)
    b = _randn((N,), 0.3, seed=54)
    e = hip_ops.f16c8_qexp(w)
    w16 = hip_ops.f16c8_encode(w, e, True)
    outs = []
    for a in (a0, a1):
        kw = {"split_k": (hip_ops.splitk_workspace(M, N), split)} if split else {}
        outs.append(hip_ops.gemm(hip_ops.f16c8_encode(a, 0, False), w16, b, prec="f16c8", w_qexp=e, out_f32=True,
                                 expect={"tile": tile, "ep": 3, "split_k": split or 1}, **kw))
    torch.cuda.synchronize()
    base, out = outs
    assert torch.isfinite(out).all()
    cold = torch.ones(M, dtype=torch.bool, device="cuda")
    cold[hot.cuda()] = False
    assert torch.equal(out[cold], base[cold]), "rows without outliers changed: an overflow leaked through a shared tile"
    ah, al, aq = (t.double()[hot.cuda()] for t in hip_ops.f16c8_decode(hip_ops.f16c8_encode(a1, 0, False)))
    wh, wl, wq = (t.double() for t in hip_ops.f16c8_decode(w16, e, True))
    assert (aq.abs().max().item() == 448.0) and (ah.abs().max().item() == 65504.0)
    ref = ah @ wh.t() + al @ wq.t() + aq @ wl.t() + b.double()
    tol = 2 * K * 2.0 ** -24 * (ah.abs() @ (wh + wl).abs().t()) + 1e-6
    err = (out[hot.cuda()].double() - ref).abs()
    assert (err <= tol).all(), f"{form}: worst err / tol {float((err / tol).max()):.3f}"


# ------------------------------------------------------------------------------------------------------------------ attention outputs
_ATTN_OUT_CLS = {"planes": "bf16x3", "planes_bf16": "bf16x3", "fp8": "fp8", "f16c8": "f16c8", "planes_f16": "f16x3"}
# softmax scale of test_attention_stores_the_v_row: the kernels fold log2(e) into it with one fp32 multiply, and this value makes the
# product exactly 2^100 -- a power of two, so that scale * score is exact and the best key's exponent s * sc - m * sc is exactly 0
ONE_HOT = float.fromhex("0x1.62e43p+99")
assert np.float32(np.float32(ONE_HOT) * np.float32(1.4426950408889634)) == np.float32(2.0 ** 100)


V_ROW_SHAPES = [(70, 64), (70, 96), (261, 64), (261, 96), (256, 64), (256, 96)]
V_ROW_BATCH, V_ROW_HEADS, V_ROW_NPRE = 2, 2, 5
V_ROW_Q_LEN = {70: 35, 261: 87, 256: 128}
# seq -> waves of attn_kernel for bd_attention, bd_attention_q (V_ROW_Q_LEN queries) and bd_attention_prefix (seq - 5 patch queries)
V_ROW_WAVES = {70: (3, 3, 3), 261: (3, 3, 4), 256: (4, 4, 4)}


def v_row_plans(variant, seq, hd):
    """The plans of the three launches of test_attention_stores_the_v_row, held against the forms the test is about: attn_kernel on
    V_ROW_WAVES, but the ping-pong kernel for bd_attention on 256 rows at head_dim 96 in the one-plane classes (the prefix call's 256
    queries of 261 rows stay on attn_kernel: 261 keys are no whole key tiles)."""
    in_prec, code, _ = _PREFIX_VARIANTS[variant]
    call = dict(prec=getattr(_lib, code), batch=V_ROW_BATCH, seq=seq, heads=V_ROW_HEADS, head_dim=hd)
    plans = [hip_ops.attention_plan("plain", **call), hip_ops.attention_plan("q", q_view=True, q_len=V_ROW_Q_LEN[seq], **call),
             hip_ops.attention_plan("prefix", n_prefix=V_ROW_NPRE, prefix_queries=0, **call)]
    want = [("tiled", w) for w in V_ROW_WAVES[seq]]
    if seq == 256 and hd == 96 and _lib.planes(in_prec) == 1:
        want[0] = ("pp", 8)
    assert [(p["kernel"], p["waves"]) for p in plans] == want and all(p["head_dim"] == hd and not p["vl"] for p in plans), plans
    q_len = V_ROW_Q_LEN[seq]
    assert [(p["q_len"], p["q_off"], p["out_rows"]) for p in plans] == [(seq, 0, seq), (q_len, 0, q_len), (seq - V_ROW_NPRE, V_ROW_NPRE, seq)]
    return plans


@pytest.mark.parametrize("seq,hd", V_ROW_SHAPES)
@pytest.mark.parametrize("variant", sorted(_PREFIX_VARIANTS))
def test_attention_stores_the_v_row(hip, variant, seq, hd):
    """Within a (sample, head) every key has the same V row, taken from the steered table of the INPUT class; Q and K are random.  The
    kernels round P to the operand type for the P V product but take the row sum of the unrounded P, so the output is V times a factor
    that is 1 only where P is exactly representable (random P: 1 +- 2^-9 for bf16, their designed precision, which the op tests bound
    with 6 EPS).  The softmax scale is therefore a power of two (after the kernel's multiplication by log2 e) so large that P is one-hot:
    exp2(0) = 1 for a row's best key and exp2((s - m) 2^100) = 0 for every other one, for any Q and K.  The row sum is then exactly 1 and
    the accumulator exactly V -- also for the largest bf16 values, which an accumulation over several keys with non-zero P overflows
    (|v| l > fp32's range: a limit of the un-normalised accumulation, not of the store).  The stored planes are the packing of the V row
    in the OUTPUT class, bit for bit: rounded where the output class is narrower (bf16 -> e4m3, split-bf16 -> F16C8 / split-f16), saturated at its
    MAX where the input exceeds its range.  attn_kernel (3 / 4 waves: seq 70, 261, and 256 at head_dim 64 or two planes) and
    attn_kernel_pp (seq 256, head_dim 96, one-plane inputs) through bd_attention, bd_attention_q (one third / half of the rows as
    queries, compact output) and bd_attention_prefix without the prefix queries, whose rows keep their fill: v_row_plans asserts the
    form of each launch."""
    batch, heads, npre = V_ROW_BATCH, V_ROW_HEADS, V_ROW_NPRE
    in_prec, code, kind = _PREFIX_VARIANTS[variant]
    v_row_plans(variant, seq, hd)
    out_cls = in_prec if kind == "native" else _ATTN_OUT_CLS[kind]
    pid = getattr(_lib, code)
    lib = _lib.load()
    qkv = torch.from_numpy(synth.bell_np("range_attn", (batch, seq, 3, heads, hd), 1.0, 0.0, seq + hd).astype(np.float32))
    qkv[:, :, 2] = steered_table(in_prec, batch * heads * hd).reshape(batch, 1, heads, hd)
    t = hip_ops.to_operand(qkv.reshape(batch * seq, -1).cuda(), in_prec)
    stored = hip_ops.from_operand(t, in_prec).cpu().reshape(batch, seq, 3, heads, hd)
    s = torch.einsum("bqhd,bkhd->bhqk", stored[:, :, 0].double(), stored[:, :, 1].double()).sort(-1)[0]
    assert ((s[..., -1] - s[..., -2]) > 1e-5).all(), "a row's two best scores must differ (beyond the kernels' fp32 rounding of a score)"
    # the V rows as stored are what every query's output is (0 + 1 * v: a -0 does not survive the accumulator's +0)
    vrow = 0.0 + stored[:, :, 2].reshape(batch, seq, heads * hd)
    assert torch.isfinite(vrow).all() and (vrow.abs().max() >= CLASS_MAX[in_prec])
    qkv_plane = t[0].numel() if _lib.planes(in_prec) == 2 else 0
    two = len(_CLS[out_cls][1]) == 2

    def alloc(rows):
        o = operand.empty(out_cls, rows, heads * hd, "cuda")
        o.view(torch.uint8).copy_(((torch.arange(o.numel() * o.element_size(), device="cuda") * 37 + 11) % 251).to(torch.uint8).reshape(o.view(torch.uint8).shape))
        return o

    def same(got, want_rows, what, rows=None):
        want = hip_ops.to_operand(want_rows.reshape(-1, heads * hd), out_cls)
        for p, (g, w) in enumerate(zip(_elements(got.cpu(), out_cls), _elements(want, out_cls))):
            if rows is not None:
                g, w = g.reshape(batch, seq, -1)[:, rows], w.reshape(batch, seq, -1)[:, rows]
            bad = (g != w).nonzero()
            assert bad.numel() == 0, f"{variant} seq {seq} head_dim {hd} {what}: plane {p} differs from the packed V row in {bad.shape[0]} elements, the first at {tuple(bad[0].tolist())}"

    plane = lambda o: o[0].numel() if two else 0
    full = alloc(batch * seq)
    _lib.check(lib.bd_attention(_lib.ptr(t), qkv_plane, _lib.ptr(full), plane(full), batch, seq, heads, hd, ONE_HOT, pid, _lib.stream()), "bd_attention")
    torch.cuda.synchronize()
    same(full, vrow, "bd_attention")
    # queries = one view of the sequence, compact output
    q_len = V_ROW_Q_LEN[seq]
    q_view = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    part = alloc(batch * q_len)
    _lib.check(lib.bd_attention_q(_lib.ptr(t), qkv_plane, _lib.ptr(part), plane(part), batch, seq, heads, hd, ONE_HOT, _lib.ptr(q_view), q_len, pid,
                                  _lib.stream()), "bd_attention_q")
    torch.cuda.synchronize()
    want = hip_ops.to_operand(vrow[:, :q_len].reshape(-1, heads * hd), out_cls)
    for p, (g, w) in enumerate(zip(_elements(part.cpu(), out_cls), _elements(want, out_cls))):
        assert torch.equal(g, w), f"{variant} seq {seq} head_dim {hd} bd_attention_q: plane {p}"
    # the patch queries only: the prefix rows keep their fill
    skip = alloc(batch * seq)
    keep = skip.clone()
    _lib.check(lib.bd_attention_prefix(_lib.ptr(t), qkv_plane, _lib.ptr(skip), plane(skip), batch, seq, heads, hd, ONE_HOT, npre, 0, pid,
                                       _lib.stream()), "bd_attention_prefix")
    torch.cuda.synchronize()
    same(skip, vrow, "bd_attention_prefix", rows=slice(npre, seq))
    for p, (g, k) in enumerate(zip(_elements(skip.cpu(), out_cls), _elements(keep.cpu(), out_cls))):
        assert torch.equal(g.reshape(batch, seq, -1)[:, :npre], k.reshape(batch, seq, -1)[:, :npre]), f"{variant}: plane {p} of a prefix row changed"
    if out_cls == "f16c8":                                      # the unused second half of plane-1 storage
        n = batch * seq * heads * hd
        assert torch.equal(skip[1].view(torch.uint8).reshape(-1)[n:], keep[1].view(torch.uint8).reshape(-1)[n:])


def _quantum(x):
    """the value of the lowest set bit of each fp64 element (inf for 0)"""
    m, e = np.frexp(x)
    k = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = k & -k
    return np.where(k == 0, np.inf, np.ldexp(low.astype(np.float64), e - 53))


@pytest.mark.parametrize("seq,hd", [(70, 64), (70, 96), (261, 64), (261, 96)])
@pytest.mark.parametrize("variant", ["bf16x3_out_f16c8", "bf16x3_out_f16x3"])
def test_attention_normalisation_rounds_once_before_the_split(hip, variant, seq, hd):
    """The attention epilogue multiplies the accumulator by 1 / l in front of the store, and hi and lo of a two-plane result must be taken
    from the fp32 PRODUCT: a compiler that folds the multiply into the f16 conversion rounds the exact product instead, which differs
    at every f16 tie (the fence in f16c8_split / split_hi_lo, csrc/bd_common.h).  Here the product is not exact but known: within a
    (sample, head) all keys are the SAME row (random across samples and heads) and the softmax scale is the power of two of
    test_attention_stores_the_v_row, so every P is exp2(0) = 1, l = seq, the accumulator seq * v (exact in fp32 for the values
    compared) and the value in front of the split fp32(seq * v * fp32(1 / seq)) -- for an f16 tie v that is v itself, while the exact
    product lies a little to one side of it.  V carries the steered table of the OUTPUT class (f16 ties, even and odd, both signs) through
    split-bf16 inputs, which hold them exactly.  Bit for bit against the packer on the host-computed product."""
    batch, heads = 2, 2
    in_prec, code, kind = _PREFIX_VARIANTS[variant]
    out_cls = _ATTN_OUT_CLS[kind]
    lib = _lib.load()
    qkv = torch.from_numpy(synth.bell_np("range_attn_eq", (batch, seq, 3, heads, hd), 1.0, 0.0, seq + hd).astype(np.float32))
    qkv[:, :, 1] = qkv[:, :1, 1]                                          # one key row per (sample, head)
    # (split-bf16 inputs: fp32's largest values would round to Inf in bf16 -- non-finite inputs are no part of the contract)
    vt = steered_table(out_cls, 768)[:batch * heads * hd].clamp(-CLASS_MAX["bf16"], CLASS_MAX["bf16"])
    vt[steered_count(out_cls):] = (torch.arange(batch * heads * hd - steered_count(out_cls)) % 33 - 16).float() / 16
    qkv[:, :, 2] = vt.reshape(batch, 1, heads, hd)
    t = hip_ops.to_operand(qkv.reshape(batch * seq, -1).cuda(), in_prec)
    vrows = t[:, :, 2 * heads * hd:].cpu()                                # [2, rows, heads * hd]: V as stored, hi and lo planes
    hi, lo = vrows[0, :seq * batch:seq].double().numpy(), vrows[1, :seq * batch:seq].double().numpy()
    v = hi + lo
    # every partial sum a * hi + b * lo (a, b <= seq < 512) is exact in fp32 where 512 |v| spans at most 24 bits above the planes' lowest bit
    exact = (512.0 * np.abs(v) * 1.01 <= 2.0 ** 24 * np.minimum(_quantum(hi), _quantum(lo))) & (np.abs(v) * seq < 3e38)
    ties = np.isin(np.arange(heads * hd * batch).reshape(batch, -1), np.arange(12, 120))      # the table's tie entries and their neighbours
    assert exact.mean() > 0.6 and (exact & ties & (v == vt.double().numpy().reshape(batch, -1))).sum() >= 30      # the ties themselves are compared
    acc = np.clip(np.float64(seq) * v, -CLASS_MAX["f32"], CLASS_MAX["f32"]).astype(np.float32)      # (entries beyond fp32 / seq are not compared)
    inv = np.float32(1.0) / np.float32(seq)
    pre = torch.from_numpy((acc * inv).astype(np.float32)) + 0.0          # fp32 product, as the kernel forms it
    assert np.float32(np.float64(acc[0, 12]) * np.float64(inv)) == pre[0, 12].item() and float(np.float64(acc[0, 12]) * np.float64(inv)) != pre[0, 12].item()
    out = operand.empty(out_cls, batch * seq, heads * hd, "cuda", zero=True)
    plan = hip_ops.attention_plan("plain", prec=getattr(_lib, code), batch=batch, seq=seq, heads=heads, head_dim=hd)
    assert (plan["kernel"], plan["planes"], plan["waves"], plan["head_dim"]) == ("tiled", 2, 3, hd), plan      # the split-bf16 epilogues of attn_kernel
    _lib.check(lib.bd_attention(_lib.ptr(t), t[0].numel(), _lib.ptr(out), out[0].numel(), batch, seq, heads, hd, ONE_HOT, getattr(_lib, code),
                                _lib.stream()), "bd_attention")
    torch.cuda.synchronize()
    want = _elements(hip_ops.to_operand(pre, out_cls), out_cls)
    mask = torch.from_numpy(exact)
    for p, (g, w) in enumerate(zip(_elements(out.cpu(), out_cls), want)):
        g = g.reshape(batch, seq, -1)
        assert torch.equal(g, g[:, :1].expand_as(g)), f"{variant}: plane {p} differs between queries of a sample"
        bad = ((g[:, 0] != w) & mask).nonzero()
        assert bad.numel() == 0, (f"{variant} seq {seq} head_dim {hd}: plane {p} is not the packing of fp32(seq * v / seq) in {bad.shape[0]} elements, "
                                  f"the first at v = {v[tuple(bad[0].tolist())]!r}")
