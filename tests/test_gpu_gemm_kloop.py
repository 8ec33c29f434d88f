"""The F16C8 GEMM's K loop is unrolled over the ring period (gemm_f16c8.hip: every fragment address = a per-lane register + an immediate
that encodes the stage).  The smallest shapes at which such a loop can go wrong: slab counts around the period (whole periods, remainders,
the two-stage ring), workgroups that walk two tiles (the stage carried from tile to tile), every kernel form, split-K's slab ranges.

Reference and tolerance are those of tests/test_gpu_ops.py::test_gemm_f16c8: fp64 arithmetic on exactly the three decoded planes the
kernel multiplies, so that only the fp32 accumulation order differs: |err| < 2e-5 sqrt(K).  Between kernel forms the project guarantees
equal bits (test_gemm_f16c8_small_form_rows_equal_the_large_form); that is asserted here on the new shapes.

bd_gemm takes K in multiples of 64 (include/boxdreamer_hip.h), so an unsplit launch has an even slab count: 6 k slabs on the three-stage
ring, 2 k on the two-stage ring -- always whole periods.  K = 96, 288 (3 and 9 slabs) and K = 160 (5 slabs) are therefore rejected before
anything is launched, which is what their cases assert; slab counts that are NOT whole periods reach the kernel through split-K only
(test_split_k_slab_ranges: 3, 9, 1 | 2, 4 | 5, 7 | 8 and 32 slabs per workgroup)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from boxdreamer_amd import _lib, hip_ops, synth

pytestmark = pytest.mark.gpu

HEAD = 300            # rows compared between forms: one whole 256-row tile and a ragged second one


def _rand(name, shape, std=1.0, seed=3):
    return torch.from_numpy(synth.bell_np(name, shape, std, 0.0, seed).astype(np.float32)).cuda()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


LARGE, SMALL = (256, 192), (128, 192)        # workgroup tiles of the two forms (hip_ops.gemm_plan: "tile")


def _stages(K):
    """ring depth of a launch: three stages where the slab count is a multiple of three"""
    return 3 if (K // 32) % 3 == 0 else 2


@functools.lru_cache(maxsize=None)
def _large_rows(N):
    """the fewest whole 256-row tiles at which the plan of a three-stage launch on this device names the 256 x 192 form"""
    return next(256 * j for j in range(1, 1 << 12)
                if all(l["tile"] == LARGE for l in hip_ops.gemm_plan(hip_ops.gemm_shape_args(256 * j, N, 768), "f16c8")))


@functools.lru_cache(maxsize=3)
def _case(M, N, K, rows=None):
    """operands of an M x N x K launch and the fp64 reference (bias included) of its first `rows` rows; shared, never modified"""
    a, w, b = _rand("ka", (M, K)), _rand("kw", (N, K), 0.03), _rand("kb", (N,), 0.1)
    e = hip_ops.f16c8_qexp(w)
    a16, w16 = hip_ops.f16c8_encode(a, 0, False), hip_ops.f16c8_encode(w, e, True)
    r = M if rows is None else rows
    ah, al, aq = (t[:r].double() for t in hip_ops.f16c8_decode(a16))
    wh, wl, wq = (t.double() for t in hip_ops.f16c8_decode(w16, e, True))
    ref = ah @ wh.t() + al @ wq.t() + aq @ wl.t() + b.double()
    return (a, a16), w16, b, e, ref


def _head(a_pair, rows):
    """the first rows as an operand of their own (packed anew: the byte plane of an activation operand is dense in rows x K)"""
    return hip_ops.f16c8_encode(a_pair[0][:rows], 0, False)


def _rejected(N, K):
    """K % 64 != 0: BD_ERR_SHAPE from bd_gemm's argument check, nothing launched"""
    if K % 64 == 0:
        return False
    ap, w16, b, e, _ = _case(HEAD, N, K)
    with pytest.raises(_lib.HipLibraryError, match="BD_ERR_SHAPE"):
        hip_ops.gemm(ap[1], w16, b, prec="f16c8", out_f32=True, w_qexp=e)
    return True


def _bits_equal(x, y, rows, N, what):
    """x: a launch of at least `rows` rows, y: a launch of exactly `rows` rows; fp32 / 16-bit planes or the F16C8 operand class"""
    if x.dim() == 3 and x.dtype == torch.float16 and x.shape[0] == 2:         # F16C8 storage: f16 plane + the byte plane's first rows * N bytes
        assert torch.equal(x[0][:rows], y[0][:rows]), (what, "f16 plane")
        nb = rows * N
        assert torch.equal(x[1].view(torch.uint8).reshape(-1)[:nb], y[1].view(torch.uint8).reshape(-1)[:nb]), (what, "lo8 plane")
    else:
        assert torch.equal(x[:rows].contiguous().view(torch.uint8), y[:rows].contiguous().view(torch.uint8)), what


# ---------------------------------------------------------------------------------------------- ring periods and remainders
@pytest.mark.parametrize("M", [256, 300])
@pytest.mark.parametrize("N", [192, 768])
@pytest.mark.parametrize("K", [96, 192, 288, 128, 160])
def test_slab_counts_around_the_ring_period(hip, M, N, K):
    """6 slabs on the three-stage form (K = 192), 4 on the two-stage form (K = 128); fp32 rows, plain and on a residual.  K = 96, 288, 160 (3, 9,
    5 slabs) are rejected: module docstring."""
    if _rejected(N, K):
        return
    ap, w16, b, e, ref = _case(HEAD, N, K)
    a = _head(ap, M)
    out = hip_ops.gemm(a, w16, b, prec="f16c8", out_f32=True, w_qexp=e, expect={"stages": _stages(K), "ep": 3})
    err = (out.double() - ref[:M]).abs().max().item()
    print(f"M {M} N {N} K {K}: max err {err:.3g} (bound {2e-5 * K ** 0.5:.3g})")
    assert err < 2e-5 * K ** 0.5, err
    res = _rand("kr", (HEAD, N))[:M]
    buf = res.clone()
    hip_ops.gemm(a, w16, b, prec="f16c8", out_f32=True, out=buf, resid=buf, w_qexp=e, expect={"stages": _stages(K), "ep": 3})
    assert (buf.double() - (ref[:M] + res.double())).abs().max().item() < 2e-5 * K ** 0.5 + 1e-6


# ---------------------------------------------------------------------------------------------- the stage carried across tiles
@pytest.mark.parametrize("K", [96, 768, 160, 128, 192])
def test_stage_carried_to_a_workgroups_second_tile(hip, K):
    """N = 768 and 8 more 256 x 192 tiles than the device has CUs (rounded up to whole tile rows): the persistent grid is one workgroup
    per CU, so some workgroups walk two tiles.  K = 768: 24 slabs, the ring is back at stage 0 for the second tile, whose first two slabs the
    producers fetch under the first tile's epilogue (its scratch overlays stage 2); K = 192 and K = 128: the shortest loops of the three- and
    the two-stage ring.  K = 96 and K = 160 (which would leave the two-stage ring
    at stage 1) are rejected: module docstring."""
    N = 768
    if _rejected(N, K):
        return
    M = 256 * -(-(_cus() + 8) // 4)
    (_, a16), w16, b, e, ref = _case(M, N, K)
    tiles = (M // 256) * (N // 192)
    out = hip_ops.gemm(a16, w16, b, prec="f16c8", out_f32=True, w_qexp=e, expect={"tile": LARGE, "stages": _stages(K), "grid": _cus()})
    assert _cus() < tiles <= 2 * _cus()
    err = (out.double() - ref).abs().max().item()
    print(f"M {M} K {K}: max err {err:.3g} (bound {2e-5 * K ** 0.5:.3g})")
    assert err < 2e-5 * K ** 0.5, err


# ---------------------------------------------------------------------------------------------- forms
@pytest.mark.parametrize("kind", ["f32", "gelu_f32"])
@pytest.mark.parametrize("N", [192, 768])
@pytest.mark.parametrize("K", [96, 192, 288, 128, 160])
def test_large_form_rows_equal_the_small_form(hip, N, K, kind):
    """256 x 192 tiles (a launch of more large tiles than half the CUs) against 128 x 192 tiles (256 and 300 rows alone): bit for bit.
    f32: the fp32 epilogue, whose small form needs the three-stage ring (the two-stage K compare the large form's whole and ragged tiles);
    gelu_f32: the generic epilogue, which has a small form at either ring depth."""
    if _rejected(N, K):
        return
    big_rows = _large_rows(N)
    ap, w16, b, e, ref = _case(big_rows, N, K, HEAD)
    a16 = ap[1]
    kw = {"act": _lib.ACT_GELU} if kind == "gelu_f32" else {}
    ep = 0 if kind == "gelu_f32" else 3
    big = hip_ops.gemm(a16, w16, b, prec="f16c8", out_f32=True, w_qexp=e, expect={"tile": LARGE, "stages": _stages(K), "ep": ep}, **kw)
    want = F.gelu(ref.float()).double() if kind == "gelu_f32" else ref
    tol = 2e-5 * K ** 0.5 * (1.13 if kind == "gelu_f32" else 1.0) + (1e-6 if kind == "gelu_f32" else 0.0)      # (|GELU'| <= 1.13)
    assert (big[:HEAD].double() - want).abs().max().item() < tol
    for rows in (256, 300):
        form = SMALL if ep == 0 or _stages(K) == 3 else LARGE
        small = hip_ops.gemm(_head(ap, rows), w16, b, prec="f16c8", out_f32=True, w_qexp=e, expect={"tile": form, "stages": _stages(K), "ep": ep}, **kw)
        _bits_equal(big, small, rows, N, (kind, N, K, rows))


def _fold_stats(M):
    """row statistics of a LayerNorm-fold consumer: eight equal (mean, M2) pairs per row -> mean_r, var_r = M2 / 96 in [1, 3] (rstd <= 1,
    so the accumulation error enters the result no larger than in the plain launch)"""
    mean = ((torch.arange(M, dtype=torch.float32) % 11) - 5) * 0.0625
    var = 1.0 + (torch.arange(M, dtype=torch.float32) % 9) * 0.25
    st = torch.stack([mean, var * 96.0], -1)[:, None, :].expand(M, 8, 2).contiguous().cuda()
    return st, mean.cuda().double(), var.cuda().double()


@pytest.mark.parametrize("K", [96, 768])
def test_layernorm_fold_consumer_with_gelu(hip, K):
    """fc1's instance: LayerNorm-fold consumer + GELU into the operand class, large and small form.  The fold exists at K = 768 only
    (gemm_common.h: ln_fold_consumer_ok); at K = 96 the library must refuse the launch rather than run another form."""
    N, eps = 768, 1e-6
    big_rows = _large_rows(N)
    ap, w16, b, e, ref = _case(big_rows, N, K, HEAD)
    a16 = ap[1]
    st, mean, var = _fold_stats(big_rows)
    colsum = _rand("ks", (N,), 0.2)
    if K != 768:
        with pytest.raises((ValueError, RuntimeError)):
            hip_ops.gemm(_head(ap, HEAD), w16, b, prec="f16c8", act=_lib.ACT_GELU, w_qexp=e, ln_apply=(st[:HEAD].contiguous(), colsum, eps))
        return
    rstd = torch.rsqrt(var[:HEAD] + eps)[:, None]
    pre = rstd * (ref - b.double()) - (mean[:HEAD, None] * rstd) * colsum.double() + b.double()
    g = F.gelu(pre.float())
    form = {"stages": 3, "ep": 1, "gelu": True, "lnf": True}
    big = hip_ops.gemm(a16, w16, b, prec="f16c8", act=_lib.ACT_GELU, w_qexp=e, ln_apply=(st, colsum, eps), expect={"tile": LARGE, **form})
    small = hip_ops.gemm(_head(ap, HEAD), w16, b, prec="f16c8", act=_lib.ACT_GELU, w_qexp=e, ln_apply=(st[:HEAD].contiguous(), colsum, eps),
                         expect={"tile": SMALL, **form})
    _bits_equal(big, small, HEAD, N, "fold consumer + GELU")
    oh, ol, oq = hip_ops.f16c8_decode(small)
    err = ((oh + ol) - g).abs().max().item()
    print(f"fold consumer + GELU K {K}: max err {err:.3g}")
    assert err < 4e-4 * max(1.0, g.abs().max().item()) * 2.0 ** -4 + 2e-5
    assert ((oq - g).abs() <= g.abs() * 2.0 ** -4 + 2.0 ** -9).all()


@pytest.mark.parametrize("K", [96, 768])
def test_gelu_instance(hip, K):
    """GELU into the operand class: EP 1 at K = 768 (large and small form); K = 96 is rejected (module docstring)"""
    N = 768
    if _rejected(N, K):
        return
    big_rows = _large_rows(N)
    ap, w16, b, e, ref = _case(big_rows, N, K, HEAD)
    a16 = ap[1]
    g = F.gelu(ref.float())
    form = {"stages": 3, "ep": 1, "gelu": True, "lnf": False}
    big = hip_ops.gemm(a16, w16, b, prec="f16c8", act=_lib.ACT_GELU, w_qexp=e, expect={"tile": LARGE, **form})
    small = hip_ops.gemm(_head(ap, HEAD), w16, b, prec="f16c8", act=_lib.ACT_GELU, w_qexp=e, expect={"tile": SMALL, **form})
    _bits_equal(big, small, HEAD, N, "GELU")
    oh, ol, oq = hip_ops.f16c8_decode(small)
    assert ((oh + ol) - g).abs().max().item() < 4e-4 * max(1.0, g.abs().max().item()) * 2.0 ** -4 + 2e-5
    assert ((oq - g).abs() <= g.abs() * 2.0 ** -4 + 2.0 ** -9).all()


@pytest.mark.parametrize("K", [96, 192, 768])
@pytest.mark.parametrize("ep", [4, 5])
def test_layernorm_fold_producers(hip, ep, K):
    """EP 4 (fp32 residual in, fp32 rows + operand copy + row statistics out) and EP 5 (the residual is the operand copy), large and small
    form.  The producers need the specialised epilogue (K >= 128): at K = 96 the library must refuse; K = 192 is their shortest loop."""
    N = 768
    big_rows = _large_rows(N)
    ap, w16, b, e, ref = _case(big_rows, N, K, HEAD)
    a16 = ap[1]
    res = _rand("kp", (big_rows, N))
    if ep == 5:                              # the residual as the kernel reads it: the decoded operand copy
        rh, rl, _ = hip_ops.f16c8_decode(hip_ops.f16c8_encode(res, 0, False))
        res = (rh + rl).float()

    def go(rows):
        form = {"tile": LARGE if rows == big_rows else SMALL, "stages": 3, "ep": ep}
        st = torch.zeros((rows, 8, 2), dtype=torch.float32, device="cuda")
        buf = res[:rows].clone()
        if ep == 4:
            op = torch.zeros_like(hip_ops.f16c8_encode(res[:rows], 0, False))
            hip_ops.gemm(_head(ap, rows), w16, b, prec="f16c8", out_f32=True, out=buf, resid=buf, w_qexp=e, ln_emit=(st, op), expect=form)
        else:
            op = hip_ops.f16c8_encode(res[:rows], 0, False)
            hip_ops.gemm(_head(ap, rows), w16, b, prec="f16c8", out_f32=True, out=buf, w_qexp=e, ln_emit=(st, op), ln_resid_in_op=True, expect=form)
        return buf, op, st

    if K < 128:
        with pytest.raises((ValueError, RuntimeError)):
            go(HEAD)
        return
    big, small = go(big_rows), go(HEAD)
    _bits_equal(big[0], small[0], HEAD, N, ("fp32 rows", ep, K))
    _bits_equal(big[1], small[1], HEAD, N, ("operand copy", ep, K))
    assert torch.equal(big[2][:HEAD], small[2]), ("row statistics", ep, K)
    want = ref + res[:HEAD].double()
    err = (small[0].double() - want).abs().max().item()
    print(f"EP {ep} K {K}: max err {err:.3g} (bound {2e-5 * K ** 0.5 + 1e-6:.3g})")
    assert err < 2e-5 * K ** 0.5 + 1e-6
    oh, ol, _ = hip_ops.f16c8_decode(small[1])
    assert ((oh + ol).double() - small[0].double()).abs().max().item() <= 2.0 ** -15 * max(1.0, want.abs().max().item())     # F16C8's half ulp
    grp = small[0].double().reshape(HEAD, 8, 96)
    assert (small[2][..., 0].double() - grp.mean(-1)).abs().max().item() < 1e-5
    m2 = ((grp - grp.mean(-1, keepdim=True)) ** 2).sum(-1)
    assert ((small[2][..., 1].double() - m2).abs() <= 1e-4 * m2 + 1e-5).all()


# ---------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("M,K,split", [(1536, 768, 0), (1536, 3072, 0), (1536, 3072, 3), (1536, 960, 4), (300, 192, 2), (300, 192, 4), (300, 576, 2),
                                       (300, 576, 4)])
def test_split_k_slab_ranges(hip, M, K, split):
    """The latency forms at 1536 rows: the factor the library picks (0), and forced factors whose slab count per workgroup is no multiple
    of the ring period (K = 3072 in three: 32 slabs each; K = 960 in four: 7, 8, 7, 8).  At 300 rows (a ragged last tile) the slab counts of
    the issue's K = 96 and 288: K = 192 in two (3 each) and in four (1, 2, 1, 2), K = 576 in two (9 each) and in four (4, 5, 4, 5).
    Deterministic over two runs."""
    N = 768
    (_, a16), w16, b, e, ref = _case(M, N, K)
    res = _rand("kq", (M, N))
    ws = hip_ops.splitk_workspace(M, N)
    assert ws is not None
    outs = []
    for _ in range(2):
        buf = res.clone()
        # a forced factor is the plan's factor, on 128 x 96 tiles; the factor the library picks is its own business
        hip_ops.gemm(a16, w16, b, prec="f16c8", out_f32=True, out=buf, resid=buf, w_qexp=e, split_k=(ws, split),
                     expect={"split_k": split, "tile": (128, 96), "ep": 3} if split else {"ep": 3})
        outs.append(buf)
    assert int(ws[:16384].view(torch.int32).abs().max()) == 0, "split-K flags must be left zero"
    assert torch.equal(outs[0], outs[1])
    err = (outs[0].double() - (ref + res.double())).abs().max().item()
    print(f"split-K K {K} factor {split}: max err {err:.3g} (bound {2e-5 * K ** 0.5 + 1e-6:.3g})")
    assert err < 2e-5 * K ** 0.5 + 1e-6
