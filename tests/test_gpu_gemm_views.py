"""bd_gemm and bd_layernorm on strided sub-views with guard bands.

Every other op-level test hands the library contiguous tensors: lda = ldw = K, ldo = ldr = N, planes rows * ld apart, pointers at the
start of their allocation.  The whole-path code launches forms in which these quantities are decoupled (a column block of a wider
buffer, weight rows inside a larger weight, planes further apart than rows * ld, row slices of a problem), and each quantity is
consumed by separately written address code.  Here every operand and every output lives in an ARENA: a larger allocation with a
leading dimension above the column count, a plane distance above rows * ld, guard rows around every plane and a data pointer off the
allocation's start.  Input padding is NaN in the operand's format (any use shows in the result); output padding is a fixed byte
pattern that is compared bytewise afterwards.  Each case runs twice, contiguous and on arenas, and asserts

  (a) the payload against fp64 arithmetic on the operands as stored (tolerances copied from the contiguous tests, cited in place),
  (b) the arena payload bit-identical to the contiguous run (a row's bits do not depend on the launch form; split-K: same factor),
  (c) every non-payload byte of every arena unchanged,
  (d) a finite payload (poisoned padding never reaches a result).

The arena helpers are plain torch and are checked on the CPU by the unmarked tests at the top."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from boxdreamer_amd import _lib, hip_ops

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ arenas
# operand class -> (storage dtype, bytes per element of each plane, NaN of each plane's format as little-endian bytes)
_NAN = {"bf16": (0xC0, 0x7F), "fp16": (0x00, 0x7E), "e4m3": (0x7F,), "f32": (0x00, 0x00, 0xC0, 0x7F)}
_CLS = {"bf16": (torch.bfloat16, (2,), ("bf16",)), "fp16": (torch.float16, (2,), ("fp16",)),
        "bf16x3": (torch.bfloat16, (2, 2), ("bf16", "bf16")), "f16x3": (torch.float16, (2, 2), ("fp16", "fp16")),
        "fp8": (torch.float8_e4m3fn, (1,), ("e4m3",)), "f32": (torch.float32, (4,), ("f32",)),
        # F16C8 (include/boxdreamer_hip.h): plane 1 of an ACTIVATION is one byte per element, rows of ld BYTES packed at the head of the
        # plane; plane 1 of a WEIGHT is two bytes per element, rows of 2 ld bytes.  The k permutation is local to 32-element blocks, so
        # both are 2-D byte copies of f16c8_encode's planes (K % 32 == 0, ld % 32 == 0).
        "f16c8": (torch.float16, (2, 1), ("fp16", "e4m3")), "f16c8_w": (torch.float16, (2, 2), ("fp16", "e4m3"))}
TAIL = 4096        # spare bytes behind the last guard row


def _pattern(n, device, mul=131, add=7):
    return ((torch.arange(n, device=device, dtype=torch.int64) * mul + add) % 251).to(torch.uint8)


class Arena:
    """buf: the whole allocation (uint8); base: byte offset of the data pointer; ld: leading dimension in elements; plane: distance of
    plane 1 in 2-byte units (0 for one plane); mask: True on payload bytes; pristine: buf as placed."""

    def seg(self, p, of=None):
        bpe = _CLS[self.cls][1][p]
        return torch.as_strided(self.buf if of is None else of, (self.rows, self.cols * bpe), (self.ld * bpe, 1), self.base + 2 * self.plane * p)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.base


def _plane_bytes(t, cls, p):
    """plane p of a contiguous operand tensor as [rows, payload bytes per row] (a view of t)"""
    rows, cols = t.shape[-2:]
    b = t.view(torch.uint8)
    if len(_CLS[cls][1]) == 1:
        return b.reshape(rows, -1)
    if cls == "f16c8" and p == 1:
        return b[1].reshape(-1)[: rows * cols].reshape(rows, cols)
    return b[p]


def place(t, cls, ld=None, plane_gap=None, guard_rows=8, poison="in"):
    """Embeds the contiguous operand / output tensor t ([rows, cols], or [2, rows, cols] for the two-plane classes) of class cls into a
    larger allocation: leading dimension ld, planes rows * ld + plane_gap elements apart, guard_rows rows before the first and after the
    last row of every plane, data pointer off the allocation's start and 256-byte aligned.  Everything that is not payload is poison:
    "in" = NaN of the plane's format, "out" = a fixed byte pattern.  ld = None: contiguous, as every other test passes its tensors."""
    dtype, bpe, nan = _CLS[cls]
    assert t.dtype == dtype and t.is_contiguous() and t.dim() == 1 + len(bpe)
    rows, cols = t.shape[-2:]
    a = Arena()
    a.cls, a.rows, a.cols, a.shape, a.dtype = cls, rows, cols, tuple(t.shape), dtype
    contiguous = ld is None
    if contiguous:
        ld, plane_gap, guard_rows = cols, 0, 0
    elif plane_gap is None:
        plane_gap = 64 * ld
    assert ld >= cols and (contiguous or ld % 4 == 0) and 2 * plane_gap >= guard_rows * ld * sum(bpe)
    a.ld, a.plane = ld, (rows * ld + plane_gap if len(bpe) == 2 else 0)
    a.base = 0 if contiguous else -(-(guard_rows * ld * bpe[0] + 1) // 256) * 256
    last = len(bpe) - 1
    end = 2 * a.plane * last + rows * ld * (2 if contiguous and last else bpe[last])     # (a contiguous tensor's planes are 16-bit storage)
    total = a.base + end + (0 if contiguous else guard_rows * ld * bpe[last] + TAIL)
    total = -(-total // 256) * 256 if not contiguous else total
    dev = t.device
    a.buf = torch.empty(total, dtype=torch.uint8, device=dev)
    if poison == "in":
        cut = a.base + 2 * a.plane - guard_rows * ld * bpe[1] if last else total
        for lo, hi, fmt in ((0, cut, nan[0]), (cut, total, nan[last])):
            if hi > lo:
                pz = _NAN[fmt]
                assert lo % 4 == 0 and (hi - lo) % len(pz) == 0
                a.buf[lo:hi].view(-1, len(pz)).copy_(torch.tensor(pz, dtype=torch.uint8, device=dev))
    else:
        a.buf.copy_(_pattern(total, dev))
    a.mask = torch.zeros(total, dtype=torch.bool, device=dev)
    for p in range(len(bpe)):
        a.seg(p).copy_(_plane_bytes(t, cls, p))
        a.seg(p, a.mask).fill_(True)
    a.pristine = a.buf.clone()
    assert a.base % 256 == 0 and (contiguous or a.base > 0)
    return a


def lift(a):
    """the payload of an arena as the contiguous tensor place() was given"""
    out = torch.zeros(a.shape, dtype=a.dtype, device=a.buf.device)
    for p in range(len(_CLS[a.cls][1])):
        _plane_bytes(out, a.cls, p).copy_(a.seg(p))
    return out


def untouched(a, what="arena"):
    """every non-payload byte still holds what place() put there"""
    bad = (a.buf != a.pristine) & ~a.mask
    if bool(bad.any()):
        off = int(bad.nonzero()[0]) - a.base
        raise AssertionError(f"{what} ({a.cls}, ld {a.ld}, plane {a.plane}): {int(bad.sum())} bytes outside the payload changed, "
                             f"the first at byte {off} from the data pointer")


def blank(cls, rows, cols, device):
    """prefill of a pure output: a byte pattern over the payload (the same for the contiguous and the arena run)"""
    dtype, bpe, _ = _CLS[cls]
    t = torch.zeros((2, rows, cols) if len(bpe) == 2 else (rows, cols), dtype=dtype, device=device)
    for p in range(len(bpe)):
        v = _plane_bytes(t, cls, p)
        v.copy_(_pattern(v.numel(), device, 113, 29 + p).reshape(v.shape))
    return t


# ------------------------------------------------------------------------------------------------------------------ host tests
def _sample(cls, rows, cols):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(rows, cols, generator=g)
    if cls in ("f16c8", "f16c8_w"):
        e = hip_ops.f16c8_qexp(x) if cls == "f16c8_w" else 0
        return hip_ops.f16c8_encode(x, e, cls == "f16c8_w"), e
    if cls == "f32":
        return x.contiguous(), 0
    return hip_ops.to_operand(x, cls), 0


@pytest.mark.parametrize("cls", sorted(_CLS))
def test_arena_round_trip(cls):
    rows, cols = 37, 96
    t, e = _sample(cls, rows, cols)
    for poison in ("in", "out"):
        a = place(t, cls, cols + 32, poison=poison)
        assert a.base > 0 and a.base % 256 == 0 and a.ld == cols + 32
        if len(_CLS[cls][1]) == 2:
            assert a.plane == rows * a.ld + 64 * a.ld and a.plane % 8 == 0
        assert torch.equal(lift(a).view(torch.uint8), t.view(torch.uint8))
        untouched(a)
        assert int(a.mask.sum()) == rows * cols * sum(_CLS[cls][1])
    assert torch.equal(lift(place(t, cls)).view(torch.uint8), t.view(torch.uint8))
    if cls in ("f16c8", "f16c8_w"):
        for x, y in zip(hip_ops.f16c8_decode(lift(place(t, cls, cols + 32)), e, cls == "f16c8_w"), hip_ops.f16c8_decode(t, e, cls == "f16c8_w")):
            assert torch.equal(x, y)


@pytest.mark.parametrize("cls", ["fp16", "f16x3", "fp8", "f32"])
def test_arena_input_poison_is_nan(cls):
    t, _ = _sample(cls, 5, 64)
    a = place(t, cls, 96)
    pad = a.buf[~a.mask]
    pad = pad[: pad.numel() // 4 * 4].view(_CLS[cls][0]).float()
    assert bool(torch.isnan(pad).all())


@pytest.mark.parametrize("cls", ["bf16x3", "f16c8", "f16c8_w", "f32"])
def test_untouched_sees_one_flipped_byte(cls):
    rows, cols, ld = 9, 64, 96
    t, _ = _sample(cls, rows, cols)
    bpe = _CLS[cls][1]
    a = place(t, cls, ld, poison="out")
    last = len(bpe) - 1
    spots = {"guard row in front": a.base - 3,
             "guard row behind": a.base + 2 * a.plane * last + rows * ld * bpe[last] + 5,
             "row padding of the last row": a.base + 2 * a.plane * last + (rows - 1) * ld * bpe[last] + cols * bpe[last] + 1}
    if last:
        spots["gap between the planes"] = a.base + rows * ld * bpe[0] + (2 * a.plane - rows * ld * bpe[0]) // 2
    for name, off in spots.items():
        assert not bool(a.mask[off]), name
        a.buf[off] ^= 0x10
        with pytest.raises(AssertionError, match="outside the payload"):
            untouched(a)
        a.buf[off] ^= 0x10
        untouched(a)
    a.buf[a.base] ^= 0x10                              # a payload byte is not the guard's business
    untouched(a)


# ------------------------------------------------------------------------------------------------------------------ GPU side
LIN = ["bf16", "fp16", "bf16x3", "f16x3", "fp8"]                     # the classes of gemm.hip
# operand rounding of the class (tests/test_gpu_ops.py: EPS; e4m3 as in test_gemm_block_sized; F16C8 keeps hi + lo to ~2^-15)
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -15, "f16x3": 2.0 ** -20, "fp8": 2.0 ** -4, "f16c8": 2.0 ** -15}
_OUT_CLS = {1: "f32", 2: "fp16", 3: "bf16", 4: "bf16x3", 5: "f16x3"}
RPG = (256, 261, 5)
SHAPE, ALIGN = -1, -3                                                # BD_ERR_SHAPE, BD_ERR_ALIGN


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _needs_256_cus():
    """for tables of shapes worked out by hand for 256 CUs (tests/test_gpu_range.py); the launches still assert their form through the plan"""
    if _cus() != 256:
        pytest.skip("the shapes of this table are worked out for 256 CUs")


def _rows(prec, N, K, ok, prefer, **fields):
    """The row count of a test that is about one launch form: `prefer` (the count worked out for 256 CUs) if this device's plan gives
    it that form -- ok(hip_ops.gemm_plan(..)) -- else the nearest count with a ragged last tile (128 j + 44) whose plan does."""
    if prec == "fp8":
        fields["wscale"] = True
    for M in [prefer] + sorted((128 * j + 44 for j in range(2, 600)), key=lambda m: abs(m - prefer)):
        if ok(hip_ops.gemm_plan(hip_ops.gemm_shape_args(M, N, K, **fields), prec)):
            return M
    pytest.fail(f"no row count gives {prec} N {N} K {K} the form under test on {_cus()} CUs")


def _is(plan, *launches):
    """does a plan consist of these launches (one dict of hip_ops.gemm_plan's fields each)?"""
    return len(plan) == len(launches) and all(all(l[k] == v for k, v in want.items()) for l, want in zip(plan, launches))


PC, LARGE, SMALL = {"family": "pc", "tile": (256, 192)}, {"tile": (256, 192)}, {"tile": (128, 192)}      # gemm.hip's persistent kernel; F16C8's forms


def _randn(shape, std=1.0, seed=3, mean=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * std + mean).contiguous()


def _out_cls(prec, kind):
    return _OUT_CLS.get(kind, prec)


def _value(t, cls):
    """fp64 value of a lifted output"""
    if cls == "f16c8":
        hi, lo, _ = hip_ops.f16c8_decode(t)
        return hi.double() + lo.double()
    return t.float().double() if len(_CLS[cls][1]) == 1 else t[0].double() + t[1].double()



def _same_bits(x, y, what):
    """bytewise equality of two tensors of one shape and type (NaN patterns compare as bytes), naming where they differ"""
    assert x.shape == y.shape and x.dtype == y.dtype, what
    bx, by = x.contiguous().view(torch.uint8).reshape(-1), y.contiguous().view(torch.uint8).reshape(-1)
    if torch.equal(bx, by):
        return
    idx = (bx != by).nonzero().reshape(-1) // x.element_size()
    first, last = int(idx[0]), int(idx[-1])
    raise AssertionError(f"{what}: {idx.numel()} bytes differ, elements {first} .. {last} of shape {tuple(x.shape)}; the first: "
                         f"{x.reshape(-1)[first].float().item()!r} vs {y.reshape(-1)[first].float().item()!r}")



def _gemm(prec, A, W, out, M, N, K, kind, *, bias=None, wscale=None, resid=None, addtab=None, rpg=(0, 0, 0), act=0, w_qexp=0, rms=None,
          ln_emit=None, ln_apply=None, resid_in_op=False, split_k=None, w_row0=0, out_col0=0, expect=None, edit=None, form=None):
    """bd_gemm on arenas: every leading dimension, plane distance and base pointer comes from the arena, not from N / K / rows.
    form: the kernel form the test is about -- bd_gemm_plan on these very arguments must name it (hip_ops._check_expect)."""
    g = _lib.GemmArgs()
    g.A, g.lda, g.a_plane = A.ptr, A.ld, A.plane
    g.W, g.ldw, g.w_plane = W.ptr + w_row0 * W.ld * _CLS[W.cls][1][0], W.ld, W.plane
    g.bias = bias.data_ptr() if bias is not None else None
    g.wscale = wscale.data_ptr() if wscale is not None else None
    if resid is not None:
        g.resid, g.ldr = resid.ptr, resid.ld
    if addtab is not None:
        g.addtab, g.tab_rows = addtab.data_ptr(), addtab.shape[0]
    g.out, g.ldo, g.out_plane, g.out_f32 = out.ptr + out_col0 * _CLS[out.cls][1][0], out.ld, out.plane, kind
    g.M, g.N, g.K, g.act, g.w_qexp = M, N, K, act, int(w_qexp)
    g.rpg_in, g.rpg_out, g.row_off = rpg
    if rms is not None:
        g.rms_wq, g.rms_wk, g.rms_eps, g.rms_parts = rms[0].data_ptr(), rms[1].data_ptr(), 1e-6, rms[2]
    if ln_emit is not None:
        st, op = ln_emit
        g.ln_stats_out, g.ln_op_out, g.ln_op_plane, g.ln_op_ld, g.ln_resid_in_op = st.data_ptr(), op.ptr, op.plane, op.ld, int(resid_in_op)
    if ln_apply is not None:
        g.ln_stats_in, g.ln_colsum, g.ln_eps = ln_apply[0].data_ptr(), ln_apply[1].data_ptr(), ln_apply[2]
    if split_k is not None:
        g.sk_ws, g.sk_split = split_k[0].data_ptr(), split_k[1]
    if edit is not None:
        edit(g)
    lib = _lib.load()
    if form is not None:
        hip_ops._check_expect(g, prec, form)
    if (ln_emit is not None or ln_apply is not None) and expect is None:
        assert lib.bd_gemm_takes_ln_fold(C.byref(g), _lib.prec_id(prec)), "no kernel form with the LayerNorm-fold epilogues"
    rc = lib.bd_gemm(C.byref(g), _lib.prec_id(prec), _lib.stream())
    if expect is None:
        _lib.check(rc, "bd_gemm")
    else:
        assert rc == expect, (rc, expect)


class _Problem:
    """Operands of one Linear as stored, and its fp64 product + bias on exactly those values."""

    def __init__(self, prec, M, N, K, seed=3, w_std=0.05, a_mean=0.0, a_std=1.0, bias=True):
        self.prec, self.M, self.N, self.K = prec, M, N, K
        a, w = _randn((M, K), a_std, seed, a_mean), _randn((N, K), w_std, seed + 1)
        self.a32 = a
        self.b = _randn((N,), 0.1, seed + 2) if bias else None
        self.ws = (torch.rand(N, generator=torch.Generator().manual_seed(5)) + 0.5).cuda() if prec == "fp8" else None
        self.e = 0
        if prec == "f16c8":
            self.e = hip_ops.f16c8_qexp(w)
            self.a_t, self.w_t = hip_ops.f16c8_encode(a, 0, False), hip_ops.f16c8_encode(w, self.e, True)
            ah, al, aq = (t.double() for t in hip_ops.f16c8_decode(self.a_t))
            wh, wl, wq = (t.double() for t in hip_ops.f16c8_decode(self.w_t, self.e, True))
            self.acc = ah @ wh.t() + al @ wq.t() + aq @ wl.t()               # as in test_gemm_f16c8
            self.a_cls, self.w_cls = "f16c8", "f16c8_w"
        else:
            self.a_t, self.w_t = hip_ops.to_operand(a, prec), hip_ops.to_operand(w, prec)
            self.acc = hip_ops.from_operand(self.a_t, prec).double() @ hip_ops.from_operand(self.w_t, prec).double().t()
            self.a_cls = self.w_cls = prec
        if self.ws is not None:
            self.acc = self.acc * self.ws.double()
        self.lin = self.acc + (self.b.double() if bias else 0.0)

    def A(self, arena):
        return place(self.a_t, self.a_cls, self.K + 32 if arena else None)       # lda = K + 32, a_plane = (M + 64) lda

    def W(self, arena):
        return place(self.w_t, self.w_cls, self.K + 32 if arena else None)


def _rms_ref(lin, parts, wq, wk):
    """q/k RMSNorm over 96-wide heads of the first two of `parts` column blocks (test_gemm_fused_qk_rmsnorm)"""
    M, N = lin.shape
    x = lin.reshape(M, parts, -1, 96).clone()
    for i, w in ((0, wq), (1, wk)):
        x[:, i] = w.double() * (x[:, i] * torch.rsqrt(x[:, i].pow(2).mean(-1, keepdim=True) + 1e-6))
    return x.reshape(M, N)


def _rms_w():
    return (_randn((96,), 0.1, 21) + 1), (_randn((96,), 0.1, 22) + 1)


def _run(P, kind, tol, *, act=0, resid=None, ldo=None, ldr=None, rms_parts=None, maptab=False, split=0, form=None):
    """One Linear of problem P, contiguous and on arenas, checked as the module docstring says.  resid: None, "inplace" (resid == out) or
    "separate" (its own arena, ldr); maptab: the row map RPG + an added table (test_gemm_epilogues).  tol(|ref| max) -> bound."""
    prec, M, N, K = P.prec, P.M, P.N, P.K
    cls = _out_cls(prec, kind)
    rows_out = (M // RPG[0]) * RPG[1] if maptab else M
    ldo = ldo if ldo is not None else N + 32
    res = _randn((rows_out, N), 1.0, 31) if resid else None
    tab = _randn((RPG[0], N), 1.0, 32) if maptab else None
    rms = (*_rms_w(), rms_parts) if rms_parts else None
    ref = P.lin
    if act:
        ref = F.gelu(ref)
    if rms:
        ref = _rms_ref(ref, 3, rms[0], rms[1])
    rows = torch.arange(M, device="cuda")
    orow = (rows // RPG[0]) * RPG[1] + rows % RPG[0] + RPG[2] if maptab else rows
    if tab is not None:
        ref = ref + tab[rows % RPG[0]].double()
    if res is not None:
        ref = ref + res[orow].double()
    got = []
    for arena in (False, True):
        A, W = P.A(arena), P.W(arena)
        if resid == "inplace":
            out = place(res, "f32", ldo if arena else None, poison="out")
        else:
            out = place(blank(cls, rows_out, N, "cuda"), cls, ldo if arena else None, poison="out")
        R = out if resid == "inplace" else (place(res, "f32", ldr if arena else None) if resid else None)
        ws = hip_ops.splitk_workspace(M, N) if split else None
        _gemm(prec, A, W, out, M, N, K, kind, bias=P.b, wscale=P.ws, resid=R, addtab=tab, rpg=RPG if maptab else (0, 0, 0), act=act,
              w_qexp=P.e, rms=rms, split_k=(ws, split) if split else None, form=form)
        torch.cuda.synchronize()
        for name, ar in (("A", A), ("W", W), ("out", out), ("resid", R)):
            if ar is not None:
                untouched(ar, f"{name} of the {'arena' if arena else 'contiguous'} run")                 # (c)
        got.append(lift(out))
    _same_bits(got[1], got[0], "arena payload vs the contiguous run")                                 # (b)
    val = _value(got[1], cls)
    if maptab:            # rows the map does not hit keep the caller's bytes
        hit = torch.zeros(rows_out, dtype=torch.bool, device="cuda")
        hit[orow] = True
        first = res if resid == "inplace" else blank(cls, rows_out, N, "cuda")
        _same_bits(got[1][..., ~hit, :], first[..., ~hit, :], "rows outside the row map")
        val = val[orow]
    assert bool(torch.isfinite(val).all()), "poisoned padding reached the result"                       # (d)
    err = (val - ref).abs().max().item()
    bound = tol(max(1.0, ref.abs().max().item()))
    print(f"[views] {prec} {M}x{N}x{K} kind {kind}: err {err:.3e} bound {bound:.3e}")
    assert err < bound, (prec, kind, err, bound)                                                        # (a)
    return got[1]


def _tol_f32(prec, K):
    """fp32 results: test_gemm_plain (operands exact: fp32 accumulation order only; split-bf16 drops lo * lo); e4m3 and every residual
    form of gemm.hip: test_gemm_block_sized's in-place residual bound, which is the wider of the two"""
    if prec == "fp8":
        return lambda m: 2e-4 * K ** 0.5
    return lambda m: 2e-5 * K ** 0.5 + (1e-4 if prec == "bf16x3" else 0.0)


def _tol_16(prec, K, eps=None):
    """16-bit results: K = 128 test_gemm_epilogues (half an operand ulp of the largest value + 2e-4); deeper K and e4m3
    test_gemm_block_sized (eps max(1, |ref|) + 3e-4 sqrt K)"""
    eps = EPS[prec] if eps is None else eps
    if K == 128 and prec != "fp8":
        return lambda m: eps * m + 2e-4
    return lambda m: eps * m + 3e-4 * K ** 0.5


def _tol_rms(eps):
    """test_gemm_fused_qk_rmsnorm"""
    return lambda m: 2 * eps * m + 1e-4


# ---- gemm.hip
@gpu
@pytest.mark.parametrize("prec,kind", [(p, 1) for p in LIN] + [(p, 0) for p in LIN if p != "fp8"])     # (e4m3: fp32 out only -- its 16-bit
def test_one_tile_narrow_epilogue(hip, prec, kind):                                                      # outputs need the wide epilogue)
    """M = 300, N = 204, K = 128: N % 8 != 0, so wide_epilogue_ok fails -- no persistent kernel (pc192_possible), and the one-tile kernel
    (launch_one_tile: 64 x 64 tiles, e64 wins at 5 x 4 tiles) stores through the scalar epilogue.  ldo = 212."""
    P = _Problem(prec, 300, 204, 128)
    _run(P, kind, _tol_f32(prec, 128) if kind else _tol_16(prec, 128), ldo=212, form={"family": "glds", "tile": (64, 64)})


@gpu
@pytest.mark.parametrize("form", ["gelu16", "f32_resid", "f32_inplace"])
@pytest.mark.parametrize("prec", LIN)
def test_one_tile_wide_epilogue(hip, prec, form):
    """M = 300, N = 200, K = 128: N % 192 != 0 and M < 1024 keep it off the persistent kernel; N % 8 == 0 and ldo = 232 (% 8 == 0) take the
    LDS-staged 16-byte epilogue of the one-tile kernel.  The residual of f32_resid lives in its own arena with ldr = 264 != ldo."""
    P = _Problem(prec, 300, 200, 128)
    if form == "gelu16":
        _run(P, 0, _tol_16(prec, 128), act=1, ldo=232, form={"family": "glds"})
    else:
        tol = (lambda m: 2e-4 * 128 ** 0.5) if prec == "fp8" else (lambda m: 3e-4)        # test_gemm_epilogues' residual form
        _run(P, 1, tol, resid="inplace" if form == "f32_inplace" else "separate", ldo=232, ldr=264, form={"family": "glds"})


@gpu
@pytest.mark.parametrize("prec", LIN)
def test_row_map_and_table_in_place(hip, prec):
    """test_gemm_epilogues' row map + table + in-place residual (M = 512, N = 256, K = 128, rpg = (256, 261, 5)) with ldo = ldr = 288:
    a.rpg_in > 0 selects the generic epilogue on every kernel; rows the map does not hit stay bytewise."""
    P = _Problem(prec, 512, 256, 128)
    tol = (lambda m: 2e-4 * 128 ** 0.5) if prec == "fp8" else (lambda m: 3e-4)            # test_gemm_epilogues
    _run(P, 1, tol, resid="inplace", ldo=288, maptab=True)


@gpu
@pytest.mark.parametrize("prec,form", [(p, f) for p in LIN for f in ("plain", "rms", "alt_rms") if f != "alt_rms" or p not in ("bf16", "fp16")])
def test_persistent_192_16bit_outputs(hip, prec, form):
    """N = 2304, K = 768 in ONE launch of the persistent 256 x 192 kernel (M = 4000 on 256 CUs: 16 x 12 = 192 tiles, 0.75 of one round).
    plain -> EP 1, fused q/k RMSNorm (8 heads x 96) -> EP 2; alt_rms: the
    non-native 16-bit kind of the class (2 = f16 plane from the split classes, 3 = bf16 plane from e4m3; the plain classes have none).  ldo = 2336."""
    kind = 0 if form != "alt_rms" else (3 if prec == "fp8" else 2)
    eps = EPS[prec] if kind == 0 else (2.0 ** -8 if kind == 3 else 2.0 ** -11)
    want = {**PC, "ep": 1 if form == "plain" else 2, "outk": kind}
    rms = {} if form == "plain" else {"rms_wq": True, "rms_wk": True, "rms_parts": 3}
    M = _rows(prec, 2304, 768, lambda plan: _is(plan, want), 4000, out_f32=kind, **rms)
    P = _Problem(prec, M, 2304, 768)
    _run(P, kind, _tol_rms(eps) if form != "plain" else _tol_16(prec, 768, eps), rms_parts=0 if form == "plain" else 3, form=want)


@gpu
@pytest.mark.parametrize("prec", LIN)
def test_persistent_192_narrow_output_in_place(hip, prec):
    """N = 768, K = 768, fp32 + residual in place (EP 3) in ONE launch of the persistent kernel with a ragged last row tile: on 256 CUs the
    tiles must fill 0.45 of their rounds, M = 7300 is 29 x 4 = 116 tiles in one round (M = 4000 goes to the one-tile kernels).
    ldo = ldr = 800."""
    want = {**PC, "ep": 3}
    M = _rows(prec, 768, 768, lambda plan: _is(plan, want), 7300, out_f32=1, resid=True)
    assert M % 256
    P = _Problem(prec, M, 768, 768)
    _run(P, 1, lambda m: (4e-4 if prec == "bf16x3" else 2e-4) * 768 ** 0.5, resid="inplace", ldo=800, form=want)       # test_gemm_block_sized, in place


@gpu
@pytest.mark.parametrize("form", ["tail_rows", "hybrid", "two_rounds_separate_resid"])
@pytest.mark.parametrize("prec", LIN)
def test_two_launch_forms(hip, prec, form):
    """Two launches over disjoint row ranges: the second one's A, out and resid are re-based by row0 * lda / ldo / ldr.  On 256 CUs:
    tail_rows: M = 16500, N = 768, K = 128 -- 65 x 4 = 260 tiles, a second round of 4: 16384 rows on the persistent kernel + 116 rows on
      the one-tile kernels.  In place, lda = 160, ldo = ldr = 800.
    hybrid: M = 16500, N = 1024, K = 2048 -- no persistent kernel (N % 192 != 0); one round of 256 x 256 tiles (64 row tiles x 4) over
      16384 rows + 128 x 128 tiles over 116 rows.  In place, ldo = ldr = 1056.
    two_rounds_separate_resid: M = 33000, N = 768, K = 128 -- 32768 rows = two tiles for every workgroup of the persistent kernel, so
      every workgroup prefetches the residual of a NEXT tile, + 232 rows; the residual has its own arena with ldr = 832 != ldo = 800."""
    tail = lambda plan: _is(plan, {**PC, "ep": 3, "row0": 0}, {"family": "glds"}) and plan[1]["row0"] == plan[0]["rows"]
    if form == "tail_rows":
        M = _rows(prec, 768, 128, tail, 16500, out_f32=1, resid=True)
        _run(_Problem(prec, M, 768, 128), 1, lambda m: (4e-4 if prec == "bf16x3" else 2e-4) * 128 ** 0.5, resid="inplace", ldo=800,
             form=[{**PC, "ep": 3}, {"family": "glds"}])
    elif form == "hybrid":
        want = [{"family": "glds", "tile": (256, 256), "row0": 0}, {"family": "glds", "tile": (128, 128)}]
        M = _rows(prec, 1024, 2048, lambda plan: _is(plan, *want) and plan[1]["row0"] == plan[0]["rows"], 16500, out_f32=1, resid=True)
        _run(_Problem(prec, M, 1024, 2048), 1, lambda m: (4e-4 if prec == "bf16x3" else 2e-4) * 2048 ** 0.5, resid="inplace", ldo=1056, form=want)
    else:
        two = lambda plan: tail(plan) and plan[0]["rows"] // 256 * 4 == 2 * plan[0]["grid"]
        M = _rows(prec, 768, 128, two, 33000, out_f32=1, resid=True)
        _run(_Problem(prec, M, 768, 128), 1, lambda m: (4e-4 if prec == "bf16x3" else 2e-4) * 128 ** 0.5, resid="separate", ldo=800, ldr=832,
             form=[{**PC, "ep": 3}, {"family": "glds"}])


@gpu
@pytest.mark.parametrize("M", [300, 4000])
@pytest.mark.parametrize("prec", LIN)
def test_column_offset_output(hip, prec, M):
    """out = buf + c0 with ldo = 3 N for c0 in {0, N, 2 N} inside one [M, 3 N] buffer (N = 768, K = 128; operand-class output, bf16 plane
    from e4m3): the other two column blocks, the guard rows and the plane gap stay bytewise."""
    N, K = 768, 128
    P = _Problem(prec, M, N, K)
    kind = 3 if prec == "fp8" else 0
    cls = _out_cls(prec, kind)
    ref = P.lin
    for c0 in (0, N, 2 * N):
        got = []
        for arena in (False, True):
            A, W = P.A(arena), P.W(arena)
            if arena:
                first = blank(cls, M, 3 * N, "cuda")
                out = place(first, cls, 3 * N, plane_gap=64 * 3 * N, poison="out")
                _gemm(prec, A, W, out, M, N, K, kind, bias=P.b, wscale=P.ws, out_col0=c0)
            else:
                out = place(blank(cls, M, N, "cuda"), cls, poison="out")
                _gemm(prec, A, W, out, M, N, K, kind, bias=P.b, wscale=P.ws)
            torch.cuda.synchronize()
            for ar in (A, W, out):
                untouched(ar, f"c0 = {c0}")
            got.append(lift(out))
        block = got[1][..., c0:c0 + N].contiguous()
        _same_bits(block, got[0], f"column block at c0 = {c0} vs the contiguous run")
        keep = torch.ones(3 * N, dtype=torch.bool, device="cuda")
        keep[c0:c0 + N] = False
        _same_bits(got[1][..., keep], first[..., keep], f"column blocks next to c0 = {c0}")
        val = _value(block, cls)
        assert bool(torch.isfinite(val).all())
        err = (val - ref).abs().max().item()
        assert err < _tol_16(prec, K, 2.0 ** -8 if kind == 3 else None)(max(1.0, ref.abs().max().item())), (prec, c0, err)


# ---- gemm_f16c8.hip (every case: activation arena with lda = K + 32, a_plane = (M + 64) lda)
D = 768


def _stats_of(x):
    """(mean, M2) per 96-column group of fp32 rows, as the producer writes them (tests/test_gpu_lnfold.py)"""
    xd = x.double().reshape(x.shape[0], 8, 96)
    mean = xd.mean(-1)
    return torch.stack([mean, ((xd - mean[..., None]) ** 2).sum(-1)], -1).float().contiguous()


def _fold_ref(acc, x, s, bias, eps):
    """rstd (acc - mean s) + bias with the row statistics of x (test_consumer_f16c8_applies_row_statistics)"""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + eps)
    return rstd * (acc - mean * s.double()[None, :]) + bias.double()[None, :]


@gpu
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("M", [1536, 8400])
def test_f16c8_v_columns_of_a_split_qkv(hip, M, fold):
    """forward.hip's qk16_v_lin: ONE [3 D, K] weight encoded once; the launch takes W + 2 D rows with w_plane still the full weight's,
    bias + 2 D (ln_colsum + 2 D with the LayerNorm-fold consumer), N = D, out = qkv + 2 D columns with ldo = 3 D, an f16 plane (kind 2).
    M = 1536: the small form (on 256 CUs: 6 x 4 = 24 large tiles, 2 x 24 <= 256); M = 8400: the large form (33 x 4 = 132 tiles).
    The reference is columns [2 D, 3 D) of the full product; columns [0, 2 D) of qkv stay bytewise."""
    K, eps = 768, 1e-5
    want = {**(SMALL if M == 1536 else LARGE), "ep": 1, "outk": 2, "lnf": fold}
    M = _rows("f16c8", D, K, lambda plan: _is(plan, want), M, out_f32=2, **({"ln_stats_in": True, "ln_colsum": True} if fold else {}))
    P = _Problem("f16c8", M, 3 * D, K, seed=5, w_std=0.04, a_mean=0.4 if fold else 0.0, a_std=1.5 if fold else 1.0)
    wh, wl, _ = hip_ops.f16c8_decode(P.w_t, P.e, True)
    s = (wh.double() + wl.double()).sum(1).float().contiguous()
    st = _stats_of(P.a32)
    ref = (_fold_ref(P.acc, P.a32, s, P.b, eps) if fold else P.lin)[:, 2 * D:]
    first = blank("fp16", M, 3 * D, "cuda")
    got = []
    for arena in (False, True):
        A, W = P.A(arena), P.W(arena)
        out = place(first, "fp16", 3 * D if arena else None, poison="out")
        _gemm("f16c8", A, W, out, M, D, K, 2, bias=P.b[2 * D:], w_qexp=P.e, w_row0=2 * D, out_col0=2 * D,
              ln_apply=(st, s[2 * D:], eps) if fold else None, form=want)
        torch.cuda.synchronize()
        for ar in (A, W, out):
            untouched(ar)
        got.append(lift(out))
    _same_bits(got[1], got[0], "arena payload vs the contiguous run")
    _same_bits(got[1][:, :2 * D], first[:, :2 * D], "the q, k columns next to the v block")
    val = got[1][:, 2 * D:].double()
    assert bool(torch.isfinite(val).all())
    err, m = (val - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    # test_gemm_f16c8, f16 plane: 2^-10 max(1, |ref|); with the fold test_consumer_f16c8_applies_row_statistics ("f16"): 2^-10 |y| + 2e-4
    assert err < (2.0 ** -10 * ref.abs().max().item() + 2e-4 if fold else 2.0 ** -10 * m), (M, fold, err)


@gpu
@pytest.mark.parametrize("fold", [False, True])
def test_f16_qk_columns_on_plane_0_of_an_f16c8_operand(hip, fold):
    """forward.hip's qkv_lin with qk16: an F16 launch whose A is plane 0 of an F16C8 arena (lda = K + 32), N = 2 D, ldo = 3 D,
    rms_parts = 2 (the fused q/k RMSNorm pins the persistent 256 x 192 kernel, EP 2).  M = 1536.  The v block stays bytewise."""
    M, K, eps = 1536, 768, 1e-5
    x = _randn((M, K), 1.5, 9, 0.4)
    a_t = hip_ops.f16c8_encode(x, 0, False)
    w16 = (_randn((2 * D, K), 0.04, 10)).half().contiguous()
    b = _randn((2 * D,), 0.3, 11)
    s = w16.double().sum(1).float().contiguous()
    st = _stats_of(x)
    wq, wk = _rms_w()
    acc = a_t[0].double() @ w16.double().t()
    ref = _rms_ref(_fold_ref(acc, x, s, b, eps) if fold else acc + b.double(), 2, wq, wk)
    first = blank("fp16", M, 3 * D, "cuda")
    got = []
    for arena in (False, True):
        A = place(a_t, "f16c8", K + 32 if arena else None)
        W = place(w16, "fp16", K + 32 if arena else None)
        out = place(first, "fp16", 3 * D if arena else None, poison="out")
        _gemm("fp16", A, W, out, M, 2 * D, K, 0, bias=b, rms=(wq, wk, 2), ln_apply=(st, s, eps) if fold else None,
              form={**PC, "ep": 2, "lnf": fold})
        torch.cuda.synchronize()
        for ar in (A, W, out):
            untouched(ar)
        got.append(lift(out))
    _same_bits(got[1], got[0], "arena payload vs the contiguous run")
    _same_bits(got[1][:, 2 * D:], first[:, 2 * D:], "the v block next to the q, k columns")
    val = got[1][:, :2 * D].double()
    assert bool(torch.isfinite(val).all())
    err, m = (val - ref).abs().max().item(), ref.abs().max().item()
    # test_gemm_fused_qk_rmsnorm_two_parts: 2 x 2^-11 max(1, |ref|) + 1e-4; with the fold test_consumer_f16_qk_launch: 2^-10 |y| + 1e-4
    assert err < (2.0 ** -10 * m + 1e-4 if fold else 2 * 2.0 ** -11 * max(1.0, m) + 1e-4), (fold, err)


@gpu
@pytest.mark.parametrize("form", ["plain", "gelu", "split_bf16", "split_f16"])
def test_f16c8_operand_class_outputs(hip, form):
    """M = 300, N = 3072, K = 768, ldo = N + 32: EP 1 (2 x 16 = 32 large tiles: on 64 CUs or more the small form).  The operand-class output's lo8 plane is rows
    of ldo BYTES; kinds 4 / 5 (split-bf16 / split-f16 planes) with out_plane = (M + 64) ldo > M ldo (kind 5 takes the generic epilogue)."""
    P = _Problem("f16c8", 300, 3072, 768)
    K = 768
    if form in ("plain", "gelu"):
        # test_gemm_f16c8, operand-class output (hi + lo against the exact value)
        _run(P, 0, lambda m: 4e-4 * m * 2.0 ** -4 + 2e-5, act=int(form == "gelu"), form={"ep": 1, "outk": 0, "gelu": form == "gelu", "stages": 3})
    elif form == "split_bf16":
        _run(P, 4, lambda m: 2.0 ** -15 * m + 2e-5 * K ** 0.5, form={"ep": 1, "outk": 4, "stages": 3})        # test_gemm_f16c8, kind 4
    else:
        _run(P, 5, lambda m: 2.0 ** -20 * m + 2e-5 * K ** 0.5, form={"ep": 0, "stages": 3})        # test_gemm_f16c8, kind 5


@gpu
@pytest.mark.parametrize("form,M,K,split", [("inplace", 4000, 768, 0), ("separate", 16500, 768, 0), ("inplace", 1536, 3072, 0),
                                            ("inplace", 300, 768, 2), ("inplace", 300, 768, 3), ("inplace", 300, 768, 4)])
def test_f16c8_fp32_residual_forms(hip, form, M, K, split):
    """N = 768, fp32 + residual (EP 3), ldo = 800; in place (ldr = ldo) or the residual in its own arena with ldr = 832.
    M = 4000: the small form (on 256 CUs: 16 x 4 = 64 tiles).  M = 16500: the large form with more tiles than workgroups (65 x 4 = 260 on
    256), so the first workgroups prefetch a NEXT tile's residual rows.  K = 3072, M = 1536: the 128 x 96 form (24 large tiles, deep K).
    M = 300 with a split-K workspace and a forced factor 2 / 3 / 4: compared with the contiguous launch of the same factor."""
    if split:
        want, ok = {"tile": (128, 96), "ep": 3, "split_k": split}, None
    elif K == 3072:
        want, ok = {"tile": (128, 96), "ep": 3, "split_k": 1}, None
    elif M == 4000:
        want, ok = {**SMALL, "ep": 3}, None
    else:
        want, ok = {**LARGE, "ep": 3}, lambda plan: _is(plan, want) and -(-plan[0]["rows"] // 256) * 4 > plan[0]["grid"]
    if not split:
        M = _rows("f16c8", 768, K, ok or (lambda plan: _is(plan, want)), M, out_f32=1, resid=True)
    P = _Problem("f16c8", M, 768, K, w_std=0.03)
    _run(P, 1, lambda m: 2e-5 * K ** 0.5 + 1e-6, resid=form, ldo=800, ldr=832, split=split, form=want)           # test_gemm_f16c8, in-place residual


@gpu
@pytest.mark.parametrize("M", [300, 1536])
@pytest.mark.parametrize("ep", [4, 5, "5_f32"])
def test_f16c8_layernorm_fold_producer(hip, ep, M):
    """The producer epilogues with ln_op_ld = 800 and ln_op_plane = (M + 64) 800: EP 4 (fp32 rows + residual in place, ldo = ldr = 800, the
    rows' F16C8 copy and their (mean, M2) pairs) and EP 5 (the residual read from and written back to the copy; fp32 rows only on request,
    `out` otherwise ignored -- its arena must stay untouched as a whole).  The copy's padding, both planes, stays bytewise; copy and
    statistics against the references of tests/test_gpu_lnfold.py."""
    N, K = 768, 768
    P = _Problem("f16c8", M, N, K, seed=7, w_std=0.04)
    x0 = _randn((M, N), 2.0, 8, 0.7)
    x0_t = hip_ops.f16c8_encode(x0, 0, False)
    r5 = ep != 4
    f32 = ep != 5
    res = (hip_ops.from_operand(x0_t, "f16c8") if r5 else x0).double()
    ref = P.lin + res
    got = []
    for arena in (False, True):
        A, W = P.A(arena), P.W(arena)
        op = place(x0_t if r5 else blank("f16c8", M, N, "cuda"), "f16c8", 800 if arena else None, poison="out")
        if r5:
            out = place(blank("f32" if f32 else "f16c8", M, N, "cuda"), "f32" if f32 else "f16c8", 800 if arena else None, poison="out")
        else:
            out = place(x0, "f32", 800 if arena else None, poison="out")
        st = torch.full((M, 8, 2), float("nan"), dtype=torch.float32, device="cuda")
        _gemm("f16c8", A, W, out, M, N, K, int(f32), bias=P.b, w_qexp=P.e, resid=None if r5 else out, ln_emit=(st, op), resid_in_op=r5,
              form={"ep": 5 if r5 else 4, "outk": int(f32), "stages": 3})
        torch.cuda.synchronize()
        for name, ar in (("A", A), ("W", W), ("out", out), ("operand copy", op)):
            untouched(ar, name)
        if not f32:
            assert torch.equal(out.buf, out.pristine), "`out` is ignored in this form"
        got.append((lift(out), lift(op), st))
    for x, y in zip(got[0], got[1]):
        _same_bits(y, x, "arena run vs the contiguous run (fp32 rows, operand copy, statistics)")
    o32, opc, st = got[1]
    val = _value(opc, "f16c8")
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(st).all())
    if f32:
        assert (o32.double() - ref).abs().max().item() <= 2e-5 * K ** 0.5 + 1e-5       # test_producer_with_the_residual_in_the_operand_copy
        _same_bits(opc, hip_ops.f16c8_encode(o32, 0, False), "the operand copy vs the reference packing of the fp32 rows")
        xd = o32.double()
    else:
        # the copy is the reference packing of fp32 rows nobody wrote: within the class's rounding of the exact sum
        assert (val - ref).abs().max().item() <= 2e-5 * K ** 0.5 + 1e-5 + 2.0 ** -15 * ref.abs().max().item()
        xd = val
    xg = xd.reshape(M, 8, 96)
    mean = xg.mean(-1)
    m2 = ((xg - mean[..., None]) ** 2).sum(-1)
    if f32:                                                # test_producer_emits_operand_copy_and_row_statistics
        assert (st[..., 0].double() - mean).abs().max().item() <= 2e-6 * float(xg.abs().max())
        assert ((st[..., 1].double() - m2).abs() / m2.clamp_min(1e-3)).max().item() <= 2e-5


@gpu
@pytest.mark.parametrize("K", [128, 192])
def test_f16c8_generic_epilogue(hip, K):
    """N = 200 (N % 192 != 0 -> EP 0), row map + table + in-place residual as in test_row_map_and_table_in_place, ldo = ldr = 232.
    K = 128: K / 32 = 4 slabs, not a multiple of 3 -> the two-stage ring; K = 192: 6 slabs -> the three-stage ring."""
    P = _Problem("f16c8", 512, 200, K, w_std=0.03)
    _run(P, 1, lambda m: 2e-5 * K ** 0.5 + 1e-6, resid="inplace", ldo=232, maptab=True, form={"ep": 0, "stages": 3 if K == 192 else 2})               # test_gemm_f16c8, in-place residual


# ---- bd_layernorm
@gpu
@pytest.mark.parametrize("variant", ["affine", "plain", "gathered"])
@pytest.mark.parametrize("cols", [768, 1024, 64])
@pytest.mark.parametrize("prec", LIN + ["f16c8"])
def test_layernorm_on_arenas(hip, prec, cols, variant):
    """bd_layernorm shares the fp32 -> operand store code.  x with ldx = cols + 4 (NaN padding), the fp32 copy with ldo = cols + 4, the
    operand copy compact (its rows are `cols` apart by contract) with out16_plane = (rows + 64) cols and guard rows; 1001 rows, or 768
    rows gathered with rpg = (256, 261, 5).  Reference and tolerance as test_layernorm."""
    eps = 1e-5 if variant == "affine" else 1e-6
    x = _randn((1001, cols), 2.0, 41, 0.3)
    g = _randn((cols,), 0.1, 42, 1.0) if variant == "affine" else None
    b = _randn((cols,), 0.1, 43) if variant == "affine" else None
    rows, rpg = (768, RPG) if variant == "gathered" else (1001, (0, 0, 0))
    idx = torch.arange(rows, device="cuda")
    src = (idx // 256) * 261 + idx % 256 + 5 if variant == "gathered" else idx
    ref = F.layer_norm(x[src].double(), (cols,), g.double() if g is not None else None, b.double() if b is not None else None, eps)
    lib = _lib.load()
    got = []
    for arena in (False, True):
        X = place(x, "f32", cols + 4 if arena else None, guard_rows=8)
        o16 = place(blank(prec, rows, cols, "cuda"), prec, cols if arena else None, plane_gap=64 * cols, poison="out")
        o32 = place(blank("f32", rows, cols, "cuda"), "f32", cols + 4 if arena else None, poison="out")
        _lib.check(lib.bd_layernorm(X.ptr, X.ld, g.data_ptr() if g is not None else None, b.data_ptr() if b is not None else None, eps,
                                    o16.ptr, o16.plane, o32.ptr, o32.ld, rows, cols, *rpg, _lib.prec_id(prec), _lib.stream()), "bd_layernorm")
        torch.cuda.synchronize()
        for name, ar in (("x", X), ("out16", o16), ("out32", o32)):
            untouched(ar, name)
        got.append((lift(o16), lift(o32)))
    for x_, y_ in zip(got[0], got[1]):
        _same_bits(y_, x_, "arena run vs the contiguous run")
    v16, v32 = _value(got[1][0], prec), got[1][1].double()
    assert bool(torch.isfinite(v16).all()) and bool(torch.isfinite(v32).all())
    assert (v32 - ref).abs().max().item() < 2e-5                                   # test_layernorm
    assert (v16 - ref).abs().max().item() < 8 * EPS[prec] + 1e-5                   # test_layernorm


# ---- refusals
@gpu
@pytest.mark.parametrize("prec", ["bf16", "f16x3", "f16c8"])
def test_refusals_come_before_any_launch(hip, prec):
    """Misaligned lda / ldw / planes: BD_ERR_ALIGN; F16C8 lda % 32 or ldo % 32: BD_ERR_SHAPE; a leading dimension below the row length
    (lda < K, ldw < K, ldo < N, ldr < N with a residual, ln_op_ld < N with a producer): BD_ERR_SHAPE -- rows would overlap.  The return
    code comes from host arithmetic alone and the output arena stays bytewise, payload included."""
    M, N, K = 300, 768, 768
    P = _Problem(prec, M, N, K)
    A, W = P.A(True), P.W(True)
    cls = _out_cls(prec, 0)
    out = place(blank(cls, M, N, "cuda"), cls, N + 32, poison="out")
    o32 = place(blank("f32", M, N, "cuda"), "f32", N + 32, poison="out")
    R = place(_randn((M, N)), "f32", N + 32)

    def set_(**kw):
        def edit(g):
            for k, v in kw.items():
                setattr(g, k, v)
        return edit

    cases = [(out, 0, set_(lda=K + 4), ALIGN), (out, 0, set_(ldw=K + 4), ALIGN),
             (out, 0, set_(lda=K - 64), SHAPE), (out, 0, set_(ldw=K - 64), SHAPE), (out, 0, set_(ldo=N - 32), SHAPE),
             (o32, 1, set_(ldr=N - 32), SHAPE), (o32, 1, set_(ldo=N - 32, ldr=N + 32), SHAPE)]
    if prec != "bf16":
        cases += [(out, 0, set_(a_plane=A.plane + 4), ALIGN), (out, 0, set_(w_plane=W.plane + 4), ALIGN)]
    if prec == "f16c8":
        cases += [(out, 0, set_(lda=K + 8), SHAPE), (out, 0, set_(ldw=K + 8), SHAPE), (out, 0, set_(ldo=N + 8), SHAPE)]
    for o, kind, edit, want in cases:
        _gemm(prec, A, W, o, M, N, K, kind, bias=P.b, w_qexp=P.e, resid=R if kind else None, edit=edit, expect=want)
    if prec == "f16c8":
        st = torch.zeros((M, 8, 2), dtype=torch.float32, device="cuda")
        op = place(blank("f16c8", M, N, "cuda"), "f16c8", N + 32, poison="out")
        _gemm(prec, A, W, o32, M, N, K, 1, bias=P.b, w_qexp=P.e, resid=R, ln_emit=(st, op), edit=set_(ln_op_ld=N - 32), expect=SHAPE)
        assert torch.equal(op.buf, op.pristine) and not bool(st.any())
    torch.cuda.synchronize()
    for ar in (out, o32, R, A, W):
        assert torch.equal(ar.buf, ar.pristine)
