"""The token-row entries of csrc/layout.hip called directly: bd_write_prefix_tokens, bd_query_substitute[_varlen],
bd_gather_query_rows_f32[_varlen], bd_gather_query_tokens[_varlen] (prefix_kernel, query_sub_kernel, gather_rows_f32_kernel,
gather_query_kernel).

They are copies plus one fixed-order add, so the check is BIT equality with torch indexing on the CPU (the substitute's
(query_token + rgb) + pos is two fp32 roundings in that order in torch too).  Every output lives inside a larger buffer filled with
a pattern (fp32: NaNs with distinct payloads, so that a stray copy shows) and every element outside the rows an entry is documented
to write must keep its bits.  The operand gather is compared with hip_ops.to_operand of the gathered fp32 rows in all six operand
formats, values beyond the fp8 / f16 range included (the kernels saturate).  No launch here carries an out-of-range view index or an
empty sample: the varlen forms clamp a query index into its sample, and an empty sample has nothing to clamp to -- the host
entry points refuse it (tested at the end, without a GPU, with the argument refusals)."""
import ctypes
import functools

import pytest
import torch

from boxdreamer_amd import _lib, hip_ops
from boxdreamer_amd.model import BoxDreamer

gpu = pytest.mark.gpu
PAD = 48                                   # guard elements (fp32) / 16-byte-multiple guard bytes either side of an output
N_PREFIX, TPI, P, DIM = 5, 261, 256, 768   # dinov2_vitb14_reg at 224 x 224: cls + 4 registers, 256 patches; BETR's 256 tokens of 768
RAGGED = [1, 17, 3, 1, 6]
EPS = {"bf16x3": 2.0 ** -15, "f16x3": 2.0 ** -20,        # tests/test_gpu_ops.py: EPS (test_im2col_and_patchify's margins: 2 EPS + 1e-7)
       "f16c8": 2.0 ** -16}                               # lo = e4m3(x - f16(x)): 2^-4 of at most half an f16 ulp (2^-12 |x|)
RANGE = {"fp16": 65504.0, "f16x3": 65504.0, "fp8": 448.0, "f16c8": 512.0}      # beyond: saturated (f16c8: lo exact below 512)
BEYOND = [1.0e5, -500.0, 65520.0, 464.0, -1.0e5, 449.0, 7.0e4, -464.0, 500.0, 480.0, 448.0, -448.0, -65520.0, 65504.0, 3.0e9, -3.0e9]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(n, salt=0):
    """n fp32 NaNs with distinct payloads (they repeat after 4M elements), as a host tensor"""
    return ((torch.arange(n, dtype=torch.int64) * 7 + salt) % 0x3FFFFD + 0x7FC00001).to(torch.int32).view(torch.float32)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _query_views(counts, q):
    """the view (of the whole packed batch) each sample's query index selects, with the varlen forms' clamp"""
    vs = _lib.view_starts(counts)
    return [vs[b] + min(max(int(q[b]), 0), c - 1) for b, c in enumerate(counts)]


def _queries(mode, counts):
    if mode == "first":
        return [0] * len(counts)
    if mode == "last":
        return [c - 1 for c in counts]
    return [(3 * b + 1) % c if b % 3 else (c - 1 if b % 2 else 0) for b, c in enumerate(counts)]      # first, last and inner views


# ------------------------------------------------------------------------------------------------------------------ prefix rows

@gpu
@pytest.mark.parametrize("n_images,tpi,n_prefix,dim", [
    (1 * 17, TPI, N_PREFIX, DIM), (32 * 6, TPI, N_PREFIX, DIM), (64 * 1, TPI, N_PREFIX, DIM),       # production
    (1, 1, 1, 4), (3, 7, 7, 20), (5, 9, 2, 8), (7, 3, 1, 1), (2, 300, 5, 4)])
def test_write_prefix_tokens(hip, n_images, tpi, n_prefix, dim):
    """x[n, :n_prefix] = prefix for every image; the patch rows of every image (and the guards) keep their bits.  n_prefix == tpi,
    totals that are no multiple of the 256 threads, dim 1 / 4 / 8 / 20."""
    lib = _lib.load()
    n = n_images * tpi * dim
    host = _sentinel(n + 2 * PAD)
    prefix = _randn((n_prefix, dim), 11 + dim)
    buf, prefix_d = host.cuda(), prefix.cuda()
    x = buf[PAD:PAD + n]
    _lib.check(lib.bd_write_prefix_tokens(_lib.ptr(x), _lib.ptr(prefix_d), n_images, tpi, n_prefix, dim, _lib.stream()),
               "bd_write_prefix_tokens")
    torch.cuda.synchronize()
    want = host.clone()
    want[PAD:PAD + n].view(n_images, tpi, dim)[:, :n_prefix] = prefix
    assert torch.equal(_bits(buf.cpu()), _bits(want))


# ------------------------------------------------------------------------------------------------------------------ query substitute

@functools.lru_cache(maxsize=2)
def _sub_operands(n_views, p, dim):
    """(rgb on the host, rgb on the device) shared by the cases of one shape"""
    rgb = _randn((n_views, p, dim), 5 + n_views + dim)
    return rgb, rgb.cuda()


def _substitute(counts, q, p, dim, varlen, uniform_t=None):
    """Launch on a sentinel-filled x; returns (whole guarded buffer on the device, its host original, rgb, pos, qtok)."""
    lib = _lib.load()
    n_views, B = sum(counts), len(counts)
    n = n_views * p * dim
    host = _sentinel(n + 2 * PAD, salt=3)
    rgb, rgb_d = _sub_operands(n_views, p, dim)
    pos, qtok = _randn((p, dim), 21 + dim, 0.5), _randn((dim,), 22 + dim, 2.0)
    buf, pos_d, qtok_d, qd, vs = host.cuda(), pos.cuda(), qtok.cuda(), _i32(q), _i32(_lib.view_starts(counts))      # (locals: alive until the sync)
    x = buf[PAD:PAD + n]
    if varlen:
        _lib.check(lib.bd_query_substitute_varlen(_lib.ptr(x), _lib.ptr(rgb_d), _lib.ptr(pos_d), _lib.ptr(qtok_d), _lib.ptr(vs), _lib.ptr(qd),
                                                  B, p, dim, _lib.stream()), "bd_query_substitute_varlen")
    else:
        _lib.check(lib.bd_query_substitute(_lib.ptr(x), _lib.ptr(rgb_d), _lib.ptr(pos_d), _lib.ptr(qtok_d), _lib.ptr(qd), B, uniform_t, p, dim,
                                           _lib.stream()), "bd_query_substitute")
    torch.cuda.synchronize()
    return buf, host, rgb, pos, qtok


def _substitute_want(host, counts, q, rgb, pos, qtok, p, dim):
    n_views = sum(counts)
    want = host.clone()
    xv = want[PAD:PAD + n_views * p * dim].view(n_views, p, dim)
    for v in _query_views(counts, q):
        xv[v] = (qtok + rgb[v]) + pos                      # betr.py's association order
    return want


@gpu
@pytest.mark.parametrize("B,T,p,dim,qmode", [
    (1, 17, P, DIM, "last"), (32, 6, P, DIM, "mixed"), (64, 1, P, DIM, "first"),                  # production
    (3, 4, 1, 4, "mixed"), (5, 3, 7, 20, "last"), (2, 6, 3, 8, "first"), (7, 2, 5, 1, "mixed")])
def test_query_substitute(hip, B, T, p, dim, qmode):
    """x[query view of b] = (query_token + rgb) + pos, bit for bit; every other view keeps its sentinel bits.  The varlen form with
    equal view counts gives the same bits as the uniform form."""
    counts = [T] * B
    q = _queries(qmode, counts)
    assert all(0 <= qi < T for qi in q)
    buf, host, rgb, pos, qtok = _substitute(counts, q, p, dim, varlen=False, uniform_t=T)
    want = _substitute_want(host, counts, q, rgb, pos, qtok, p, dim)
    assert torch.equal(_bits(buf.cpu()), _bits(want))
    buf_v = _substitute(counts, q, p, dim, varlen=True)[0]
    assert torch.equal(_bits(buf_v), _bits(buf))


@gpu
@pytest.mark.parametrize("p,dim", [(P, DIM), (3, 20)])
@pytest.mark.parametrize("q", [[0, 0, 0, 0, 0], [0, 16, 2, 0, 5], [0, 9, 1, 0, 3], [-1, 99, 3, 1, -7]])
def test_query_substitute_ragged(hip, p, dim, q):
    """View counts [1, 17, 3, 1, 6]: first, last and inner query views; q < 0 takes the sample's view 0 and q >= n its view n - 1
    (query_view_of's clamp), never a neighbour's."""
    if q[0] < 0:
        assert _query_views(RAGGED, q) == [0, 17, 20, 21, 22]
    buf, host, rgb, pos, qtok = _substitute(RAGGED, q, p, dim, varlen=True)
    want = _substitute_want(host, RAGGED, q, rgb, pos, qtok, p, dim)
    assert torch.equal(_bits(buf.cpu()), _bits(want))


# ------------------------------------------------------------------------------------------------------------------ gathers

@functools.lru_cache(maxsize=2)
def _rows(n_views, p, dim):
    """token rows [n_views, p, dim] fp32 (host, device).  The first elements of every row carry values beyond the fp8 / f16 range."""
    x = _randn((n_views, p, dim), 7 + n_views + p + dim) * torch.logspace(-3, 2, p).view(1, p, 1)
    k = min(dim, len(BEYOND))
    x[:, :, :k] = torch.tensor(BEYOND[:k])
    return x, x.cuda()


def _gather_rows_f32(counts, q, p, dim, varlen, uniform_t=None):
    lib = _lib.load()
    B, n = len(counts), len(counts) * p * dim
    x, xd = _rows(sum(counts), p, dim)
    host = _sentinel(n + 2 * PAD, salt=9)
    buf, qd, vs = host.cuda(), _i32(q), _i32(_lib.view_starts(counts))
    out = buf[PAD:PAD + n]
    if varlen:
        _lib.check(lib.bd_gather_query_rows_f32_varlen(_lib.ptr(xd), _lib.ptr(vs), _lib.ptr(qd), _lib.ptr(out), B, p, dim, _lib.stream()),
                   "bd_gather_query_rows_f32_varlen")
    else:
        _lib.check(lib.bd_gather_query_rows_f32(_lib.ptr(xd), _lib.ptr(qd), _lib.ptr(out), B, uniform_t, p, dim, _lib.stream()),
                   "bd_gather_query_rows_f32")
    torch.cuda.synchronize()
    want = host.clone()
    want[PAD:PAD + n].view(B, p, dim)[:] = x[_query_views(counts, q)]
    return buf, want


@gpu
@pytest.mark.parametrize("B,T,p,dim,qmode", [
    (1, 17, P, DIM, "mixed"), (32, 6, P, DIM, "mixed"), (64, 1, P, DIM, "first"),
    (3, 4, 1, 4, "last"), (5, 3, 7, 20, "mixed"), (2, 6, 3, 8, "first")])
def test_gather_query_rows_f32(hip, B, T, p, dim, qmode):
    """out[b] = x[query view of b] as fp32 rows (dim % 4 == 0: 20 is valid here), bit for bit, nothing else written; uniform == varlen."""
    counts = [T] * B
    q = _queries(qmode, counts)
    assert all(0 <= qi < T for qi in q)
    buf, want = _gather_rows_f32(counts, q, p, dim, varlen=False, uniform_t=T)
    assert torch.equal(_bits(buf.cpu()), _bits(want))
    buf_v, _ = _gather_rows_f32(counts, q, p, dim, varlen=True)
    assert torch.equal(_bits(buf_v), _bits(buf))


@gpu
@pytest.mark.parametrize("p,dim", [(P, DIM), (3, 20)])
@pytest.mark.parametrize("q", [[0, 16, 2, 0, 5], [0, 0, 1, 0, 3], [-1, 99, 3, 1, -7]])
def test_gather_query_rows_f32_ragged(hip, p, dim, q):
    buf, want = _gather_rows_f32(RAGGED, q, p, dim, varlen=True)
    assert torch.equal(_bits(buf.cpu()), _bits(want))


PRECS6 = ["bf16", "fp16", "bf16x3", "f16x3", "fp8", "f16c8"]


def _gather_tokens(counts, q, p, dim, prec, form, uniform_t=None):
    """form: "uniform" (q a device array), "null" (query_idx == NULL: view 0) or "varlen".  -> (raw bytes of the guarded buffer on the
    host, the fill pattern it started from, bytes of one plane, the gathered fp32 rows)."""
    lib = _lib.load()
    B, rows = len(counts), len(counts) * p
    x, xd = _rows(sum(counts), p, dim)
    np_, esz = _lib.planes(prec), (1 if prec == "fp8" else 2)
    plane_bytes = rows * dim * esz
    padb = PAD * 4
    fill = torch.randint(0, 256, (2 * padb + np_ * plane_bytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(rows + dim))
    buf = fill.cuda()
    out = buf[padb:padb + np_ * plane_bytes]
    out_plane = rows * dim if np_ == 2 else 0             # in elements of plane 0, as forward.hip passes it
    pid = _lib.prec_id(prec)
    qd, vs = (_i32(q) if form != "null" else None), _i32(_lib.view_starts(counts))
    if form == "varlen":
        _lib.check(lib.bd_gather_query_tokens_varlen(_lib.ptr(xd), _lib.ptr(vs), _lib.ptr(qd), _lib.ptr(out), out_plane, B, p, dim, pid,
                                                     _lib.stream()), "bd_gather_query_tokens_varlen")
    else:
        _lib.check(lib.bd_gather_query_tokens(_lib.ptr(xd), _lib.ptr(qd), _lib.ptr(out), out_plane, B, uniform_t, p, dim, pid,
                                              _lib.stream()), "bd_gather_query_tokens")
    torch.cuda.synchronize()
    src = x[_query_views(counts, q)].reshape(rows, dim)
    return buf.cpu(), fill, plane_bytes, src


def _check_tokens(got, fill, plane_bytes, src, prec):
    """One-plane formats and the hi plane: the bytes of hip_ops.to_operand(src).  Split formats: hi + lo within the format's margin of
    the fp32 value wherever that lies inside the format's range, and finite everywhere (saturated, never Inf).  Guards -- and the unused
    second half of F16C8's plane 1 -- keep the fill pattern."""
    rows, dim = src.shape
    np_, padb = _lib.planes(prec), PAD * 4
    want = hip_ops.to_operand(src, prec)
    hi = (want[0] if np_ == 2 else want).contiguous().view(torch.uint8).reshape(-1)
    assert torch.isfinite((want[0] if np_ == 2 else want).float()).all()                  # the expectation itself is saturated, not Inf
    assert torch.equal(got[:padb], fill[:padb]) and torch.equal(got[padb + np_ * plane_bytes:], fill[padb + np_ * plane_bytes:])
    assert torch.equal(got[padb:padb + plane_bytes], hi), f"{prec}: plane 0 differs from to_operand of the gathered rows"
    if np_ == 1:
        return
    planes = got[padb:padb + 2 * plane_bytes].view(_lib.op_dtype(prec)).reshape(2, rows, dim)
    if prec == "f16c8":
        lo_unused = slice(padb + plane_bytes + rows * dim, padb + 2 * plane_bytes)
        assert torch.equal(got[lo_unused], fill[lo_unused])
        h, lo, _ = hip_ops.f16c8_decode(planes)
        assert torch.isfinite(lo).all()
        val = h + lo
    else:
        assert torch.isfinite(planes.float()).all()
        val = hip_ops.from_operand(planes, prec)
    inside = src.abs() < RANGE.get(prec, float("inf"))
    assert inside.float().mean().item() >= 0.4 and (~inside).any() == (prec != "bf16x3")
    margin = 2 * EPS[prec] * src.abs().clamp_min(1.0) + 1e-7
    assert ((val - src).abs() <= margin)[inside].all(), f"{prec}: hi + lo is further than the format's margin from the fp32 row"


# B, T, tokens, dim: production (the product calls the uniform form with query_idx == NULL and T = 1 only) and awkward sizes
TOKEN_SHAPES = [(1, 17, P, DIM), (32, 6, P, DIM), (64, 1, P, DIM), (3, 4, 1, 8), (2, 3, 5, 32), (5, 2, 33, 40)]
# (F16C8 operand rows are laid out in 32-element blocks: that class takes the shapes with dim % 32 == 0)
TOKEN_CASES = [(prec, *shape) for shape in TOKEN_SHAPES for prec in PRECS6 if not (prec == "f16c8" and shape[3] % 32)]


@gpu
@pytest.mark.parametrize("prec,B,T,p,dim", TOKEN_CASES)
def test_gather_query_tokens(hip, prec, B, T, p, dim):
    """The operand gather in all six formats: uniform form, the varlen form at equal view counts (same bits) and query_idx == NULL
    (view 0 of every sample)."""
    counts = [T] * B
    q = _queries("mixed", counts)
    assert all(0 <= qi < T for qi in q)
    got, fill, pb, src = _gather_tokens(counts, q, p, dim, prec, "uniform", T)
    _check_tokens(got, fill, pb, src, prec)
    got_v = _gather_tokens(counts, q, p, dim, prec, "varlen")[0]
    assert torch.equal(got_v, got)
    got_0, fill, pb, src0 = _gather_tokens(counts, [0] * B, p, dim, prec, "null", T)
    _check_tokens(got_0, fill, pb, src0, prec)
    assert torch.equal(src0, _rows(B * T, p, dim)[0][::T].reshape(B * p, dim))


@gpu
@pytest.mark.parametrize("prec", PRECS6)
@pytest.mark.parametrize("p,dim", [(P, DIM), (3, 32)])
@pytest.mark.parametrize("q", [[0, 16, 2, 0, 5], [-1, 99, 3, 1, -7]])
def test_gather_query_tokens_ragged(hip, prec, p, dim, q):
    """bd_gather_query_tokens_varlen (no caller in the product yet) on view counts [1, 17, 3, 1, 6], the clamp included."""
    got, fill, pb, src = _gather_tokens(RAGGED, q, p, dim, prec, "varlen")
    _check_tokens(got, fill, pb, src, prec)


# ------------------------------------------------------------------------------------------------------------------ refusals (no GPU)

P1 = ctypes.c_void_p(0x10000)          # a non-NULL, aligned address that no refused call may touch


def test_token_row_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.bd_write_prefix_tokens(P1, P1, 2, 5, 6, 768, None) == -1          # n_prefix > tokens_per_image
    assert lib.bd_write_prefix_tokens(P1, P1, 2, 261, 0, 768, None) == -1 and lib.bd_write_prefix_tokens(P1, P1, 0, 261, 5, 768, None) == -1
    assert lib.bd_write_prefix_tokens(None, P1, 2, 261, 5, 768, None) == -5 and lib.bd_write_prefix_tokens(P1, None, 2, 261, 5, 768, None) == -5
    assert lib.bd_query_substitute(P1, P1, P1, P1, None, 2, 3, 256, 768, None) == -5
    assert lib.bd_query_substitute(P1, P1, P1, P1, P1, 2, 0, 256, 768, None) == -1
    for dim in (770, 6, 3):                                                      # fp32 row gather: whole float4s
        assert lib.bd_gather_query_rows_f32(P1, P1, P1, 2, 3, 256, dim, None) == -1
        assert lib.bd_gather_query_rows_f32_varlen(P1, P1, P1, P1, 2, 256, dim, None) == -1
    assert lib.bd_gather_query_rows_f32(P1, None, P1, 2, 3, 256, 768, None) == -5
    for dim in (20, 772, 4):                                                     # operand gather: whole 8-element chunks
        assert lib.bd_gather_query_tokens(P1, P1, P1, 0, 2, 3, 256, dim, _lib.PREC_BF16, None) == -1
        assert lib.bd_gather_query_tokens_varlen(P1, P1, P1, P1, 0, 2, 256, dim, _lib.PREC_BF16, None) == -1
    for prec in (99, -1, 7, _lib.PREC_F16_OUT_BF16X3, _lib.PREC_F16C8_QK16):     # not an operand class
        assert lib.bd_gather_query_tokens(P1, P1, P1, 0, 2, 3, 256, 768, prec, None) == -2
        assert lib.bd_gather_query_tokens_varlen(P1, P1, P1, P1, 0, 2, 256, 768, prec, None) == -2
    assert lib.bd_gather_query_tokens(None, P1, P1, 0, 2, 3, 256, 768, 0, None) == -5 and lib.bd_gather_query_tokens(P1, P1, None, 0, 2, 3, 256, 768, 0, None) == -5


def test_an_empty_sample_is_refused_on_the_host():
    """query_view_of has no view to clamp an empty sample's query to (it would address the next sample's rows, or rows past the buffer
    for the last sample): whoever builds view_start refuses it before anything is launched."""
    for counts in ([2, 0, 3], [0], [3, -1], [2, 3, 0]):
        with pytest.raises(ValueError):
            _lib.view_starts(counts)
        with pytest.raises(ValueError):                                           # the ragged wrapper: raises before it needs a device
            hip_ops.attention_varlen(torch.zeros(8, 3 * 768, dtype=torch.float16), counts, 256, 8, 96, 0.1, prec="fp16")
        with pytest.raises(ValueError):                                           # the facade
            BoxDreamer._view_counts({"view_counts": counts, "query_idx": torch.zeros(len(counts), dtype=torch.long)}, len(counts), 17)
    assert _lib.view_starts([1, 17, 3, 1, 6]) == [0, 1, 18, 21, 22, 28]           # one-view samples stay valid for the unit operators
