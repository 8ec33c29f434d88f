"""The split-bf16 head_dim-64 attention instances (DINOv2's strict attention), whose K / V tiles go global -> LDS by LDS-DMA and whose
V^T fragments come from the transposing LDS read (csrc/attention.hip: DMA).  What can go wrong there is addressing: a piece of a tile
landing in another row or chunk, a swizzle applied on one side only, a ragged tail that reads past the sample or leaves stale LDS rows
in the P.V product.  So: every sequence length at which the staging takes another path, against fp64 and -- where the same rows are
computed twice -- bit for bit.

    seq  64   one whole tile                      seq  81   a tail of 17 keys: the masked generic tile
    seq  65   a tail of one key (peeled tile)     seq 261   4 tiles + a peeled 5-key tail (DINOv2)
    seq  80   a tail of 16 keys, the peeled       seq   5   fewer keys than one fragment, one tile
              instance's edge
"""
import functools

import pytest
import torch

from boxdreamer_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu

HEADS, HD, BATCH = 2, 64, 3
SEQS = (64, 65, 80, 81, 261, 5)
EPS = 2.0 ** -15          # operand rounding of the split-bf16 pass (tests/test_gpu_steered.py: _VARIANTS)
# name -> (attention code, how the result is stored): the three result classes of the split-bf16 input class
OUTS = {"bf16x3": ("PREC_BF16X3", "planes"), "f16c8": ("PREC_BF16X3_OUT_F16C8", "f16c8"), "f16x3": ("PREC_BF16X3_OUT_F16X3", "planes_f16")}


def _values(batch, seq, hd=HD, seed=0):
    g = torch.Generator().manual_seed(1000 * seq + hd + seed)
    return torch.randn(batch * seq, 3 * HEADS * hd, generator=g)


@functools.lru_cache(maxsize=None)
def _case(seq):
    """(split-bf16 qkv operand on the device [2, BATCH * seq, 3 * HEADS * HD], fp64 reference [BATCH, seq, HEADS, HD] as fp32)"""
    t = hip_ops.to_operand(_values(BATCH, seq).cuda(), "bf16x3")
    src = hip_ops.from_operand(t, "bf16x3").cpu().reshape(BATCH, seq, 3, HEADS, HD).double()
    q, k, v = (src[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref = (((q @ k.transpose(-1, -2)) * HD ** -0.5).softmax(-1) @ v).permute(0, 2, 1, 3).float()
    return t, ref


def _out(kind, rows, cols):
    dt = torch.bfloat16 if kind == "planes" else torch.float16
    return torch.full((2, rows, cols), 7.0, dtype=dt, device="cuda")


def _read(o, kind):
    if kind == "f16c8":
        hi, lo, _ = hip_ops.f16c8_decode(o)
        return (hi + lo).cpu()
    return (o[0].float() + o[1].float()).cpu()


def _bits(o, kind, r0, r1):
    """The stored bits of result rows [r0, r1): the 16-bit planes, or the f16 plane and the rows' bytes of the e4m3 plane."""
    if kind != "f16c8":
        return o[:, r0:r1].contiguous().view(torch.int16).cpu()
    rows, cols = o.shape[1:]
    lo8 = o[1].contiguous().view(torch.uint8).reshape(-1)[:rows * cols].reshape(rows, cols)
    return torch.cat([o[0, r0:r1].contiguous().view(torch.uint8).reshape(r1 - r0, -1), lo8[r0:r1]], 1).cpu()


def _plain(t, out_name, batch, seq, hd=HD):
    code, kind = OUTS[out_name]
    o = _out(kind, batch * seq, HEADS * hd)
    _lib.check(_lib.load().bd_attention(_lib.ptr(t), t[0].numel(), _lib.ptr(o), o[0].numel(), batch, seq, HEADS, hd, hd ** -0.5,
                                        getattr(_lib, code), _lib.stream()), "bd_attention")
    torch.cuda.synchronize()
    return o, kind


def _assert_close(got, ref, what):
    tol = 6 * EPS * max(1.0, ref.abs().max().item()) + 2e-5          # tests/test_gpu_steered.py: _attn_assert
    err = (got - ref).abs().max().item()
    assert err < tol, (what, err, tol)


@pytest.mark.parametrize("out_name", sorted(OUTS))
@pytest.mark.parametrize("seq", SEQS)
def test_plan_is_the_dma_instance(hip, seq, out_name):
    """Every case here runs attn_kernel's two-plane head_dim-64 instance (3 or 4 waves by the query waste, never the ragged form)."""
    plan = hip_ops.attention_plan("plain", prec=getattr(_lib, OUTS[out_name][0]), batch=BATCH, seq=seq, heads=HEADS, head_dim=HD)
    assert (plan["kernel"], plan["planes"], plan["head_dim"], plan["vl"]) == ("tiled", 2, HD, False), plan


@pytest.mark.parametrize("out_name", sorted(OUTS))
@pytest.mark.parametrize("seq", SEQS)
def test_reference_and_swapped_samples(hip, seq, out_name):
    """Against fp64, and the batch with samples 1 and 2 swapped gives every sample the same bits: a staging address that depends on the
    sample's place in the batch, or reaches into a neighbour, shows here."""
    t, ref = _case(seq)
    o, kind = _plain(t, out_name, BATCH, seq)
    got = _read(o, kind).reshape(BATCH, seq, HEADS, HD)
    for b in range(BATCH):
        _assert_close(got[b], ref[b], (seq, out_name, b))
    order = [0, 2, 1]
    ts = t.reshape(2, BATCH, seq, -1)[:, order].reshape(t.shape).contiguous()
    os_, _ = _plain(ts, out_name, BATCH, seq)
    for b, src in enumerate(order):
        assert torch.equal(_bits(os_, kind, b * seq, (b + 1) * seq), _bits(o, kind, src * seq, (src + 1) * seq)), (seq, out_name, b)


@pytest.mark.parametrize("fill", (3e38, float("inf")), ids=("3e38", "inf"))
@pytest.mark.parametrize("seq", SEQS)
def test_tail_does_not_read_the_next_sample(hip, seq, fill):
    """The last sample's K / V rows filled with 3e38 or with inf: the samples before it keep their bits and stay finite -- the tail rows
    of a ragged last tile are out of the sample's descriptor, never the next sample's rows.  (A leaked row has P exactly 0: 0 x 3e38 is
    still 0, 0 x inf is NaN, so the inf fill is the one that shows a V row read past the end.)"""
    t, _ = _case(seq)
    x = _values(BATCH, seq)
    x[(BATCH - 1) * seq:, HEADS * HD:] = fill
    hot = hip_ops.to_operand(x.cuda(), "bf16x3")
    keep = (BATCH - 1) * seq
    assert torch.equal(hot[:, :keep], t[:, :keep])
    for out_name in ("f16c8", "f16x3"):
        o, kind = _plain(t, out_name, BATCH, seq)
        oh, _ = _plain(hot, out_name, BATCH, seq)
        assert torch.equal(_bits(oh, kind, 0, keep), _bits(o, kind, 0, keep)), (seq, out_name)
        assert torch.isfinite(_read(oh, kind)[:keep]).all(), (seq, out_name)


_Q_LEN = {64: 32, 65: 13, 80: 40, 81: 27, 261: 87, 5: 1}          # a proper divisor of seq each (bd_attention_q: seq % q_len == 0)


@pytest.mark.parametrize("out_name", ("f16c8", "f16x3"))
@pytest.mark.parametrize("seq", SEQS)
def test_prefix_and_query_view_match_the_plain_launch(hip, seq, out_name):
    """bd_attention_prefix(prefix_queries = 0) and bd_attention_q place the queries differently in the grid; the same (query, keys) rows
    are bit-equal to the plain launch's."""
    t, _ = _case(seq)
    code, kind = OUTS[out_name]
    lib, pid, cols = _lib.load(), getattr(_lib, code), HEADS * HD
    o, _ = _plain(t, out_name, BATCH, seq)
    npre = 5 if seq > 5 else 1
    op = _out(kind, BATCH * seq, cols)
    _lib.check(lib.bd_attention_prefix(_lib.ptr(t), t[0].numel(), _lib.ptr(op), op[0].numel(), BATCH, seq, HEADS, HD, HD ** -0.5, npre, 0, pid,
                                       _lib.stream()), "bd_attention_prefix")
    qv = torch.tensor([1, 0, seq // _Q_LEN[seq] - 1], dtype=torch.int32)
    qvd, ql = qv.cuda(), _Q_LEN[seq]
    oq = _out(kind, BATCH * ql, cols)
    _lib.check(lib.bd_attention_q(_lib.ptr(t), t[0].numel(), _lib.ptr(oq), oq[0].numel(), BATCH, seq, HEADS, HD, HD ** -0.5, _lib.ptr(qvd), ql, pid,
                                  _lib.stream()), "bd_attention_q")
    torch.cuda.synchronize()
    for b in range(BATCH):
        r = b * seq
        assert torch.equal(_bits(op, kind, r + npre, r + seq), _bits(o, kind, r + npre, r + seq)), ("prefix", seq, out_name, b)
        q0 = r + int(qv[b]) * ql
        assert torch.equal(_bits(oq, kind, b * ql, (b + 1) * ql), _bits(o, kind, q0, q0 + ql)), ("q", seq, out_name, b)
