"""GPU parity on inputs STEERED into the data-dependent paths of three kernels.

The decode, top-k mask and attention kernels choose their control path from the values they read, not from the shape; random-normal
inputs almost never reach some of those paths.  Every test here builds its input so that it reaches one named path, asserts on the host
that the input really has the property that path needs (so a change to a generator cannot quietly stop covering it), and compares the
kernel with a plain reference:
  - decode (bd_decode_topk): the oracle's stable descending sort -- index lists in order and pixel corners exactly;
  - top-k mask (bd_topk_mask): the first k of a stable descending sort, exactly k ones per row;
  - attention: fp64 torch softmax on the operands exactly as stored.
Nothing here falls back to PyTorch compute."""
import functools
import math

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops
from oracle import boxdreamer_oracle as orc

pytestmark = pytest.mark.gpu

THREADS = 1024          # decode_kernel_regs: element i of a map lives in thread i % 1024
REGS_MAX_HW = 49 * 1024  # larger maps (and k > 64) take the slice kernel decode_kernel<VEC>: 256 threads, contiguous slices


# ----------------------------------------------------------------------------------------------------------------- decode

def _background(n, H, W, seed, hi=0.2):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(-1.0, hi, (n, H * W)).astype(np.float32)), rng


def _plant(flat, idx, rng, lo=0.3, hi=1.0):
    """distinct hot values in [lo, hi) at the flat indices idx, in a random order"""
    vals = np.sort(rng.uniform(lo, hi, len(idx)).astype(np.float32))[::-1].copy()
    rng.shuffle(vals)
    flat[torch.as_tensor(np.asarray(idx), dtype=torch.long)] = torch.from_numpy(vals)


def _thread_idx(t, hw):
    return [t + THREADS * j for j in range((hw - 1 - t) // THREADS + 1)] if t < hw else []


def _residue_counts(idx):
    """per map: the largest number of top-k picks that share one thread of the register kernel"""
    return [int(np.bincount(row % THREADS).max()) for row in idx.numpy()]


def _check_decode(heat, k, idx_ref=None):
    """heat: fp32 [n, H, W] on the host.  The kernel's index list, corners and normalised corners against the oracle; and the facade's
    form (want_idx=False, topk_idx = NULL) must give the same corners.  Returns the oracle's index list."""
    n, H, W = heat.shape
    on, okp, oidx = orc.recover_bb8_corners(heat.unsqueeze(0), k)
    on, okp, oidx = on[0], okp[0], oidx[0]
    dev = heat.cuda()
    kp, kn, idx = hip_ops.decode_topk(dev, k=k)
    kp2, kn2, none = hip_ops.decode_topk(dev, k=k, want_idx=False)
    torch.cuda.synchronize()
    assert none is None
    assert torch.equal(idx.cpu().long(), oidx), "index list (order included) differs from the oracle's"
    assert torch.equal(kp.cpu(), okp)
    assert (kn.cpu() - on).abs().max().item() <= 1e-6
    assert torch.equal(kp2.cpu(), kp.cpu()) and torch.equal(kn2.cpu(), kn.cpu())
    return oidx


@pytest.mark.parametrize("H,W,k", [(128, 128, 16), (128, 128, 20), (100, 150, 20), (224, 224, 20), (128, 129, 20)])
def test_decode_one_thread_holds_the_top_k(hip, H, W, k):
    """A map's top-k picks live in ONE thread of the register kernel (where that thread holds fewer than k elements -- NE = 16 maps,
    hw <= 16384 -- the rest in a second thread, below them): it wins every round, promotes its second candidate every other round and
    rescans its registers in between.  NE = 49 maps (up to 224 x 224) hold 49 elements per thread."""
    hw = H * W
    heat, rng = _background(3, H, W, seed=H * 1000 + W + k)
    owns = []
    for m in range(3):
        own = _thread_idx(777 + 37 * m, hw)
        _plant(heat[m], own, rng, 0.4, 1.0)
        if len(own) < k:
            _plant(heat[m], _thread_idx(123 + m, hw)[: k - len(own) + 4], rng, 0.3, 0.4)
        owns.append(min(len(own), k))
    heat = heat.reshape(3, H, W)
    oidx = _check_decode(heat, k)
    assert _residue_counts(oidx) == owns and min(owns) >= 14


@pytest.mark.parametrize("H,W", [(128, 128), (224, 224), (33, 97)])
def test_decode_two_threads_win_alternately(hip, H, W):
    """Two threads hold the top 20 and their values interleave: each wins every other round, so promotion and rescan of the two threads
    alternate (a rescan filters on a pick made by the OTHER thread)."""
    hw = H * W
    heat, rng = _background(2, H, W, seed=hw)
    for m, (ta, tb) in enumerate([(5, 900), (1000, 3)]):
        a, b = _thread_idx(ta, hw), _thread_idx(tb, hw)
        n = min(len(a), len(b), 12)
        vals = np.sort(rng.uniform(0.3, 1.0, 2 * n).astype(np.float32))[::-1]
        heat[m, a[:n]] = torch.from_numpy(vals[0::2].copy())
        heat[m, b[:n]] = torch.from_numpy(vals[1::2].copy())
    heat = heat.reshape(2, H, W)
    k = min(20, 2 * min(len(_thread_idx(5, hw)), len(_thread_idx(900, hw)), 12))
    oidx = _check_decode(heat, k)
    res = oidx.numpy() % THREADS
    assert (res[:, 0::2] == res[:, :1]).all() and (res[:, 1::2] == res[:, 1:2]).all() and (res[:, 0] != res[:, 1]).all()
    assert min(_residue_counts(oidx)) >= 3


@pytest.mark.parametrize("H,W", [(128, 128), (200, 128), (150, 256)])
def test_decode_vertical_blob_aliases_onto_few_threads(hip, H, W):
    """A realistic aliasing case: a tall, narrow heat-map peak on a map whose width divides 1024.  Rows 1024 / W apart land in the same
    thread, so a blob 20+ rows tall puts several of its top-20 pixels into each of a few threads."""
    heat, _ = _background(2, H, W, seed=W, hi=-0.5)
    heat = heat.reshape(2, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    for m, (cy, cx, sy) in enumerate([(H / 2 + 0.3, W // 3 + 0.2, 9.0), (H / 3, W - 20.4, 14.0)]):
        blob = torch.exp(-((ys - cy) ** 2) / (2 * sy ** 2) - ((xs - cx) ** 2) / (2 * 0.45 ** 2))
        heat[m] = torch.maximum(heat[m], 2 * blob - 1)
    oidx = _check_decode(heat, 20)
    rows = oidx // W
    assert ((rows.max(-1)[0] - rows.min(-1)[0]) >= 19).all()                  # the top 20 span 20+ rows
    assert min(_residue_counts(oidx)) >= 3


def test_decode_ties_inside_one_thread_and_across_two(hip):
    """Equal values at the rescan: one thread holds a run of equal values (the (x == pv) & (i > pi) half of the rescan filter decides
    which comes next); and equal values split between a rescanning thread and another one, whose indices interleave."""
    H, W = 224, 224
    hw = H * W
    heat, rng = _background(3, H, W, seed=11)
    # map 0: thread 300 holds 12 equal values on top, k = 20 reaches 8 more below them in thread 301
    heat[0, _thread_idx(300, hw)[:12]] = 0.75
    _plant(heat[0], _thread_idx(301, hw)[:10], rng, 0.3, 0.7)
    # map 1: threads 40 and 41 both hold 0.5 at their first 10 elements: ties interleave 40 < 41 < 1064 < 1065 ...; above them thread 40
    # has 3 larger values (so it has rescanned before the ties start)
    heat[1, _thread_idx(40, hw)[:10]] = 0.5
    heat[1, _thread_idx(41, hw)[:10]] = 0.5
    heat[1, _thread_idx(40, hw)[20:23]] = torch.tensor([0.9, 0.8, 0.7])
    # map 2: the tie straddles the rank-20 boundary inside one thread: 6 larger values, then 30 equal ones, all in thread 1023
    own = _thread_idx(1023, hw)
    heat[2, own[:30]] = 0.25
    _plant(heat[2], own[30:36], rng, 0.3, 1.0)
    heat = heat.reshape(3, H, W)
    oidx = _check_decode(heat, 20)
    h = (heat.reshape(3, hw) + 1) / 2
    for m in (0, 2):
        v = h[m, oidx[m]]
        same = (v[1:] == v[:-1]) & (oidx[m, 1:] % THREADS == oidx[m, :-1] % THREADS)
        assert int(same.sum()) >= 10, m                                        # equal values picked one after another in one thread
    v, res = h[1, oidx[1]], oidx[1] % THREADS
    assert (v[3:] == 0.75).all() and res[3:].tolist() == [40, 41] * 8 + [40]   # equal values alternate between the two threads
    assert (res[:3] == 40).all()


def _boundary_map(H, W, k, seed):
    """random background; for maps of 2+ elements per thread, the top picks planted on few threads; a tie straddles rank k"""
    hw = H * W
    heat, rng = _background(1, H, W, seed)
    flat = heat[0]
    if hw > THREADS:
        idx, t = [], 0
        while len(idx) < k + 6:
            idx += _thread_idx((t * 211 + 7) % THREADS, hw)
            t += 1
        if hw <= 2 * THREADS:
            idx = [0, 1024] + [i for i in idx if i not in (0, 1024)]
        _plant(flat, idx[: k + 6], rng)
    if k < hw:
        order = torch.sort((flat + 1) / 2, descending=True, stable=True)[1]
        flat[order[k]] = flat[order[k - 1]]
    return heat.reshape(1, H, W)


_SIZES = [(1, 1), (4, 4), (28, 28), (31, 33), (32, 32), (25, 41), (128, 128), (128, 129), (224, 224)]
_BOUNDARY = [(H, W, k) for H, W in _SIZES for k in sorted({1, 20, 64, min(H * W, 64)}) if k <= H * W]


@pytest.mark.parametrize("H,W,k", _BOUNDARY)
def test_decode_boundary_sizes(hip, H, W, k):
    """The register kernel at its size edges: hw = 1, k = hw = 16, hw below / at / one past 1024 (one map, a buffer of exactly hw floats),
    the largest NE = 16 map (128 x 128) and one past it (128 x 129, NE = 49), the largest NE = 49 map (224 x 224); k = 1, 20, 64."""
    hw = H * W
    heat = _boundary_map(H, W, k, seed=hw * 7 + k)
    assert heat.numel() == hw
    oidx = _check_decode(heat, k)
    if hw > 2 * THREADS and k >= 3:
        assert max(_residue_counts(oidx)) >= 3
    if k < hw:                                                                 # the rank-k tie is real
        h = (heat.reshape(hw) + 1) / 2
        assert h[oidx[0, k - 1]] == h.sort(descending=True)[0][k]


def test_decode_refuses_k_beyond_the_map(hip):
    heat = torch.zeros((1, 4, 4), device="cuda")
    with pytest.raises(_lib.HipLibraryError, match="BD_ERR_SHAPE"):
        hip_ops.decode_topk(heat, k=17)


def _slice_maps(H, W, per, seed):
    """two maps: 0 = the top 20 (with ties) inside ONE thread's contiguous slice; 1 = random with a plateau across slices"""
    hw = H * W
    heat, rng = _background(2, H, W, seed)
    t = 101
    lo = t * per
    sl = list(range(lo, min(lo + per, hw)))
    _plant(heat[0], sl[::3][:24], rng, 0.5, 1.0)
    heat[0, sl[1::7][:12]] = 0.8                                               # ties inside the slice, straddling rank 20
    heat[1, hw // 2 - 40: hw // 2 + 40] = 0.9                                  # 80-way tie over several slices
    return heat.reshape(2, H, W), t


@pytest.mark.parametrize("H,W,k", [(256, 256, 20), (225, 230, 20), (224, 224, 65), (224, 224, 100), (256, 256, 64)])
def test_decode_slice_kernel(hip, H, W, k):
    """Maps above 49 x 1024 elements or k > 64 take decode_kernel<VEC> (256 threads, contiguous slices; float4 scans where the map is a
    multiple of 1024 floats and 16-byte aligned, scalar otherwise).  Map 0 holds its top k inside one slice, so the same owner wave rescans
    in every round; map 1 an 80-way plateau."""
    hw = H * W
    assert hw > REGS_MAX_HW or k > 64
    per = hw // 256 if hw % 1024 == 0 else (hw + 255) // 256
    heat, t = _slice_maps(H, W, per, seed=hw + k)
    oidx = _check_decode(heat, k)
    if k <= 20:
        assert (oidx[0] // per == t).all()                                     # one owner, every round


def test_decode_slice_kernel_scalar_form_on_a_misaligned_map(hip):
    """The same 256 x 256 maps through a pointer one float past a 16-byte boundary: the alignment check must choose the scalar form, whose
    picks equal the float4 form's and the oracle's.  (A direct library call on a view: the wrapper's .contiguous() would realign.)"""
    H, W, k = 256, 256, 20
    heat, t = _slice_maps(H, W, H * W // 256, seed=5)
    n = heat.shape[0]
    big = torch.zeros(n * H * W + 4, device="cuda")
    view = big[1:1 + n * H * W]
    view.copy_(heat.reshape(-1).cuda())
    assert view.data_ptr() % 16 == 4
    lib = _lib.load()
    kp = torch.empty((n, 2), device="cuda")
    kn = torch.empty_like(kp)
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    _lib.check(lib.bd_decode_topk(_lib.ptr(view), n, H, W, k, _lib.ptr(kp), _lib.ptr(kn), _lib.ptr(idx), _lib.stream()), "bd_decode_topk")
    torch.cuda.synchronize()
    on, okp, oidx = (x[0] for x in orc.recover_bb8_corners(heat.unsqueeze(0), k))
    assert (oidx[0] // (H * W // 256) == t).all()
    assert torch.equal(idx.cpu().long(), oidx)
    assert torch.equal(kp.cpu(), okp)
    assert (kn.cpu() - on).abs().max().item() <= 1e-6


# ----------------------------------------------------------------------------------------------------------------- top-k mask

def _mask_rows(N, seed):
    rng = np.random.default_rng(seed)
    rows = []
    spread = (37 * np.arange(N) + 5) % N                                       # a permutation: consecutive picks in different threads / waves
    r = rng.standard_normal(N).astype(np.float32)
    rows.append(r)                                                             # distinct values
    r = (0.3 * rng.standard_normal(N)).astype(np.float32)
    r[spread[:15]] = 4.0
    r[spread[15:45]] = 2.5                                                     # 30-way tie across waves straddling rank 20
    rows.append(r)
    r = (0.5 * rng.standard_normal(N)).astype(np.float32)
    r[spread[:40]] = 3.0                                                       # 40-way tie on top
    rows.append(r)
    r = np.full(N, -np.inf, np.float32)
    r[spread[:10]] = rng.standard_normal(10)                                   # fewer than k finite scores
    rows.append(r)
    rows.append(np.full(N, -np.inf, np.float32))                               # every score -inf
    r = np.full(N, -1e4, np.float32)                                           # all-background reference views score exactly -1e4
    r[spread[:8]] = rng.standard_normal(8)
    r[spread[8:12]] = -np.inf
    rows.append(r)
    r = rng.standard_normal(N).astype(np.float32)
    r[spread[:N // 3]] = -np.inf
    r[spread[N // 3: N // 3 + 2]] = np.inf
    r[N - 1] = -1e4
    rows.append(r)
    return torch.from_numpy(np.stack(rows))


@pytest.mark.parametrize("N", [257, 700, 1024])
@pytest.mark.parametrize("k", [1, 20, "N"])
def test_topk_mask_steered(hip, N, k):
    """bd_topk_mask with several elements per thread over all four waves: ties straddling rank k across threads and waves, rows with
    -inf (fewer than k finite scores, all -inf), blocks of exactly -1e4 and +inf entries.  The mask must be the first k of a stable
    descending sort, with exactly k ones in every row."""
    k = N if k == "N" else k
    s = _mask_rows(N, seed=N)
    B = s.shape[0]
    finite = torch.isfinite(s).sum(1)
    assert finite[3] == 10 and finite[4] == 0 and (s[5] == -1e4).sum() == N - 12 and torch.isposinf(s[6]).sum() == 2
    srt = s.sort(-1, descending=True)[0]
    if k < N:                                                                  # a tie straddles rank k in some row
        assert (srt[:, k - 1] == srt[:, k]).any()
    lib = _lib.load()
    sd = s.cuda()
    m = torch.full((B, N), 7, dtype=torch.uint8, device="cuda")
    _lib.check(lib.bd_topk_mask(_lib.ptr(sd), B, N, k, _lib.ptr(m), _lib.stream()), "bd_topk_mask")
    torch.cuda.synchronize()
    order = torch.sort(s, dim=-1, descending=True, stable=True)[1][:, :k]
    want = torch.zeros((B, N), dtype=torch.uint8).scatter_(1, order, 1)
    got = m.cpu()
    assert (got.sum(1) == k).all(), got.sum(1).tolist()
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------------- attention

# name -> (input operand class, attention code, how the result is stored, operand rounding of the mode)
_VARIANTS = {
    "bf16": ("bf16", "PREC_BF16", "native", 2.0 ** -8),
    "fp16": ("fp16", "PREC_F16", "native", 2.0 ** -11),
    "bf16x3": ("bf16x3", "PREC_BF16X3", "planes", 2.0 ** -15),
    "f16_out_f16c8": ("fp16", "PREC_F16_OUT_F16C8", "f16c8", 2.0 ** -11),
    "bf16x3_out_f16c8": ("bf16x3", "PREC_BF16X3_OUT_F16C8", "f16c8", 2.0 ** -15),
}
KT = 64                   # key tile of both attention kernels
PATTERNS = "abcdef"       # one per head, see _steer
QSTEER = 8.0              # the steering q component (a power of two: the steering products are exact in every operand class)


def _steer(batch, seq, hd, seed):
    """qkv [batch, seq, 3, 6, hd] fp32 whose logits (log2 units, scale * log2 e * q.k) follow one pattern per head, steered by
    dimension 0 (q = QSTEER there, k = the pattern / (sc * QSTEER), rounded to 8 significant bits so that it is exact in bf16 and f16);
    the other dimensions carry small noise:
      a: the max rises by ~6 in every 64-key tile (it moves every tile; alpha ~ 2^-6)
      b: the max sits on key 0 and never moves
      c: the max is the last key (of the ragged tail tile where seq % 64 != 0)
      d: a hot key ~155+ above every other arrives late (tile >= 1): the other probabilities and alpha underflow to 0
      e: equal maxima on two keys in different tiles (identical k rows)
      f: q = 0: every logit is 0, the output is the mean of V"""
    heads = len(PATTERNS)
    rng = np.random.default_rng(seed)
    sc = hd ** -0.5 * math.log2(math.e)
    qkv = 0.25 * rng.standard_normal((batch, seq, 3, heads, hd))
    qkv[:, :, 2] = rng.standard_normal((batch, seq, heads, hd))
    qkv[:, :, 0, :, 0] = QSTEER
    nt = (seq + KT - 1) // KT
    tile = np.arange(seq) // KT
    L = np.empty((batch, heads, seq))
    for b in range(batch):
        u = lambda lo, hi: rng.uniform(lo, hi, seq)
        L[b, 0] = 6.0 * tile - u(1.5, 5.0)
        for t in range(nt):                                                    # one key per tile exactly at 6 t, anywhere in the tile
            L[b, 0, min(t * KT + int(rng.integers(0, KT)), seq - 1)] = 6.0 * t
        L[b, 1] = u(-4.0, 9.0)
        L[b, 1, 0] = 12.0
        L[b, 2] = u(-4.0, 9.0)
        L[b, 2, seq - 1] = 12.0
        L[b, 3] = u(-4.0, 12.0)
        L[b, 3, seq - 40] = 170.0
        L[b, 4] = u(-4.0, 9.0)
        L[b, 4, [3, _e_second(seq)]] = 12.0
        L[b, 5] = 0.0
    c = torch.from_numpy(L / (sc * QSTEER)).to(torch.bfloat16).double().numpy()
    qkv[:, :, 1, :, 0] = c.transpose(0, 2, 1)
    qkv[:, _e_second(seq), 1, 4] = qkv[:, 3, 1, 4]                             # pattern e: the two maxima's k rows are identical
    qkv[:, :, 0, 5] = 0.0                                                      # pattern f
    return torch.from_numpy(qkv.astype(np.float32))


def _e_second(seq):
    return ((seq - 1) // KT) * KT - 30 if seq > 2 * KT else seq - 1           # a key in a later tile than key 3


def _assert_patterns(logits2, seq):
    """logits2: fp64 [batch, heads, queries, seq] in log2 units, from the operands as stored.  Each head's pattern holds for every query."""
    nt = (seq + KT - 1) // KT
    pad = torch.full(logits2.shape[:-1] + (nt * KT,), -math.inf, dtype=torch.float64)
    pad[..., :seq] = logits2
    tmax = pad.reshape(*logits2.shape[:-1], nt, KT).max(-1)[0]               # per-tile maxima
    run = torch.cummax(tmax, -1)[0]
    # a: the running max moves in every tile, by 2+ (alpha <= 1/4)
    a = tmax[:, 0]
    assert ((a[..., 1:] - run[:, 0, :, :-1]) > 2.0).sum(-1).min().item() >= nt - 1
    # b: the max is key 0 (tile 0) and nothing later comes within 1
    b = logits2[:, 1]
    assert (b.argmax(-1) == 0).all() and (b[..., KT:].max(-1)[0] < b[..., 0] - 1.0).all() and (run[:, 1, :, 0] == run[:, 1, :, -1]).all()
    # c: the max is the last key, in the last (ragged) tile, 1+ above the rest
    cc = logits2[:, 2]
    assert (cc.argmax(-1) == seq - 1).all() and (cc[..., :-1].max(-1)[0] < cc[..., -1] - 1.0).all()
    # d: the hot key, in tile >= 1, is 150+ above every other key: exp2 of the others and alpha underflow to 0 in fp32
    d = logits2[:, 3]
    hot = seq - 40
    assert hot // KT >= 1 and (d.argmax(-1) == hot).all()
    others = torch.cat([d[..., :hot], d[..., hot + 1:]], -1).max(-1)[0]
    assert (d[..., hot] - others > 150.0).all()
    # e: two keys in different tiles share the max (their k rows are identical: checked on the operands), the rest 1+ below
    e = logits2[:, 4]
    j2 = _e_second(seq)
    assert 3 // KT != j2 // KT
    assert ((e[..., 3] - e[..., j2]).abs() < 1e-9).all() and (e.max(-1)[0] - e[..., 3] < 1e-9).all()
    rest = e.clone()
    rest[..., [3, j2]] = -math.inf
    assert (rest.max(-1)[0] < e[..., 3] - 1.0).all()
    # f: every logit is 0
    assert (logits2[:, 5] == 0).all()


@functools.lru_cache(maxsize=None)
def _steered_case(batch, seq, hd, in_prec):
    """(qkv operand on the device, fp64 reference output [batch, seq, heads, hd]); the patterns asserted on the stored operands"""
    qkv = _steer(batch, seq, hd, seed=seq * 131 + hd + batch)
    heads = qkv.shape[3]
    flat = qkv.reshape(batch * seq, -1)
    t = hip_ops.to_operand(flat.cuda(), in_prec)
    src = hip_ops.from_operand(hip_ops.to_operand(flat, in_prec), in_prec).reshape(batch, seq, 3, heads, hd).double()
    q, k, v = (src[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    assert torch.equal(k[:, 4, 3], k[:, 4, _e_second(seq)]) and (q[:, 5] == 0).all()
    logits = (q @ k.transpose(-1, -2)) * hd ** -0.5
    _assert_patterns(logits * math.log2(math.e), seq)
    ref = (logits.softmax(-1) @ v).permute(0, 2, 1, 3).float()
    return t, ref


def _attn_out(kind, in_prec, rows, cols):
    if kind == "native":
        return torch.full((rows, cols), 7.0, dtype=_lib.op_dtype(in_prec), device="cuda")
    if kind == "fp8":
        return torch.full((rows, cols), 7.0, device="cuda").to(torch.float8_e4m3fn)
    return torch.full((2, rows, cols), 7.0, dtype=torch.bfloat16 if kind == "planes" else torch.float16, device="cuda")


def _attn_out_plane(o, kind):
    return 0 if kind in ("native", "fp8") else o[0].numel()


def _attn_read(o, kind):
    if kind in ("native", "fp8"):
        return o.float().cpu()
    if kind == "f16c8":
        hi, lo, _ = hip_ops.f16c8_decode(o)
        return (hi + lo).cpu()
    return (o[0].float() + o[1].float()).cpu()


def _attn_assert(got, ref, eps, what, kind="native"):
    err = (got - ref).abs()
    tol = 6 * eps * max(1.0, ref.abs().max().item()) + 2e-5
    if kind == "fp8":       # on top of the pass's bound the e4m3 rounding of the result: 2^-4 relative (3 mantissa bits), 2^-10 below 2^-6
        assert (err < tol + ref.abs() * 2.0 ** -4 + 2.0 ** -10).all(), (what, err.max().item())
        return
    assert err.max().item() < tol, (what, err.max().item())


# (seq, head_dim) -> the kernel form bd_attention runs it on: (kernel, waves) of hip_ops.attention_plan, asserted before the launch.  The
# split-bf16 classes have no ping-pong instance: where the one-plane classes take it they run attn_kernel on 4 waves.
_FORMS = {
    (261, 64): ("tiled", 3),     # attn_kernel, 3 waves (96-query blocks), ragged tail of 5 keys (the peeled small-tail tile)
    (257, 64): ("tiled", 3),     # 3 waves, a tail tile with ONE live key
    (250, 64): ("tiled", 4),     # attn_kernel, 4 waves, ragged tail of 58 keys
    (300, 96): ("tiled", 4),     # attn_kernel hd 96, ragged tail of 44 keys
    (321, 96): ("tiled", 4),     # hd 96, a tail tile with one live key
    (1000, 96): ("tiled", 4),    # hd 96, 16 key tiles, ragged
    (512, 96): ("pp", 8),        # attn_kernel_pp for single-pass classes (256-query blocks, whole tiles); split-bf16: attn_kernel NS = 2
    (1536, 96): ("pp", 8),       # attn_kernel_pp, 24 key tiles (BETR's sequence at T = 6)
}
# The table rows (bd_attention_instance) that no other GPU test launches, one case each (tests/test_attention_plan_host.py counts them):
# the ragged instance of attn_kernel for the one-plane classes -- bd_attention_varlen takes it where tokens_per_view is no multiple of
# 256 -- on a packed batch of 1 and 2 views of 128 tokens.  Three of those classes have no entry in _VARIANTS; their result classes are
# no less exact than their f16 / bf16 pass (split planes: ~2^-16 and ~2^-22), except e4m3 (_attn_assert).
RAGGED = "ragged"
_ROW_VARIANTS = {
    **_VARIANTS,
    "f16_out_bf16x3": ("fp16", "PREC_F16_OUT_BF16X3", "planes", 2.0 ** -11),
    "f16_out_f16x3": ("fp16", "PREC_F16_OUT_F16X3", "planes_f16", 2.0 ** -11),
    "bf16_out_fp8": ("bf16", "PREC_BF16_OUT_FP8", "fp8", 2.0 ** -8),
}
_ROW_CASES = [(v, RAGGED, 96) for v in ("bf16", "fp16", "f16_out_f16c8", "f16_out_bf16x3", "f16_out_f16x3", "bf16_out_fp8")]
RAGGED_TPV, RAGGED_COUNTS = 128, (1, 2)
_STEERED = [(v, seq, hd) for seq, hd in _FORMS for v in sorted(_VARIANTS)] + _ROW_CASES


def steered_plan(variant, seq, hd):
    """The plan of a case of test_attention_online_softmax_steered, held against the form the case is about."""
    in_prec, code, _, _ = _ROW_VARIANTS[variant]
    heads, pid = len(PATTERNS), getattr(_lib, code)
    if seq == RAGGED:
        plan = hip_ops.attention_plan("varlen", prec=pid, batch=len(RAGGED_COUNTS), n_views=sum(RAGGED_COUNTS), max_views=max(RAGGED_COUNTS),
                                      tokens_per_view=RAGGED_TPV, heads=heads, head_dim=hd)
        assert (plan["kernel"], plan["waves"], plan["vl"], plan["planes"]) == ("tiled", 4, True, 1), plan
        return plan
    plan = hip_ops.attention_plan("plain", prec=pid, batch=1, seq=seq, heads=heads, head_dim=hd)
    want = ("tiled", 4) if in_prec == "bf16x3" and _FORMS[seq, hd][0] == "pp" else _FORMS[seq, hd]
    assert (plan["kernel"], plan["waves"], plan["head_dim"], plan["vl"]) == (*want, hd, False), plan
    return plan


@pytest.mark.parametrize("variant,seq,hd", _STEERED, ids=[f"{seq}-{hd}-{v}" for v, seq, hd in _STEERED])
def test_attention_online_softmax_steered(hip, variant, seq, hd):
    """Online softmax under steered logits (one pattern per head, _steer): the rescale branch taken in every tile, never taken, taken on
    the last key of a ragged tail, an alpha that underflows to 0, equal maxima, all-zero logits -- against fp64 torch.  Every case
    asserts through the plan that it runs the kernel form it is about (_FORMS, _ROW_CASES)."""
    in_prec, code, kind, eps = _ROW_VARIANTS[variant]
    heads = len(PATTERNS)
    steered_plan(variant, seq, hd)
    lib = _lib.load()
    split = in_prec == "bf16x3"
    if seq == RAGGED:                                    # every sample its own steered sequence, packed back to back
        parts = [_steered_case(1, c * RAGGED_TPV, hd, in_prec) for c in RAGGED_COUNTS]
        t = torch.cat([p[0] for p in parts], 1 if split else 0).contiguous()
        ref = torch.cat([p[1] for p in parts], 1)
        rows = ref.shape[1]
        out = _attn_out(kind, in_prec, rows, heads * hd)
        vs = torch.tensor(_lib.view_starts(RAGGED_COUNTS), dtype=torch.int32).cuda()
        _lib.check(lib.bd_attention_varlen(_lib.ptr(t), t[0].numel() if split else 0, _lib.ptr(out), _attn_out_plane(out, kind), _lib.ptr(vs),
                                           len(RAGGED_COUNTS), sum(RAGGED_COUNTS), max(RAGGED_COUNTS), RAGGED_TPV, heads, hd, hd ** -0.5, None,
                                           getattr(_lib, code), _lib.stream()), "bd_attention_varlen")
    else:
        t, ref = _steered_case(1, seq, hd, in_prec)
        rows = seq
        out = _attn_out(kind, in_prec, rows, heads * hd)
        _lib.check(lib.bd_attention(_lib.ptr(t), t[0].numel() if split else 0, _lib.ptr(out), _attn_out_plane(out, kind),
                                    1, seq, heads, hd, hd ** -0.5, getattr(_lib, code), _lib.stream()), "bd_attention")
    torch.cuda.synchronize()
    got = _attn_read(out, kind).reshape(1, rows, heads, hd)
    for h, pat in enumerate(PATTERNS):
        _attn_assert(got[:, :, h], ref[:, :, h], eps, (variant, seq, hd, pat), kind)


@pytest.mark.parametrize("variant", sorted(_VARIANTS))
def test_attention_prefix_patch_queries_steered(hip, variant):
    """bd_attention_prefix with prefix_queries = 0 (the last DINOv2 block: only the patch queries, exact query tiles) on the steered
    logits."""
    in_prec, code, kind, eps = _VARIANTS[variant]
    batch, seq, hd, npre, heads = 1, 261, 64, 5, len(PATTERNS)
    t, ref = _steered_case(batch, seq, hd, in_prec)
    out = _attn_out(kind, in_prec, batch * seq, heads * hd)
    lib = _lib.load()
    _lib.check(lib.bd_attention_prefix(_lib.ptr(t), t[0].numel() if in_prec == "bf16x3" else 0, _lib.ptr(out),
                                       0 if kind == "native" else out[0].numel(), batch, seq, heads, hd, hd ** -0.5, npre, 0,
                                       getattr(_lib, code), _lib.stream()), "bd_attention_prefix")
    torch.cuda.synchronize()
    got = _attn_read(out, kind).reshape(batch, seq, heads, hd)
    for h, pat in enumerate(PATTERNS):
        _attn_assert(got[:, npre:, h], ref[:, npre:, h], eps, (variant, pat))


@pytest.mark.parametrize("variant", sorted(_VARIANTS))
def test_attention_query_view_steered(hip, variant):
    """bd_attention_q (the last decoder block): the queries of one 256-row view per sample, all 512 keys, on the steered logits."""
    in_prec, code, kind, eps = _VARIANTS[variant]
    batch, seq, hd, P, heads = 2, 512, 96, 256, len(PATTERNS)
    t, ref = _steered_case(batch, seq, hd, in_prec)
    qv = torch.tensor([1, 0], dtype=torch.int32)
    out = _attn_out(kind, in_prec, batch * P, heads * hd)
    lib = _lib.load()
    qvd = qv.cuda()
    _lib.check(lib.bd_attention_q(_lib.ptr(t), t[0].numel() if in_prec == "bf16x3" else 0, _lib.ptr(out),
                                  0 if kind == "native" else out[0].numel(), batch, seq, heads, hd, hd ** -0.5, _lib.ptr(qvd), P,
                                  getattr(_lib, code), _lib.stream()), "bd_attention_q")
    torch.cuda.synchronize()
    got = _attn_read(out, kind).reshape(batch, P, heads, hd)
    for b in range(batch):
        _attn_assert(got[b], ref[b, qv[b] * P:(qv[b] + 1) * P], eps, (variant, b))
