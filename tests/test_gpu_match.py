"""bd_dino_match_scores (csrc/match.hip: match_sums_kernel, match_scores_kernel) called directly, so that all three outputs are seen:
`sums` (per view: the sum of the foreground patches' unit vectors), `counts` (per view: foreground patches) and `scores`.

References, all on the CPU (oracle/dense_oracle.py):
  - foreground_mask: the reference's fp32 luminance mask -- `counts` must equal its count EXACTLY (one flipped patch moves a score by
    1e4 c_other / L^2, far more than any rounding);
  - an fp64 restatement of sums / counts (below) and dino_matching_scores_closed_form for the values, within bounds derived from the
    kernels' summation orders (_check), not a flat tolerance;
  - dino_matching_scores (the reference's own order of operations) for what empty views and non-finite features must give.
Every launch writes into the middle of larger buffers filled with a bit pattern (nothing outside the documented extents may change)
and runs twice (identical bits).  The argument refusals at the end need no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib
from oracle import dense_oracle as do

gpu = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24            # fp32 unit roundoff
PAD = 67                  # guard elements either side of every output (odd: the outputs start at no special alignment)
GUARD = 0x7FC0BD00        # guard words: NaNs with a payload
THR = 0.05


def _guarded(n):
    buf = (torch.arange(n + 2 * PAD, dtype=torch.int32) % 251 + GUARD).cuda()
    return buf, buf.clone()


def _launch(feats, images, q, B, T, L, D, H, W, thr=THR):
    """One direct call.  feats / images / q: device tensors.  -> (sums [B T, D], counts [B T], scores [B, T - 1]) on the host as fp32,
    after checking that nothing outside those extents changed."""
    lib = _lib.load()
    bufs = [_guarded(n) for n in (B * T * D, B * T, B * (T - 1))]
    outs = [b[0].view(torch.float32)[PAD:PAD + n] for b, n in zip(bufs, (B * T * D, B * T, B * (T - 1)))]
    _lib.check(lib.bd_dino_match_scores(_lib.ptr(feats), _lib.ptr(images), _lib.dtype_id(images), _lib.ptr(q), B, T, L, D, H, W, thr,
                                        _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream()), "bd_dino_match_scores")
    torch.cuda.synchronize()
    for (buf, orig), n in zip(bufs, (B * T * D, B * T, B * (T - 1))):
        assert torch.equal(buf[:PAD], orig[:PAD]) and torch.equal(buf[PAD + n:], orig[PAD + n:]), "wrote outside its output"
    return outs[0].cpu().reshape(B * T, D), outs[1].cpu(), outs[2].cpu().reshape(B, T - 1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(feats, images, q, thr=THR):
    """feats (B, T, L, D) fp32, images (B, T, 3, H, W), q (B,) on the host -> the three outputs; launched twice, identical bits."""
    B, T, L, D = feats.shape
    H, W = images.shape[-2:]
    fd, im, qd = feats.contiguous().cuda(), images.contiguous().cuda(), q.to(torch.int32).cuda()
    a = _launch(fd, im, qd, B, T, L, D, H, W, thr)
    b = _launch(fd, im, qd, B, T, L, D, H, W, thr)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), "two identical calls gave different bits"
    return a


def _reference(feats, images, thr=THR):
    """fp64 restatement of match_sums_kernel's outputs on the oracle's fp32 mask: (mask (V, L), sums (V, D), sum of |terms| (V, D),
    counts (V,))."""
    B, T, L, D = feats.shape
    m = do.foreground_mask(images.reshape(B * T, *images.shape[2:]).float(), L, thr).double()
    f = feats.reshape(B * T, L, D).double()
    n = f / f.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    n = torch.where(m.unsqueeze(-1) > 0, n, torch.zeros_like(n))           # a background patch contributes nothing, whatever it holds
    return m, n.sum(1), n.abs().sum(1), m.sum(1)


def _refs_of(q, T):
    return torch.stack([torch.tensor([t for t in range(T) if t != int(qb)]) for qb in q])           # (B, T - 1): view order


def _closed_form(s, c, q, L):
    """fp64 scores from per-view sums (B, T, D) and counts (B, T); also the sum of |s_q s_r| the dot product's bound needs."""
    B, T, D = s.shape
    r = _refs_of(q, T)
    ar = torch.arange(B)
    sq, cq = s[ar, q.long()].unsqueeze(1), c[ar, q.long()].unsqueeze(1)
    sr, cr = s[ar.unsqueeze(1), r], c[ar.unsqueeze(1), r]
    invalid = L * L - cq * cr
    return ((sq * sr).sum(-1) - 1e4 * invalid) / float(L * L), (sq * sr).abs().sum(-1), invalid


def _check(feats, images, q, got, thr=THR):
    """counts exactly; sums and scores within their summation bounds.  Returns the largest error / bound of (sums, scores).
      sums:   L fused multiply-adds in patch order, each term f * inv with inv = 1 / max(sqrt(ss), 1e-12) a few ulps from exact:
              |err| <= (L + 8) 2^-24 sum_l |n_l[d]| m_l   (recursive summation of L terms + the few-ulp inverse norm)
      scores: (dot - 1e4 (L^2 - c_q c_r)) / L^2:  three roundings at the magnitude of 1e4 (L^2 - c_q c_r) (product, difference, quotient;
              half a spacing each: 2 spacings cover them), and the dot product of two computed sums: D fused terms + the wave's tree,
              each factor carrying its own (L + 8) 2^-24 from above: (D + 2 L + 16) 2^-24 sum_d |s_q[d] s_r[d]|."""
    B, T, L, D = feats.shape
    sums, counts, scores = got
    m, s64, sabs, c64 = _reference(feats, images, thr)
    assert torch.equal(counts.double(), c64), "foreground counts differ from the reference's fp32 luminance mask"
    bound_s = (L + 8) * U * sabs + 1e-30
    r_s = ((sums.double() - s64).abs() / bound_s).max().item()
    # the oracle's closed form on the same inputs is the fp64 value of the scores ...
    ex, dabs, invalid = _closed_form(s64.reshape(B, T, D), c64.reshape(B, T), q, L)
    r = _refs_of(q, T)
    ar = torch.arange(B)
    orc = do.dino_matching_scores_closed_form(feats[ar.unsqueeze(1), r], feats[ar, q.long()], images[ar.unsqueeze(1), r].float(),
                                              images[ar, q.long()].float())
    assert (orc - ex).abs().max().item() <= 1e-9 * (1 + ex.abs().max().item())
    spacing = torch.from_numpy(np.spacing((1e4 * invalid).numpy().astype(np.float32)).astype(np.float64))
    bound = (2 * torch.where(invalid > 0, spacing, torch.zeros_like(spacing)) + (D + 2 * L + 16) * U * dabs) / float(L * L) + 1e-30
    r_m = ((scores.double() - ex).abs() / bound).max().item()
    print(f"match B={B} T={T} L={L} D={D} HxW={tuple(images.shape[-2:])} {images.dtype}: sums err/bound {r_s:.3f}, "
          f"scores err/bound {r_m:.3f}, fg {c64.sum().item() / m.numel():.2f}")
    assert r_s <= 1.0, f"sums: error / bound = {r_s}"
    assert r_m <= 1.0, f"scores: error / bound = {r_m}"
    return r_s, r_m


def _inputs(seed, B, T, L, D, H, W, dtype):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((B, T, L, D)).astype(np.float32) * rng.uniform(0.05, 20.0, (B, T, L, 1)).astype(np.float32)
    rgb = rng.uniform(0.0, 1.0, (B, T, 3, H, W)).astype(np.float32)
    rgb *= rng.uniform(0.0, 1.0, (B, T, 1, H, W)) < 0.6                     # black pixels: ~40 % background
    rgb[:, :, :, : H // 3] *= np.float32(0.1)                                  # and a dim band whose luminance straddles the threshold
    return torch.from_numpy(feats), torch.from_numpy(rgb).to(dtype)


def _queries(mode, B, T, seed):
    if mode == "first":
        return torch.zeros(B, dtype=torch.int32)
    if mode == "last":
        return torch.full((B,), T - 1, dtype=torch.int32)
    if mode == "middle":
        return torch.full((B,), T // 2, dtype=torch.int32)
    q = torch.from_numpy(np.random.default_rng(seed).integers(0, T, B).astype(np.int32))
    q[0], q[-1] = T - 1, 0
    return q


# B, T, L, D, H, W, image dtype, query view.  Every L in {1, 4, 49, 256, 1024} (1024 = MAXL), D in {1, 64, 96, 384, 768, 1000}
# (a partial wave, a partial 256-thread stride, production), (H, W) in {224^2, 225 x 131, 37 x 80, 8^2 under g = 16 (nearest UPsampling),
# 518^2, (g, g)}, T in {2, 3, 17}, B in {1, 5, 64}, every dtype and every query placement occurs.
CASES = [
    (1, 2, 1, 1, 1, 1, F32, "first"),
    (1, 3, 1, 64, 37, 80, BF16, "last"),
    (64, 2, 1, 96, 37, 80, BF16, "per"),
    (5, 2, 4, 1, 2, 2, F16, "per"),
    (64, 2, 4, 64, 8, 8, F32, "per"),
    (5, 3, 4, 1000, 225, 131, F32, "middle"),
    (1, 17, 4, 384, 224, 224, F16, "last"),
    (1, 17, 49, 96, 224, 224, BF16, "middle"),
    (5, 3, 49, 384, 37, 80, F16, "per"),
    (1, 2, 49, 768, 7, 7, F32, "first"),
    (64, 3, 49, 96, 37, 80, F32, "per"),
    (1, 3, 49, 1, 518, 518, F32, "first"),
    (5, 17, 49, 64, 8, 8, F16, "per"),
    (1, 3, 256, 768, 224, 224, F32, "last"),
    (5, 2, 256, 64, 8, 8, BF16, "per"),
    (1, 2, 256, 384, 518, 518, F16, "first"),
    (1, 3, 256, 96, 225, 131, F32, "middle"),
    (5, 17, 256, 64, 16, 16, F32, "per"),
    (1, 2, 256, 1000, 37, 80, F32, "first"),
    (64, 3, 256, 1, 16, 16, BF16, "per"),
    (1, 2, 1024, 64, 224, 224, F32, "last"),
    (1, 3, 1024, 1, 32, 32, BF16, "middle"),
    (1, 2, 1024, 96, 518, 518, F32, "first"),
    (1, 3, 1024, 1000, 37, 80, F16, "per"),
    (1, 2, 1024, 768, 225, 131, BF16, "last"),
]


@gpu
@pytest.mark.parametrize("B,T,L,D,H,W,dtype,qmode", CASES)
def test_match_outputs_against_fp64(hip, B, T, L, D, H, W, dtype, qmode):
    """Random features and images with ~40 % black pixels and a dim band around the threshold.  Largest error / bound over the 25 cases
    on an MI355X: sums 0.29, scores 0.38 (see _check for the bounds)."""
    seed = 1000 * L + D + 7 * B + T
    feats, images = _inputs(seed, B, T, L, D, H, W, dtype)
    q = _queries(qmode, B, T, seed)
    _check(feats, images, q, _run(feats, images, q))


@gpu
def test_sample_alone_equals_the_sample_inside_a_batch_of_64(hip):
    B, T, L, D, H, W = 64, 3, 49, 96, 37, 80
    feats, images = _inputs(4242, B, T, L, D, H, W, F32)
    q = _queries("per", B, T, 4242)
    sums, counts, scores = _run(feats, images, q)
    for b in (0, 17, 63):
        s1, c1, m1 = _run(feats[b:b + 1], images[b:b + 1], q[b:b + 1])
        assert torch.equal(_bits(s1), _bits(sums[b * T:(b + 1) * T])) and torch.equal(_bits(c1), _bits(counts[b * T:(b + 1) * T]))
        assert torch.equal(_bits(m1), _bits(scores[b:b + 1]))


# ------------------------------------------------------------------------------------------------------------------ steered data

G, LS, DS = 7, 49, 96            # steered views: (g, g) images, so every pixel is one patch's sample


def _views_from_masks(masks, seed):
    """masks (V, 49) 0/1 -> images (V, 3, 7, 7): foreground pixels mid-grey-ish, background pixels black; random features"""
    rng = np.random.default_rng(seed)
    V = masks.shape[0]
    rgb = rng.uniform(0.3, 1.0, (V, 3, G, G)).astype(np.float32) * masks.reshape(V, 1, G, G).astype(np.float32)
    feats = rng.standard_normal((V, LS, DS)).astype(np.float32)
    return torch.from_numpy(feats), torch.from_numpy(rgb)


def _steered_views(seed):
    """One sample of 5 views: 0 no foreground, 1 all foreground, 2 exactly one foreground patch, 3 and 4 random masks"""
    rng = np.random.default_rng(seed)
    masks = np.zeros((5, LS), np.int64)
    masks[1] = 1
    masks[2, 23] = 1
    masks[3:] = rng.uniform(size=(2, LS)) < 0.5
    masks[3, 5], masks[3, 6] = 1, 0                      # view 3: patch 5 foreground, patch 6 background (the non-finite tests rely on it)
    feats, rgb = _views_from_masks(masks, seed)
    return feats.unsqueeze(0), rgb.unsqueeze(0), torch.from_numpy(masks)


def _ref_order(feats, images, q):
    """the reference's own order of operations (fp32 bmm, masked_fill, mean, nan_to_num) on the CPU"""
    B, T = feats.shape[:2]
    r, ar = _refs_of(q, T), torch.arange(B)
    return do.dino_matching_scores(feats[ar.unsqueeze(1), r], feats[ar, q.long()], images[ar.unsqueeze(1), r], images[ar, q.long()])


REF_ORDER_NOISE = 2e-2           # the reference-order fp32 mean of L^2 terms of magnitude 1e4 against its fp64 value (test_dense_mode.py)


@gpu
@pytest.mark.parametrize("qv", [0, 1, 2, 3])
def test_empty_full_and_single_patch_views(hip, qv):
    """A view without foreground scores exactly -1e4 as query and as reference; all-foreground and one-patch views; a zero feature row
    in a foreground patch (counted, contributes a zero vector)."""
    feats, images, masks = _steered_views(31)
    feats[0, 1, 10] = 0.0                                # view 1, foreground patch 10: a zero row
    feats[0, 3, 5] = 0.0
    q = torch.tensor([qv], dtype=torch.int32)
    m = do.foreground_mask(images[0], LS)
    assert torch.equal(m.long(), masks) and m.sum(1).tolist()[:3] == [0.0, 49.0, 1.0]
    got = _run(feats, images, q)
    _check(feats, images, q, got)
    sums, counts, scores = got
    ref = _ref_order(feats, images, q)
    r = _refs_of(q, 5)[0].tolist()
    assert torch.equal(sums[0], torch.zeros(DS)) and _bits(sums[0]).eq(0).all()                    # +0, not -0
    if qv == 0:
        assert (scores == -1e4).all() and (ref == -1e4).all()
    else:
        assert scores[0, r.index(0)].item() == -1e4 and ref[0, r.index(0)].item() == -1e4
    assert (scores.double() - ref.double()).abs().max().item() <= REF_ORDER_NOISE


@gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", ["foreground", "background"])
@pytest.mark.parametrize("qv", [3, 1])
def test_non_finite_features(hip, value, where, qv):
    """One non-finite feature element in view 3 (the query view, or a reference).  In a FOREGROUND patch the reference's normalised row is
    NaN and nan_to_num turns every score touching the view into 0 -- except against the view without foreground (view 0), where the
    reference's masked_fill replaces every pair with -1e4 first: exactly -1e4.  In a BACKGROUND patch masked_fill replaces every pair
    of that patch, so the scores are what they are without the element.  Other pairs are unaffected either way."""
    feats, images, masks = _steered_views(57)
    clean = feats.clone()
    patch = 5 if where == "foreground" else 6
    assert masks[3, patch] == (1 if where == "foreground" else 0)
    feats[0, 3, patch, 11] = value
    q = torch.tensor([qv], dtype=torch.int32)
    ref = _ref_order(feats, images, q)
    ref_clean = _ref_order(clean, images, q)
    r = _refs_of(q, 5)[0].tolist()
    touched = [True] * 4 if qv == 3 else [v == 3 for v in r]
    other = [v for v in r] if qv == 3 else [qv] * 4       # the pair's view that is not view 3
    expect = [-1e4 if masks[o].sum() == 0 else 0.0 for o in other]
    assert -1e4 in expect or qv != 3
    for n, t in enumerate(touched):                      # what the reference does, asserted on the host
        if t and where == "foreground":
            assert ref[0, n].item() == expect[n]
        else:
            assert abs(ref[0, n].item() - ref_clean[0, n].item()) <= REF_ORDER_NOISE and ref[0, n].item() != 0.0
    sums, counts, scores = _run(feats, images, q)
    assert torch.equal(counts.long(), masks.sum(1))
    if where == "background":                            # the element is never used: the same BITS as without it
        s0, c0, m0 = _run(clean, images, q)
        assert torch.equal(_bits(sums), _bits(s0)) and torch.equal(_bits(scores), _bits(m0))
        _check(clean, images, q, (sums, counts, scores))
    else:
        s0, c0, m0 = _run(clean, images, q)
        for n, t in enumerate(touched):
            if t:
                assert scores[0, n].item() == expect[n] and (expect[n] != 0.0 or _bits(scores)[0, n].item() == 0)
            else:
                assert _bits(scores)[0, n].item() == _bits(m0)[0, n].item()
        others = [v for v in range(5) if v != 3]
        assert torch.equal(_bits(sums[others]), _bits(s0[others]))
    assert (scores.double() - ref.double()).abs().max().item() <= REF_ORDER_NOISE


# ------------------------------------------------------------------------------------------------------------------ the threshold

C_R, C_G, C_B = np.float32(0.299), np.float32(0.587), np.float32(0.114)


def _lum_separate(R, G, B):
    """fp32, every product and sum rounded: what torch computes for 0.299 R + 0.587 G + 0.114 B"""
    return ((C_R * R + C_G * G).astype(np.float32) + C_B * B).astype(np.float32)


def _fma32(a, b, c):
    """fp32 fma(a, b, c) through fp64: the product of two fp32 numbers is exact in fp64; the fp64 sum is rounded once more to fp32 (a
    double rounding in rare cases -- immaterial here: this emulation only has to show that a fused order CAN differ on the draw)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lum_fused(R, G, B):
    """the contracted order: fma(0.114, B, fma(0.299, R, 0.587 G))"""
    return _fma32(np.full_like(B, C_B), B, _fma32(np.full_like(R, C_R), R, (C_G * G).astype(np.float32)))


def _threshold_pixels(n, seed):
    """n float pixels whose exact luminance is the threshold to within the rounding of B: R uniform in [0, 0.1), G uniform in [0, 0.04),
    B solved in fp64.  Their fp32 luminance lands on the threshold or an ulp either side of it."""
    rng = np.random.default_rng(seed)
    R = rng.uniform(0.0, 0.1, n).astype(np.float32)
    G = rng.uniform(0.0, 0.04, n).astype(np.float32)
    B = ((THR - 0.299 * R.astype(np.float64) - 0.587 * G.astype(np.float64)) / 0.114).astype(np.float32)
    return R, G, B


def _assert_draw_has_teeth(R, G, B):
    thr = np.float32(THR)
    sep, fused = _lum_separate(R, G, B), _lum_fused(R, G, B)
    n = R.size
    differ = np.count_nonzero((sep > thr) != (fused > thr)) / n
    assert differ >= 0.01, f"only {differ:.3%} of the steered pixels tell the fused order from the separately rounded one"
    # the draw covers the threshold itself (strict >: background) and both sides of it
    assert min(np.count_nonzero(sep == thr), np.count_nonzero(sep > thr), np.count_nonzero(sep < thr)) >= n // 20
    return differ


def _one_hot_feats(V, L):
    """features whose patch l is the unit vector e_l (D = L): sums[v, d] is exactly 1.0 where patch d is foreground, else 0"""
    return torch.eye(L).expand(V, L, L).contiguous()


@gpu
@pytest.mark.parametrize("planted", [False, True])
def test_threshold_sweep(hip, planted):
    """Float pixels within an ulp of the luminance threshold.  The kernel's mask (read back through one-hot features) and its counts must
    equal the reference's fp32 mask, whose luminance rounds every product and sum: a fused evaluation flips ~18 % of these pixels
    (asserted on the host first: at least 1 %).  A pixel whose fp32 luminance EQUALS the threshold is background.  planted: the same
    kind of pixels at the nearest-resize sample positions of 224 x 224 images, random pixels elsewhere."""
    g, L = 16, 256
    B, T = (8, 4) if planted else (32, 4)
    V = B * T
    R, G, Bl = _threshold_pixels(V * L, seed=99 + planted)
    differ = _assert_draw_has_teeth(R, G, Bl)
    pix = np.stack([R, G, Bl], 0).reshape(3, V, g, g).transpose(1, 0, 2, 3)
    if planted:
        H = W = 224
        img = np.random.default_rng(5).uniform(0.0, 0.1, (V, 3, H, W)).astype(np.float32)
        img[:, :, ::14, ::14] = pix                      # floor(i * 224 / 16) = 14 i
    else:
        H = W = g
        img = np.ascontiguousarray(pix)
    images = torch.from_numpy(img).reshape(B, T, 3, H, W)
    want = do.foreground_mask(images.reshape(V, 3, H, W), L)
    thr = np.float32(THR)
    sep = _lum_separate(R, G, Bl).reshape(V, L)
    assert np.array_equal(want.numpy() > 0, sep > thr)                        # the oracle is the separately rounded order, strict >
    assert np.count_nonzero(sep == thr) >= V * L // 20 and not want.numpy()[sep == thr].any()
    feats = _one_hot_feats(V, L).reshape(B, T, L, L)
    q = torch.arange(B, dtype=torch.int32) % T
    sums, counts, scores = _run(feats, images, q)
    wrong = (sums != want)
    print(f"threshold sweep planted={planted}: {V * L} pixels, fused/separate disagree on {differ:.1%} on the host, "
          f"kernel mask differs from the reference's on {int(wrong.sum())}")
    assert not wrong.any(), f"{int(wrong.sum())} of {V * L} patches on the other side of the threshold than in the reference"
    assert torch.equal(counts, want.sum(1))
    _check(feats, images, q, (sums, counts, scores))


@gpu
def test_luminance_equal_to_the_threshold_is_background(hip):
    """Grey and single-channel pixels whose fp32 luminance is exactly the threshold, one ulp above it and one below it, with a threshold
    that is itself a computed luminance (so equality is certain, in 16-bit images too)."""
    for dtype in (F32, BF16, F16):
        v = torch.tensor([0.3, 0.3, 0.3]).to(dtype).float().numpy()
        lum = _lum_separate(v[0:1], v[1:2], v[2:3])[0]
        up, down = np.nextafter(lum, np.float32(1)), np.nextafter(lum, np.float32(0))
        img = torch.from_numpy(np.tile(v.reshape(1, 3, 1, 1), (2, 1, 2, 2))).to(dtype).reshape(1, 2, 3, 2, 2)
        feats = _one_hot_feats(2, 4).reshape(1, 2, 4, 4)
        q = torch.zeros(1, dtype=torch.int32)
        for thr, fg in ((float(lum), 0.0), (float(down), 4.0), (float(up), 0.0)):
            sums, counts, scores = _run(feats, img, q, thr)
            assert counts.tolist() == [fg, fg], (dtype, thr)
            assert torch.equal(counts, do.foreground_mask(img[0].float(), 4, thr).sum(1))


# ------------------------------------------------------------------------------------------------------------------ refusals (no GPU)

P1 = ctypes.c_void_p(0x10000)          # a non-NULL address that no refused call may touch


def test_match_scores_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()

    def call(feats=P1, images=P1, dt=_lib.DTYPE_F32, q=P1, B=2, T=3, L=256, D=768, H=224, W=224, sums=P1, counts=P1, scores=P1):
        return lib.bd_dino_match_scores(feats, images, dt, q, B, T, L, D, H, W, THR, sums, counts, scores, None)

    for name in ("feats", "images", "q", "sums", "counts", "scores"):
        assert call(**{name: None}) == -5, name                                  # BD_ERR_NULL
    assert call(T=1) == -1 and call(T=0) == -1                                   # BD_ERR_SHAPE: a query needs a reference
    assert call(L=0) == -1 and call(L=1025) == -1                                # MAXL = 1024
    assert call(D=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(B=0) == -1
    assert call(dt=3) == -2 and call(dt=-1) == -2                                # BD_ERR_DTYPE: f32 / bf16 / f16 images only
