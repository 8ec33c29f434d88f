"""GPU: a pose stream that chooses each frame's references on the device (stream.PoseStream(select_k=...); csrc/stream.hip:
bd_stream_select_rows).

The kernel against the two kernels whose arithmetic it shares (bd_match_select_rows, bd_pose_select_rows) and against its host
mirror, on whole guarded buffers; a selecting session against the eager banked forward over the references the existing wrappers
choose for the same frame, bit for bit."""
import gc

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, synth
from boxdreamer_amd import preprocess as pp
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.stream import PoseStream, select_rows_host
from test_dense_rounds_host import spread_poses
from test_gpu_ragged import _to_dev
from test_gpu_stream import H, S, W, _assert_step, _eq, _guard_intact, _guarded, _inputs, _shared

pytestmark = pytest.mark.gpu

NO_VIEW = 0x7FFFFFFF
DINO, TRACK = _lib.STREAM_SELECT_DINO, _lib.STREAM_SELECT_TRACK


# ---- the kernel
def _rigid(n, seed):
    """n seeded rigid poses in front of the camera, fp32 (n, 4, 4)."""
    r = np.random.default_rng(seed)
    q = r.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    out = np.zeros((n, 4, 4), np.float32)
    out[:, :3, :3] = R
    out[:, :3, 3] = np.stack([r.uniform(-0.5, 0.5, n), r.uniform(-0.5, 0.5, n), r.uniform(2, 6, n)], 1)
    out[:, 3, 3] = 1.0
    return torch.from_numpy(out)


def _identity_cand(n_refs, n_max):
    return torch.tensor([[i if i < n else -1 for i in range(n_max)] for n in n_refs], dtype=torch.int32, device="cuda")


def _prev_rows(pred, ok, rms):
    prev = torch.zeros((len(ok), _lib.STREAM_ROW_FLOATS), dtype=torch.float32)
    prev[:, :16] = pred.reshape(-1, 16)
    prev[:, 16], prev[:, 17] = torch.tensor(rms, dtype=torch.float32), torch.tensor(ok, dtype=torch.float32)
    prev[:, 18:] = 7.5                                          # (the corner and box slots are not the kernel's business)
    return prev


def _src_of(sel, rows, R):
    """The source table that goes with a host selection: the chosen slots' rows (0x7fffffff: none, or outside the store), then -(b + 1)."""
    rows = rows.cpu().tolist()
    return [[(rows[b][i] if i >= 0 and 0 <= rows[b][i] < R else NO_VIEW) for i in row] + [-(b + 1)] for b, row in enumerate(sel.tolist())]


def _run_guarded(sums, counts, poses, R, q_sums, q_counts, prev, rows, n_refs, force, L, k, rule, max_rms):
    """One launch into guarded buffers -> (scores, dist, used, sel, src), the guards checked."""
    B, n_max = rows.shape
    bufs = [_guarded(B, (n_max,), torch.float32, -77.0), _guarded(B, (n_max,), torch.float32, -77.0), _guarded(B, (), torch.int32, -77),
            _guarded(B, (k,), torch.int32, -77), _guarded(B * (k + 1), (), torch.int32, -77)]
    if poses is None:
        bufs[1] = (None, None)
    out = hip_ops.stream_select_rows(sums, counts, poses, R, q_sums, q_counts, prev, rows, n_refs, force, L, k, rule, max_rms,
                                     scores=bufs[0][1], dist=bufs[1][1], used=bufs[2][1], sel=bufs[3][1], src=bufs[4][1])
    for (buf, _), fill in zip(bufs, (-77.0, -77.0, -77, -77, -77)):
        assert buf is None or _guard_intact(buf, fill)
    return out


def test_kernel_equals_the_two_selection_kernels_on_whole_buffers(hip):
    B, n_max, k, D, L, R, max_rms = 5, 7, 3, 100, 16, 9, 2.0
    n_refs_h = [7, 5, 3, 7, 7]
    g = torch.Generator().manual_seed(11)
    sums = torch.randn((R, D), generator=g).cuda()
    counts = torch.randint(1, L + 1, (R,), generator=g).float().cuda()
    q_sums = torch.randn((B, D), generator=g).cuda()
    q_counts = torch.randint(1, L + 1, (B,), generator=g).float().cuda()
    poses = _rigid(R, 12)
    poses[8, 0, 0] = float("nan")                               # a NaN distance ranks after every number
    pred = _rigid(B, 13)
    pred[0, :3, :3], pred[0, :3, 3] = poses[4, :3, :3], poses[4, :3, 3] + 0.01
    poses = poses.cuda()
    rows_h = [[5, 2, 0, 4, 7, 1, 8], [3, 8, 6, 0, 2, -1, -1], [1, 7, 4, -1, -1, -1, -1], [6, 0, 3, 8, 5, 2, 1], [2, 4, 8, 1, 7, 3, 0]]
    rows_h[3][2] = R + 3                                        # a row outside [0, R): no view under either rule
    # the five objects take: the pose rule, ok = 0, rms > max, rms = NaN, force
    prev = _prev_rows(pred, ok=[1, 0, 1, 1, 1], rms=[1.0, 1.0, 3.0, float("nan"), 1.0]).cuda()
    force = torch.tensor([0, 0, 0, 0, 5], dtype=torch.int32, device="cuda")
    n_refs = torch.tensor(n_refs_h, dtype=torch.int32, device="cuda")
    cand = _identity_cand(n_refs_h, n_max)
    # one object names the same private row twice, placed where the tie decides the selection: the slot that ranks 4th by distance
    # (object 0, the pose rule) gets the row of the slot that ranks 3rd
    rows = torch.tensor(rows_h, dtype=torch.int32, device="cuda")
    d0 = hip_ops.pose_select_rows(poses, R, pred.cuda(), rows, cand, k)[0][0].cpu().tolist()
    order = sorted(range(n_max), key=lambda i: (d0[i] != d0[i], 0.0 if d0[i] != d0[i] else d0[i], i))
    a, b = sorted(order[2:4])
    rows_h[0][b] = rows_h[0][a] = rows_h[0][order[2]]
    rows = torch.tensor(rows_h, dtype=torch.int32, device="cuda")

    want_scores, sel_m, src_m = hip_ops.match_select_rows(sums, counts, R, q_sums, q_counts, rows, n_refs, L, k)
    want_dist, sel_p, src_p = hip_ops.pose_select_rows(poses, R, pred.cuda(), rows, cand, k)
    src_m, src_p = src_m.reshape(B, k + 1), src_p.reshape(B, k + 1)
    assert want_scores[0, a] == want_scores[0, b] and want_dist[0, a] == want_dist[0, b]       # the tie, in both value arrays
    assert a in sel_p[0].tolist() and b not in sel_p[0].tolist()                               # ... and it decides: the lower slot
    assert torch.isinf(want_scores[3, 2]) and torch.isinf(want_dist[3, 2]) and torch.isnan(want_dist).any()

    scores, dist, used, sel, src = _run_guarded(sums, counts, poses, R, q_sums, q_counts, prev, rows, n_refs, force, L, k, TRACK, max_rms)
    assert _eq(scores, want_scores) and _eq(dist, want_dist)
    h_used, h_sel = select_rows_host(scores, dist, prev, force, n_refs, k, "track", max_rms)
    assert used.cpu().tolist() == h_used.tolist() == [1, 0, 0, 0, 0]
    want_sel = torch.where(used[:, None] == 1, sel_p, sel_m)
    want_src = torch.where(used[:, None] == 1, src_p, src_m)
    assert torch.equal(sel, want_sel) and torch.equal(src.reshape(B, k + 1), want_src)
    assert sel.cpu().tolist() == h_sel.tolist() and src.reshape(B, k + 1).tolist() == _src_of(h_sel, rows, R)
    assert sel[2].tolist() == [0, 1, 2]                         # n_refs == k: everything is chosen
    assert (src.reshape(B, k + 1)[:, k].cpu() == -(torch.arange(B) + 1)).all()
    # an object's bits do not depend on the batch
    one = _run_guarded(sums, counts, poses, R, q_sums[3:4], q_counts[3:4], prev[3:4], rows[3:4], n_refs[3:4], force[3:4], L, k, TRACK, max_rms)
    assert _eq(one[0], scores[3:4]) and _eq(one[1], dist[3:4]) and torch.equal(one[3], sel[3:4])
    assert one[4].tolist() == src_m[3, :k].tolist() + [-1]
    # the pose rule for everybody (no force, every pose trusted): a slot outside the store is never chosen, fewer than k valid slots
    trusted = _prev_rows(pred, ok=[1] * B, rms=[0.0] * B).cuda()
    rows_short = rows.clone()
    rows_short[2, 1] = -5
    want = hip_ops.pose_select_rows(poses, R, pred.cuda(), rows_short, cand, k)
    got = _run_guarded(sums, counts, poses, R, q_sums, q_counts, trusted, rows_short, n_refs, torch.zeros_like(force), L, k, TRACK, max_rms)
    assert got[2].tolist() == [1] * B and torch.equal(got[3], want[1]) and torch.equal(got[4], want[2]) and _eq(got[1], want[0])
    assert got[3][2].tolist() == [0, 2, -1] and got[4].reshape(B, k + 1)[2].tolist() == [rows_h[2][0], rows_h[2][2], NO_VIEW, -3]
    assert got[3].cpu().tolist() == select_rows_host(got[0], got[1], trusted, torch.zeros_like(force), n_refs, k, TRACK, max_rms)[1].tolist()
    # rule = DINO with poses = NULL: bd_match_select_rows, whatever the rows say
    scores, dist, used, sel, src = _run_guarded(sums, counts, None, R, q_sums, q_counts, prev, rows, n_refs, force, L, k, DINO, max_rms)
    assert dist is None and used.tolist() == [0] * B
    assert _eq(scores, want_scores) and torch.equal(sel, sel_m) and torch.equal(src.reshape(B, k + 1), src_m)
    assert sel.cpu().tolist() == select_rows_host(scores, None, prev, force, n_refs, k, "dino")[1].tolist()


def test_kernel_at_the_largest_database(hip):
    """N_max = 1024 with full n_refs: the strided loops; one object per rule."""
    B, n_max, k, D, L, R = 2, 1024, 20, 100, 16, 1100
    g = torch.Generator().manual_seed(21)
    sums = torch.randn((R, D), generator=g).cuda()
    counts = torch.randint(0, L + 1, (R,), generator=g).float().cuda()
    q_sums = torch.randn((B, D), generator=g).cuda()
    q_counts = torch.tensor([9.0, 12.0], device="cuda")
    poses, pred = _rigid(R, 22).cuda(), _rigid(B, 23)
    rows = torch.stack([torch.randperm(R, generator=g)[:n_max] for _ in range(B)]).to(torch.int32).cuda()
    n_refs = torch.full((B,), n_max, dtype=torch.int32, device="cuda")
    prev = _prev_rows(pred, ok=[1, 0], rms=[0.5, 0.5]).cuda()
    force = torch.zeros((B,), dtype=torch.int32, device="cuda")
    want_scores, sel_m, src_m = hip_ops.match_select_rows(sums, counts, R, q_sums, q_counts, rows, n_refs, L, k)
    want_dist, sel_p, src_p = hip_ops.pose_select_rows(poses, R, pred.cuda(), rows, _identity_cand([n_max] * B, n_max), k)
    scores, dist, used, sel, src = _run_guarded(sums, counts, poses, R, q_sums, q_counts, prev, rows, n_refs, force, L, k, TRACK, 1.0)
    assert _eq(scores, want_scores) and _eq(dist, want_dist) and used.tolist() == [1, 0]
    assert torch.equal(sel[0], sel_p[0]) and torch.equal(sel[1], sel_m[1])
    src, src_m, src_p = src.reshape(B, k + 1), src_m.reshape(B, k + 1), src_p.reshape(B, k + 1)
    assert torch.equal(src[0], src_p[0]) and torch.equal(src[1], src_m[1])
    h_used, h_sel = select_rows_host(scores, dist, prev, force, n_refs, k, "track", 1.0)
    assert h_used.tolist() == [1, 0] and sel.cpu().tolist() == h_sel.tolist() and src.tolist() == _src_of(h_sel, rows, R)
    assert int(sel.max()) >= 256                                # slots past a workgroup's first pass were in play


# ---- a selecting session against the eager forward
DATABASES, K_SEL, MAX_RMS = [[0, 1, 2, 3], [2, 3, 4]], 2, 25.0
_BANKS = {}


def _bank(model, latency=False, fresh=False):
    """Five seeded views with their heat maps and seeded spread poses, in a bank that keeps entry tokens, match summaries and poses."""
    if fresh or latency not in _BANKS:
        bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder, match_threshold=0.05, keep_poses=True)
        refs = synth.make_batch(seed=47, B=1, T=5)
        rows = bank.add(refs["images"][0].cuda(), bbox_feat=refs["bbox_feat"][0].cuda(), poses=spread_poses(5, 48)[0].cuda())
        assert rows.tolist() == [0, 1, 2, 3, 4]
        if fresh:
            return bank
        _BANKS[latency] = bank
    return _BANKS[latency]


def _bbox_3d(B):
    return _to_dev(synth.make_batch(seed=51, B=B, T=K_SEL + 1))["bbox_3d"][:, K_SEL]


def _expected_selection(model, bank, frames, det, fidx, prev_host, force, rule):
    """This frame's selection through the existing wrappers, on the eagerly encoded query: (scores, dist, used, sel (B, k) host)."""
    B, k = len(DATABASES), K_SEL
    n_max = max(len(d) for d in DATABASES)
    win = pp.square_bbox(det.cuda(), 0.1)
    crops = pp.crop_resize_frames(frames.cuda(), win, frame_idx=fidx.cuda())
    fresh = model.rgb_encoder.predict(crops)
    q_sums, q_counts = hip_ops.match_view_sums(fresh, crops, 0.05)
    rows = torch.tensor([d + [-1] * (n_max - len(d)) for d in DATABASES], dtype=torch.int32, device="cuda")
    n_refs_h = [len(d) for d in DATABASES]
    n_refs = torch.tensor(n_refs_h, dtype=torch.int32, device="cuda")
    scores, sel_m, _ = hip_ops.match_select_rows(bank._msums, bank._mcounts, len(bank), q_sums, q_counts, rows, n_refs, bank.tokens_per_view, k)
    pred = prev_host[:, :16].reshape(B, 4, 4).contiguous().cuda()
    dist, sel_p, _ = hip_ops.pose_select_rows(bank.poses, len(bank), pred, rows, _identity_cand(n_refs_h, n_max), k)
    used = [int(rule == "track" and not force[b] and float(prev_host[b, 17]) == 1.0 and float(prev_host[b, 16]) <= MAX_RMS) for b in range(B)]
    sel = [(sel_p if used[b] else sel_m)[b].tolist() for b in range(B)]
    return scores, dist, used, sel


def _eager(model, bank, ref_rows, frames, det, K, fidx, seed=51):
    """The plain eager banked forward on the frame over the given bank rows + [-1] (test_gpu_stream._eager with its own table)."""
    B, T = len(ref_rows), len(ref_rows[0]) + 1
    base = {k: v for k, v in _to_dev(synth.make_batch(seed=seed, B=B, T=T)).items() if k not in ("images", "bbox_feat")}
    win = pp.square_bbox(det.cuda(), 0.1)
    Kc = pp.crop_intrinsics(K.cuda(), win, S)
    boxes = torch.tensor([0, 0, 16, 16], dtype=torch.int32, device="cuda").repeat(B, T, 1)
    boxes[:, T - 1] = win
    fi = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    fi[:, T - 1] = fidx.cuda()
    base["non_ndc_intrinsics"] = base["non_ndc_intrinsics"].clone()
    base["non_ndc_intrinsics"][:, T - 1] = Kc
    out = model(dict(base, frames=frames.cuda(), crop_boxes=boxes, frame_idx=fi, ref_bank=bank, ref_rows=[r + [-1] for r in ref_rows],
                     query_idx=torch.full((B,), T - 1, dtype=torch.long)))
    ar = torch.arange(B, device="cuda")
    return dict(heat=out["pred_query_bbox"].clone(), corners=out["pred_corners_px"].clone(), poses=out["pred_poses"][ar, T - 1].clone(),
                rms=out["pred_pose_rms_px"].clone(), windows=win, K_crop=Kc, bbox_3d=base["bbox_3d"][:, T - 1].clone())


def _checked_step(s, model, bank, step, prev_host, rule, relocalise=None):
    """One step of the session, everything compared with the eager side; returns what the comparisons kept."""
    B = s.B
    frames, det, K, fidx = _inputs(B, 3, step)
    force = [0] * B if relocalise is None else [int(x) for x in relocalise]
    rows = s.step(frames.pin_memory(), det, K, frame_idx=fidx, relocalise=None if relocalise is None else torch.tensor(relocalise))
    scores, dist, used, sel = _expected_selection(model, bank, frames, det, fidx, prev_host, force, rule)
    print(f"step {step}: used {s.used.tolist()} sel {s.sel.tolist()} ok {rows[:, 17].tolist()} rms {rows[:, 16].tolist()}")
    assert s.used.tolist() == used and s.sel.tolist() == sel, (step, used, sel)
    assert _eq(s.scores, scores), step
    if rule == "track":
        assert _eq(s.dist, dist), step
    else:
        assert s.dist is None
    assert s.ref_rows_of(s.sel) == [[DATABASES[b][i] for i in sel[b]] for b in range(B)]
    want = _eager(model, bank, s.ref_rows_of(sel), frames, det, K, fidx)
    assert model._graph is None
    _assert_step(s, rows, want, K, (rule, step))
    return dict(rows=rows.clone(), heat=s.heat.clone(), poses=s.poses.clone(), used=used, sel=sel)


def _track_session(latency):
    sh = _shared(latency)
    model, bank = sh["model"], _bank(sh["model"], latency)
    s = PoseStream(model, bank, DATABASES, _bbox_3d(2), frame_shape=(H, W), n_frames=2, select_k=K_SEL, select="track", max_rms_px=MAX_RMS)
    assert len(s.host_syncs_per_step) == 1 and s.replays == 0 and s.T == K_SEL + 1
    assert not s.rows.any()                                     # (the warm-up's own result rows are gone)
    zero = torch.zeros((2, 66))
    kept = [_checked_step(s, model, bank, 0, zero, "track")]
    assert kept[0]["used"] == [0, 0]                            # no last pose: by appearance
    # resumed from known poses, near database slot 3 of object 0 (bank row 3) and slot 2 of object 1 (bank row 4)
    near = torch.stack([bank.poses_of(3), bank.poses_of(4)]).cpu().clone()
    near[:, :3, 3] += 0.003
    s.reset(poses=near if not latency else near.cuda())
    resumed = zero.clone()
    resumed[:, :16], resumed[:, 17] = near.reshape(2, 16), 1.0
    assert _eq(s.rows.cpu(), resumed)
    kept.append(_checked_step(s, model, bank, 1, resumed, "track"))
    assert kept[1]["used"] == [1, 1] and 3 in kept[1]["sel"][0] and 2 in kept[1]["sel"][1]
    kept.append(_checked_step(s, model, bank, 2, kept[1]["rows"], "track"))
    kept.append(_checked_step(s, model, bank, 3, kept[2]["rows"], "track", relocalise=[1, 0]))
    assert kept[3]["used"][0] == 0
    for b in range(2):                                          # both rules chose at least once per object ...
        assert {st["used"][b] for st in kept} == {0, 1}, b
    assert any(st["sel"][b] != [0, 1] for st in kept for b in range(2))       # ... and not always the first two slots
    assert s.replays == 4 and len(s.host_syncs_per_step) == 1
    # reset(): the next step re-localises by appearance; relocalise held for one step only
    s.reset()
    assert not s.rows.any()
    again = _checked_step(s, model, bank, 0, zero, "track")
    assert again["used"] == [0, 0] and _eq(again["heat"], kept[0]["heat"]) and _eq(again["rows"], kept[0]["rows"])
    return s


def test_track_session_equals_the_eager_forward_over_the_chosen_rows(hip):
    s = _track_session(latency=False)
    frames, det, K, fidx = _inputs(2, 3, 0)
    with pytest.raises(ValueError, match=r"relocalise must be \(2,\)"):
        s.step(frames, det, K, relocalise=torch.tensor([1]))
    with pytest.raises(ValueError, match="poses must be"):
        s.reset(poses=torch.zeros((3, 4, 4)))
    assert s.replays == 5
    del s
    gc.collect()


def test_track_session_with_latency_forms(hip):
    s = _track_session(latency=True)
    assert s.model.decoder.hip_latency and s.model.rgb_encoder.model.latency
    del s
    gc.collect()


def test_dino_session_carries_nothing_from_frame_to_frame(hip):
    sh = _shared()
    model, bank = sh["model"], _bank(sh["model"])
    s = PoseStream(model, bank, DATABASES, _bbox_3d(2), frame_shape=(H, W), n_frames=2, select_k=K_SEL, select="dino")
    assert s.dist is None and s._poses is None
    kept, prev = [], torch.zeros((2, 66))
    for step in range(3):                                       # (the third step repeats the first frame)
        kept.append(_checked_step(s, model, bank, step, prev, "dino", relocalise=[0, 1] if step == 1 else None))
        prev = kept[-1]["rows"]
        assert kept[-1]["used"] == [0, 0]
    assert not torch.equal(kept[0]["heat"], kept[1]["heat"])
    assert all(_eq(kept[0][n], kept[2][n]) for n in ("rows", "heat", "poses")) and kept[0]["sel"] == kept[2]["sel"]
    assert s.replays == 3
    del s
    gc.collect()


def test_session_outlives_the_bank_and_plain_sessions_allocate_nothing_new(hip):
    sh = _shared()
    model = sh["model"]
    bank = _bank(model, fresh=True)
    s = PoseStream(model, bank, DATABASES, _bbox_3d(2), frame_shape=(H, W), n_frames=2, select_k=K_SEL, select="track", max_rms_px=MAX_RMS)
    frames, det, K, fidx = _inputs(2, 3, 0)
    near = torch.stack([bank.poses_of(1), bank.poses_of(3)]).cpu()
    s.reset(poses=near)
    first = s.step(frames, det, K, frame_idx=fidx).clone()
    heat, sel, dist = s.heat.clone(), s.sel.clone(), s.dist.clone()
    assert s.used.tolist() == [1, 1]
    plain = PoseStream(model, bank, [[0, 1], [2, 3]], _bbox_3d(2), frame_shape=(H, W), n_frames=2)     # built before the clear, too
    bank.clear()
    assert len(bank) == 0 and bank.poses is None
    s.reset(poses=near.cuda())
    again = s.step(frames, det, K)
    assert _eq(again, first) and _eq(s.heat, heat) and torch.equal(s.sel, sel) and _eq(s.dist, dist)
    # a session without select_k: none of the new buffers, none of the new calls
    for name in ("sel", "used", "scores", "dist", "force"):
        assert getattr(plain, name) is None, name
    for name in ("_msums", "_mcounts", "_poses", "_db_rows", "_n_refs", "_q_sums", "_q_counts", "_pin_force", "_pin_reset"):
        assert not hasattr(plain, name), name
    assert plain.select_k is None and plain.T == 3
    with pytest.raises(ValueError, match="without select_k"):
        plain.step(frames, det, K, relocalise=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="without select_k"):
        plain.reset()
    with pytest.raises(ValueError, match="without select_k"):
        plain.ref_rows_of([[0, 1], [0, 1]])
    assert plain.replays == 0 and torch.isfinite(plain.step(frames, det, K, frame_idx=fidx)[:, :16]).all()
    del s, plain
    gc.collect()
