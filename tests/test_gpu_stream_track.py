"""GPU: a pose stream that follows each object's box from its own last pose (stream.PoseStream(track_boxes=True); csrc/stream.hip:
bd_stream_track_windows).

The kernel against its host twin on whole guarded buffers; a tracking session next to a plain session that is fed, step by step, the
box the tracking session reports: everything the step computes must be bit-identical, and the reported box and source must be what the
numpy mirror (stream.track_windows_host) derives from the previous step's result rows."""
import gc

import numpy as np
import pytest
import torch

from boxdreamer_amd import hip_ops, synth
from boxdreamer_amd import preprocess as pp
from boxdreamer_amd.stream import BOX_DETECTOR, BOX_HELD, BOX_TRACKED, PoseStream, track_windows_host
from test_gpu_ragged import _to_dev
from test_gpu_stream import CASES, H, S, W, _eq, _guard_intact, _guarded, _inputs, _shared
from test_gpu_stream_select import DATABASES, K_SEL, MAX_RMS, _bank, _bbox_3d
from test_stream_host import bits
from test_stream_track_host import FRAME, MAX_SIDE, MIN_SIDE, track_case
from test_stream_track_host import MAX_RMS as CASE_MAX_RMS

pytestmark = pytest.mark.gpu

INF = float("inf")


# ---- the kernel
@pytest.mark.parametrize("want_keep", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_kernel_equals_its_host_twin_on_whole_buffers(hip, n, want_keep):
    pick = np.random.default_rng(n).permutation(500)[:n]
    args = tuple(np.ascontiguousarray(a[pick]) for a in track_case()["args"])
    kw = dict(frame_shape=FRAME, max_rms_px=CASE_MAX_RMS, min_side_px=MIN_SIDE, max_side_px=MAX_SIDE)
    for padding, out_size in ((0.1, 224), (0.0, 56)):
        want = hip_ops.stream_track_windows_host(*args, padding, out_size, want_keep=want_keep, **kw)
        if n > 1:
            assert len(set(want["box_src"].tolist())) == 3                      # every source is in the launch
        dev = [torch.from_numpy(a).cuda() for a in args[:6]]
        sbuf, state = _guarded(n, (4,), torch.float32, -77.0)
        state.copy_(torch.from_numpy(args[6]))
        wbuf, w = _guarded(n, (4,), torch.int32, -77)
        kbuf, k = _guarded(n, (3, 3), torch.float32, -77.0)
        cbuf, c = _guarded(n, (), torch.int32, -77)
        tbuf, t = _guarded(n, (5,), torch.float32, -77.0)
        ebuf, e = _guarded(n, (4,), torch.int32, -77) if want_keep else (None, None)
        inputs = [a.clone() for a in dev]
        out = hip_ops.stream_track_windows(*dev, state, padding, out_size, windows=w, K_crop=k, box_src=c, keep_boxes=e, track=t, **kw)
        assert out[0] is w and out[1] is k and out[2] is c
        where = (n, want_keep, padding, out_size)
        assert np.array_equal(w.cpu().numpy(), want["windows"]) and np.array_equal(bits(k.cpu().numpy()), bits(want["K_crop"])), where
        assert np.array_equal(c.cpu().numpy(), want["box_src"]), where
        assert np.array_equal(bits(state.cpu().numpy()), bits(want["state_box"])), where         # updated in place
        assert np.array_equal(bits(t.cpu().numpy()), bits(want["track"])), where
        if want_keep:
            assert np.array_equal(e.cpu().numpy(), want["keep_boxes"]) and _guard_intact(ebuf, -77), where
        assert _guard_intact(sbuf, -77.0) and _guard_intact(wbuf, -77) and _guard_intact(kbuf, -77.0) and _guard_intact(cbuf, -77)
        assert _guard_intact(tbuf, -77.0)
        assert all(_eq(a, b) for a, b in zip(dev, inputs))                      # the inputs are only read
        # without the optional outputs the others are the same
        state2 = torch.from_numpy(args[6]).cuda()
        w2, k2, c2 = hip_ops.stream_track_windows(*dev, state2, padding, out_size, **kw)
        assert torch.equal(w2, w) and _eq(k2, k) and torch.equal(c2, c) and _eq(state2, state), where


# ---- sessions
def _box_3d(B, T):
    return _to_dev(synth.make_batch(seed=51, B=B, T=T))["bbox_3d"][:, T - 1]


def _resume_poses(bbox_3d):
    """(B, 4, 4) host poses that put every object's projected box inside the 96 x 128 frame: no rotation, the middle of the box's x and
    y ranges on the optical axis, at the depth where its larger range spans about 40 pixels of the 150-pixel focal length (the
    principal point is near (64, 48)); every corner stays in front of the camera."""
    pts = bbox_3d.cpu().float()
    lo, hi = pts.min(1)[0], pts.max(1)[0]
    P = torch.eye(4).repeat(pts.shape[0], 1, 1)
    P[:, 0, 3], P[:, 1, 3] = -(lo[:, 0] + hi[:, 0]) / 2, -(lo[:, 1] + hi[:, 1]) / 2
    P[:, 2, 3] = 150.0 * torch.maximum(hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1]) / 40.0 - lo[:, 2] + 0.5
    return P


def _resumed_rows(P):
    rows = torch.zeros((P.shape[0], 66))
    rows[:, :16], rows[:, 17] = P.reshape(-1, 16), 1.0
    return rows


def _script(B):
    """The four steps: (reset poses or None, detections offered?, det_valid or None, relocalise or None)."""
    first = [1, 0][:B] if B > 1 else [0]
    return [(False, True, first, None),                         # sources 0 and 2 (B = 1: 2)
            (True, False, None, None),                          # resumed from known poses, nobody has a detection: source 1
            (False, True, None, [1] + [0] * (B - 1)),           # object 0 distrusts its pose and a detection is offered: source 0
            (False, False, None, None)]                         # on its own: tracked, or held


def _mirror(prev_rows, bbox_3d, K, det, det_valid, force, state, max_rms=INF):
    return track_windows_host(prev_rows, bbox_3d.cpu(), K, det, det_valid, force, state, frame_shape=(H, W), max_rms_px=max_rms)


def _tracked_against_fed(tracking, fed, B, T, bbox_3d, max_rms=INF, after=None):
    """Run the script on a tracking session and on one that is fed the boxes the first reports; returns the sources seen."""
    default = torch.tensor([0.0, 0.0, float(min(H, W)), float(min(H, W))]).repeat(B, 1)
    prev, state, seen, kept = torch.zeros((B, 66)), default, [], []
    assert tracking.track_boxes and tracking.track_host.shape == (B, 5) and tracking.track.shape == (B, 5)
    assert _eq(tracking.state_box.cpu(), default) and not tracking.rows.any() and not tracking.box_src.any()      # the warm-up left nothing
    for step, (resume, offered, valid, reloc) in enumerate(_script(B)):
        frames, det, K, fidx = _inputs(B, T, step)
        if resume:
            P = _resume_poses(bbox_3d)
            tracking.reset(poses=P)
            fed.reset(poses=P.cuda()) if fed.select_k is not None else None
            prev = _resumed_rows(P)
        kw = dict(frame_idx=fidx, relocalise=None if reloc is None else torch.tensor(reloc))
        rows = tracking.step(frames.pin_memory(), det if offered else None, K, det_valid=None if valid is None else torch.tensor(valid), **kw)
        box, src = tracking.track_host[:, :4].clone(), tracking.track_host[:, 4].to(torch.int32).tolist()
        # the reported box and source: the mirror on the previous step's rows
        dv = valid if valid is not None else [int(offered)] * B
        m = _mirror(prev, bbox_3d, K, det if offered else torch.zeros((B, 4)), dv, reloc or [0] * B, state, max_rms)
        print(f"step {step}: src {src} box {box.tolist()} ok {rows[:, 17].tolist()} rms {rows[:, 16].tolist()} valid {m['valid'].tolist()}")
        assert src == m["src"].tolist() == tracking.box_src.tolist(), (step, src, m["src"])
        assert np.array_equal(bits(box.numpy()), bits(m["box"])) and _eq(tracking.state_box.cpu(), box), step
        assert _eq(tracking.track.cpu(), tracking.track_host), step
        # the other session, given that box from outside: the same bits everywhere
        if fed.select_k is None:
            kw.pop("relocalise")
        fed_rows = fed.step(frames.pin_memory(), box, K, **kw)
        for name in ("windows", "K_crop", "heat", "corners_px", "poses", "rms_px", "rows", "crops"):
            assert _eq(getattr(tracking, name), getattr(fed, name)), (step, name)
        assert np.array_equal(bits(rows.numpy()), bits(fed_rows.numpy())) and _eq(tracking.rows.cpu(), rows), step
        want_w, want_k = hip_ops.stream_windows_host(box.numpy(), K.numpy(), 0.1, S)
        assert np.array_equal(tracking.windows.cpu().numpy(), want_w) and np.array_equal(bits(tracking.K_crop.cpu().numpy()), bits(want_k)), step
        if after is not None:
            after(step, m)
        prev, state = rows.clone(), box
        seen.append(src)
        kept.append(rows.clone())
    assert tracking.replays == fed.replays == 4
    return seen, kept


def _track_session(latency, B, T):
    sh = _shared(latency)
    model, bank = sh["model"], sh["bank"]
    bbox_3d = _box_3d(B, T)
    kw = dict(frame_shape=(H, W), n_frames=2)
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, track_boxes=True, **kw)
    plain = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, **kw)
    n_bytes = B * (66 + 5) * 4
    assert s.host_syncs_per_step == [f"result rows and box tail: ONE D2H of {n_bytes} bytes into a pinned buffer, one wait for its event"]
    assert s.max_rms_px == INF and s.min_side_px == 8.0 and s.max_side_px == 4.0 * W
    seen, _ = _tracked_against_fed(s, plain, B, T, bbox_3d)
    assert seen[0] == ([BOX_DETECTOR, BOX_HELD] if B > 1 else [BOX_HELD])
    assert seen[1] == [BOX_TRACKED] * B and seen[2][0] == BOX_DETECTOR
    assert {x for step in seen for x in step} == {BOX_DETECTOR, BOX_TRACKED, BOX_HELD}
    assert len(s.host_syncs_per_step) == 1
    return s, plain


@pytest.mark.parametrize("shape", [(2, 3), (1, 2)])
def test_tracking_session_equals_a_plain_session_fed_its_boxes(hip, shape):
    s, plain = _track_session(False, *shape)
    B = shape[0]
    frames, det, K, fidx = _inputs(*shape, 0)
    with pytest.raises(ValueError, match="keep_boxes given to a session built with track_boxes"):
        s.step(frames, det, K, keep_boxes=torch.zeros((B, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"det_valid must be \("):
        s.step(frames, det, K, det_valid=torch.zeros((B + 1,), dtype=torch.int32))
    with pytest.raises(ValueError, match="det_boxes=None given to a session built without track_boxes"):
        plain.step(frames, None, K)
    with pytest.raises(ValueError, match="det_valid given to a session built without track_boxes"):
        plain.step(frames, det, K, det_valid=torch.ones((B,), dtype=torch.int32))
    assert s.replays == 4 and plain.replays == 4
    # device inputs take the other copy path: the same step again, bit for bit
    s.reset(poses=_resume_poses(s.bbox_3d.cpu()).cuda())
    a = s.step(frames.cuda(), det.cuda(), K.cuda(), frame_idx=fidx, det_valid=torch.zeros((B,), dtype=torch.bool, device="cuda")).clone()
    s.reset(poses=_resume_poses(s.bbox_3d.cpu()))
    b = s.step(frames, None, K, frame_idx=fidx)
    assert np.array_equal(bits(a.numpy()), bits(b.numpy())) and s.track_host[:, 4].tolist() == [float(BOX_TRACKED)] * B
    del s, plain
    gc.collect()


@pytest.mark.parametrize("shape", [(2, 3), (1, 2)])
def test_tracking_session_with_latency_forms(hip, shape):
    s, plain = _track_session(True, *shape)
    assert s.model.decoder.hip_latency and s.model.rgb_encoder.model.latency
    del s, plain
    gc.collect()


def test_selecting_session_that_tracks_equals_one_fed_its_boxes(hip):
    """select="track" and track_boxes decide from the same row by the same rule: `used` and `box_src` agree whenever the box is usable."""
    sh = _shared()
    model, bank = sh["model"], _bank(sh["model"])
    B, bbox_3d = 2, _bbox_3d(2)
    kw = dict(frame_shape=(H, W), n_frames=2, select_k=K_SEL, select="track", max_rms_px=MAX_RMS)
    s = PoseStream(model, bank, DATABASES, bbox_3d, track_boxes=True, **kw)
    fed = PoseStream(model, bank, DATABASES, bbox_3d, **kw)
    assert fed.track is None and fed.state_box is None
    agreed = []

    def after(step, m):
        used, src = s.used.tolist(), s.box_src.tolist()
        assert used == fed.used.tolist() and torch.equal(s.sel, fed.sel) and _eq(s.scores, fed.scores) and _eq(s.dist, fed.dist), step
        for b in range(B):
            if m["valid"][b]:
                assert (used[b] == 1) == (src[b] == BOX_TRACKED), (step, b)
                agreed.append(used[b])
            else:
                assert src[b] != BOX_TRACKED, (step, b)

    seen, _ = _tracked_against_fed(s, fed, B, K_SEL + 1, bbox_3d, max_rms=MAX_RMS, after=after)
    assert seen[1] == [BOX_TRACKED] * B and seen[2][0] == BOX_DETECTOR
    # resumed from known poses with object 0 told to re-localise: a usable box under both verdicts, in one step
    frames, det, K, fidx = _inputs(B, K_SEL + 1, 0)
    P = _resume_poses(bbox_3d)
    s.reset(poses=P)
    fed.reset(poses=P)
    rows = s.step(frames, det, K, frame_idx=fidx, relocalise=torch.tensor([1, 0])).clone()
    m = _mirror(_resumed_rows(P), bbox_3d, K, det, [1, 1], [1, 0], s.track_host[:, :4], MAX_RMS)
    assert m["valid"].all() and s.used.tolist() == [0, 1] and s.box_src.tolist() == [BOX_DETECTOR, BOX_TRACKED] == m["src"].tolist()
    fed_rows = fed.step(frames, s.track_host[:, :4].clone(), K, frame_idx=fidx, relocalise=torch.tensor([1, 0]))
    assert np.array_equal(bits(rows.numpy()), bits(fed_rows.numpy())) and _eq(s.heat, fed.heat) and torch.equal(s.sel, fed.sel)
    assert fed.used.tolist() == [0, 1] and 1 in agreed
    del s, fed
    gc.collect()


def test_step_inputs_from_host_or_device_land_alike(hip):
    """Wherever a step's small inputs live -- all on the host, all on the device, or mixed -- the session's static buffers hold exactly
    what was given before the replay, `force` holds for one step only, and the step's result does not depend on the residency."""
    sh = _shared()
    model, bank = sh["model"], sh["bank"]
    B, T = 2, 3
    bbox_3d = _box_3d(B, T)
    kw = dict(frame_shape=(H, W), n_frames=2)
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, track_boxes=True, **kw)
    frames, det, K, fidx = _inputs(B, T, 0)
    valid = torch.tensor([1, 0], dtype=torch.int32)
    zeros, ones = torch.zeros((B,), dtype=torch.int32), torch.ones((B,), dtype=torch.int32)

    def landed(det_, K_, valid_, fidx_, force_, where):
        assert _eq(s.det_boxes.cpu(), det_) and _eq(s.K.cpu(), K_), where
        assert s.det_valid.dtype == torch.int32 and torch.equal(s.det_valid.cpu(), valid_), where
        assert s.frame_idx.dtype == torch.int32 and torch.equal(s.frame_idx.cpu(), fidx_), where
        assert s.force.dtype == torch.int32 and torch.equal(s.force.cpu(), force_), where

    # all on the host (a pinned frame), then all on the device: the same inputs from reset() give the same rows
    s.reset()
    a = s.step(frames.pin_memory(), det, K, frame_idx=fidx, det_valid=valid).clone()
    landed(det, K, valid, fidx, zeros, "host")
    tail = s.track_host.clone()
    s.reset()
    b = s.step(frames.cuda(), det.cuda(), K.cuda(), frame_idx=fidx.cuda(), det_valid=valid.cuda())
    landed(det, K, valid, fidx, zeros, "device")
    assert np.array_equal(bits(a.numpy()), bits(b.numpy())) and _eq(s.track_host, tail)
    # K on the device, the boxes and their flags on the host (bools: stored as 0 / 1)
    det2, K2 = det + 1.25, K * 1.5
    s.step(frames, det2, K2.cuda(), det_valid=torch.tensor([False, True]))
    landed(det2, K2, torch.tensor([0, 1], dtype=torch.int32), fidx, zeros, "K on the device")
    # frame_idx on the device; no det_valid: all ones with a detection, all zeros (and the boxes left alone) without one
    fidx2 = torch.tensor([1, 0], dtype=torch.int32)
    s.step(frames, det, K2, frame_idx=fidx2.cuda())
    landed(det, K2, ones, fidx2, zeros, "frame_idx on the device")
    s.step(frames, None, K)
    landed(det, K, zeros, fidx2, zeros, "no detection, host")
    s.step(frames, det2.cuda(), K)
    landed(det2, K, ones, fidx2, zeros, "boxes on the device, no det_valid")
    s.step(frames, None, K2.cuda())
    landed(det2, K2, zeros, fidx2, zeros, "no detection, device")
    # relocalise on the device, from the host, and then a step without it: the flags hold for one step
    s.step(frames, det, K, relocalise=torch.tensor([0, 3]).cuda())
    landed(det, K, ones, fidx2, torch.tensor([0, 1], dtype=torch.int32), "relocalise on the device")
    s.step(frames, det, K, relocalise=[True, False])
    landed(det, K, ones, fidx2, torch.tensor([1, 0], dtype=torch.int32), "relocalise on the host")
    s.step(frames, det, K)
    landed(det, K, ones, fidx2, zeros, "the step after relocalise")
    assert s.replays == 10
    del s
    gc.collect()
    # keep_boxes of a session that is given them, from the host and from the device
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, use_keep_boxes=True, **kw)
    keep = torch.tensor([[0, 10, 60, 80], [70, 35, 127, 95]], dtype=torch.int32)
    for given in (keep, (keep + 3).cuda()):
        s.step(frames, det, K, frame_idx=fidx, keep_boxes=given)
        assert s.keep_boxes.dtype == torch.int32 and torch.equal(s.keep_boxes.cpu(), given.cpu()), given.device
        assert _eq(s.det_boxes.cpu(), det) and _eq(s.K.cpu(), K) and torch.equal(s.frame_idx.cpu(), fidx)
    s.step(frames, det, K)                                      # (None: as in the last step)
    assert torch.equal(s.keep_boxes.cpu(), keep + 3)
    del s
    gc.collect()


def test_tracking_writes_the_keep_boxes_and_two_sessions_agree(hip):
    sh = _shared()
    model, bank = sh["model"], sh["bank"]
    B, T = 2, 3
    bbox_3d = _box_3d(B, T)
    kw = dict(frame_shape=(H, W), n_frames=2)
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, track_boxes=True, use_keep_boxes=True, **kw)
    twin = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, track_boxes=True, use_keep_boxes=True, **kw)
    plain = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, use_keep_boxes=True, **kw)
    # a session built without track_boxes: none of the new buffers, the D2H it had
    assert plain.track is None and plain.track_host is None and plain.state_box is None and plain.box_src is None and plain.det_valid is None
    assert plain.force is None and not hasattr(plain, "_pin_force")
    assert plain.host_syncs_per_step == [f"result rows: ONE D2H of {B * 66 * 4} bytes into a pinned buffer, one wait for its event"]
    assert plain._in_f.numel() == B * 13 and plain.rows.shape == (B, 66) and plain.rows_host.is_pinned()
    masked = 0
    for step, (resume, offered, valid, reloc) in enumerate(_script(B)):
        frames, det, K, fidx = _inputs(B, T, step)
        if resume:
            for x in (s, twin):
                x.reset(poses=_resume_poses(bbox_3d))
        args = dict(frame_idx=fidx, det_valid=None if valid is None else torch.tensor(valid), relocalise=None if reloc is None else torch.tensor(reloc))
        rows = s.step(frames, det if offered else None, K, **args).clone()
        again = twin.step(frames, det if offered else None, K, **args)
        assert np.array_equal(bits(rows.numpy()), bits(again.numpy())) and _eq(s.track_host, twin.track_host), step
        for name in ("heat", "crops", "windows", "keep_boxes", "state_box", "box_src"):
            assert _eq(getattr(s, name), getattr(twin, name)), (step, name)
        box = s.track_host[:, :4].clone()
        keep = box.double().trunc().to(torch.int32)
        assert torch.equal(s.keep_boxes.cpu(), keep), step
        plain_rows = plain.step(frames, box, K, frame_idx=fidx, keep_boxes=keep)
        assert _eq(s.crops, plain.crops) and _eq(s.heat, plain.heat) and np.array_equal(bits(rows.numpy()), bits(plain_rows.numpy())), step
        unmasked = pp.crop_resize_frames(frames.cuda(), s.windows, frame_idx=fidx.cuda())
        masked += int(not torch.equal(unmasked, s.crops))
    assert masked >= 1                                          # the keep box did mask something
    del s, twin, plain
    gc.collect()
