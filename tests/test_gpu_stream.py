"""GPU: the pose stream (boxdreamer_amd/stream.py: PoseStream; csrc/stream.hip: bd_stream_windows, bd_stream_results).

The two kernels against their host twins on whole output buffers with a guard band, and a streaming session against the eager
forward over the same entry-token bank: the captured step must give the eager forward's bits (heat map, corners, pose, RMS), its
result rows must be bd_stream_results_host of those tensors, and nothing may be carried from frame to frame."""
import gc

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, synth
from boxdreamer_amd import preprocess as pp
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.stream import PoseStream
from test_gpu_ragged import _facade, _to_dev
from test_stream_host import bits, results_case, seeded_boxes, seeded_K

pytestmark = pytest.mark.gpu

H, W, S = 96, 128, 224
GUARD = 3


def _guarded(n, tail, dtype, fill):
    """A (n + 2 GUARD, *tail) buffer filled with a pattern and its contiguous middle (n, *tail): what a launch may write."""
    buf = torch.full((n + 2 * GUARD,) + tail, fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guard_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("n", [1, 64, 65])
def test_kernels_equal_their_host_twins_on_whole_buffers(hip, n):
    nan, inf = float("nan"), float("inf")
    boxes = seeded_boxes(seed=n)[np.random.default_rng(n).permutation(500)[:n]].copy()
    special = np.array([[nan, 10, 50, 60], [10, 10, inf, 60], [0, 0, 1e12, 100], [4.5, 7.5, 4.75, 7.75]], np.float32)
    boxes[:min(n, 4)] = special[:min(n, 4)]
    K = seeded_K(n, seed=n)
    for padding, out_size in ((0.1, 224), (0.0, 56), (0.25, 224)):
        want_w, want_k = hip_ops.stream_windows_host(boxes, K, padding, out_size)
        wbuf, w = _guarded(n, (4,), torch.int32, -77)
        kbuf, k = _guarded(n, (3, 3), torch.float32, -77.0)
        hip_ops.stream_windows(torch.from_numpy(boxes).cuda(), torch.from_numpy(K).cuda(), padding, out_size, w, k)
        assert np.array_equal(w.cpu().numpy(), want_w), (n, padding, out_size)
        assert np.array_equal(bits(k.cpu().numpy()), bits(want_k)), (n, padding, out_size)
        assert _guard_intact(wbuf, -77) and _guard_intact(kbuf, -77.0)
    case = tuple(a[:n] for a in results_case(n=max(n, 12), seed=n))
    for out_size in (224, 56):
        want = hip_ops.stream_results_host(*case, out_size)
        rbuf, r = _guarded(n, (_lib.STREAM_ROW_FLOATS,), torch.float32, -77.0)
        hip_ops.stream_results(*(torch.from_numpy(a).cuda() for a in case), out_size, r)
        assert np.array_equal(bits(r.cpu().numpy()), bits(want)), (n, out_size)
        assert _guard_intact(rbuf, -77.0)


# ---- a session against the eager forward over the same bank
_SHARED = {}


def _shared(latency=False):
    """One model per flag (default mode, wave PnP on the device; its first forward runs the load-time calibration), an entry bank of
    three reference views and two seeded 96 x 128 frames."""
    if latency not in _SHARED:
        model = _facade(_lib.DEFAULT_PREC, pnp_on_device="wave", **({"hip_latency": True} if latency else {}))
        assert bool(model.decoder.hip_latency) == latency and bool(model.rgb_encoder.model.latency) == latency
        model(_to_dev(synth.make_batch(seed=41, B=2, T=3)))
        bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
        refs = synth.make_batch(seed=43, B=1, T=3)
        rows = bank.add(refs["images"][0].cuda(), bbox_feat=refs["bbox_feat"][0].cuda()).tolist()
        _SHARED[latency] = dict(model=model, bank=bank, rows=rows, refs=refs)
    return _SHARED[latency]


def _frames():
    """Two steps' worth of two seeded 96 x 128 uint8 frames."""
    if "frames" not in _SHARED:
        g = torch.Generator().manual_seed(7)
        _SHARED["frames"] = [torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    return _SHARED["frames"]


# (B, T) -> (ref_rows, frame_idx, det boxes of step 1 / step 2: partly outside the 96 x 128 frame)
CASES = {
    (2, 3): ([[0, 1], [1, 2]], [0, 1], [[[-10.3, 5.2, 70.8, 90.1], [60.5, 30.25, 140.7, 110.0]], [[20.0, -14.5, 100.5, 60.0], [5.25, 8.0, 90.0, 99.5]]]),
    (1, 2): ([[2]], [1], [[[30.7, 20.1, 131.2, 101.9]], [[-6.0, 11.0, 80.0, 94.0]]]),
}


def _inputs(B, T, step):
    _, fidx, dets = CASES[(B, T)]
    i = step % 2                                                # the third step repeats the first
    K = torch.tensor([[150.0, 0.0, 64.0], [0.0, 140.0, 48.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    K[:, 0, 2] += torch.arange(B) * 1.5 + i
    return _frames()[i], torch.tensor(dets[i], dtype=torch.float32), K, torch.tensor(fidx, dtype=torch.int32)


def _eager(model, bank, B, T, frames, det, K, fidx, seed=51):
    """The eager banked forward on the frame: windows and crop intrinsics through the torch forms, no bbox_feat."""
    ref_rows = CASES[(B, T)][0]
    base = {k: v for k, v in _to_dev(synth.make_batch(seed=seed, B=B, T=T)).items() if k not in ("images", "bbox_feat")}
    win = pp.square_bbox(det.cuda(), 0.1)
    Kc = pp.crop_intrinsics(K.cuda(), win, S)
    assert win.dtype == torch.int32 and Kc.dtype == torch.float32
    boxes = torch.tensor([0, 0, 16, 16], dtype=torch.int32, device="cuda").repeat(B, T, 1)      # (banked slots: never used)
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


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_step(s, rows, want, K, where):
    assert _eq(s.windows, want["windows"]) and _eq(s.K_crop, want["K_crop"]), where
    assert _eq(s.heat, want["heat"]), where
    assert _eq(s.corners_px, want["corners"]), where
    assert _eq(s.poses, want["poses"]), where
    assert _eq(s.rms_px, want["rms"]), where
    host = hip_ops.stream_results_host(s.poses.cpu(), s.rms_px.cpu(), s.corners_px.cpu(), s.windows.cpu(), K, s.bbox_3d.cpu(), S)
    assert rows.shape == (s.B, 66) and rows.is_pinned() and np.array_equal(bits(rows.numpy()), bits(host)), where
    assert _eq(s.rows.cpu(), rows), where                    # (as bits: a corner behind the camera is NaN in the box slots)


def _session_against_eager(sh, B, T, graph_flag=False):
    model, bank = sh["model"], sh["bank"]
    bbox_3d = _to_dev(synth.make_batch(seed=51, B=B, T=T))["bbox_3d"][:, T - 1]
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, frame_shape=(H, W), n_frames=2)
    assert len(s.host_syncs_per_step) == 1 and s.replays == 0
    kept = []
    for step in range(3):
        frames, det, K, fidx = _inputs(B, T, step)
        rows = s.step(frames.pin_memory() if step != 1 else frames.cuda(), det, K if step != 1 else K.cuda(), frame_idx=fidx)
        kept.append((rows.clone(), s.heat.clone(), s.poses.clone()))
        model.hip_graph = graph_flag
        try:
            want = _eager(model, bank, B, T, frames, det, K, fidx)
            assert model._graph is None                       # a banked batch keeps taking the eager branch
        finally:
            model.hip_graph = False
        _assert_step(s, rows, want, K, (B, T, step))
        assert torch.isfinite(rows[:, :16]).all(), (B, T, step)
    assert not torch.equal(kept[0][1], kept[1][1])                   # the steps did differ ...
    assert all(_eq(a, b) for a, b in zip(kept[0], kept[2]))          # ... and the third is the first again, bit for bit
    assert s.replays == 3 and len(s.host_syncs_per_step) == 1
    return s


@pytest.mark.parametrize("shape", [(2, 3), (1, 2)])
def test_stream_equals_the_eager_banked_forward(hip, shape):
    s = _session_against_eager(_shared(), *shape, graph_flag=True)
    # what step() refuses, before anything is copied
    frames, det, K, fidx = _inputs(*shape, 0)
    with pytest.raises(ValueError, match="frame shape is fixed"):
        s.step(frames[:, :-1], det, K)
    with pytest.raises(ValueError, match="uint8"):
        s.step(frames.float(), det, K)
    with pytest.raises(ValueError, match="B = "):
        s.step(frames, torch.cat([det, det]), K)
    with pytest.raises(ValueError, match="float"):
        s.step(frames, det.long(), K)
    with pytest.raises(ValueError, match="use_keep_boxes"):
        s.step(frames, det, K, keep_boxes=torch.zeros((shape[0], 4), dtype=torch.int32))
    assert s.replays == 3
    del s
    gc.collect()


def test_stream_with_latency_forms_equals_the_eager_forward_with_them(hip):
    sh = _shared(latency=True)
    s = _session_against_eager(sh, 1, 2)
    assert sh["model"].decoder.hip_latency and sh["model"].rgb_encoder.model.latency
    del s
    gc.collect()


def test_stream_keep_boxes_and_independence_from_the_bank(hip):
    """The session copied the rows it references: the bank may grow (its stores move) or be cleared, the next step gives the same
    bits.  With use_keep_boxes the crops are the masked crops of bd_crop_resize_frames."""
    sh = _shared()
    model, refs = sh["model"], sh["refs"]
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    bank.add(refs["images"][0].cuda(), bbox_feat=refs["bbox_feat"][0].cuda())
    B, T = 2, 3
    bbox_3d = _to_dev(synth.make_batch(seed=51, B=B, T=T))["bbox_3d"][:, T - 1]
    s = PoseStream(model, bank, CASES[(B, T)][0], bbox_3d, frame_shape=(H, W), n_frames=2, use_keep_boxes=True)
    frames, det, K, fidx = _inputs(B, T, 0)
    keep = torch.tensor([[0, 10, 60, 80], [70, 35, 127, 95]], dtype=torch.int32)
    first = s.step(frames, det, K, frame_idx=fidx, keep_boxes=keep).clone()
    heat = s.heat.clone()
    want = pp.crop_resize_frames(frames.cuda(), s.windows, frame_idx=fidx.cuda(), keep_boxes=keep.cuda())
    assert torch.equal(s.crops, want) and not torch.equal(want, pp.crop_resize_frames(frames.cuda(), s.windows, frame_idx=fidx.cuda()))
    store = bank.entry_tokens.data_ptr()
    for _ in range(2):                                          # 3 + 3 + 3 rows: past the bank's first capacity of 8, its stores move
        bank.add(refs["images"][0].cuda(), bbox_feat=refs["bbox_feat"][0].cuda())
    assert len(bank) == 9 and bank.entry_tokens.data_ptr() != store
    bank.entry_tokens.fill_(float("nan"))
    again = s.step(frames, det, K)                              # (frame_idx / keep_boxes: as in the last step)
    assert np.array_equal(bits(again.numpy()), bits(first.numpy())) and _eq(s.heat, heat)
    bank.clear()
    assert len(bank) == 0
    again = s.step(frames, det, K)
    assert np.array_equal(bits(again.numpy()), bits(first.numpy())) and _eq(s.heat, heat)
    assert s.replays == 3
    del s
    gc.collect()


def test_stream_freezes_the_modules_and_needs_a_calibrated_model(hip):
    sh = _shared()
    model, bank = sh["model"], sh["bank"]
    bbox_3d = torch.zeros((1, 8, 3))
    s = PoseStream(model, bank, [[0]], bbox_3d, frame_shape=(H, W))
    big = torch.zeros((16, 3, S, S), device="cuda")
    with pytest.raises(RuntimeError, match="delete the graph first"):
        model.rgb_encoder.predict(big)                          # a larger workspace than the one the captured step replays on
    with pytest.raises(RuntimeError, match="delete the graph first"):
        model.decoder.float()
    del s
    gc.collect()
    assert model.rgb_encoder.predict(big).shape[0] == 16
    # the precision self-check cannot run inside a capture: an unsettled model is refused before anything is captured
    settled = model._calibrated_for
    model._calibrated_for = None
    try:
        with pytest.raises(RuntimeError, match="mark_calibrated"):
            PoseStream(model, bank, [[0]], bbox_3d, frame_shape=(H, W))
        assert not len(model.decoder._frozen_by) and not len(model.rgb_encoder.model._frozen_by)
    finally:
        model._calibrated_for = settled
