"""Host: the two kernels of the pose stream through their host twins (bd_stream_windows_host / bd_stream_results_host: the SAME
__host__ __device__ arithmetic the kernels run, csrc/stream.hip), the argument checks of all four entry points (they run before any
launch, so they need no GPU) and the refusals of stream.PoseStream that need no device.

Bits are compared as int32 views.  A NaN is compared as "NaN at the same place": which of the NaN encodings an invalid operation
(inf - inf, 0 x inf) returns is a property of the processor that ran it, not of the arithmetic under test; every finite value,
every infinity and every zero's sign must match exactly."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops
from boxdreamer_amd import preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def seeded_boxes(seed=0):
    """~500 fp32 boxes x0 y0 x1 y1 for a 480 x 640 frame: ordinary, sub-pixel, negative / leaving the frame, and centres and
    extents that sit on .5 and integer boundaries (where trunc and the fp64 products decide the window)."""
    r = np.random.default_rng(seed)
    out = []
    x0, y0 = r.uniform(0, 500, 160), r.uniform(0, 380, 160)                       # ordinary
    out.append(np.stack([x0, y0, x0 + r.uniform(8, 320, 160), y0 + r.uniform(8, 320, 160)], 1))
    x0, y0 = r.uniform(0, 639, 60), r.uniform(0, 479, 60)                         # sub-pixel
    out.append(np.stack([x0, y0, x0 + r.uniform(0, 1, 60), y0 + r.uniform(0, 1, 60)], 1))
    x0, y0 = r.uniform(-300, 700, 120), r.uniform(-300, 500, 120)                 # negative coordinates, leaving the frame
    out.append(np.stack([x0, y0, x0 + r.uniform(1, 400, 120), y0 + r.uniform(1, 400, 120)], 1))
    q = r.integers(-40, 1300, (120, 2)) * 0.5                                     # on .5 / integer boundaries
    wh = r.integers(1, 600, (120, 2)) * 0.5
    out.append(np.concatenate([q, q + wh], 1))
    q = r.integers(-10, 600, (40, 2)).astype(np.float64)                          # integer boxes, equal sides among them
    s = r.integers(1, 300, (40, 1)).astype(np.float64)
    out.append(np.concatenate([q, q + s], 1))
    return np.concatenate(out).astype(np.float32)


def seeded_K(n, seed=1):
    r = np.random.default_rng(seed)
    K = np.zeros((n, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = r.uniform(300, 900, n), r.uniform(300, 900, n)
    K[:, 0, 1] = r.uniform(-1, 1, n)
    K[:, 0, 2], K[:, 1, 2] = r.uniform(200, 440, n), r.uniform(150, 330, n)
    K[:, 2, 2] = 1.0
    K[::7, 2, 0] = 0.25                                                          # entries the functions leave alone are copied
    return K


def torch_windows(boxes, K, padding, out_size):
    """The torch forms the kernel replaces, on the same fp32 inputs."""
    win = pp.square_bbox(torch.from_numpy(boxes), padding)
    assert win.dtype == torch.int32
    Kc = pp.crop_intrinsics(torch.from_numpy(K), win, out_size)
    assert Kc.dtype == torch.float32
    return win.numpy(), Kc.numpy()


@pytest.mark.parametrize("out_size", [224, 56])
@pytest.mark.parametrize("padding", [0.0, 0.1, 0.25])
def test_windows_equal_square_bbox_and_crop_intrinsics_bit_for_bit(padding, out_size):
    boxes = seeded_boxes()
    K = seeded_K(len(boxes))
    assert len(boxes) == 500
    want_w, want_k = torch_windows(boxes, K, padding, out_size)
    got_w, got_k = hip_ops.stream_windows_host(boxes, K, padding, out_size)
    assert got_w.dtype == np.int32 and got_k.dtype == np.float32
    assert np.array_equal(got_w, want_w)
    assert np.array_equal(bits(got_k), bits(want_k))
    # the cases are what they claim to be: degenerate windows, windows that leave the frame, windows whose sides differ
    side_x, side_y = got_w[:, 2] - got_w[:, 0], got_w[:, 3] - got_w[:, 1]
    assert (side_x == 0).any() and (got_w[:, 0] < 0).any() and (got_w[:, 2] > 640).any() and (got_w[:, 3] > 480).any()
    assert np.isfinite(got_k[side_x > 0][:, 0]).all()
    for n in (1, 65):                                        # a sample's bits do not depend on the others of the call
        w, k = hip_ops.stream_windows_host(boxes[100:100 + n], K[100:100 + n], padding, out_size)
        assert np.array_equal(w, want_w[100:100 + n]) and np.array_equal(bits(k), bits(want_k[100:100 + n]))


def test_windows_of_non_finite_and_huge_boxes_are_zero():
    nan, inf = float("nan"), float("inf")
    boxes = np.array([[nan, 10, 50, 60], [10, 10, inf, 60], [-inf, 0, 5, 5], [10, nan, 20, nan], [0, 0, 1e12, 100], [-1e12, 5, 7, 9],
                      [3e9, 3e9, 3.1e9, 3.1e9], [10, 20, 110, 100]], np.float32)
    K = seeded_K(len(boxes))
    w, k = hip_ops.stream_windows_host(boxes, K, 0.1, 224)
    assert np.array_equal(w[:7], np.zeros((7, 4), np.int32))
    ref_w, ref_k = torch_windows(boxes[7:], K[7:], 0.1, 224)
    assert np.array_equal(w[7:], ref_w) and np.array_equal(bits(k[7:]), bits(ref_k))
    # the largest window int32 holds is kept
    big = np.array([[-2.0e9, -2.0e9, 2.0e9, 2.0e9]], np.float32)
    w, _ = hip_ops.stream_windows_host(big, K[:1], 0.0, 224)
    assert np.array_equal(w, torch_windows(big, K[:1], 0.0, 224)[0]) and w[0, 0] == -2000000000


def results_reference(poses, rms, kp, win, K, box, S):
    """bd_stream_results restated in numpy fp64, in the stated operation order (numpy contracts nothing)."""
    n = len(poses)
    f64 = np.float64
    rows = np.zeros((n, 66), np.float32)
    p = poses.reshape(n, 16)
    fin = np.isfinite(p)
    rows[:, 0:16] = np.where(fin, p, np.float32(0))
    rows[:, 16] = rms
    ok = fin.all(1) & (p[:, 15] == 1)
    rows[:, 17] = ok
    rows[:, 18:34] = kp.reshape(n, 16)
    w = win.astype(f64)
    x0, y0 = w[:, 0:1], w[:, 1:2]
    sx, sy = w[:, 2:3] - x0, w[:, 3:4] - y0
    rows[:, 34:50:2] = x0 + kp[..., 0].astype(f64) * sx / f64(S)
    rows[:, 35:50:2] = y0 + kp[..., 1].astype(f64) * sy / f64(S)
    P, X, Kd = poses.astype(f64), box.astype(f64), K.astype(f64)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        xc, yc, zc = (((P[:, r, 0:1] * x + P[:, r, 1:2] * y) + P[:, r, 2:3] * z) + P[:, r, 3:4] for r in range(3))
        u = ((Kd[:, 0, 0:1] * xc + Kd[:, 0, 1:2] * yc) + Kd[:, 0, 2:3] * zc) / zc
        v = (Kd[:, 1, 1:2] * yc + Kd[:, 1, 2:3] * zc) / zc
        behind = zc <= 0
    u, v = np.where(behind, np.nan, u), np.where(behind, np.nan, v)
    rows[:, 50:66:2] = np.where(ok[:, None], u, 0.0)
    rows[:, 51:66:2] = np.where(ok[:, None], v, 0.0)
    return rows


def results_case(n=70, seed=5):
    """n samples: seeded rigid poses in front of the camera, then the special ones (NaN / inf entries, an all-zero pose, a pose whose
    [3][3] is not 1, a box that straddles the camera plane, a window that leaves the frame)."""
    r = np.random.default_rng(seed)
    rv = r.uniform(-1, 1, (n, 3))
    poses = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        th = np.linalg.norm(rv[i])
        k = rv[i] / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        poses[i, :3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    poses[:, :3, 3] = np.stack([r.uniform(-0.5, 0.5, n), r.uniform(-0.5, 0.5, n), r.uniform(2, 6, n)], 1)
    poses[:, 3, 3] = 1.0
    poses[1, 0, 1] = np.nan                        # nan_to_num slots: ok = 0, the box slots are 0
    poses[2, 1, 3] = np.inf
    poses[3, 2, 0] = -np.inf
    poses[4] = 0.0                                 # the solver's failure value
    poses[5, 3, 3] = 0.5                           # finite, but no pose
    poses[6, 2, 3] = 0.1                           # the box straddles the camera plane: some corners have zc <= 0
    poses[7, 2, 3] = -4.0                          # all of it behind the camera
    rms = r.uniform(0, 9, n).astype(np.float32)
    kp = r.uniform(-20, 244, (n, 8, 2)).astype(np.float32)
    x0, y0 = r.integers(-200, 600, n), r.integers(-200, 440, n)
    side = r.integers(1, 500, n)
    win = np.stack([x0, y0, x0 + side, y0 + side], 1).astype(np.int32)
    win[8] = [-120, 300, 380, 800]                 # leaves a 480 x 640 frame on two sides
    win[9] = [5, 5, 5, 5]                          # a degenerate window
    win[10] = [10, 20, 110, 90]                    # sides that differ are taken as they are
    box = r.uniform(-0.5, 0.5, (n, 8, 3)).astype(np.float32)
    return poses, rms, kp, win, seeded_K(n, seed + 1), box


@pytest.mark.parametrize("out_size", [224, 56])
def test_results_equal_the_fp64_restatement_bit_for_bit(out_size):
    case = results_case()
    want = results_reference(*case, out_size)
    got = hip_ops.stream_results_host(*case, out_size)
    assert got.shape == (70, _lib.STREAM_ROW_FLOATS) and got.dtype == np.float32
    for name, sl in (("pose", slice(0, 16)), ("rms", slice(16, 17)), ("ok", slice(17, 18)), ("corners, crop", slice(18, 34)),
                     ("corners, frame", slice(34, 50)), ("box, frame", slice(50, 66))):
        assert np.array_equal(bits(got[:, sl]), bits(want[:, sl])), name
    # the special samples are what they claim to be
    assert got[:, 17].tolist() == [1.0] + [0.0] * 5 + [1.0] * 64
    assert np.isfinite(got[:, :16]).all() and (got[1:6, 50:] == 0).all() and got[1, 1] == 0 and got[2, 7] == 0 and got[3, 8] == 0
    behind = np.isnan(got[6, 50:])
    assert behind.any() and not behind.all() and np.isnan(got[7, 50:]).all()
    assert np.isfinite(got[0, 50:]).all() and np.isfinite(got[8:, 34:50]).all()
    for n in (1, 65):
        part = hip_ops.stream_results_host(*(a[3:3 + n] for a in case), out_size)
        assert np.array_equal(bits(part), bits(got[3:3 + n]))


def test_argument_checks_run_before_any_launch():
    lib = _lib.load()
    f = np.zeros(66 * 4, np.float32)
    w = np.zeros(16, np.int32)
    p, q = f.ctypes.data, w.ctypes.data                      # non-NULL addresses; no call below gets as far as using them
    NULL, SHAPE, OK = -5, -1, 0
    for dev in (True, False):
        win = lib.bd_stream_windows if dev else lib.bd_stream_windows_host
        res = lib.bd_stream_results if dev else lib.bd_stream_results_host
        tail = (None,) if dev else ()                        # the stream
        good = [p, p, 0.1, 224, q, p, 1]
        for i in (0, 1, 4, 5):
            bad = list(good)
            bad[i] = None
            assert win(*bad, *tail) == NULL, (dev, i)
        for n, size in ((-1, 224), (65536, 224), (1, 0), (1, -3)):
            assert win(p, p, 0.1, size, q, p, n, *tail) == SHAPE, (dev, n, size)
        assert win(None, p, 0.1, 224, q, p, 0, *tail) == NULL          # NULL is looked at first
        assert win(p, p, 0.1, 224, q, p, 0, *tail) == OK               # nothing to do: no launch
        good = [p, p, p, q, p, p, 224, p, 1]
        for i in (0, 1, 2, 3, 4, 5, 7):
            bad = list(good)
            bad[i] = None
            assert res(*bad, *tail) == NULL, (dev, i)
        for n, size in ((-1, 224), (65536, 224), (1, 0)):
            assert res(p, p, p, q, p, p, size, p, n, *tail) == SHAPE, (dev, n, size)
        assert res(p, p, p, q, p, p, 224, p, 0, *tail) == OK
    # the host forms take the largest n the device forms take
    n = 65535
    boxes = np.tile(np.array([[10, 20, 110, 100]], np.float32), (n, 1))
    wins, _ = hip_ops.stream_windows_host(boxes, np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)))
    assert (wins == wins[0]).all() and wins[0].tolist() == pp.square_bbox(torch.from_numpy(boxes[:1]), 0.1)[0].tolist()
    assert ctypes.sizeof(ctypes.c_float) * _lib.STREAM_ROW_FLOATS == 264


@pytest.mark.parametrize("track_boxes", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_flat_buffer_layout_is_contiguous_and_the_same_on_both_sides(B, track_boxes):
    """stream._layout describes a session's flat input and output buffers once; stream._cut makes the device views and the pinned views
    from it (two host buffers stand in for them here)."""
    from boxdreamer_amd import stream
    ins, outs = stream._layout(B, track_boxes)
    assert [f[0] for f in ins] == ["det_boxes", "K"] + (["det_valid"] if track_boxes else [])
    assert [f[0] for f in outs] == ["rows"] + (["track"] if track_boxes else [])
    shapes = dict(det_boxes=(B, 4), K=(B, 3, 3), det_valid=(B,), rows=(B, 66), track=(B, 5))
    for fields, words in ((ins, B * (14 if track_boxes else 13)), (outs, B * (71 if track_boxes else 66))):
        assert sum(int(np.prod(shape)) for _, shape, _ in fields) == words
        (dev, dev_views), (pin, pin_views) = stream._cut(fields, device="cpu"), stream._cut(fields)
        assert dev.dtype == pin.dtype == torch.float32 and dev.shape == pin.shape == (words,) and dev.data_ptr() != pin.data_ptr()
        assert list(dev_views) == list(pin_views) == [f[0] for f in fields]
        at = 0
        for name, shape, dtype in fields:
            d, p = dev_views[name], pin_views[name]
            assert dtype == (torch.int32 if name == "det_valid" else torch.float32) and dtype.itemsize == 4
            assert d.dtype == p.dtype == dtype and tuple(d.shape) == tuple(p.shape) == tuple(shape) == shapes[name]
            assert d.is_contiguous() and p.is_contiguous()
            assert d.storage_offset() == p.storage_offset() == at                    # the next field starts where the last one ended
            assert (d.data_ptr() - dev.data_ptr()) == (p.data_ptr() - pin.data_ptr()) == 4 * at and d.data_ptr() % 4 == 0
            d.fill_(1)                                                              # a view of the flat buffer, and of its own words only
            assert int((dev.view(torch.int32) != 0).sum()) == d.numel() and bool((dev[at:at + d.numel()].view(torch.int32) != 0).all())
            dev.zero_()
            at += d.numel()
        assert at == words == dev.numel()


def _host_model(depth=1):
    from boxdreamer_amd.model import BoxDreamer
    path = os.path.join(ROOT, "tests", "golden", "model_modules_config.json")
    m = copy.deepcopy(json.load(open(path))["modules"])
    m["decoder"].update(num_decoder_layers=depth)
    m["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=depth)
    return BoxDreamer({"modules": m}).eval()


def test_constructor_refusals_that_need_no_device():
    from boxdreamer_amd.cache import RefFeatureBank
    from boxdreamer_amd.stream import PoseStream
    model, other = _host_model(), _host_model()
    box = torch.zeros((1, 8, 3))
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    kw = dict(frame_shape=(96, 128))
    with pytest.raises(ValueError, match=r"RefFeatureBank\(encoder, decoder=model\.decoder\)"):      # a feature-only bank
        PoseStream(model, RefFeatureBank(model.rgb_encoder), [[0]], box, **kw)
    with pytest.raises(ValueError, match="another encoder"):
        PoseStream(model, RefFeatureBank(other.rgb_encoder, decoder=model.decoder), [[0]], box, **kw)
    with pytest.raises(ValueError, match="another decoder"):
        PoseStream(model, RefFeatureBank(model.rgb_encoder, decoder=other.decoder), [[0]], box, **kw)
    with pytest.raises(ValueError, match="nor a row of the bank"):                                   # out of range (the bank is empty)
        PoseStream(model, bank, [[0]], box, **kw)
    with pytest.raises(ValueError, match="nor a row of the bank"):
        PoseStream(model, bank, torch.tensor([[-2, 0]]), box, **kw)
    with pytest.raises(ValueError, match=r"\(B, T_max\)"):                                           # not (B, T - 1)
        PoseStream(model, bank, [[0, 1], [2]], torch.zeros((2, 8, 3)), **kw)
    with pytest.raises(ValueError, match=r"\(B, T - 1\)"):
        PoseStream(model, bank, torch.zeros((2, 2, 2), dtype=torch.int64), torch.zeros((2, 8, 3)), **kw)
    with pytest.raises(ValueError, match="T < 2"):
        PoseStream(model, bank, [[]], box, **kw)
    with pytest.raises(ValueError, match="B >= 1"):
        PoseStream(model, bank, [], box, **kw)
    with pytest.raises(ValueError, match="eval mode"):
        PoseStream(model.train(), bank, [[0]], box, **kw)
    model.eval()
    from boxdreamer_amd.stream import _ref_rows                   # a bank of three rows: -1 (encode this slot) is no reference
    assert _ref_rows([[0, 2], [2, 1]], 3) == ([[0, 2], [2, 1]], 2, 3)
    with pytest.raises(ValueError, match="encodes the query only"):
        _ref_rows([[0, -1]], 3)
    with pytest.raises(ValueError, match="nor a row of the bank"):
        _ref_rows([[0, 3]], 3)
    for bad in (torch.zeros((1, 2)), torch.zeros((1, 2), dtype=torch.bool)):       # a tensor of another kind: the table's own refusal
        with pytest.raises(TypeError, match="must be an integer tensor"):
            _ref_rows(bad, 3)
    assert _ref_rows(torch.tensor([[0, 2], [2, 1]]), 3) == ([[0, 2], [2, 1]], 2, 3)
