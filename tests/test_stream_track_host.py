"""Host: a pose stream that follows each object's box from its own last pose (stream.PoseStream(track_boxes=True); csrc/stream.hip:
bd_stream_track_windows) -- the kernel's host twin (bd_stream_track_windows_host, the SAME __host__ __device__ arithmetic) against the
numpy mirror of its decision and box (stream.track_windows_host), bit for bit, on ~500 seeded objects built so that every source and
every way a tracked box is refused occurs; the entry points' argument checks, which run before any launch; and the session's
refusals that need no device.  Bits are compared as test_stream_host.bits compares them (a NaN: "NaN at the same place")."""
import math
import os
import re

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, stream
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.stream import BOX_DETECTOR, BOX_HELD, BOX_TRACKED, PoseStream, track_windows_host
from test_stream_host import _host_model, bits, seeded_boxes

FRAME = (480, 640)
MAX_RMS, MIN_SIDE, MAX_SIDE = 4.0, 8.0, 4.0 * 640
FX, FY, CX, CY = (float(np.float32(v)) for v in (600.0, 540.0, 320.0, 240.0))
HALF = float(np.float32(0.2))                               # half the side of the 3-D box, as the fp32 value the kernel reads


def _rotations(n, r, angle):
    rv = r.uniform(-1, 1, (n, 3))
    out = np.zeros((n, 3, 3))
    for i in range(n):
        k = rv[i] / np.linalg.norm(rv[i])
        th = r.uniform(0, angle)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        out[i] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return out


def track_case(seed=3):
    """500 objects for a 480 x 640 frame.  The 3-D box is a cube of side 0.4 around the origin, K has no skew; a group's translation puts
    the projected box where the group's name says.  With the identity rotation the extreme corners are known in closed form: max u =
    FX (tx + HALF) / (tz -+ HALF) + CX, on the near face (z = -HALF) where tx + HALF > 0 and on the far face where it is negative,
    which places an edge a chosen fraction of a pixel from a threshold."""
    r = np.random.default_rng(seed)
    groups, R, t = [], [], []

    def add(name, n, tx, ty, tz, rot=None):
        groups.extend([name] * n)
        R.append(np.tile(np.eye(3), (n, 1, 1)) if rot is None else rot)
        t.append(np.stack([np.broadcast_to(tx, (n,)), np.broadcast_to(ty, (n,)), np.broadcast_to(tz, (n,))], 1))

    tz = r.uniform(2, 6, 110)
    add("inside", 110, r.uniform(-0.35, 0.35, 110) * tz, r.uniform(-0.25, 0.25, 110) * tz, tz, _rotations(110, r, 1.0))
    tz = r.uniform(2, 6, 60)                                                                # the centre near the frame's left / top edge
    add("partly outside", 60, (r.uniform(-20, 20, 60) - CX) / FX * tz, (r.uniform(-20, 500, 60) - CY) / FY * tz, tz, _rotations(60, r, 1.0))
    tz = r.uniform(2, 6, 40)
    add("wholly outside", 40, r.choice([-1.0, 1.0], 40) * r.uniform(0.8, 2.0, 40) * tz, r.uniform(-0.2, 0.2, 40) * tz, tz)
    add("behind", 30, r.uniform(-0.1, 0.1, 30), r.uniform(-0.1, 0.1, 30), np.concatenate([r.uniform(-0.15, 0.15, 20), r.uniform(-5, -1, 10)]))
    # the visible extent (0 .. max u) a fraction of a pixel under / over MIN_SIDE: the box leaves the frame on the left, where
    # tx + HALF < 0 and the largest u belongs to the FAR face, z = +HALF
    d = np.concatenate([-r.uniform(0.01, 0.5, 20), r.uniform(0.01, 0.5, 20)])
    tz = r.uniform(3, 5, 40)
    add("min side", 40, (MIN_SIDE + d - CX) * (tz + HALF) / FX - HALF, r.uniform(-0.1, 0.1, 40), tz)
    # the unclipped extent 2 FX HALF / (tz - HALF) a fraction of a pixel under / over MAX_SIDE: the object nearly on the camera
    d = np.concatenate([-r.uniform(0.05, 0.5, 20), r.uniform(0.05, 0.5, 20)])
    add("max side", 40, 0.0, 0.0, HALF + 2.0 * FX * HALF / (MAX_SIDE + d))
    for name, n in (("ok 0", 40), ("rms nan", 20), ("rms equal", 20), ("rms above", 20), ("force", 40), ("det not finite", 40)):
        tz = r.uniform(2, 6, n)
        add(name, n, r.uniform(-0.3, 0.3, n) * tz, r.uniform(-0.2, 0.2, n) * tz, tz, _rotations(n, r, 1.0))
    groups = np.array(groups)
    n = len(groups)
    assert n == 500
    prev = r.uniform(-5, 5, (n, _lib.STREAM_ROW_FLOATS)).astype(np.float32)                 # (the other slots are not the kernel's business)
    pose = np.zeros((n, 4, 4), np.float32)
    pose[:, :3, :3], pose[:, :3, 3], pose[:, 3, 3] = np.concatenate(R), np.concatenate(t), 1.0
    prev[:, :16] = pose.reshape(n, 16)
    prev[:, 16] = r.uniform(0, MAX_RMS, n)
    prev[:, 17] = 1.0
    prev[groups == "ok 0", 17] = np.repeat([0.0, 0.5], 20)                                  # (ok is compared with 1: 0.5 is no pose either)
    prev[groups == "rms nan", 16] = np.nan
    prev[groups == "rms equal", 16] = MAX_RMS
    prev[groups == "rms above", 16] = np.concatenate([np.nextafter(np.float32(MAX_RMS), np.float32(9)).repeat(10), r.uniform(4.5, 90, 9), [np.inf]])
    force = np.zeros(n, np.int32)
    force[groups == "force"] = r.choice([1, -3, 7], 40)
    det_valid = r.choice([0, 1, 5], n).astype(np.int32)
    det = seeded_boxes(seed + 1)[r.permutation(500)[:n]]
    bad = np.flatnonzero(groups == "det not finite")
    prev[bad, 17] = 0.0                                                                     # not trusted, so the detection is what counts
    det_valid[bad] = 1
    det[bad[0::4], 0], det[bad[1::4], 3], det[bad[2::4], 2], det[bad[3::4], 1] = np.nan, np.inf, -np.inf, 1e12
    state = seeded_boxes(seed + 2)[r.permutation(500)[:n]]
    box = np.zeros((n, 8, 3), np.float32)
    box[:] = np.array([[sx, sy, sz] for sx in (-HALF, HALF) for sy in (-HALF, HALF) for sz in (-HALF, HALF)], np.float32)
    K = np.zeros((n, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = FX, FY, CX, CY, 1.0
    return dict(groups=groups, args=(prev, box, K, det, det_valid, force, state))


_CASE = {}


def _case():
    if not _CASE:
        c = track_case()
        c["mirror"] = track_windows_host(*c["args"], frame_shape=FRAME, max_rms_px=MAX_RMS, min_side_px=MIN_SIDE, max_side_px=MAX_SIDE)
        _CASE.update(c)
    return _CASE


def test_the_cases_cover_every_source_and_every_refusal():
    """A condition on the inputs, met by the mirror alone."""
    c = _case()
    g, m = c["groups"], c["mirror"]
    prev, _, _, det, det_valid, force, _ = c["args"]
    for src in (BOX_DETECTOR, BOX_TRACKED, BOX_HELD):
        assert (m["src"] == src).sum() >= 10, src
    assert (~m["finite"]).sum() >= 10 and (m["finite"] & ~m["visible"]).sum() >= 10 and (m["finite"] & ~m["bounded"]).sum() >= 10
    t = m["tracked"].astype(np.float64)
    vis_x = np.minimum(t[:, 2], 640.0) - np.maximum(t[:, 0], 0.0)
    ext_x = t[:, 2] - t[:, 0]
    inside = (t[:, 0] >= 0) & (t[:, 1] >= 0) & (t[:, 2] <= 640) & (t[:, 3] <= 480)
    assert (inside & m["trusted"]).sum() >= 10
    assert (m["trusted"] & ~inside).sum() >= 10                                 # partly outside, and taken unclipped
    assert (m["finite"] & ((t[:, 2] < 0) | (t[:, 0] > 640))).sum() >= 10        # wholly outside
    assert (np.isnan(m["tracked"]).any(1) & (g == "behind")).sum() >= 10
    s = g == "min side"
    assert ((vis_x[s] < MIN_SIDE) & (vis_x[s] > MIN_SIDE - 1) & ~m["visible"][s]).sum() >= 10
    assert ((vis_x[s] >= MIN_SIDE) & (vis_x[s] < MIN_SIDE + 1) & m["trusted"][s]).sum() >= 10
    s = g == "max side"
    assert ((ext_x[s] > MAX_SIDE) & (ext_x[s] < MAX_SIDE + 1) & ~m["bounded"][s]).sum() >= 10
    assert ((ext_x[s] <= MAX_SIDE) & (ext_x[s] > MAX_SIDE - 1) & m["trusted"][s]).sum() >= 10
    # every way a usable box is still not trusted, and the boundary that is
    for name in ("ok 0", "rms nan", "rms above", "force"):
        assert m["valid"][g == name].sum() >= 10 and not m["trusted"][g == name].any(), name
    assert m["trusted"][g == "rms equal"].sum() >= 10 and (prev[g == "rms equal", 16] == MAX_RMS).all()
    untrusted = ~m["trusted"]
    assert (untrusted & (det_valid == 0)).sum() >= 10 and (untrusted & (det_valid != 0)).sum() >= 10
    assert (~np.isfinite(det).all(1) & (m["src"] == BOX_DETECTOR)).sum() >= 10
    assert (force != 0).sum() >= 10


@pytest.mark.parametrize("out_size", [224, 56])
@pytest.mark.parametrize("padding", [0.0, 0.1])
def test_host_twin_equals_the_numpy_mirror_bit_for_bit(padding, out_size):
    c = _case()
    m, args = c["mirror"], c["args"]
    prev, box3, K, det, det_valid, force, state = args
    kw = dict(frame_shape=FRAME, max_rms_px=MAX_RMS, min_side_px=MIN_SIDE, max_side_px=MAX_SIDE)
    before = [a.copy() for a in args]
    got = hip_ops.stream_track_windows_host(*args, padding, out_size, want_keep=True, **kw)
    assert all(np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b) for a, b in zip(args, before))
    assert got["box_src"].dtype == np.int32 and np.array_equal(got["box_src"], m["src"])
    assert np.array_equal(bits(got["state_box"]), bits(m["box"]))
    assert got["keep_boxes"].dtype == np.int32 and np.array_equal(got["keep_boxes"], m["keep"])
    assert np.array_equal(bits(got["track"][:, :4]), bits(m["box"])) and np.array_equal(got["track"][:, 4], m["src"].astype(np.float32))
    want_w, want_k = hip_ops.stream_windows_host(m["box"], K, padding, out_size)
    assert np.array_equal(got["windows"], want_w) and np.array_equal(bits(got["K_crop"]), bits(want_k))
    # a detector-sourced object gets bd_stream_windows' window and intrinsics for its detection; a held one, for the box it held
    from_det, held = m["src"] == BOX_DETECTOR, m["src"] == BOX_HELD
    det_w, det_k = hip_ops.stream_windows_host(det, K, padding, out_size)
    assert np.array_equal(got["windows"][from_det], det_w[from_det]) and np.array_equal(bits(got["K_crop"][from_det]), bits(det_k[from_det]))
    assert np.array_equal(bits(got["state_box"][from_det]), bits(det[from_det])) and np.array_equal(bits(got["state_box"][held]), bits(state[held]))
    bad = from_det & ~np.isfinite(det).all(1)
    assert bad.sum() >= 10 and not got["windows"][bad].any() and not got["keep_boxes"][bad].any()
    # the tracked box is the min / max of the row slots bd_stream_results would write for that pose
    tr = m["src"] == BOX_TRACKED
    rows = hip_ops.stream_results_host(prev[:, :16].reshape(-1, 4, 4), prev[:, 16], np.zeros((500, 8, 2), np.float32),
                                       np.zeros((500, 4), np.int32), K, box3, out_size)
    uv = rows[tr, 50:66].reshape(-1, 8, 2)
    assert np.array_equal(bits(got["state_box"][tr]), bits(np.concatenate([uv.min(1), uv.max(1)], 1)))
    # the keep box: towards zero, the object's own box
    assert np.array_equal(got["keep_boxes"][tr], np.trunc(got["state_box"][tr].astype(np.float64)).astype(np.int32))
    assert (got["state_box"][tr] < 0).any() and (got["keep_boxes"][tr] != np.floor(got["state_box"][tr])).any()
    # without the keep output nothing else moves; an object's bits do not depend on the others of the call
    plain = hip_ops.stream_track_windows_host(*args, padding, out_size, **kw)
    assert "keep_boxes" not in plain and all(np.array_equal(bits(plain[k]) if plain[k].dtype == np.float32 else plain[k],
                                                            bits(got[k]) if got[k].dtype == np.float32 else got[k]) for k in plain)
    for start, n in ((100, 1), (180, 65), (330, 65)):
        part = hip_ops.stream_track_windows_host(*(a[start:start + n] for a in args), padding, out_size, want_keep=True, **kw)
        for k, v in part.items():
            assert np.array_equal(bits(v) if v.dtype == np.float32 else v,
                                  bits(got[k][start:start + n]) if v.dtype == np.float32 else got[k][start:start + n]), (k, start, n)


def test_abi_declares_the_entries_and_they_validate_before_any_launch():
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "boxdreamer_hip.h")).read()
    for name in ("bd_stream_track_windows", "bd_stream_track_windows_host"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"^int {name}\(", header, re.M), name
    for i, name in enumerate(("DETECTOR", "TRACKED", "HELD")):
        assert re.search(rf"^#define BD_STREAM_BOX_{name} {i}$", header, re.M)
    assert (_lib.STREAM_BOX_DETECTOR, _lib.STREAM_BOX_TRACKED, _lib.STREAM_BOX_HELD) == (0, 1, 2) == (BOX_DETECTOR, BOX_TRACKED, BOX_HELD)
    assert lib.bd_abi_version() == 9                                # the entries are additions
    p = [0x10000000 * (i + 1) for i in range(12)]                   # made-up addresses: every call below returns before anything is dereferenced
    NULL, SHAPE, OK = -5, -1, 0
    for dev in (True, False):
        fn = lib.bd_stream_track_windows if dev else lib.bd_stream_track_windows_host
        tail = (None,) if dev else ()

        def call(ptrs=p, out_size=224, fh=480, fw=640, min_side=8.0, max_side=2560.0, n=1):
            return fn(*ptrs[:7], 0.1, out_size, fh, fw, 4.0, min_side, max_side, *ptrs[7:12], n, *tail)

        for i in range(10):                                         # every pointer but keep_boxes (10) and track (11)
            assert call(ptrs=[None if j == i else x for j, x in enumerate(p)]) == NULL, (dev, i)
        nan = math.nan
        for kw in (dict(n=-1), dict(n=65536), dict(out_size=0), dict(out_size=-3), dict(fh=0), dict(fw=0), dict(fw=-640), dict(min_side=0.0),
                   dict(min_side=-8.0), dict(min_side=nan), dict(max_side=0.0), dict(max_side=-1.0), dict(max_side=nan)):
            assert call(**kw) == SHAPE, (dev, kw)
        assert call(ptrs=[None] * 12, n=-1) == NULL                 # NULL is looked at first
        for optional in ([10], [11], [10, 11]):                     # the optional outputs may be NULL; n == 0: nothing to do, no launch
            assert call(ptrs=[None if j in optional else x for j, x in enumerate(p)], n=0) == OK, (dev, optional)
        assert call(max_side=math.inf, n=0) == OK                   # (no upper bound at all is a positive bound)
    with pytest.raises(ValueError, match=r"shape \(3, 66\)"):
        hip_ops.stream_track_windows_host(np.zeros((3, 60), np.float32), *(_case()["args"][i][:3] for i in range(1, 7)))


def test_session_refusals_that_need_no_device():
    model = _host_model()
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    bank._n = 3                                                 # (nothing is encoded without a device: the length alone is looked at)
    box, kw = torch.zeros((2, 8, 3)), dict(frame_shape=(96, 128), track_boxes=True)
    rows = [[0, 1], [1, 2]]
    nan = math.nan
    for bad in (dict(min_side_px=nan), dict(min_side_px=0.0), dict(min_side_px=-1.0), dict(max_side_px=nan), dict(max_side_px=0.0),
                dict(max_side_px=-5.0)):
        with pytest.raises(ValueError, match=f"{next(iter(bad))} = .*positive number of pixels"):
            PoseStream(model, bank, rows, box, **kw, **bad)
    with pytest.raises(ValueError, match="max_rms_px is NaN"):                  # meaningful without select_k too
        PoseStream(model, bank, rows, box, max_rms_px=nan, **kw)
    with pytest.raises(ValueError, match=r"bbox_3d must be a tensor of shape \(2, 8, 3\)"):      # the existing refusals come first
        PoseStream(model, bank, rows, torch.zeros((1, 8, 3)), min_side_px=nan, **kw)
    assert stream._track_limits(True, 4, 8, None, 96, 128) == (4.0, 8.0, 512.0) and stream._track_limits(True, math.inf, 1, 9, 480, 640)[2] == 9.0
    assert stream._track_limits(False, nan, nan, nan, 480, 640)[2] != 0         # a session that does not track ignores them, as today
    # step(): who supplies the boxes
    det, valid, keep = torch.zeros((2, 4)), torch.tensor([1, 0]), torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="det_boxes=None given to a session built without track_boxes"):
        stream._step_boxes(False, None, None, None, 2)
    with pytest.raises(ValueError, match="det_valid given to a session built without track_boxes"):
        stream._step_boxes(False, det, valid, None, 2)
    with pytest.raises(ValueError, match="keep_boxes given to a session built with track_boxes"):
        stream._step_boxes(True, det, None, keep, 2)
    with pytest.raises(ValueError, match="det_valid given without det_boxes"):
        stream._step_boxes(True, None, valid, None, 2)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.bool), [1], 1):
        with pytest.raises(ValueError, match=r"det_valid must be \(2,\)"):
            stream._step_boxes(True, det, bad, None, 2)
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.float64), [0.5, 1.0]):
        with pytest.raises(ValueError, match="det_valid must be integers or bools"):
            stream._step_boxes(True, det, bad, None, 2)
    assert stream._step_boxes(True, det, [1, 0], None, 2).tolist() == [1, 0] and stream._step_boxes(True, det, torch.tensor([True, False]), None, 2).dtype == torch.bool
    assert stream._step_boxes(True, None, None, None, 2) is None and stream._step_boxes(True, det, None, None, 2) is None
    assert stream._step_boxes(False, det, None, keep, 2) is None                # (use_keep_boxes is step()'s own check, unchanged)


def test_mirror_by_hand():
    """The mirror against values worked out by hand: the identity pose at depth 4, a cube of side 2, f = 100, c = (64, 48)."""
    prev = np.zeros((4, 66), np.float32)
    prev[:, 0], prev[:, 5], prev[:, 10], prev[:, 15], prev[:, 11], prev[:, 17] = 1, 1, 1, 1, 4, 1
    box = np.tile(np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32), (4, 1, 1))
    K = np.tile(np.array([[100, 0, 64], [0, 100, 48], [0, 0, 1]], np.float32), (4, 1, 1))
    det = np.tile(np.array([[1.5, -2.5, 30.25, 40.75]], np.float32), (4, 1))
    state = np.tile(np.array([[5, 6, 7, 8]], np.float32), (4, 1))
    prev[3, 16] = 2.5
    m = track_windows_host(prev, box, K, det, [1, 1, 0, 1], [0, 1, 1, 0], state, frame_shape=(96, 128), max_rms_px=2.0)
    third = np.float32(100 / 3)                                 # the near face, z = 3: 64 +- 100 / 3, 48 +- 100 / 3
    assert m["src"].tolist() == [BOX_TRACKED, BOX_DETECTOR, BOX_HELD, BOX_DETECTOR] and m["valid"].all() and m["trusted"].tolist() == [True, False, False, False]
    assert np.allclose(m["box"][0], [64 - third, 48 - third, 64 + third, 48 + third], rtol=1e-6, atol=0) and m["keep"][0].tolist() == [30, 14, 97, 81]
    assert m["box"][1].tolist() == det[0].tolist() and m["keep"][1].tolist() == [1, -2, 30, 40] and m["box"][2].tolist() == [5, 6, 7, 8]
    small = track_windows_host(prev, box, K, det, [0] * 4, [0] * 4, state, frame_shape=(96, 128), min_side_px=67.0)
    assert not small["visible"].any() and small["bounded"].all() and small["src"].tolist() == [BOX_HELD] * 4
    large = track_windows_host(prev, box, K, det, [0] * 4, [0] * 4, state, frame_shape=(96, 128), max_side_px=66.0)
    assert large["visible"].all() and not large["bounded"].any()
