"""Pose stream: the reference demo's per-frame call (src/demo/demo.py:1451-1514: one `model(batch)` per frame at batch 1, the same
reference views for every frame) as ONE captured HIP graph per frame over banked references.

    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)        # once per object: the references' decoder-entry tokens
    rows = bank.add(ref_images, bbox_feat=ref_heatmaps)
    s = PoseStream(model, bank, [rows.tolist()], bbox_3d, frame_shape=(480, 640))
    for frame in camera:                                                   # pinned uint8 (480, 640, 3)
        row = s.step(frame, det_box, K)[0]                                 # pinned fp32 (66,): pose, rms, ok, corners, projected box

`graph.GraphedPath` replays the whole path but re-encodes all T views every frame; a forward over an entry-token bank encodes the
query only but runs eagerly (about 150 short launches plus the facade's torch glue per frame).  A PoseStream owns one streaming
session -- B tracked objects, each with its T - 1 banked references, a fixed frame shape -- and captures its step once:

    bd_stream_windows -> bd_crop_resize_frames -> encoder (the B query crops) -> BETR.forward_entry (private copy of the bank's
    rows) -> bd_decode_topk -> bd_solve_pnp_wave -> bd_stream_results

(`frame_format=`: bd_crop_resize_frames_fmt in that place, on BGR, RGBA / BGRA or NV12 frames as the source delivers them.)

`step()` copies the frame, the detector boxes and K into static buffers, replays the graph, enqueues ONE D2H of the result rows into
a pinned buffer and waits for that copy's event.  Nothing is carried from frame to frame.

With `select_k=k` each object's `ref_rows` is its whole DATABASE of banked views (up to 1024, lengths may differ) and the k views the
decoder reads are chosen on the device every frame, inside the same captured graph (T = k + 1):

    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder, match_threshold=0.05, keep_poses=True)
    rows = bank.add(db_images, bbox_feat=db_heatmaps, poses=db_poses)
    s = PoseStream(model, bank, [rows.tolist()], bbox_3d, frame_shape=(480, 640), select_k=5, select="track", max_rms_px=4.0)

    ... encoder -> bd_match_view_sums (the B query crops) -> bd_stream_select_rows (writes the decoder's source table) ->
    BETR.forward_entry -> ...

`select="dino"` chooses by appearance, the dense-reference mode's DINO filter (bd_match_select_rows' scores and ranking); nothing is
carried from frame to frame there either.  `select="track"` chooses the k views nearest to the LAST frame's pose
(bd_pose_select_rows' distance and ranking, the dense mode's fine level with the last pose standing in for the coarse pose) while
that pose is trustworthy -- the last row's ok == 1 and its rms_px <= max_rms_px -- and by appearance otherwise: on the first step,
after `reset()`, after a failed or poor solve, and for the objects `step(..., relocalise=...)` names.  A "track" step therefore
DEPENDS on the previous step's result rows: that is the one thing such a session carries from frame to frame.

With `track_boxes=True` a session needs no detector box per frame: the step's first node is bd_stream_track_windows, which takes
each object's crop box from its OWN last pose -- the min / max of the 3-D box's 8 corners projected with the last result row's pose
and this frame's K (the rule of the OnePose reproj_box files, src/datasets/onepose.py:437-455) -- while that pose is trusted (the
rule above, `relocalise` included) and the box is usable (every corner in front of the camera, at least min_side_px of it inside the
frame on both axes, at most max_side_px across), a detector box when one is offered and the pose is not trusted, and the last box
otherwise:

    s = PoseStream(model, bank, [rows.tolist()], bbox_3d, frame_shape=(480, 640), track_boxes=True, max_rms_px=4.0)
    s.step(frame, det_box, K)                   # no pose yet: the detection
    s.step(frame, None, K)                      # nobody has a detection: the box follows the last pose
    x0, y0, x1, y1, src = s.track_host[0]       # the box this step used and its source (BOX_DETECTOR / BOX_TRACKED / BOX_HELD)

One node for one node, decided inside the captured graph; the box lags the pose by one frame, which `padding` covers.

Limits: an entry-token bank only; the same T for every sample; a fixed frame shape and frame count; the encoder and the decoder are
frozen while the session lives (a larger eager batch, .to() or a checkpoint load raises; `del` the session first).
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib, calibrate, graph, hip_ops
from .betr import BETR
from .box_utils import solve_poses_device
from .preprocess import crop_resize_frames, frame_shape_of, resolve_format

ROW_POSE, ROW_RMS, ROW_OK = slice(0, 16), 16, 17
ROW_CORNERS_CROP, ROW_CORNERS_FRAME, ROW_BOX_FRAME = slice(18, 34), slice(34, 50), slice(50, 66)


def _host_lists(ref_rows, refusal: str):
    """`ref_rows` as nested host lists -> one list per tracked object, or ValueError(refusal); tensors and entries are the caller's to check."""
    try:
        return [list(r) for r in ref_rows]
    except TypeError:
        raise ValueError(refusal) from None


def _ref_rows(ref_rows, bank_len: int):
    """`ref_rows` (host ints (B, T - 1): a nested list or a CPU int tensor) -> (B lists of T - 1 bank rows, B, T), validated."""
    if isinstance(ref_rows, torch.Tensor):
        if ref_rows.dim() != 2:
            raise ValueError(f"ref_rows must be (B, T - 1) host integers, got shape {tuple(ref_rows.shape)}")
        B, R = int(ref_rows.shape[0]), int(ref_rows.shape[1])
    else:
        ref_rows = _host_lists(ref_rows, "ref_rows must be (B, T - 1) host integers: one list of bank rows per tracked object")
        B, R = len(ref_rows), (len(ref_rows[0]) if ref_rows else 0)
    if B < 1:
        raise ValueError("ref_rows names no sample: a pose stream tracks B >= 1 objects")
    rows = _lib.ref_rows_table(ref_rows, B, R)          # (every sample has the same number of references: ValueError otherwise)
    if R < 1:
        raise ValueError("T < 2: every sample needs at least one banked reference next to its query (ref_rows is (B, T - 1))")
    _lib.check_ref_rows(rows, [R] * B, bank_len)
    for b, row in enumerate(rows):
        for t, r in enumerate(row):
            if r < 0:
                raise ValueError(f"ref_rows[{b}][{t}] = {r}: a pose stream encodes the query only, every reference is a row of the bank")
    return rows, B, R + 1


SELECT_RULES = {"dino": _lib.STREAM_SELECT_DINO, "track": _lib.STREAM_SELECT_TRACK}
MAX_DATABASE = 1024         # slots one bd_stream_select_rows workgroup ranks


def _ref_database(ref_rows, bank_len: int, k):
    """`ref_rows` of a session that selects (host ints: B lists of bank rows, lengths may differ) -> (B lists, n_refs, N_max), validated
    against the bank's length and `select_k`."""
    refusal = "ref_rows must be host integers: one list of bank rows (its database) per tracked object"
    if isinstance(ref_rows, torch.Tensor):
        if ref_rows.device.type != "cpu" or ref_rows.dtype.is_floating_point or ref_rows.dtype == torch.bool or ref_rows.dim() != 2:
            raise ValueError(refusal)
        ref_rows = ref_rows.tolist()
    rows = _host_lists(ref_rows, refusal)
    if len(rows) < 1:
        raise ValueError("ref_rows names no sample: a pose stream tracks B >= 1 objects")
    if any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) for row in rows for r in row):
        raise ValueError("ref_rows must be integers: every entry of a database is a row of the bank")
    rows = [[int(r) for r in row] for row in rows]
    for b, row in enumerate(rows):
        for t, r in enumerate(row):
            if not 0 <= r < bank_len:
                raise ValueError(f"ref_rows[{b}][{t}] = {r} is not a row of the bank (it holds {bank_len}): every entry of a database is")
    n_refs = [len(r) for r in rows]
    if max(n_refs) > MAX_DATABASE:
        raise ValueError(f"a database of {max(n_refs)} views: one bd_stream_select_rows launch ranks at most {MAX_DATABASE} per object")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"select_k must be a positive integer, got {k!r}")
    if k > min(n_refs):
        raise ValueError(f"select_k = {k} exceeds the smallest database ({min(n_refs)} views, object {n_refs.index(min(n_refs))}): every "
                         "frame decodes against k views of the object's own")
    return rows, n_refs, max(n_refs)


def _flags(t, B: int, name: str) -> torch.Tensor:
    """step()'s `relocalise` / `det_valid`, one integer or bool flag per tracked object -> a (B,) tensor, host or device, never read here."""
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise ValueError(f"{name} must be integers or bools, got {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"{name} must be ({B},) for this session of B = {B}: one flag per tracked object, got {tuple(t.shape)}")
    return t


def _relocalise(relocalise, B: int) -> torch.Tensor:
    return _flags(relocalise, B, "relocalise")


def _rank_key(v: float, slot: int):
    """bd_pose_select_rows' order on a stored fp32 distance: numbers before NaNs, smaller first (+inf ordinary), then the position."""
    nan = v != v
    return (nan, 0.0 if nan else v, slot)


def select_rows_host(scores, dist, prev_rows, force, n_refs, k, rule, max_rms_px=float("inf")):
    """bd_stream_select_rows' decision and rankings on the host, from the two value arrays the kernel writes: scores (B, N_max), dist
    (B, N_max) or None (rule "dino"), prev_rows (B, 66), force (B,), n_refs (B,), rule "dino" / "track" (or _lib.STREAM_SELECT_*) ->
    (used int32 (B,), sel int32 (B, k)), numpy.  Plain sorts, not the kernels' rounds:
      rule        pose when rule is "track", force[b] == 0, prev ok == 1 and prev rms_px <= max_rms_px (a NaN rms fails it)
      appearance  the slots [0, n_refs[b]) by (score descending, slot ascending), -inf an ordinary value, a NaN never picked
      pose        the VALID slots by (number before NaN, distance ascending, slot ascending), +inf an ordinary value; a slot whose
                  row lies outside the private store is no candidate -- it is the one whose score is -inf (a pair's score is finite)
    The first k of either order, ascending; -1 where fewer exist."""
    rule = SELECT_RULES.get(rule, rule)
    if rule not in SELECT_RULES.values():
        raise ValueError(f"unknown rule {rule!r}: choose from {sorted(SELECT_RULES)}")
    sc = np.asarray(torch.as_tensor(scores).cpu(), dtype=np.float32)
    B, n_max = sc.shape
    ds = None if dist is None else np.asarray(torch.as_tensor(dist).cpu(), dtype=np.float32)
    prev = np.asarray(torch.as_tensor(prev_rows).cpu(), dtype=np.float32).reshape(B, _lib.STREAM_ROW_FLOATS)
    force = np.asarray(torch.as_tensor(force).cpu()).reshape(B)
    n_refs = np.asarray(torch.as_tensor(n_refs).cpu()).reshape(B)
    k, max_rms = int(k), np.float32(max_rms_px)
    used, sel = np.zeros((B,), np.int32), np.full((B, k), -1, np.int32)
    for b in range(B):
        n = min(max(int(n_refs[b]), 0), n_max)
        by_pose = bool(rule == _lib.STREAM_SELECT_TRACK and force[b] == 0 and prev[b, ROW_OK] == 1.0 and prev[b, ROW_RMS] <= max_rms)
        if by_pose:
            if ds is None:
                raise ValueError("the pose rule applies and no distances were given")
            order = sorted((i for i in range(n) if sc[b, i] != -math.inf), key=lambda i: _rank_key(float(ds[b, i]), i))
        else:
            order = sorted((i for i in range(n) if sc[b, i] == sc[b, i]), key=lambda i: (-float(sc[b, i]), i))
        chosen = sorted(order[:k])
        used[b] = int(by_pose)
        sel[b, :len(chosen)] = chosen
    return used, sel


BOX_DETECTOR, BOX_TRACKED, BOX_HELD = _lib.STREAM_BOX_DETECTOR, _lib.STREAM_BOX_TRACKED, _lib.STREAM_BOX_HELD
TRACK_FLOATS = 5            # the tail a tracking session reports per object: x0 y0 x1 y1 of the box it used, then its source


def _step_boxes(track_boxes: bool, det_boxes, det_valid, keep_boxes, B: int):
    """What step() refuses about who supplies the boxes, before anything is copied -> det_valid as a validated tensor, or None."""
    if not track_boxes:
        if det_boxes is None:
            raise ValueError("det_boxes=None given to a session built without track_boxes: every step needs a box per tracked object")
        if det_valid is not None:
            raise ValueError("det_valid given to a session built without track_boxes: its boxes are always taken as given")
        return None
    if keep_boxes is not None:
        raise ValueError("keep_boxes given to a session built with track_boxes: bd_stream_track_windows writes them from the box it uses")
    if det_valid is None:
        return None
    if det_boxes is None:
        raise ValueError("det_valid given without det_boxes: there is no detection to call valid")
    return _flags(det_valid, B, "det_valid")


def _track_limits(track_boxes: bool, max_rms_px, min_side_px, max_side_px, H: int, W: int):
    """The constructor's track_boxes arguments -> (max_rms_px, min_side_px, max_side_px) as floats, validated."""
    max_rms_px, min_side_px = float(max_rms_px), float(min_side_px)
    max_side_px = 4.0 * max(H, W) if max_side_px is None else float(max_side_px)
    if track_boxes:
        if max_rms_px != max_rms_px:
            raise ValueError("max_rms_px is NaN: no solve would ever be trusted; give a number or inf")
        for name, v in (("min_side_px", min_side_px), ("max_side_px", max_side_px)):
            if not v > 0.0:
                raise ValueError(f"{name} = {v}: it must be a positive number of pixels (max_side_px=None: 4 x the longer frame side)")
    return max_rms_px, min_side_px, max_side_px


def track_windows_host(prev_rows, bbox_3d, K, det_boxes, det_valid, force, state_box, frame_shape=(480, 640), max_rms_px=float("inf"),
                       min_side_px=8.0, max_side_px=None):
    """bd_stream_track_windows' decision and box on the host, in plain numpy (fp64 from the fp32 inputs, numpy contracts nothing):
    prev_rows (n, 66), bbox_3d (n, 8, 3), K (n, 3, 3), det_boxes (n, 4), det_valid (n,), force (n,), state_box (n, 4) -> a dict of numpy
    arrays: box fp32 (n, 4) the box each object uses, src int32 (n,) BOX_DETECTOR / BOX_TRACKED / BOX_HELD, keep int32 (n, 4) the box
    truncated towards zero (zeros when not finite or outside int32), tracked fp32 (n, 4) the projected box whatever was decided, and
    the reasons, bool (n,): finite, visible (clipped extent >= min_side_px), bounded (extent <= max_side_px), valid, trusted.
      tracked  (min u, min v, max u, max v) of the 8 corners projected with prev_rows[:, 0:16] and K, each rounded to fp32; a corner
               with zc <= 0 is NaN
      trusted  prev ok == 1, prev rms_px <= max_rms_px (a NaN fails), force == 0, and the box finite, visible and bounded
      box      tracked when trusted, else det_boxes where det_valid != 0, else state_box"""
    f64 = np.float64
    prev = np.asarray(torch.as_tensor(prev_rows).cpu(), dtype=np.float32)
    n = len(prev)
    prev = prev.reshape(n, _lib.STREAM_ROW_FLOATS)
    X = np.asarray(torch.as_tensor(bbox_3d).cpu(), dtype=np.float32).reshape(n, 8, 3).astype(f64)
    Kd = np.asarray(torch.as_tensor(K).cpu(), dtype=np.float32).reshape(n, 3, 3).astype(f64)
    det = np.asarray(torch.as_tensor(det_boxes).cpu(), dtype=np.float32).reshape(n, 4)
    det_valid = np.asarray(torch.as_tensor(det_valid).cpu()).reshape(n)
    force = np.asarray(torch.as_tensor(force).cpu()).reshape(n)
    state = np.asarray(torch.as_tensor(state_box).cpu(), dtype=np.float32).reshape(n, 4)
    H, W = (int(v) for v in frame_shape)
    max_side = f64(4.0 * max(H, W) if max_side_px is None else max_side_px)
    P = prev[:, ROW_POSE].reshape(n, 4, 4).astype(f64)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        xc, yc, zc = (((P[:, r, 0:1] * x + P[:, r, 1:2] * y) + P[:, r, 2:3] * z) + P[:, r, 3:4] for r in range(3))
        u = ((Kd[:, 0, 0:1] * xc + Kd[:, 0, 1:2] * yc) + Kd[:, 0, 2:3] * zc) / zc
        v = (Kd[:, 1, 1:2] * yc + Kd[:, 1, 2:3] * zc) / zc
        u = np.where(zc <= 0, np.nan, u).astype(np.float32)
        v = np.where(zc <= 0, np.nan, v).astype(np.float32)
        finite = np.isfinite(u).all(1) & np.isfinite(v).all(1)
        lo_u, hi_u, lo_v, hi_v = u[:, 0], u[:, 0], v[:, 0], v[:, 0]
        for j in range(1, 8):               # (the order of the comparisons is the kernel's: it decides nothing but the sign of a zero)
            lo_u, hi_u = np.where(u[:, j] < lo_u, u[:, j], lo_u), np.where(u[:, j] > hi_u, u[:, j], hi_u)
            lo_v, hi_v = np.where(v[:, j] < lo_v, v[:, j], lo_v), np.where(v[:, j] > hi_v, v[:, j], hi_v)
        tracked = np.stack([lo_u, lo_v, hi_u, hi_v], 1).astype(np.float32)
        t = tracked.astype(f64)
        vis_x = np.minimum(t[:, 2], f64(W)) - np.maximum(t[:, 0], 0.0)
        vis_y = np.minimum(t[:, 3], f64(H)) - np.maximum(t[:, 1], 0.0)
        visible = finite & (vis_x >= f64(min_side_px)) & (vis_y >= f64(min_side_px))
        bounded = finite & (t[:, 2] - t[:, 0] <= max_side) & (t[:, 3] - t[:, 1] <= max_side)
        valid = finite & visible & bounded
        trusted = (prev[:, ROW_OK] == 1.0) & (prev[:, ROW_RMS] <= np.float32(max_rms_px)) & (force == 0) & valid
    offered = det_valid != 0
    box = np.where(trusted[:, None], tracked, np.where(offered[:, None], det, state)).astype(np.float32)
    src = np.where(trusted, BOX_TRACKED, np.where(offered, BOX_DETECTOR, BOX_HELD)).astype(np.int32)
    with np.errstate(all="ignore"):
        tr = np.trunc(box.astype(f64))
        fits = (np.isfinite(tr) & (tr >= -2147483648.0) & (tr < 2147483648.0)).all(1)
        keep = np.where(fits[:, None], np.where(np.isfinite(tr), tr, 0.0), 0.0).astype(np.int64).astype(np.int32)
    return dict(box=box, src=src, keep=keep, tracked=tracked, finite=finite, visible=visible, bounded=bounded, valid=valid, trusted=trusted)


_Plan = namedtuple("_Plan", "rows B T n_refs n_max H W n_frames select_k select max_rms_px min_side_px max_side_px track_boxes "
                            "use_keep_boxes padding crop_dtype frame_format")


def _plan(model, bank, ref_rows, bbox_3d, frame_shape, n_frames, padding, crop_dtype, use_keep_boxes, select_k, select, max_rms_px,
          track_boxes, min_side_px, max_side_px, frame_format="rgb", colorspace=None, range=None) -> _Plan:
    """What a session is, decided from the constructor's arguments on the host: every refusal that needs no device, then the record."""
    if getattr(model, "training", False):
        raise ValueError("PoseStream needs the model in eval mode (model.eval()): the captured step is the evaluation path")
    decoder, encoder = getattr(model, "decoder", None), getattr(model, "rgb_encoder", None)
    if not isinstance(decoder, BETR):
        raise ValueError("PoseStream needs a BoxDreamer with the BETR decoder")
    if bank is None or not getattr(bank, "has_entry_tokens", False):
        raise ValueError("PoseStream runs over a reference bank that keeps decoder-entry tokens: build it with "
                         "RefFeatureBank(encoder, decoder=model.decoder)")
    if bank.encoder is not encoder:
        raise ValueError("the reference bank was built on another encoder than this model's rgb_encoder")
    if bank.decoder is not decoder:
        raise ValueError("the reference bank keeps the entry tokens of another decoder than this model's")
    if select not in SELECT_RULES:
        raise ValueError(f"unknown select {select!r}: choose from {sorted(SELECT_RULES)}")
    fmt = resolve_format(frame_format, colorspace, range)       # (an unknown name, a colorspace for frames that are not NV12: ValueError)
    if select_k is None:
        rows, B, T = _ref_rows(ref_rows, len(bank))
        n_refs = n_max = None
    else:
        if not getattr(bank, "has_match_summaries", False):
            raise ValueError("a selecting PoseStream scores the database by appearance and the reference bank keeps no match "
                             "summaries: build it with RefFeatureBank(encoder, decoder=model.decoder, match_threshold=0.05)")
        if select == "track" and not getattr(bank, "has_poses", False):
            raise ValueError('select="track" ranks the database by distance to the last pose and the reference bank keeps no poses: '
                             "build it with RefFeatureBank(encoder, decoder=model.decoder, match_threshold=0.05, keep_poses=True) "
                             "and add(images, bbox_feat=..., poses=...)")
        max_rms_px = float(max_rms_px)
        if max_rms_px != max_rms_px:
            raise ValueError("max_rms_px is NaN: no solve would ever be trusted; give a number or inf")
        rows, n_refs, n_max = _ref_database(ref_rows, len(bank), select_k)
        B, T, select_k = len(rows), int(select_k) + 1, int(select_k)
    if not isinstance(bbox_3d, torch.Tensor) or tuple(bbox_3d.shape) != (B, 8, 3):
        raise ValueError(f"bbox_3d must be a tensor of shape {(B, 8, 3)}, got {tuple(getattr(bbox_3d, 'shape', ()))}")
    H, W = (int(x) for x in frame_shape)
    n_frames = int(n_frames)
    if H < 1 or W < 1 or n_frames < 1:
        raise ValueError(f"frame_shape = {(H, W)} and n_frames = {n_frames} must be positive")
    frame_shape_of(fmt, n_frames, H, W)                         # (NV12 with an odd side)
    if crop_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"crop_dtype must be float32, float16 or bfloat16, got {crop_dtype}")
    track_boxes = bool(track_boxes)
    max_rms_px, min_side_px, max_side_px = _track_limits(track_boxes, max_rms_px, min_side_px, max_side_px, H, W)
    return _Plan(rows, B, T, n_refs, n_max, H, W, n_frames, select_k, select, max_rms_px, min_side_px, max_side_px, track_boxes,
                 bool(use_keep_boxes), float(padding), crop_dtype, fmt)


def _layout(B: int, track_boxes: bool):
    """A session's two flat buffers, each as its ordered fields (name, shape, dtype) of 4-byte words -> (input, output).  ONE H2D carries
    the input buffer, ONE D2H the output buffer; a tracking session's flags and box tail (x0 y0 x1 y1 src per object) ride along."""
    ins = [("det_boxes", (B, 4), torch.float32), ("K", (B, 3, 3), torch.float32)]
    outs = [("rows", (B, _lib.STREAM_ROW_FLOATS), torch.float32)]
    if track_boxes:
        ins.append(("det_valid", (B,), torch.int32))
        outs.append(("track", (B, TRACK_FLOATS), torch.float32))
    return ins, outs


def _cut(fields, **where):
    """One flat zeroed buffer (`where`: torch.zeros' device / pin_memory) -> (the buffer, {name: its view}), the fields in the order given."""
    flat = torch.zeros((sum(math.prod(shape) for _, shape, _ in fields),), dtype=torch.float32, **where)
    views, at = {}, 0
    for name, shape, dtype in fields:
        views[name] = flat[at:at + math.prod(shape)].view(dtype).view(shape)
        at += math.prod(shape)
    return flat, views


def _put(dev, pin, src, upload: bool = True) -> None:
    """step()'s staging rule, `src` into the static device tensor `dev`: a device source is copied on the device; a host source goes into
    the pinned twin `pin` (a copy from pageable memory would wait for the stream) and on in one non-blocking H2D (upload=False: the
    caller's own H2D of a whole buffer follows).  pin=None: straight into `dev` wherever the source lives."""
    if src.is_cuda or pin is None:
        dev.copy_(src, non_blocking=True)
    else:
        pin.copy_(src)
        if upload:
            dev.copy_(pin, non_blocking=True)


class PoseStream:
    """One streaming session over an entry-token bank, its step captured as one HIP graph (the module docstring has the sequence).

    model: a BoxDreamer in eval mode with a BETR decoder, its precision self-check settled (one forward, or mark_calibrated()).
    bank: a cache.RefFeatureBank(model.rgb_encoder, decoder=model.decoder).  ref_rows: host ints (B, T - 1), each tracked object's
    references by bank row (samples may share rows).  bbox_3d: (B, 8, 3), constant for the session.  frame_shape: (H, W) of the
    uint8 frames; n_frames: frames per step.  padding: square_bbox's.  crop_dtype: dtype of the encoder's input crops.
    use_keep_boxes: take per-sample object boxes for background masking (bd_crop_resize_frames' keep_boxes).

    After a step, `heat`, `corners_px`, `poses`, `rms_px`, `windows`, `K_crop` and `rows` are the static device tensors of that step
    (the next step overwrites them).

    select_k (None: the fixed references above, today's session launch for launch and buffer for buffer): `ref_rows` is then a list
    of B lists of bank rows, each object's DATABASE -- lengths may differ, at most 1024, objects may share rows -- and every step
    decodes against the select_k <= min(length) views bd_stream_select_rows chooses (T = select_k + 1).  select: "dino" (by
    appearance; the bank keeps match summaries: match_threshold=0.05) or "track" (by distance to the last frame's pose while its
    ok == 1 and its rms_px <= max_rms_px, by appearance otherwise; the bank also keeps poses: keep_poses=True).  After a step `sel`
    (B, select_k) database slots, ascending, `used` (B,) 1 = the pose rule chose, `scores` (B, N_max) and `dist` (B, N_max; None with
    "dino") are that step's device tensors as well; `ref_rows_of(sel)` names the bank rows.  With "track" a step depends on the
    previous step's result rows (`rows`): the first step after construction and after `reset()` re-localises by appearance.

    track_boxes (False: bd_stream_windows on the boxes given, today's session): the first node is bd_stream_track_windows (the module
    docstring has the rule); min_side_px, max_side_px (None: 4 x max(H, W)) bound the usable tracked box, max_rms_px the trusted pose
    (shared with select="track": both kernels decide alike from the same row).  The tail `track` (B, 5) = x0 y0 x1 y1 src per object
    follows `rows` in the step's one D2H, into `track_host` (_layout).  After a step `state_box` (B, 4) and `box_src` (B,) are that
    step's device tensors too; with use_keep_boxes the kernel writes `keep_boxes` (the box truncated towards zero, not squared).  Such
    a session also depends on the previous step's result rows.

    frame_format ("rgb": packed RGB frames and bd_crop_resize_frames, today's session launch for launch and buffer for buffer): the
    layout the frames arrive in -- "bgr" (n_frames, H, W, 3), "rgba" / "bgra" (n_frames, H, W, 4), "nv12" (n_frames, H + H / 2, W) with
    even H and W, converted with colorspace ("bt601" / "bt709") and range ("limited" / "full"; None: "bt601", "limited"; they are
    refused for another format).  The static frame buffer takes that shape and the captured crop node is bd_crop_resize_frames_fmt,
    which converts the pixels under the crops as it stages them: every output equals, bit for bit, a default session's on
    preprocess.frames_to_rgb(frames, ...).  It combines freely with select_k, track_boxes and use_keep_boxes: none of them looks at
    pixels."""

    def __init__(self, model, bank, ref_rows, bbox_3d, frame_shape, n_frames: int = 1, padding: float = 0.1,
                 crop_dtype: torch.dtype = torch.float32, use_keep_boxes: bool = False, capture_error_mode: str = "global",
                 select_k=None, select: str = "dino", max_rms_px: float = float("inf"), track_boxes: bool = False,
                 min_side_px: float = 8.0, max_side_px=None, frame_format="rgb", colorspace=None, range=None):
        p = _plan(model, bank, ref_rows, bbox_3d, frame_shape, n_frames, padding, crop_dtype, use_keep_boxes, select_k, select, max_rms_px,
                  track_boxes, min_side_px, max_side_px, frame_format, colorspace, range)
        _lib.require_gpu()
        self.model, self.encoder, self.decoder = model, model.rgb_encoder, model.decoder
        if self.decoder._signature() != model._calibrated_for and calibrate.applicable(self.encoder, self.decoder):
            raise RuntimeError("the model's precision self-check has not run for these decoder weights, and it cannot run inside a graph "
                               "capture: run one forward (or model.calibrate(data)) first, or call model.mark_calibrated() to keep the "
                               "promotion state that is in place")
        self.B, self.T, self.H, self.W, self.n_frames = p.B, p.T, p.H, p.W, p.n_frames
        self.padding, self.out_size, self.use_keep_boxes = p.padding, int(self.decoder.img_size), p.use_keep_boxes
        self.select_k, self.select, self.max_rms_px = p.select_k, p.select, p.max_rms_px
        self.track_boxes, self.min_side_px, self.max_side_px = p.track_boxes, p.min_side_px, p.max_side_px
        self.frame_format = p.frame_format
        self._make_stores(bank, p.rows, p.n_refs, p.n_max)
        self._make_buffers(bbox_3d, p.crop_dtype)
        self._capture(capture_error_mode)

    def _make_stores(self, bank, rows, n_refs, n_max) -> None:
        """The referenced entry rows -- with select_k the distinct database rows, and their match summaries and poses -- are COPIED into
        a private store: afterwards the bank may grow, be cleared or be refreshed without affecting the session.  The source table:
        sample b's references, then -(b + 1): its query, in the last slot."""
        B, T, k = self.B, self.T, self.select_k
        bank.ensure_fresh()
        dev = bank.entry_tokens.device
        distinct = sorted({r for row in rows for r in row})
        place = {r: i for i, r in enumerate(distinct)}
        take = torch.tensor(distinct, dtype=torch.int64).to(dev)
        self._entry = bank.entry_tokens.index_select(0, take).contiguous()
        self.sel = self.used = self.scores = self.dist = self.force = None
        src = [x for b, row in enumerate(rows) for x in [place[r] for r in row[:k]] + [-(b + 1)]]      # (a database: its first k views)
        self._src = torch.tensor(src, dtype=torch.int32).to(dev)
        if k is not None:
            # the database in private row space: one `place` map serves the entry tokens, the match summaries and the poses
            self._database = rows
            self._msums, self._mcounts = bank._msums.index_select(0, take).contiguous(), bank._mcounts.index_select(0, take).contiguous()
            self._poses = bank.poses.index_select(0, take).contiguous() if self.select == "track" else None
            self._match = (float(bank.match_threshold), int(bank.tokens_per_view))
            self._db_rows = torch.tensor([[place[r] for r in row] + [-1] * (n_max - len(row)) for row in rows], dtype=torch.int32).to(dev)
            self._n_refs = torch.tensor(n_refs, dtype=torch.int32).to(dev)
            self._q_sums = torch.zeros((B, int(bank.feature_dim)), dtype=torch.float32, device=dev)
            self._q_counts = torch.zeros((B,), dtype=torch.float32, device=dev)
            self.scores = torch.zeros((B, n_max), dtype=torch.float32, device=dev)
            self.dist = torch.zeros((B, n_max), dtype=torch.float32, device=dev) if self.select == "track" else None
            self.used = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.sel = torch.zeros((B, k), dtype=torch.int32, device=dev)
        self._mask = torch.zeros((B, T), dtype=torch.bool, device=dev)
        self._mask[:, T - 1] = True

    def _make_buffers(self, bbox_3d, crop_dtype) -> None:
        """The static device buffers of a step and the pinned twins of those the host fills (_layout has the two flat ones)."""
        B, S, H, W, dev = self.B, self.out_size, self.H, self.W, self._entry.device
        ins, outs = _layout(B, self.track_boxes)
        self.frames = torch.zeros(frame_shape_of(self.frame_format, self.n_frames, H, W), dtype=torch.uint8, device=dev)
        (self._in_f, self._in), (self._pin_f, self._pin) = _cut(ins, device=dev), _cut(ins, pin_memory=True)
        (self._out, out), (self._out_host, host) = _cut(outs, device=dev), _cut(outs, pin_memory=True)
        self.det_boxes, self.K, self.det_valid = self._in["det_boxes"], self._in["K"], self._in.get("det_valid")
        self.rows, self.track, self.rows_host, self.track_host = out["rows"], out.get("track"), host["rows"], host.get("track")
        self.K.copy_(torch.eye(3, device=dev).expand(B, 3, 3))
        self._default_box = torch.tensor([0.0, 0.0, float(min(H, W)), float(min(H, W))], device=dev).expand(B, 4)
        self.det_boxes.copy_(self._default_box)
        self.frame_idx = (torch.arange(B, dtype=torch.int32) % self.n_frames).to(dev)
        self.keep_boxes = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32).repeat(B, 1).to(dev) if self.use_keep_boxes else None
        self._pin_idx = torch.zeros((B,), dtype=torch.int32).pin_memory()
        self._pin_keep = torch.zeros((B, 4), dtype=torch.int32).pin_memory()
        self.state_box = self.box_src = None
        if self.track_boxes:
            self.state_box = torch.zeros((B, 4), dtype=torch.float32, device=dev)
            self.box_src = torch.zeros((B,), dtype=torch.int32, device=dev)
        if self.select_k is not None or self.track_boxes:   # what a step carries from frame to frame is distrusted per object through `force`
            self.force = torch.zeros((B,), dtype=torch.int32, device=dev)
            self._pin_force = torch.zeros((B,), dtype=torch.int32).pin_memory()
            self._pin_reset, self._reset_done, self._forced = None, None, False
        self.bbox_3d = bbox_3d.detach().to(dev).float().contiguous().clone()
        self.windows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.K_crop = torch.zeros((B, 3, 3), dtype=torch.float32, device=dev)
        self.crops = torch.zeros((B, 3, S, S), dtype=crop_dtype, device=dev)
        self._done = torch.cuda.Event()
        self._pending = False
        self.replays = 0
        what = "result rows and box tail" if self.track_boxes else "result rows"
        self.host_syncs_per_step = [f"{what}: ONE D2H of {self._out.numel() * 4} bytes into a pinned buffer, one wait for its event"]

    def _capture(self, mode: str) -> None:
        """Warm up and capture the step (graph.capture), then put back what the warm-up's runs left in the carried state."""
        mask_error = self.decoder.mask_error
        self.graph, (self.heat, self.corners_px, self.poses, self.rms_px) = graph.capture(self, self._run, self.encoder, self.decoder, self.frames.device, mode)
        self.decoder.mask_error = mask_error            # (the warm-up's verdict on the session's own mask is nobody's business)
        if self.force is not None:      # (the warm-up left its own result rows: the first step re-localises by appearance)
            self.rows.zero_()
        if self.track_boxes:            # ... and its own box: the first step holds the whole-frame default unless a detection is offered
            self.state_box.copy_(self._default_box)
            self.box_src.zero_()
            self.track.zero_()
            self.track[:, :4].copy_(self.state_box)

    def _run(self):
        S = self.out_size
        if self.track_boxes:
            # the same first node, fed from the last step's result rows (read here, overwritten by bd_stream_results below)
            hip_ops.stream_track_windows(self.rows, self.bbox_3d, self.K, self.det_boxes, self.det_valid, self.force, self.state_box,
                                         self.padding, S, (self.H, self.W), self.max_rms_px, self.min_side_px, self.max_side_px,
                                         windows=self.windows, K_crop=self.K_crop, box_src=self.box_src, keep_boxes=self.keep_boxes,
                                         track=self.track)
        else:
            hip_ops.stream_windows(self.det_boxes, self.K, self.padding, S, self.windows, self.K_crop)
        crop_resize_frames(self.frames, self.windows, frame_idx=self.frame_idx, keep_boxes=self.keep_boxes, out_size=S, out=self.crops,
                           frame_format=self.frame_format)
        fresh = self.encoder.predict(self.crops)
        if self.select_k is not None:
            # which k database views the decoder reads this frame: the query's summary, then ONE launch that reads the last step's
            # result rows and writes the source table forward_entry reads from device memory
            (threshold, L), R = self._match, self._entry.shape[0]
            hip_ops.match_view_sums(fresh, self.crops, threshold, self._q_sums, self._q_counts)
            hip_ops.stream_select_rows(self._msums, self._mcounts, self._poses, R, self._q_sums, self._q_counts, self.rows, self._db_rows,
                                       self._n_refs, self.force, L, self.select_k, SELECT_RULES[self.select], self.max_rms_px,
                                       scores=self.scores, dist=self.dist, used=self.used, sel=self.sel, src=self._src)
        heat = self.decoder.forward_entry(self._entry, self._entry.shape[0], self._src, fresh, self._mask, S)
        kp_px = hip_ops.decode_topk(heat, want_idx=False)[0]
        poses, rms_px = solve_poses_device(kp_px, self.bbox_3d, self.K_crop, form="wave", want_rms=True)
        hip_ops.stream_results(poses, rms_px, kp_px, self.windows, self.K, self.bbox_3d, S, self.rows)
        return heat, kp_px, poses, rms_px

    # -- per-step input checks (host values only: nothing here reads the device)
    def _check_frames(self, frames):
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f"frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames).__name__)}")
        if frames.dim() == self.frames.dim() - 1 and self.n_frames == 1:
            frames = frames[None]
        if tuple(frames.shape) != tuple(self.frames.shape):
            raise ValueError(f"frames must be {tuple(self.frames.shape)} (the session's frame shape is fixed; its frame_format is "
                             f"{self.frame_format.name!r}), got {tuple(frames.shape)}")
        return frames

    def _check(self, t, shape, floating: bool, name: str):
        if not isinstance(t, torch.Tensor) or t.dtype.is_floating_point != floating or t.dtype == torch.bool:
            raise ValueError(f"{name} must be {'a float' if floating else 'an integer'} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {tuple(shape)} for this session of B = {self.B}, got {tuple(t.shape)}")
        return t

    def step(self, frames, det_boxes, K, frame_idx=None, keep_boxes=None, wait: bool = True, relocalise=None, det_valid=None) -> torch.Tensor:
        """One frame: frames uint8 (n_frames, H, W, 3) (or (H, W, 3) when n_frames == 1; with a frame_format, that format's shape,
        e.g. (n_frames, H * 3 / 2, W) or (H * 3 / 2, W) for "nv12"; a pinned host tensor is copied
        asynchronously, a device tensor on the device), det_boxes float (B, 4) x0 y0 x1 y1, K float (B, 3, 3) full-frame intrinsics
        (host or device), frame_idx integers (B,): the frame each sample reads (None: as in the last step; initially b % n_frames),
        keep_boxes integers (B, 4) when the session was built with use_keep_boxes (None: as in the last step; initially the whole
        frame), relocalise integers or bools (B,) for a session built with select_k: nonzero = choose this object's references by
        appearance on THIS step, whatever its last pose (None: nobody).  With track_boxes: det_boxes may be None (nobody has a
        detection); det_valid integers or bools (B,), nonzero = det_boxes[b] is a detection (None: all ones when det_boxes is given,
        all zeros otherwise); relocalise also means "distrust this object's last pose for its BOX on this step"; keep_boxes is refused
        (the kernel writes them).  After the step `track_host` (B, 5) holds x0 y0 x1 y1 of the box each object used and its source
        (BOX_DETECTOR / BOX_TRACKED / BOX_HELD), copied with the rows.  Returns the pinned (B, 66) fp32 rows (the layout: include/boxdreamer_hip.h, bd_stream_results; ROW_* here) --
        valid once the copy's event has completed: wait=True (the default) waits for it, wait=False leaves that to `wait()`."""
        B = self.B
        det_valid = _step_boxes(self.track_boxes, det_boxes, det_valid, keep_boxes, B)
        frames = self._check_frames(frames)
        if det_boxes is not None:
            self._check(det_boxes, (B, 4), True, "det_boxes")
        self._check(K, (B, 3, 3), True, "K")
        if frame_idx is not None:
            self._check(frame_idx, (B,), False, "frame_idx")
        if keep_boxes is not None:
            if not self.use_keep_boxes:
                raise ValueError("keep_boxes given to a session built with use_keep_boxes=False")
            self._check(keep_boxes, (B, 4), False, "keep_boxes")
        if relocalise is not None:
            if self.select_k is None and not self.track_boxes:
                raise ValueError("relocalise given to a session built without select_k: its references are fixed")
            relocalise = _relocalise(relocalise, B)
        self.wait()                     # (an un-waited step: its copies still read the pinned staging buffers)
        self.frames.copy_(frames, non_blocking=True)
        on_device = K.is_cuda or (det_boxes is not None and det_boxes.is_cuda) or (det_valid is not None and det_valid.is_cuda)
        # all on the host: every field into the pinned twin (upload=False), then ONE H2D of the whole input buffer.  Any of them on the
        # device: `pin` is empty, so _put() gets pin=None and copies each straight into its device field, a host tensor among them too
        pin = {} if on_device else self._pin
        flags = None if det_valid is None else det_valid != 0
        for name, src in (("det_boxes", det_boxes), ("K", K), ("det_valid", flags)):
            if src is not None:
                _put(self._in[name], pin.get(name), src, upload=False)
        if self.track_boxes and flags is None:
            (self._in if on_device else self._pin)["det_valid"].fill_(0 if det_boxes is None else 1)
        if not on_device:
            self._in_f.copy_(self._pin_f, non_blocking=True)
        if frame_idx is not None:
            _put(self.frame_idx, self._pin_idx, frame_idx)
        if keep_boxes is not None:
            _put(self.keep_boxes, self._pin_keep, keep_boxes)
        if relocalise is not None:
            _put(self.force, self._pin_force, relocalise != 0)
            self._forced = True
        elif self.force is not None and self._forced:           # (the flags hold for one step)
            self.force.zero_()
            self._forced = False
        self.graph.replay()
        self._out_host.copy_(self._out, non_blocking=True)
        self._done.record()
        self._pending = True
        self.replays += 1
        if wait:
            self.wait()
        return self.rows_host

    def wait(self) -> torch.Tensor:
        """Wait for the last step's D2H (its event, not the stream); returns the pinned rows."""
        if self._pending:
            self._done.synchronize()
            self._pending = False
        return self.rows_host

    # -- a session that carries its last poses from frame to frame (select_k, track_boxes)
    def reset(self, poses=None) -> None:
        """Forget the last poses (enqueued on the current stream, nothing waits).  None: the result rows become zero, so the next step
        re-localises by appearance.  poses float (B, 4, 4), host or device: they become the last poses with ok = 1 and rms_px = 0 -- a
        session resumed from a known pose, whose next "track" step ranks by distance to them.  With track_boxes: after reset() the
        next step takes a detection or holds the last box (`state_box` is left alone); after reset(poses) its box is bbox_3d projected
        with those poses and that step's K."""
        if self.select_k is None and not self.track_boxes:
            raise ValueError("reset() on a session built without select_k: nothing is carried from frame to frame there")
        if poses is None:
            self.rows.zero_()
            return
        self._check(poses, (self.B, 4, 4), True, "poses")
        host = not poses.is_cuda
        if host and self._pin_reset is None:
            self._pin_reset, self._reset_done = torch.zeros_like(self.rows_host).pin_memory(), torch.cuda.Event()
        elif host:
            self._reset_done.synchronize()          # (the last reset's copy still reads the staging buffer)
        rows = self._pin_reset if host else self.rows           # filled in place: the pinned staging buffer, or the device rows themselves
        rows.zero_()
        rows[:, ROW_POSE].copy_(poses.reshape(self.B, 16), non_blocking=True)
        rows[:, ROW_OK].fill_(1.0)
        if host:
            self.rows.copy_(rows, non_blocking=True)
            self._reset_done.record()

    def ref_rows_of(self, sel) -> list:
        """Database slots (B, k) -- `sel`, read back -- -> the bank rows they name, B lists; -1 stays -1."""
        if self.select_k is None:
            raise ValueError("ref_rows_of() on a session built without select_k: its references are ref_rows")
        slots = torch.as_tensor(sel).cpu().tolist()
        if len(slots) != self.B:
            raise ValueError(f"sel must have one row per tracked object (B = {self.B}), got {len(slots)}")
        return [[self._database[b][int(i)] if int(i) >= 0 else -1 for i in row] for b, row in enumerate(slots)]
