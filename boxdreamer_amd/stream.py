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

`step()` copies the frame, the detector boxes and K into static buffers, replays the graph, enqueues ONE D2H of the result rows into
a pinned buffer and waits for that copy's event.  Nothing is carried from frame to frame.

Limits: an entry-token bank only; the same T for every sample; a fixed frame shape and frame count; the encoder and the decoder are
frozen while the session lives (a larger eager batch, .to() or a checkpoint load raises; `del` the session first).
"""
from __future__ import annotations

import torch

from . import _lib, calibrate, hip_ops
from .betr import BETR
from .box_utils import solve_poses_device
from .preprocess import crop_resize_frames

ROW_POSE, ROW_RMS, ROW_OK = slice(0, 16), 16, 17
ROW_CORNERS_CROP, ROW_CORNERS_FRAME, ROW_BOX_FRAME = slice(18, 34), slice(34, 50), slice(50, 66)


def _ref_rows(ref_rows, bank_len: int):
    """`ref_rows` (host ints (B, T - 1): a nested list or a CPU int tensor) -> (B lists of T - 1 bank rows, B, T), validated."""
    if isinstance(ref_rows, torch.Tensor):
        if ref_rows.dim() != 2:
            raise ValueError(f"ref_rows must be (B, T - 1) host integers, got shape {tuple(ref_rows.shape)}")
        B, R = int(ref_rows.shape[0]), int(ref_rows.shape[1])
    else:
        try:
            ref_rows = [list(r) for r in ref_rows]
        except TypeError:
            raise ValueError("ref_rows must be (B, T - 1) host integers: one list of bank rows per tracked object") from None
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


class PoseStream:
    """One streaming session over an entry-token bank, its step captured as one HIP graph (the module docstring has the sequence).

    model: a BoxDreamer in eval mode with a BETR decoder, its precision self-check settled (one forward, or mark_calibrated()).
    bank: a cache.RefFeatureBank(model.rgb_encoder, decoder=model.decoder).  ref_rows: host ints (B, T - 1), each tracked object's
    references by bank row (samples may share rows).  bbox_3d: (B, 8, 3), constant for the session.  frame_shape: (H, W) of the
    uint8 frames; n_frames: frames per step.  padding: square_bbox's.  crop_dtype: dtype of the encoder's input crops.
    use_keep_boxes: take per-sample object boxes for background masking (bd_crop_resize_frames' keep_boxes).

    The referenced entry rows are COPIED into a private store at construction: afterwards the bank may grow, be cleared or be
    refreshed without affecting the session.  After a step, `heat`, `corners_px`, `poses`, `rms_px`, `windows`, `K_crop` and `rows`
    are the static device tensors of that step (the next step overwrites them)."""

    def __init__(self, model, bank, ref_rows, bbox_3d, frame_shape, n_frames: int = 1, padding: float = 0.1,
                 crop_dtype: torch.dtype = torch.float32, use_keep_boxes: bool = False, capture_error_mode: str = "global"):
        # ---- host-side refusals, before a device is needed
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
        rows, B, T = _ref_rows(ref_rows, len(bank))
        if not isinstance(bbox_3d, torch.Tensor) or tuple(bbox_3d.shape) != (B, 8, 3):
            raise ValueError(f"bbox_3d must be a tensor of shape {(B, 8, 3)}, got {tuple(getattr(bbox_3d, 'shape', ()))}")
        H, W = (int(x) for x in frame_shape)
        n_frames = int(n_frames)
        if H < 1 or W < 1 or n_frames < 1:
            raise ValueError(f"frame_shape = {(H, W)} and n_frames = {n_frames} must be positive")
        if crop_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"crop_dtype must be float32, float16 or bfloat16, got {crop_dtype}")
        _lib.require_gpu()
        if decoder._signature() != model._calibrated_for and calibrate.applicable(encoder, decoder):
            raise RuntimeError("the model's precision self-check has not run for these decoder weights, and it cannot run inside a graph "
                               "capture: run one forward (or model.calibrate(data)) first, or call model.mark_calibrated() to keep the "
                               "promotion state that is in place")
        self.model, self.encoder, self.decoder = model, encoder, decoder
        self.B, self.T, self.H, self.W, self.n_frames = B, T, H, W, n_frames
        self.padding, self.out_size, self.use_keep_boxes = float(padding), int(decoder.img_size), bool(use_keep_boxes)

        # ---- the private entry store and its source table: sample b's references, then -(b + 1): its query, in the last slot
        bank.ensure_fresh()
        store = bank.entry_tokens
        dev = store.device
        distinct = sorted({r for row in rows for r in row})
        place = {r: i for i, r in enumerate(distinct)}
        self._entry = store.index_select(0, torch.tensor(distinct, dtype=torch.int64).to(dev)).contiguous()
        src = [x for b, row in enumerate(rows) for x in [place[r] for r in row] + [-(b + 1)]]
        self._src = torch.tensor(src, dtype=torch.int32).to(dev)
        self._mask = torch.zeros((B, T), dtype=torch.bool, device=dev)
        self._mask[:, T - 1] = True

        # ---- static buffers
        S = self.out_size
        self.frames = torch.zeros((n_frames, H, W, 3), dtype=torch.uint8, device=dev)
        self._in_f = torch.zeros((B * 13,), dtype=torch.float32, device=dev)           # det_boxes, then K: one H2D per step
        self.det_boxes, self.K = self._in_f[:B * 4].view(B, 4), self._in_f[B * 4:].view(B, 3, 3)
        self.K.copy_(torch.eye(3, device=dev).expand(B, 3, 3))
        self.det_boxes.copy_(torch.tensor([0.0, 0.0, float(min(H, W)), float(min(H, W))], device=dev).expand(B, 4))
        self.frame_idx = (torch.arange(B, dtype=torch.int32) % n_frames).to(dev)
        self.keep_boxes = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32).repeat(B, 1).to(dev) if self.use_keep_boxes else None
        self.bbox_3d = bbox_3d.detach().to(dev).float().contiguous().clone()
        self.windows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.K_crop = torch.zeros((B, 3, 3), dtype=torch.float32, device=dev)
        self.crops = torch.zeros((B, 3, S, S), dtype=crop_dtype, device=dev)
        self.rows = torch.zeros((B, _lib.STREAM_ROW_FLOATS), dtype=torch.float32, device=dev)
        self.rows_host = torch.zeros((B, _lib.STREAM_ROW_FLOATS), dtype=torch.float32).pin_memory()
        # pinned staging of the small host inputs (a copy from pageable memory would wait for the stream)
        self._pin_f = torch.zeros((B * 13,), dtype=torch.float32).pin_memory()
        self._pin_idx = torch.zeros((B,), dtype=torch.int32).pin_memory()
        self._pin_keep = torch.zeros((B, 4), dtype=torch.int32).pin_memory()
        self._done = torch.cuda.Event()
        self._pending = False
        self.replays = 0
        self.host_syncs_per_step = [f"result rows: ONE D2H of {B * _lib.STREAM_ROW_FLOATS * 4} bytes into a pinned buffer, one wait for its event"]

        # ---- warm up on a side stream (workspaces, packed weights: allocated outside the capture), then capture -- as graph.GraphedPath
        with torch.cuda.device(dev):
            _lib.check(_lib.load().bd_lanes_prepare(), "bd_lanes_prepare")
        mask_error = decoder.mask_error
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._run()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        decoder.mask_error = mask_error                 # (the warm-up's verdict on the session's own mask is nobody's business)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode=capture_error_mode):
            self.heat, self.corners_px, self.poses, self.rms_px = self._run()
        # the captured launches hold raw pointers into the modules' workspaces and packed weights: keep those alive and freeze the
        # modules, as graph.GraphedPath does; deleting the session lifts the freeze
        enc_model = getattr(encoder, "model", encoder)
        self._pinned = [enc_model._ws, decoder._ws, list(enc_model._packed.values()), list(decoder._packed.values())]
        enc_model._frozen_by.add(self)
        decoder._frozen_by.add(self)

    def _run(self):
        S = self.out_size
        hip_ops.stream_windows(self.det_boxes, self.K, self.padding, S, self.windows, self.K_crop)
        crop_resize_frames(self.frames, self.windows, frame_idx=self.frame_idx, keep_boxes=self.keep_boxes, out_size=S, out=self.crops)
        fresh = self.encoder.predict(self.crops)
        heat = self.decoder.forward_entry(self._entry, self._entry.shape[0], self._src, fresh, self._mask, S)
        kp_px = hip_ops.decode_topk(heat, want_idx=False)[0]
        poses, rms_px = solve_poses_device(kp_px, self.bbox_3d, self.K_crop, form="wave", want_rms=True)
        hip_ops.stream_results(poses, rms_px, kp_px, self.windows, self.K, self.bbox_3d, S, self.rows)
        return heat, kp_px, poses, rms_px

    # -- per-step input checks (host values only: nothing here reads the device)
    def _check_frames(self, frames):
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f"frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames).__name__)}")
        if frames.dim() == 3 and self.n_frames == 1:
            frames = frames[None]
        if tuple(frames.shape) != tuple(self.frames.shape):
            raise ValueError(f"frames must be {tuple(self.frames.shape)} (the session's frame shape is fixed), got {tuple(frames.shape)}")
        return frames

    def _check(self, t, shape, floating: bool, name: str):
        if not isinstance(t, torch.Tensor) or t.dtype.is_floating_point != floating or t.dtype == torch.bool:
            raise ValueError(f"{name} must be {'a float' if floating else 'an integer'} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {tuple(shape)} for this session of B = {self.B}, got {tuple(t.shape)}")
        return t

    def step(self, frames, det_boxes, K, frame_idx=None, keep_boxes=None, wait: bool = True) -> torch.Tensor:
        """One frame: frames uint8 (n_frames, H, W, 3) (or (H, W, 3) when n_frames == 1; a pinned host tensor is copied
        asynchronously, a device tensor on the device), det_boxes float (B, 4) x0 y0 x1 y1, K float (B, 3, 3) full-frame intrinsics
        (host or device), frame_idx integers (B,): the frame each sample reads (None: as in the last step; initially b % n_frames),
        keep_boxes integers (B, 4) when the session was built with use_keep_boxes (None: as in the last step; initially the whole
        frame).  Returns the pinned (B, 66) fp32 rows (the layout: include/boxdreamer_hip.h, bd_stream_results; ROW_* here) --
        valid once the copy's event has completed: wait=True (the default) waits for it, wait=False leaves that to `wait()`."""
        B = self.B
        frames = self._check_frames(frames)
        self._check(det_boxes, (B, 4), True, "det_boxes")
        self._check(K, (B, 3, 3), True, "K")
        if frame_idx is not None:
            self._check(frame_idx, (B,), False, "frame_idx")
        if keep_boxes is not None:
            if not self.use_keep_boxes:
                raise ValueError("keep_boxes given to a session built with use_keep_boxes=False")
            self._check(keep_boxes, (B, 4), False, "keep_boxes")
        if self._pending:               # (an un-waited step: its copies still read the pinned staging buffers)
            self._done.synchronize()
            self._pending = False
        self.frames.copy_(frames, non_blocking=True)
        if det_boxes.is_cuda or K.is_cuda:
            self.det_boxes.copy_(det_boxes, non_blocking=True)
            self.K.copy_(K, non_blocking=True)
        else:
            self._pin_f[:B * 4].view(B, 4).copy_(det_boxes)
            self._pin_f[B * 4:].view(B, 3, 3).copy_(K)
            self._in_f.copy_(self._pin_f, non_blocking=True)
        for given, pin, static in ((frame_idx, self._pin_idx, self.frame_idx), (keep_boxes, self._pin_keep, self.keep_boxes)):
            if given is None:
                continue
            if given.is_cuda:
                static.copy_(given, non_blocking=True)
            else:
                pin.copy_(given)
                static.copy_(pin, non_blocking=True)
        self.graph.replay()
        self.rows_host.copy_(self.rows, non_blocking=True)
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
