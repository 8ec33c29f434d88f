"""Raw frames in, encoder input out: the dataset's per-view host work (PIL crop with black padding, ToTensor, antialiased
Resize -- /root/reference/src/datasets/utils/preprocess.py:123-199 `pad_and_resize_image`, :202-274 `_crop_image`, called from
src/datasets/base.py:541-566) as ONE launch of `bd_crop_resize_frames` (csrc/preprocess.hip) on uint8 device frames.

    boxes = square_bbox(det_boxes_xyxy)                      # torch, on the device: int32 [m, 4], the reference's truncation
    images = crop_resize_frames(frames_u8, boxes)            # [m, 3, 224, 224], what the reference's dataset would have produced
    K_crop = crop_intrinsics(K, boxes, 224)                  # adjust_intrinsic_matrix (:277-300)

`FramePreprocessor` keeps the buffers of a fixed (m, out_size, dtype) so that a streaming caller allocates nothing per frame.
`BoxDreamer.forward` takes `data["frames"]` + `data["crop_boxes"]` in place of `data["images"]` (boxdreamer_amd/model.py).
There is no CPU fallback: the resize is the HIP kernel or an error.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def square_bbox(bbox, padding: float = 0.1):
    """preprocess.py:22-45.  A numpy / list box [x0, y0, x1, y1] returns the reference's float64 square box (centre +- the larger
    half-extent x (1 + padding)).  A torch tensor [..., 4] (any device) returns the INTEGER crop windows int32 [..., 4] that
    `_crop_image` would cut for those square boxes (`integer_box`): the batched form a detector's float boxes go through without
    visiting the host."""
    if isinstance(bbox, torch.Tensor):
        b = bbox.to(torch.float64)
        center = (b[..., :2] + b[..., 2:]) / 2
        extents = (b[..., 2:] - b[..., :2]) / 2
        size = extents.amax(dim=-1, keepdim=True) * (1 + padding)
        return integer_box(torch.cat([center - size, center + size], dim=-1))
    b = np.asarray(bbox, dtype=np.float64)
    center = (b[:2] + b[2:]) / 2
    extents = (b[2:] - b[:2]) / 2
    size = max(extents) * (1 + padding)
    return np.array([center[0] - size, center[1] - size, center[0] + size, center[1] + size], dtype=np.float64)


def integer_box(bbox):
    """The window `_crop_image` cuts for a float box (preprocess.py:253-259): left = int(x0), top = int(y0), width = int(x1 - x0),
    height = int(y1 - y0), every int() towards zero -> [left, top, left + width, top + height].  numpy in, int64 numpy out; torch in
    (fp64 arithmetic on its device), int32 torch out."""
    if isinstance(bbox, torch.Tensor):
        b = bbox.to(torch.float64)
        lt = b[..., :2].trunc()
        wh = (b[..., 2:] - b[..., :2]).trunc()
        return torch.cat([lt, lt + wh], dim=-1).to(torch.int32)
    b = np.asarray(bbox, dtype=np.float64)
    lt = np.trunc(b[..., :2])
    wh = np.trunc(b[..., 2:] - b[..., :2])
    return np.concatenate([lt, lt + wh], axis=-1).astype(np.int64)


def crop_intrinsics(K, boxes, out_size: int):
    """Intrinsics of the resized crop: `adjust_intrinsic_matrix` (preprocess.py:277-300) with scale = out_size / side and
    crop_offset = (x0, y0).  K [..., 3, 3], boxes integer [..., 4] (same leading shape); fp64 inside, returns K's dtype (fp64 for
    integer input) on K's device."""
    if isinstance(K, torch.Tensor):
        k = K.to(torch.float64).clone()
        b = torch.as_tensor(boxes, device=K.device).to(torch.float64)
        sx = float(out_size) / (b[..., 2] - b[..., 0])
        sy = float(out_size) / (b[..., 3] - b[..., 1])
        k[..., 0, 0] = k[..., 0, 0] * sx
        k[..., 1, 1] = k[..., 1, 1] * sy
        k[..., 0, 2] = k[..., 0, 2] * sx - b[..., 0] * sx
        k[..., 1, 2] = k[..., 1, 2] * sy - b[..., 1] * sy
        return k.to(K.dtype if K.dtype.is_floating_point else torch.float64)
    k = np.array(K, dtype=np.float64)
    b = np.asarray(boxes, dtype=np.float64)
    sx = float(out_size) / (b[..., 2] - b[..., 0])
    sy = float(out_size) / (b[..., 3] - b[..., 1])
    k[..., 0, 0] *= sx
    k[..., 1, 1] *= sy
    k[..., 0, 2] = k[..., 0, 2] * sx - b[..., 0] * sx
    k[..., 1, 2] = k[..., 1, 2] * sy - b[..., 1] * sy
    return k


def _int32_rows(t, name: str, m: int | None):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name} must be an int32 tensor (got {getattr(t, 'dtype', type(t))})")
    t = t.reshape(-1, 4) if name != "frame_idx" else t.reshape(-1)
    if m is not None and t.shape[0] != m:
        raise ValueError(f"{name} has {t.shape[0]} rows for {m} crops")
    return t.contiguous()


def crop_resize_frames(frames: torch.Tensor, boxes: torch.Tensor, *, frame_idx: torch.Tensor | None = None,
                       keep_boxes: torch.Tensor | None = None, out_size: int = 224, out: torch.Tensor | None = None,
                       dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """`bd_crop_resize_frames` on the current stream.  frames: uint8 device [n, H, W, 3] (HWC RGB; the pixel must be 3 contiguous
    bytes, rows and frames may be strided: a slice of a larger tensor is read in place).  boxes: int32 device [m, 4] (or [B, T, 4])
    square windows x0 y0 x1 y1; frame_idx int32 [m] (default: crop i reads frame i); keep_boxes int32 [m, 4]: pixels outside it are 0,
    edges inclusive (the reference's `bbox_obj`).  Returns [m, 3, S, S] (or boxes' leading shape) in `dtype`, or writes `out`
    ([m, 3, S, S] / [B, T, 3, S, S], contiguous; its dtype wins).  A degenerate box gives zeros (include/boxdreamer_hip.h).
    No allocation when `out` is given, no synchronisation."""
    lib = _lib.load()
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise TypeError("frames must be a uint8 tensor [n, H, W, 3]")
    if frames.numel() == 0:
        raise ValueError("frames is empty")
    n, H, W, _ = frames.shape
    if frames.stride(3) != 1 or frames.stride(2) != 3:
        raise ValueError("frames needs unit channel stride and 3-byte pixels (HWC); rows and frames may be strided")
    lead = tuple(boxes.shape[:-1]) if isinstance(boxes, torch.Tensor) else None
    b = _int32_rows(boxes, "boxes", None)
    m = b.shape[0]
    fi = _int32_rows(frame_idx, "frame_idx", m)
    kb = _int32_rows(keep_boxes, "keep_boxes", m)
    S = int(out_size)
    if out is None:
        out = torch.empty(lead + (3, S, S), dtype=dtype, device=frames.device)
    else:
        if tuple(out.shape[-3:]) != (3, S, S) or out.numel() != m * 3 * S * S:
            raise ValueError(f"out has shape {tuple(out.shape)}; {m} crops of size {S} need [{m}, 3, {S}, {S}] (or [B, T, 3, {S}, {S}])")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (a slice along the leading dimension is)")
    _lib.same_device(frames, b, fi, kb, out)
    rc = lib.bd_crop_resize_frames(_lib.ptr(frames), n, H, W, frames.stride(1), frames.stride(0), _lib.ptr(b), _lib.ptr(fi), _lib.ptr(kb),
                                   m, S, _lib.ptr(out), _lib.dtype_id(out), _lib.stream())
    _lib.check(rc, "bd_crop_resize_frames")
    return out


class FramePreprocessor:
    """Frames + float boxes -> (images, intrinsics of the crops, integer boxes) for a fixed number of crops `m`.

    Owns the int32 box / frame-index buffers and the output buffer; after the first call nothing is allocated by the launch path
    and nothing waits for the device (`square_bbox` / `crop_intrinsics` are a handful of small torch kernels on the same stream).
    The returned tensors are the object's own buffers: the next call overwrites them."""

    def __init__(self, m: int, out_size: int = 224, dtype: torch.dtype = torch.float32, device="cuda", padding: float = 0.1):
        _lib.require_gpu()
        self.m, self.out_size, self.padding = int(m), int(out_size), float(padding)
        dev = torch.device(device)
        self.boxes = torch.zeros((self.m, 4), dtype=torch.int32, device=dev)
        self.frame_idx = torch.zeros((self.m,), dtype=torch.int32, device=dev)
        self.keep_boxes = torch.zeros((self.m, 4), dtype=torch.int32, device=dev)
        self.images = torch.zeros((self.m, 3, self.out_size, self.out_size), dtype=dtype, device=dev)

    def __call__(self, frames: torch.Tensor, bboxes: torch.Tensor, K: torch.Tensor | None = None, *, frame_idx: torch.Tensor | None = None,
                 keep_boxes: torch.Tensor | None = None, square: bool = True):
        """bboxes: float [m, 4] detector boxes on the device (squared with `padding` unless square=False: then they are taken as the
        square float boxes and only truncated).  K: [m, 3, 3] intrinsics of the frames each crop reads (optional).  frame_idx:
        [m] integers (default: crop i reads frame i).  keep_boxes: float / int [m, 4] object boxes for background masking."""
        if bboxes.shape != (self.m, 4):
            raise ValueError(f"bboxes must be [{self.m}, 4], got {tuple(bboxes.shape)}")
        self.boxes.copy_(square_bbox(bboxes, self.padding) if square else integer_box(bboxes))
        fi = None
        if frame_idx is not None:
            self.frame_idx.copy_(frame_idx)
            fi = self.frame_idx
        kb = None
        if keep_boxes is not None:
            self.keep_boxes.copy_(keep_boxes.to(torch.float64).trunc() if keep_boxes.dtype.is_floating_point else keep_boxes)
            kb = self.keep_boxes
        crop_resize_frames(frames, self.boxes, frame_idx=fi, keep_boxes=kb, out_size=self.out_size, out=self.images)
        K_crop = crop_intrinsics(K, self.boxes, self.out_size) if K is not None else None
        return self.images, K_crop, self.boxes
