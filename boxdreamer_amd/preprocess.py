"""Raw frames in, encoder input out: the dataset's per-view host work (PIL crop with black padding, ToTensor, antialiased
Resize -- /root/reference/src/datasets/utils/preprocess.py:123-199 `pad_and_resize_image`, :202-274 `_crop_image`, called from
src/datasets/base.py:541-566) as ONE launch of `bd_crop_resize_frames` (csrc/preprocess.hip) on uint8 device frames.

    boxes = square_bbox(det_boxes_xyxy)                      # torch, on the device: int32 [m, 4], the reference's truncation
    images = crop_resize_frames(frames_u8, boxes)            # [m, 3, 224, 224], what the reference's dataset would have produced
    K_crop = crop_intrinsics(K, boxes, 224)                  # adjust_intrinsic_matrix (:277-300)

`FramePreprocessor` keeps the buffers of a fixed (m, out_size, dtype) so that a streaming caller allocates nothing per frame.
`BoxDreamer.forward` takes `data["frames"]` + `data["crop_boxes"]` in place of `data["images"]` (boxdreamer_amd/model.py).
There is no CPU fallback: the resize is the HIP kernel or an error.

Frames need not be packed RGB: `frame_format=` "bgr", "rgba", "bgra" or "nv12" (with `colorspace`, `range`) reads what a camera, a
compositor or a video decoder delivers, through `bd_crop_resize_frames_fmt`, which converts the pixels under the crops as it stages
them.  `frames_to_rgb` is the definition of that conversion (numpy or torch); a crop of a frame in any format is, bit for bit, the
crop of `frames_to_rgb(frame, ...)`.
"""
from __future__ import annotations

import math
from collections import namedtuple

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


# ---- pixel formats: the layouts a camera (bgr), a compositor (rgba / bgra) or a video decoder (nv12) delivers
FRAME_FORMATS = {"rgb": _lib.PIXEL_RGB, "bgr": _lib.PIXEL_BGR, "rgba": _lib.PIXEL_RGBA, "bgra": _lib.PIXEL_BGRA, "nv12": _lib.PIXEL_NV12}
COLORSPACES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb)
RANGES = ("limited", "full")
_LAYOUT = {"rgb": "[n, H, W, 3] (HWC, 3-byte pixels)", "bgr": "[n, H, W, 3] (HWC, 3-byte pixels)",
           "rgba": "[n, H, W, 4] (HWC, 4-byte pixels)", "bgra": "[n, H, W, 4] (HWC, 4-byte pixels)",
           "nv12": "[n, H + H / 2, W] (H luma rows, then H / 2 rows of interleaved U, V pairs; H and W even)"}

FrameFormat = namedtuple("FrameFormat", "name id channels colorspace range coef")


def yuv_coefficients(colorspace: str = "bt601", range: str = "limited") -> tuple:
    """(cy, crv, cgu, cgv, cbu, y_off) of the integer NV12 -> RGB rule (include/boxdreamer_hip.h, bd_crop_resize_frames_fmt): each gain
    is floor(x * 65536 + 0.5)."""
    if colorspace not in COLORSPACES:
        raise ValueError(f"unknown colorspace {colorspace!r}: choose from {sorted(COLORSPACES)}")
    if range not in RANGES:
        raise ValueError(f"unknown range {range!r}: choose from {list(RANGES)}")
    kr, kb = COLORSPACES[colorspace]
    kg = 1.0 - kr - kb
    limited = range == "limited"
    s = 255.0 / 224.0 if limited else 1.0
    gains = (255.0 / 219.0 if limited else 1.0, 2.0 * (1.0 - kr) * s, 2.0 * kb * (1.0 - kb) / kg * s, 2.0 * kr * (1.0 - kr) / kg * s,
             2.0 * (1.0 - kb) * s)
    return tuple(int(math.floor(g * 65536.0 + 0.5)) for g in gains) + (16 if limited else 0,)


def resolve_format(name="rgb", colorspace=None, range=None) -> FrameFormat:
    """A pixel format by name -> its record; `name` may also be a dict with the fields frame_format / colorspace / range, or a record.
    colorspace and range belong to "nv12" (None: "bt601", "limited"); naming one for another format is refused."""
    if isinstance(name, FrameFormat):
        return name
    if isinstance(name, dict):
        unknown = sorted(set(name) - {"frame_format", "colorspace", "range"})
        if unknown or "frame_format" not in name:
            raise ValueError(f"frame_format as a dict has the fields frame_format, colorspace, range (got {sorted(name)})")
        return resolve_format(name["frame_format"], name.get("colorspace", colorspace), name.get("range", range))
    if not isinstance(name, str) or name not in FRAME_FORMATS:
        raise ValueError(f"unknown frame_format {name!r}: choose from {sorted(FRAME_FORMATS)}")
    if name != "nv12":
        if colorspace is not None or range is not None:
            raise ValueError(f"colorspace / range describe NV12 frames and frame_format is {name!r}: {name} has no conversion to choose")
        return FrameFormat(name, FRAME_FORMATS[name], 4 if name in ("rgba", "bgra") else 3, None, None, (0,) * 6)
    colorspace, range = colorspace or "bt601", range or "limited"
    return FrameFormat(name, FRAME_FORMATS[name], 1, colorspace, range, yuv_coefficients(colorspace, range))


def frame_shape_of(fmt: FrameFormat, n: int, H: int, W: int) -> tuple:
    """The shape of n frames of H x W pixels in `fmt` (ValueError: NV12 with an odd side)."""
    if fmt.name == "nv12":
        if H % 2 or W % 2:
            raise ValueError(f"nv12 frames need even H and W (one U, V pair per 2 x 2 block), got {(H, W)}")
        return (n, H + H // 2, W)
    return (n, H, W, fmt.channels)


def _frame_geometry(frames, fmt: FrameFormat, what=(np.ndarray, torch.Tensor)):
    """frames in `fmt` -> (n, H, W), after the shape checks that need no device."""
    if not isinstance(frames, what) or frames.dtype not in (torch.uint8, np.uint8):
        raise TypeError(f"{fmt.name} frames must be a uint8 tensor {_LAYOUT[fmt.name]}")
    if fmt.name == "nv12":
        if frames.ndim != 3:
            raise TypeError(f"nv12 frames must be a uint8 tensor {_LAYOUT['nv12']}")
        n, rows, W = (int(v) for v in frames.shape)
        H = rows * 2 // 3
        if rows % 3 or H % 2 or W % 2:
            raise ValueError(f"nv12 frames are {_LAYOUT['nv12']}: {rows} rows x {W} columns are no such frame")
        return n, H, W
    if frames.ndim != 4 or frames.shape[-1] != fmt.channels:
        raise TypeError(f"{fmt.name} frames must be a uint8 tensor {_LAYOUT[fmt.name]}")
    return tuple(int(v) for v in frames.shape[:3])


def frames_to_rgb(frames, frame_format: str = "rgb", colorspace: str = "bt601", range: str = "limited"):
    """Whole frames of any format -> packed RGB uint8 [n, H, W, 3]: the DEFINITION bd_crop_resize_frames_fmt and bd_frames_to_rgb_host
    are tested against.  numpy in, numpy out; a torch tensor (any device) in, a torch tensor out, plain integer tensor ops.  "bgr" /
    "rgba" / "bgra" permute bytes (the fourth is dropped); "nv12" is the int32 rule of include/boxdreamer_hip.h with nearest chroma:
    pixel (x, y) takes pair (x >> 1, y >> 1).  colorspace / range are read for "nv12" only."""
    fmt = _named_format(frame_format, colorspace, range)
    n, H, W = _frame_geometry(frames, fmt)
    is_np = isinstance(frames, np.ndarray)
    if fmt.name != "nv12":
        order = [2, 1, 0] if fmt.name in ("bgr", "bgra") else [0, 1, 2]
        picked = frames[..., order]
        return np.ascontiguousarray(picked) if is_np else picked.contiguous()
    f = frames.astype(np.int32) if is_np else frames.to(torch.int32)
    pairs = f[:, H:, :].reshape(n, H // 2, W // 2, 2)
    if is_np:
        pairs = pairs.repeat(2, axis=1).repeat(2, axis=2)
    else:
        pairs = pairs.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return yuv_to_rgb(f[:, :H, :], pairs[..., 0], pairs[..., 1], fmt.coef)


def yuv_to_rgb(Y, U, V, coef):
    """The integer rule on arrays of equal shape (numpy or torch, any integer dtype; int32 inside) -> uint8 [..., 3].  coef:
    yuv_coefficients(...)."""
    cy, crv, cgu, cgv, cbu, y_off = coef
    if isinstance(Y, np.ndarray):
        Y, U, V = (a.astype(np.int32) for a in (Y, U, V))
        shift, stack = np.right_shift, np.stack
    else:
        Y, U, V = (a.to(torch.int32) for a in (Y, U, V))
        shift, stack = torch.bitwise_right_shift, torch.stack
    y, u, v = cy * (Y - y_off) + 32768, U - 128, V - 128
    rgb = stack([shift(y + crv * v, 16), shift(y - cgu * u - cgv * v, 16), shift(y + cbu * u, 16)], -1)     # (>> on int32: arithmetic)
    return rgb.clip(0, 255).astype(np.uint8) if isinstance(rgb, np.ndarray) else rgb.clamp(0, 255).to(torch.uint8)


def _named_format(name, colorspace, range) -> FrameFormat:
    """The call form of crop_resize_frames / frames_to_rgb, whose colorspace / range have string defaults: they are validated, and
    read for "nv12" only."""
    if isinstance(name, (FrameFormat, dict)):
        return resolve_format(name)
    yuv_coefficients(colorspace, range)
    return resolve_format(name, colorspace, range) if name == "nv12" else resolve_format(name)


def frames_to_rgb_host(frames: np.ndarray, frame_format: str = "rgb", colorspace: str = "bt601", range: str = "limited",
                       chroma_offset: int | None = None) -> np.ndarray:
    """`bd_frames_to_rgb_host`: the kernel's own per-pixel text (csrc/pixel_format.h) on a numpy array, in the calling thread; no GPU.
    Rows and frames may be strided (the pixel's bytes are contiguous); returns uint8 [n, H, W, 3]."""
    lib = _lib.load()
    fmt = _named_format(frame_format, colorspace, range)
    n, H, W = _frame_geometry(frames, fmt, np.ndarray)
    if frames.strides[-1] != 1 or (fmt.name != "nv12" and frames.strides[2] != fmt.channels):
        raise ValueError(f"{fmt.name} frames need contiguous pixels: {_LAYOUT[fmt.name]}; rows and frames may be strided")
    out = np.empty((n, H, W, 3), np.uint8)
    off = H * frames.strides[1] if chroma_offset is None else int(chroma_offset)
    rc = lib.bd_frames_to_rgb_host(frames.ctypes.data, n, H, W, frames.strides[1], frames.strides[0], fmt.id, off, *fmt.coef, out.ctypes.data)
    _lib.check(rc, "bd_frames_to_rgb_host")
    return out


def crop_resize_frames(frames: torch.Tensor, boxes: torch.Tensor, *, frame_idx: torch.Tensor | None = None,
                       keep_boxes: torch.Tensor | None = None, out_size: int = 224, out: torch.Tensor | None = None,
                       dtype: torch.dtype = torch.float32, frame_format="rgb", colorspace: str = "bt601",
                       range: str = "limited") -> torch.Tensor:
    """`bd_crop_resize_frames` on the current stream.  frames: uint8 device [n, H, W, 3] (HWC RGB; the pixel must be 3 contiguous
    bytes, rows and frames may be strided: a slice of a larger tensor is read in place).  boxes: int32 device [m, 4] (or [B, T, 4])
    square windows x0 y0 x1 y1; frame_idx int32 [m] (default: crop i reads frame i); keep_boxes int32 [m, 4]: pixels outside it are 0,
    edges inclusive (the reference's `bbox_obj`).  Returns [m, 3, S, S] (or boxes' leading shape) in `dtype`, or writes `out`
    ([m, 3, S, S] / [B, T, 3, S, S], contiguous; its dtype wins).  A degenerate box gives zeros (include/boxdreamer_hip.h).
    No allocation when `out` is given, no synchronisation.

    frame_format: "rgb" (the default: the call above), "bgr" [n, H, W, 3], "rgba" / "bgra" [n, H, W, 4] (the fourth byte is ignored),
    "nv12" [n, H + H / 2, W] with even H and W: H luma rows, then H / 2 rows of interleaved U, V pairs, converted with `colorspace`
    ("bt601" / "bt709") and `range` ("limited" / "full"); both are read for "nv12" only.  These run `bd_crop_resize_frames_fmt`, whose
    result is bit for bit this function's on `frames_to_rgb(frames, ...)`; only the pixels under a crop are converted."""
    lib = _lib.load()
    fmt = _named_format(frame_format, colorspace, range)
    if fmt.name == "rgb":
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise TypeError("frames must be a uint8 tensor [n, H, W, 3]")
        n, H, W, _ = frames.shape
    else:
        n, H, W = _frame_geometry(frames, fmt, torch.Tensor)
    if frames.numel() == 0:
        raise ValueError("frames is empty")
    if fmt.name == "rgb":
        if frames.stride(3) != 1 or frames.stride(2) != 3:
            raise ValueError("frames needs unit channel stride and 3-byte pixels (HWC); rows and frames may be strided")
    elif frames.stride(-1) != 1 or (fmt.name != "nv12" and frames.stride(2) != fmt.channels):
        raise ValueError(f"{fmt.name} frames need contiguous pixels: {_LAYOUT[fmt.name]}; rows and frames may be strided")
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
    if fmt.name == "rgb":
        rc = lib.bd_crop_resize_frames(_lib.ptr(frames), n, H, W, frames.stride(1), frames.stride(0), _lib.ptr(b), _lib.ptr(fi), _lib.ptr(kb),
                                       m, S, _lib.ptr(out), _lib.dtype_id(out), _lib.stream())
        _lib.check(rc, "bd_crop_resize_frames")
        return out
    # (the tensor form of NV12 has its chroma rows right below the luma rows: H * row_stride)
    rc = lib.bd_crop_resize_frames_fmt(_lib.ptr(frames), n, H, W, frames.stride(1), frames.stride(0), _lib.ptr(b), _lib.ptr(fi),
                                       _lib.ptr(kb), m, S, _lib.ptr(out), _lib.dtype_id(out), fmt.id, H * frames.stride(1), *fmt.coef,
                                       _lib.stream())
    _lib.check(rc, "bd_crop_resize_frames_fmt")
    return out


class FramePreprocessor:
    """Frames + float boxes -> (images, intrinsics of the crops, integer boxes) for a fixed number of crops `m`.

    Owns the int32 box / frame-index buffers and the output buffer; after the first call nothing is allocated by the launch path
    and nothing waits for the device (`square_bbox` / `crop_intrinsics` are a handful of small torch kernels on the same stream).
    The returned tensors are the object's own buffers: the next call overwrites them."""

    def __init__(self, m: int, out_size: int = 224, dtype: torch.dtype = torch.float32, device="cuda", padding: float = 0.1,
                 frame_format="rgb", colorspace: str = "bt601", range: str = "limited"):
        self.frame_format = _named_format(frame_format, colorspace, range)      # (crop_resize_frames': the layout of every call's frames)
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
        crop_resize_frames(frames, self.boxes, frame_idx=fi, keep_boxes=kb, out_size=self.out_size, out=self.images,
                           frame_format=self.frame_format)
        K_crop = crop_intrinsics(K, self.boxes, self.out_size) if K is not None else None
        return self.images, K_crop, self.boxes
