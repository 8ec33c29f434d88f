"""The byte layout of an operand tensor (include/boxdreamer_hip.h), in one place: plain functions over (tensor, operand class).

A 16-bit operand of `rows` x `cols` is [rows, cols], or [2, rows, cols] for the two-plane classes; the plane distance the C ABI takes
is the first plane's element count (0 for one plane).  Split-bf16 / split-f16: two elementwise planes.  F16C8: plane 0 is f16, plane 1
is one e4m3 BYTE per element -- rows of `cols` bytes packed at the head of plane-1 storage, the rest unused -- so it moves as uint8
rows, never as 16-bit rows.  A tensor may hold more rows than are in use (the reference bank's): its planes are its capacity apart.
"""
from __future__ import annotations

import torch

from . import _lib


def empty(cls, rows: int, cols: int, device, zero: bool = False) -> torch.Tensor:
    tr = _lib.traits(cls)
    return (torch.zeros if zero else torch.empty)((2, rows, cols) if tr.planes == 2 else (rows, cols), dtype=tr.dtype, device=device)


def plane_offset(t: torch.Tensor, cls) -> int:
    """Distance of plane 1 from plane 0 in storage elements, as the C ABI takes it."""
    return t[0].numel() if _lib.planes(cls) == 2 else 0


def row_planes(t: torch.Tensor, cls, rows: int):
    """Rows [0, rows) of every plane as a [rows, cols] view, each in the plane's own element type."""
    tr = _lib.traits(cls)
    assert t.dim() == tr.planes + 1, f"an operand of class {tr.cls} is [rows, cols] per plane, got {tuple(t.shape)}"
    if tr.planes == 1:
        return [t[:rows]]
    cols = t.shape[-1]
    if tr.plane_bytes[1] == t.element_size():
        return [t[0][:rows], t[1][:rows]]
    return [t[0][:rows], t[1].view(torch.uint8).reshape(-1)[:rows * cols].reshape(rows, cols)]


def copy_rows(dst: torch.Tensor, dst_row0: int, src: torch.Tensor, n_rows: int, cls) -> None:
    """Rows [0, n_rows) of src -> rows [dst_row0, dst_row0 + n_rows) of dst; the two may differ in capacity."""
    for d, s in zip(row_planes(dst, cls, dst_row0 + n_rows), row_planes(src, cls, n_rows)):
        d[dst_row0:].copy_(s)


def row_bytes(cls, cols: int) -> int:
    """Bytes of one row over all planes."""
    return cols * sum(_lib.traits(cls).plane_bytes)
