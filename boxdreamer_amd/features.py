"""Explicit hand-off of the encoder's operand-dtype feature copy to the decoder.

`bd_encoder_forward` writes the patch features twice: fp32 (what the reference's `predict` returns,
/root/reference/src/models/modules/encoder/dinov2.py:45-60) and in the GEMM operand format of the active precision mode
(what `bd_decoder_forward` consumes).  The operand copy travels with the fp32 tensor OBJECT: `attach` ties it to that
object's lifetime, `operand_of` returns it only when the object still describes the same data, and `carry` moves it onto
another tensor object that aliases the same storage (a `.view()` / `.reshape()` / `.contiguous()` no-op).  Anything else
-- a copy, a slice, features computed elsewhere -- has NO operand copy: `operand_of` returns None and the decoder re-casts
explicitly (counted in `BETR.recast_count`, warned about once), never silently on stale data.

Features that exist as an operand copy ONLY (cache.RefFeatureBank: no fp32 tensor is ever made) travel in `OperandOnly`, an explicit
carrier the decoder checks and never re-casts.
"""
from __future__ import annotations

import torch

_ATTR = "_bd_operand"


def _version(t: torch.Tensor):
    """In-place-modification stamp of `t`.  Tensors created under `torch.inference_mode()` (Lightning's test / validate /
    predict loops run there by default) do not track a version counter -- reading `_version` raises -- and cannot be
    modified in place outside inference mode; for them the identity check is storage address + element count only."""
    return None if t.is_inference() else t._version


def attach(feats32: torch.Tensor, feats16: torch.Tensor, pid: int, stamp=None) -> torch.Tensor:
    """`stamp`: what produced the features beyond the operand class -- the encoder's per-Linear promotion state (calibrate.py): two
    feature sets of the same class computed under different promotion states are NOT interchangeable (cache.py checks it)."""
    setattr(feats32, _ATTR, (feats16, int(pid), feats32.data_ptr(), feats32.numel(), _version(feats32), stamp))
    return feats32


def operand_of(feats32: torch.Tensor, pid: int):
    """The operand copy for precision id `pid`, or None if `feats32` carries none / was modified in place since."""
    tag = getattr(feats32, _ATTR, None)
    if tag is None:
        return None
    f16, tpid, ptr, numel, version = tag[:5]
    if tpid != int(pid) or ptr != feats32.data_ptr() or numel != feats32.numel() or version != _version(feats32):
        return None
    return f16


def tag_of(feats32: torch.Tensor):
    """(operand copy, precision id) or None -- for the reference-feature cache, which re-packs both copies."""
    tag = getattr(feats32, _ATTR, None)
    if tag is None or tag[2] != feats32.data_ptr() or tag[4] != _version(feats32):
        return None
    return tag[0], tag[1]


def require_tag(feats32: torch.Tensor):
    """tag_of for callers that cannot go on without the operand copy (the feature cache and the reference bank)."""
    tag = tag_of(feats32)
    if tag is None:
        raise ValueError("features were not produced by the HIP encoder (no operand-dtype copy attached)")
    return tag


def stamp_of(feats32: torch.Tensor):
    """The producer stamp `attach` recorded (None: none recorded / no tag)."""
    tag = getattr(feats32, _ATTR, None)
    return tag[5] if tag is not None and len(tag) > 5 else None


def carry(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """Move src's operand copy onto dst when dst aliases exactly the same elements (same storage start, same count)."""
    tag = getattr(src, _ATTR, None)
    if tag is not None and dst is not src and dst.data_ptr() == tag[2] and dst.numel() == tag[3] and dst.is_contiguous():
        setattr(dst, _ATTR, (tag[0], tag[1], tag[2], tag[3], _version(dst), tag[5] if len(tag) > 5 else None))
    return dst


class OperandOnly:
    """Features that exist in the decoder's operand format ONLY -- what cache.RefFeatureBank assembles with bd_gather_view_rows: there
    is no fp32 tensor behind them, so nothing to re-cast from.  `shape` is the logical (B, T, P, C) or packed (n_views, P, C) shape,
    `operand` the operand tensor ([rows, C], or [2, rows, C] for the two-plane classes), `class_id` its operand class and `stamp` the
    encoder state it was produced under.  BETR.forward checks it the way it checks an attached copy (class, element count, device) and
    raises where it would have re-cast."""

    def __init__(self, shape, operand: torch.Tensor, class_id: int, stamp=None):
        self.shape, self.operand, self.class_id, self.stamp = tuple(int(s) for s in shape), operand, int(class_id), stamp

    @property
    def device(self):
        return self.operand.device

    def dim(self) -> int:
        return len(self.shape)

    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n

    def checked(self, class_id: int, numel: int, device) -> torch.Tensor:
        """The operand tensor when it is what the decoder reads (class, element count over all planes, device); ValueError otherwise."""
        if self.class_id != int(class_id):
            raise ValueError(f"operand-only features are in operand class {self.class_id}, the decoder reads class {int(class_id)} (its "
                             "adapter's first Linear changed class after the features were made, or they come from another precision "
                             "mode); there is no fp32 copy to re-cast from -- refill the reference bank")
        if self.operand.numel() != int(numel) or self.operand.device != device:
            raise ValueError(f"operand-only features hold {self.operand.numel()} elements on {self.operand.device}, the decoder needs "
                             f"{int(numel)} on {device}")
        return self.operand


def resolve(feat, cls: int, n_elems: int, device):
    """The operand tensor the decoder reads for `feat` -- class `cls`, `n_elems` elements over all planes, on `device` -- or None when
    the caller has to re-cast: an OperandOnly that does not fit raises (nothing to re-cast from), a tagged fp32 tensor gives its copy
    when that fits, anything else (computed elsewhere, copied, sliced) gives None."""
    if isinstance(feat, OperandOnly):
        return feat.checked(cls, n_elems, device)
    f16 = operand_of(feat, cls)
    return f16 if f16 is not None and f16.numel() == n_elems and f16.device == device else None
