"""Decoder plugin: `BETR` with the reference's constructor, parameter names (so reference
checkpoints load with strict=True) and forward signature
(/root/reference/src/models/modules/backbone/betr.py:11-437), backed by `bd_decoder_forward`.

Only the released configuration is on the MI355X hot path: pose_representation='bb8',
bbox_representation='heatmap', use_pretrained=True.  Inference only.
"""
from __future__ import annotations

import os
import weakref
import warnings

import torch
from torch import nn

from . import _lib, features, hip_ops, operand, pack


class _Norm(nn.Module):
    """Parameter container named like nn.LayerNorm / LlamaRMSNorm (blocks.py:35-56)."""

    def __init__(self, n, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))
        if bias:
            self.bias = nn.Parameter(torch.zeros(n))


class _Mlp(nn.Module):
    def __init__(self, d_in, d_hidden, d_out):
        super().__init__()
        self.fc1 = nn.Linear(d_in, d_hidden)
        self.fc2 = nn.Linear(d_hidden, d_out)


class _Attention(nn.Module):
    """Parameters of blocks.py:208-241 (qkv, q_norm, k_norm, proj)."""

    def __init__(self, dim, heads):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3)
        self.q_norm = _Norm(dim // heads, bias=False)
        self.k_norm = _Norm(dim // heads, bias=False)
        self.proj = nn.Linear(dim, dim)


class SelfAttentionBlock(nn.Module):
    """Parameters of blocks.py:808-874 (norm1, attn, norm2, mlp)."""

    def __init__(self, hidden_size, num_heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = _Norm(hidden_size)
        self.attn = _Attention(hidden_size, num_heads)
        self.norm2 = _Norm(hidden_size)
        self.mlp = _Mlp(hidden_size, int(hidden_size * mlp_ratio), hidden_size)


class _Views:
    """Which of a forward's (B, T) view slots are views: all of them (counts None), or per sample the first counts[b] -- a ragged
    batch, with its device tables (BETR.ragged_index): the packing index of the valid slots and the samples' view offsets."""

    def __init__(self, decoder, B: int, T: int, counts, dev):
        self.n_views, self.max_views = (B * T, T) if counts is None else (sum(counts), max(counts))
        self.index, self.view_start = decoder.ragged_index(counts, T, dev) if counts is not None else (None, None)

    def pack(self, x):
        """(B, T, ...) -> the views sample by sample: n_views leading rows (a uniform batch's slots already are that, in place)."""
        return x.contiguous() if self.index is None else x.flatten(0, 1).index_select(0, self.index)


class _Call:
    """What forward() and forward_entry() share of one call on (B, T) view slots: the view counts (None: IS the uniform batch), all
    checked before a GPU is needed; then the device of `tensors` (`masks` among them), the precision, the packed weights with the latency forms as
    `hip_latency` says, the call's _Views, the query view per sample (BETR._one_hot_query) and the class the features are read in."""

    def __init__(self, decoder, B: int, T: int, view_counts, masks, *tensors):
        self.B, self.T, self.counts = B, T, None
        if view_counts is not None:
            self.counts = _lib.view_counts_list(view_counts, B)
            _lib.check_view_counts(self.counts, T)
            if all(c == T for c in self.counts):      # IS the uniform batch
                self.counts = None
        _lib.require_gpu()
        self.lib = _lib.load()
        self.dev = _lib.same_device(*tensors)
        self.prec = decoder.hip_precision
        self.pid = _lib.prec_id(self.prec)
        self.w = w = decoder._weights(self.dev, self.prec).struct
        if self.counts is None and w.latency_mode != int(decoder.hip_latency):      # (the ragged entry points have no latency forms)
            decoder._check_not_frozen("switching hip_latency (the workspace layout changes)")
            w.latency_mode = int(decoder.hip_latency)
        self.P, self.D = w.grid * w.grid, w.dim
        self.views = _Views(decoder, B, T, self.counts, self.dev)
        self.query_idx = decoder._one_hot_query(masks, B, T, self.counts, self.views, self.dev)
        self.fcls = decoder.feats_class(self.prec)


class BETR(nn.Module):
    """Box Estimation TRansformer on MI355X (HIP kernels behind the reference interface)."""

    def __init__(self, d_model=512, nhead=8, num_decoder_layers=6, **kwargs):
        super().__init__()
        self.d_model, self.nhead, self.att_depth = d_model, nhead, num_decoder_layers
        self.decoder_only = kwargs["decoder_only"]
        self.patch_size = kwargs["patch_size"]
        self.img_size = kwargs["img_size"]
        self.nvs_supervision = kwargs.get("nvs_supervision", False)
        self.ray_supervision = kwargs.get("ray_supervision", False)
        self.use_mask = kwargs.get("use_mask", False)
        self.patchify_rays = kwargs.get("patchify_rays", False)
        self.pose_representation = kwargs.get("pose_representation", "bb8")
        self.bbox_representation = kwargs.get("bbox_representation", "voting")
        self.diff_emb = kwargs["diff_emb"]
        self.use_pretrained = kwargs["use_pretrained"]
        assert self.nvs_supervision or self.ray_supervision, "At least one supervision should be True"
        if (self.pose_representation != "bb8" or self.bbox_representation != "heatmap"
                or not self.use_pretrained or self.nvs_supervision):
            raise NotImplementedError(
                "the MI355X path implements the released configuration only: pose_representation='bb8', "
                "bbox_representation='heatmap', use_pretrained=True, nvs_supervision=False")
        self.box_dim = 8
        self.cat_dim = 3 + 8
        self.hip_precision = kwargs.get("hip_precision", os.environ.get("BOXDREAMER_HIP_PREC", _lib.DEFAULT_PREC))
        # per-Linear promotion (F16C8 family -> split-f16, e4m3 -> bf16) (include/boxdreamer_hip.h: BD_PROMOTE_*): one mask per block and
        # one for the Linears outside the blocks; all zero until boxdreamer_amd/calibrate.py (or the caller) sets them
        self.hip_lanes = kwargs.get("hip_lanes", "auto")   # sub-batch lanes of one forward ("auto" | 1..4; bit-identical results)
        # OPT-IN latency forms for calls of one or two poses (bd_betr_weights.latency_mode: split-K residual Linears; deterministic, within
        # the mode's tolerance, NOT bit-identical to the same sample inside a larger batch) -- the reference demo's per-frame call
        self.hip_latency = bool(kwargs.get("hip_latency", False))
        self.hip_promote = [0] * num_decoder_layers
        self.hip_promote_misc = 0
        if self.hip_precision == "fp8_mixed":
            self.hip_promote, self.hip_promote_misc = _lib.fp8_mixed_policy(num_decoder_layers, normed=True)
        self.hip_calibration = None   # report of the last calibrate.calibrate() that looked at this decoder

        self.attn = nn.Sequential(*[SelfAttentionBlock(d_model, nhead) for _ in range(num_decoder_layers)])
        self.bbox_proj = nn.Linear(d_model, self.patch_size ** 2 * 8)
        self.input_transform = _Mlp(d_model, d_model, d_model)
        self.norm = nn.Module()          # LayerNorm(elementwise_affine=False): no parameters (betr.py:161)
        self.bbox_learnable_query = nn.Parameter(torch.zeros(1, d_model))
        self.bbox_emb = nn.Linear(self.patch_size ** 2 * 8, d_model)

        self._packed = {}          # (device, operand class) -> (content signature, pack.Packed)
        self._ws = None
        self._frozen_by = weakref.WeakSet()   # live GraphedPaths that captured raw pointers into _packed / _ws (graph.py)
        self.last_logits = None
        # one-hot check of `masks`: True = checked here (costs a device sync per forward); "deferred" = the verdict is left ON THE DEVICE in
        # `self.mask_error` (a 0-dim bool tensor) for a caller that moves it to the host with data it transfers anyway (model.py: with the
        # corners' one D2H); False = no check (graph capture does this by itself)
        self.validate_inputs = True
        self.mask_error = None
        self.recast_count = 0         # forwards that had to re-cast features lacking an operand copy (features.py)
        self._ragged_index = {}       # (view counts, T_max, device) -> (packing index, view_start) on the device (ragged batches)

    # -- packed-weight cache: invalidated by CONTENT, not by hooks.  The key carries every parameter's storage address
    # and version counter, so a checkpoint loaded through the PARENT module (`BoxDreamer.load_state_dict`, which recurses
    # through `_load_from_state_dict` and never calls this module's `load_state_dict`), an in-place edit, `.to()` or
    # `.half()` all re-pack on the next forward.
    def _signature(self):
        """(storage, version) of every parameter: what the packed weights, the load-time calibration and a captured graph are valid for.
        Called on every forward, so the module tree is walked once (nn.Module.parameters() costs 0.55 ms per call here -- round 6: a third
        of the facade's host time between two batches) and only the modules' own parameter dicts are re-read: in-place updates
        (load_state_dict, an optimizer step) and replaced Parameters are seen; sub-modules added after construction are not part of BETR."""
        mods = self.__dict__.get("_sig_modules")
        if mods is None:
            mods = [m for m in self.modules() if m._parameters]
            self.__dict__["_sig_modules"] = mods
        return tuple((p.data_ptr(), None if p.is_inference() else p._version) for m in mods for p in m._parameters.values() if p is not None)

    def _apply(self, fn, *a, **k):
        self._check_not_frozen("moving / casting the module")
        self._packed = {}
        return super()._apply(fn, *a, **k)

    def _check_not_frozen(self, what: str):
        if len(self._frozen_by):
            raise RuntimeError(f"{what} would free memory a live GraphedPath still replays on; delete the graph first")

    def _weights(self, device, prec) -> pack.Packed:
        key = (str(device), _lib.operand_prec(prec))
        sig = self._signature()
        hit = self._packed.get(key)
        if hit is None or hit[0] != sig:
            self._check_not_frozen("re-packing the decoder weights")
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            hit = (sig, pack.pack_betr(sd, _lib.operand_prec(prec), device, self.nhead, self.patch_size, self.img_size))
            self._packed[key] = hit
        pk = hit[1]
        if _lib.operand_prec(prec) in (_lib.PREC_F16C8, _lib.PREC_FP8):
            want = (tuple(m | _lib.PROMOTE_FC2 if m & _lib.PROMOTE_FC1 else m for m in self.hip_promote),
                    self.hip_promote_misc | (_lib.PROMOTE_ADAPTER_FC2 if self.hip_promote_misc & _lib.PROMOTE_ADAPTER_FC1 else 0), 0)
            if pk.promote != want:
                self._check_not_frozen("changing the per-Linear promotion")
                pk.set_promote(self.hip_promote, self.hip_promote_misc)
        return pk

    def feats_class(self, prec=None) -> int:
        """Operand class in which this decoder reads `pretrain_rgb_feat`'s 16-bit copy (the class of its adapter's first Linear)."""
        cls = _lib.operand_prec(self.hip_precision if prec is None else prec)
        return _lib.promoted_class(cls) if self.hip_promote_misc & _lib.PROMOTE_ADAPTER_FC1 else cls

    def _workspace(self, need: int, dev) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._check_not_frozen("growing the decoder workspace (a larger B or T than the captured one)")
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    # -- reference helpers kept for API compatibility (host-side, tiny)
    def patchify(self, imgs, c):
        p = self.patch_size
        h = w = imgs.shape[2] // p
        x = imgs.reshape(imgs.shape[0], c, h, p, w, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * w, p ** 2 * c)

    def unpatchify(self, x, c):
        p = self.patch_size
        h = w = int(x.shape[1] ** 0.5)
        x = x.reshape(x.shape[0], h, w, p, p, c)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], c, h * p, h * p)

    def ragged_index(self, counts, t_max: int, dev):
        """(packing index int64 [n_views], view_start int32 [B + 1]) on `dev` for host view counts: built on the host, uploaded once per
        distinct (counts, T_max) and kept (a serving process sees the same few mixes again and again)."""
        key = (tuple(counts), int(t_max), str(dev))
        hit = self._ragged_index.get(key)
        if hit is None:
            if len(self._ragged_index) >= 64:
                self._ragged_index.clear()
            hit = (torch.tensor(_lib.packing_index(counts, t_max), dtype=torch.int64).to(dev),
                   torch.tensor(_lib.view_starts(counts), dtype=torch.int32).to(dev))
            self._ragged_index[key] = hit
        return hit

    def _one_hot_query(self, masks, B: int, T: int, counts, views, dev):
        """The one-hot check of `masks` as `validate_inputs` asks for it (forward()'s rule), then the query view per sample, int32 [B]."""
        if masks.dtype != torch.bool or masks.shape != (B, T):
            raise ValueError("masks must be a (B, T) bool tensor")
        if self.validate_inputs and not torch.cuda.is_current_stream_capturing():
            bad = masks.sum(dim=1) != 1
            if counts is not None:       # ... and among the sample's own views (a padded slot is never a view)
                valid = torch.arange(T, device=dev)[None, :] < (views.view_start[1:] - views.view_start[:-1])[:, None]
                bad = bad | (masks & ~valid).any(dim=1)
            bad = bad.any()
            if self.validate_inputs == "deferred":
                self.mask_error = bad                  # stays on the device; the caller raises (no sync here)
            elif bool(bad):
                raise ValueError("masks must mark exactly one query view per sample" +
                                 (", among the sample's view_counts views" if counts is not None else ""))
        return masks.to(torch.int32).argmax(dim=1).to(torch.int32).contiguous()

    @torch.no_grad()
    def entry_tokens(self, pose_feat, pretrain_rgb_feat, out=None):
        """The decoder-ENTRY token rows of free-standing views (bd_decoder_entry_tokens; betr.py:313-329, :367-399):
        x = bbox_emb(patchify(pose_feat)) + pos + adapter(feat), the row forward() builds for a reference view before its first block.
        pose_feat (N, 8, H, W); pretrain_rgb_feat (N, P, C) from the HIP encoder (with its operand copy, in this decoder's feature
        class: ValueError otherwise -- nothing is re-cast for a bank) -> fp32 (N, P, d_model), written into `out` when given.  What
        cache.RefFeatureBank(decoder=...) keeps per reference and forward_entry() consumes."""
        _lib.require_gpu()
        lib = _lib.load()
        only = isinstance(pretrain_rgb_feat, features.OperandOnly)
        dev = _lib.same_device(pose_feat, pretrain_rgb_feat.operand if only else pretrain_rgb_feat, out)
        prec = self.hip_precision
        pid = _lib.prec_id(prec)
        w = self._weights(dev, prec).struct
        P, D, N = w.grid * w.grid, w.dim, int(pose_feat.shape[0])
        if pose_feat.dim() != 4 or tuple(pose_feat.shape[1:]) != (self.box_dim, self.img_size, self.img_size):
            raise ValueError(f"pose_feat must be (N, {self.box_dim}, {self.img_size}, {self.img_size}), got {tuple(pose_feat.shape)}")
        if tuple(pretrain_rgb_feat.shape) != (N, P, D):
            raise ValueError(f"pretrain_rgb_feat must be ({N}, {P}, {D}), got {tuple(pretrain_rgb_feat.shape)}")
        fcls = self.feats_class(prec)
        feats16 = features.resolve(pretrain_rgb_feat, fcls, _lib.planes(fcls) * N * P * D, dev)
        if feats16 is None:
            raise ValueError(f"entry tokens need the HIP encoder's operand copy of the features in this decoder's feature class ({fcls}); "
                             "these carry none (computed elsewhere, copied or sliced), or one of another class")
        if out is None:
            out = torch.empty((N, P, D), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (N, P, D) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous fp32 ({N}, {P}, {D}) tensor")
        ws = self._workspace(lib.bd_decoder_entry_tokens_workspace_bytes(w, N, pid), dev)
        hip_ops.decoder_entry_tokens(w, pose_feat.contiguous(), feats16, operand.plane_offset(feats16, fcls), out, ws, prec=pid)
        return out

    @torch.no_grad()
    def forward_entry(self, entry_rows, n_rows, src, query_feat, masks, img_size=None, view_counts=None):
        """forward() on banked decoder-entry tokens (bd_decoder_forward_entry): no heat map is read, patchified or embedded.
        entry_rows: fp32 (capacity, P, d_model), cache.RefFeatureBank.entry_tokens, its first n_rows rows in use; src: device int32
        [n_views], the source table of the batch's views in sample order -- a reference by its bank row, sample b's query as -(b + 1)
        (RefFeatureBank.tables / select); query_feat (B, P, C): the encoder's output for the B query crops, in sample order; masks
        (B, T) bool: the query position per sample (T: the batch's view slots); view_counts: as in forward(), a ragged batch (one
        lane).  Returns (B, 8, H, W) fp32 in [-1, 1], bit-identical to forward() on the same views; `last_logits` as there."""
        B, T = masks.shape
        only = isinstance(query_feat, features.OperandOnly)
        c = _Call(self, B, T, view_counts, masks, entry_rows, src, masks, query_feat.operand if only else query_feat)
        P, D, n_views = c.P, c.D, c.views.n_views
        if entry_rows.dtype != torch.float32 or entry_rows.dim() != 3 or tuple(entry_rows.shape[1:]) != (P, D) or not entry_rows.is_contiguous() \
                or not 0 <= int(n_rows) <= entry_rows.shape[0]:
            raise ValueError(f"entry_rows must be a contiguous fp32 (rows >= {int(n_rows)}, {P}, {D}) tensor, got {tuple(entry_rows.shape)} {entry_rows.dtype}")
        if src.dtype != torch.int32 or src.numel() != n_views or not src.is_contiguous():
            raise ValueError(f"src must be a contiguous int32 tensor of the batch's {n_views} views, got {tuple(src.shape)} {src.dtype}")
        if tuple(query_feat.shape) != (B, P, D):
            raise ValueError(f"query_feat must be ({B}, {P}, {D}), got {tuple(query_feat.shape)}")
        feats16 = features.resolve(query_feat, c.fcls, _lib.planes(c.fcls) * B * P * D, c.dev)
        if feats16 is None:
            raise ValueError(f"forward_entry needs the HIP encoder's operand copy of the query features in this decoder's feature class ({c.fcls})")
        return self._launch(c, True, (_lib.ptr(entry_rows), int(n_rows), _lib.ptr(src)), feats16, self.img_size if img_size is None else int(img_size))

    def _launch(self, c: _Call, banked: bool, source, feats16, H: int):
        """The one decoder launch of a call, uniform (sub-batch lanes) or ragged, on the workspace it asks for.  `source`: the C entry
        point's arguments that name the entry tokens' source -- (heat maps, their dtype), or banked: (entry rows, rows in use, src)."""
        lib, w, B, T, pid, views = c.lib, c.w, c.B, c.T, c.pid, c.views
        logits = torch.empty((B, 8, H, H), dtype=torch.float32, device=c.dev)
        heat = torch.empty_like(logits)
        feats = (_lib.ptr(feats16), operand.plane_offset(feats16, c.fcls))
        if c.counts is None:
            lanes = _lib.resolve_lanes(self.hip_lanes, B * T, B, c.prec)
            if banked:
                name = "bd_decoder_forward_entry"
                need = max(lib.bd_decoder_entry_workspace_bytes(w, B, T, pid, 1), lib.bd_decoder_entry_workspace_bytes(w, B, T, pid, lanes))
            else:
                name = "bd_decoder_forward_lanes"
                need = max(lib.bd_decoder_workspace_bytes(w, B, T, pid), lib.bd_decoder_workspace_bytes_lanes(w, B, T, pid, lanes))
            ws = self._workspace(need, c.dev)
            rc = getattr(lib, name)(w, *source, *feats, _lib.ptr(c.query_idx), B, T, H, _lib.ptr(logits), _lib.ptr(heat), _lib.ptr(ws),
                                    ws.numel(), pid, lanes, _lib.stream())
        else:
            name = "bd_decoder_forward_entry_ragged" if banked else "bd_decoder_forward_ragged"
            need = (lib.bd_decoder_entry_workspace_bytes_ragged if banked else lib.bd_decoder_workspace_bytes_ragged)(w, views.n_views, B, pid)
            ws = self._workspace(need, c.dev)
            rc = getattr(lib, name)(w, *source, *feats, _lib.ptr(views.view_start), _lib.ptr(c.query_idx), B, views.n_views, views.max_views, H,
                                    _lib.ptr(logits), _lib.ptr(heat), _lib.ptr(ws), ws.numel(), pid, _lib.stream())
        _lib.check(rc, name)
        self.last_logits = logits
        return heat

    @torch.no_grad()
    def forward(self, pose_feat, rgbs=None, masks=None, pretrain_rgb_feat=None, image_masks=None, view_counts=None):
        """pose_feat (B,T,8,H,W) in [-1,1]; rgbs (B,T,3,H,W) (shape check only); masks (B,T) bool, one query
        view per sample; pretrain_rgb_feat (B,T,P,C) from the encoder.  Returns (B,8,H,W) fp32 in [-1,1].

        view_counts (host ints, length B; optional): a RAGGED batch.  The inputs stay (B, T_max, ...); sample b's valid views are the
        slots [0, view_counts[b]) and its query view (`masks`) must be one of them.  The other slots are never read.  The sample
        attends over its own views only, on packed token rows (bd_decoder_forward_ragged): its result is bit-identical to the sample
        run alone at T = view_counts[b].  pretrain_rgb_feat is then either the packed features of the sum(view_counts) valid views,
        (n_views, P, C) in sample order -- what the encoder returns for the packed images, with its operand copy -- or padded
        (B, T_max, P, C), which is packed and re-cast here (slow path).

        pretrain_rgb_feat may also be a features.OperandOnly (the operand copy alone, from cache.RefFeatureBank): (B, T, P, C), or
        packed (n_views, P, C) for a ragged batch.  It must be in this decoder's feature class; ValueError otherwise."""
        assert rgbs is not None, "rgbs input should not be None"
        B, T, _, H, W = rgbs.shape
        assert H == W == self.img_size, f"H and W should be equal to img_size {self.img_size}, got {H}x{W}"
        if pretrain_rgb_feat is None:
            raise NotImplementedError("the MI355X path requires pretrained RGB features (use_pretrained=True)")
        only = isinstance(pretrain_rgb_feat, features.OperandOnly)       # an operand copy with no fp32 tensor behind it (a reference bank)
        # (the reference writes the query token through `pose_feat[masks] = ...` (betr.py:286-290), which fails unless every sample marks
        # exactly one view; argmax would silently pick view 0 for an empty row: _one_hot_query)
        c = _Call(self, B, T, view_counts, masks, pose_feat, rgbs, masks, pretrain_rgb_feat.operand if only else pretrain_rgb_feat)
        counts, views, fcls, P, D = c.counts, c.views, c.fcls, c.P, c.D
        if tuple(pose_feat.shape) != (B, T, self.box_dim, H, W):
            raise ValueError(f"pose_feat must be (B, T, {self.box_dim}, H, W) = {(B, T, self.box_dim, H, W)}, got "
                             f"{tuple(pose_feat.shape)}")
        n_views, shape = views.n_views, tuple(pretrain_rgb_feat.shape)
        # `packed`: the features are the n_views views in order (a uniform batch's always are); else padded (B, T_max, P, D) of a ragged one
        packed = counts is None or shape == (n_views, P, D)
        if counts is None and (pretrain_rgb_feat.numel() != B * T * P * D or shape[-1] != D):
            raise ValueError(f"pretrain_rgb_feat must be (B, T, {P}, {D}), got {shape}")
        if not packed and shape != (B, T, P, D):
            raise ValueError(f"pretrain_rgb_feat must be packed ({n_views}, {P}, {D}) or padded ({B}, {T}, {P}, {D}), got {shape}")
        if only and not packed:
            raise ValueError(f"operand-only features of a ragged batch must be packed ({n_views}, {P}, {D}), got {shape}")
        # (padded features of a ragged batch are never taken as they are: their copy holds the padded slots too)
        feats16 = features.resolve(pretrain_rgb_feat, fcls, _lib.planes(fcls) * n_views * P * D, c.dev) if packed else None
        if feats16 is None:   # features without an operand copy (computed elsewhere, copied, sliced): explicit re-cast
            self.recast_count += 1
            if self.recast_count == 1:
                warnings.warn("BETR: pretrain_rgb_feat carries no operand-dtype copy from the HIP encoder; re-casting it "
                              "(slow path, see boxdreamer_amd/features.py)", stacklevel=2)
            f32 = pretrain_rgb_feat if packed else views.pack(pretrain_rgb_feat)
            feats16 = hip_ops.to_operand(f32.reshape(n_views * P, D).float(), fcls)
        pose = views.pack(pose_feat)                       # the valid views only: [n_views, 8, H, W]
        return self._launch(c, False, (_lib.ptr(pose), _lib.dtype_id(pose)), feats16, H)
