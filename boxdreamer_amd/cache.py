"""Reference-feature caching across queries ("next" row f1 of SURVEY.md §8).

In the test / demo loops the SAME N posed reference crops accompany every query frame of an object, but the reference
re-encodes them for every query (/root/reference/src/models/BoxDreamerModel.py:274-285; SURVEY.md §7 "hard parts").
DINOv2 features are per-image and input-independent of the other views, so they can be computed once per object:
per pose the encoder then runs on 1 crop instead of T (T=6: 282 -> 47 GFLOP of the 638 GFLOP/pose).

Usage (caller side):
    cache = RefFeatureCache(model.rgb_encoder)
    ref_feats = cache.encode(ref_images)                      # (B, T-1, 3, H, W) -> tagged features, once per object
    data["cached_rgb_feat"], data["cached_rgb_mask"] = cache.place(ref_feats, query_idx, T)
    model(data)                                               # encodes only the views whose mask is False
Results are bit-identical to the uncached forward (tests/test_gpu_facade.py).

The cached features carry the encoder state they were computed under (operand class + per-Linear promotion state, features.stamp_of).
The facade's load-time calibration (model.py / calibrate.py) runs inside the FIRST forward and may promote encoder Linears: features cached
BEFORE that are stale.  `merge_cached_features` notices (stamp mismatch), warns once, and encodes every view of the batch afresh instead --
never a silent mix of two promotion states, never an exception in the middle of a sweep.  Call `model.calibrate(data)` (or one forward)
before `cache.encode` to keep the saving.

RefFeatureBank (below) is the serving form of the same idea: many objects, each with its own number of references, encoded once
into ONE device-resident store in the decoder's operand format (no fp32 copy: 3 bytes per element in the default mode against 7);
a batch -- uniform or ragged (`view_counts`) -- names its references by bank row and one bd_gather_view_rows launch assembles the
decoder's feature operand from those rows and the freshly encoded query views:
    bank = RefFeatureBank(model.rgb_encoder, keep_images=True)
    rows = bank.add(ref_images)                               # (R, 3, S, S) or (B, R, 3, S, S) -> CPU int64 row ids, stable for good
    data["ref_bank"], data["ref_rows"] = bank, table          # (B, T_max) host ints: >= 0 bank row, -1 "encode this slot of data['images']"
    model(data)
With `match_threshold=0.05` the bank also keeps each row's dense-reference match summary (bd_match_view_sums), and a model with
`dense_cfg.enable` selects its `filter_topk` references among a sample's whole banked database (bd_match_select_rows): the table then
holds one -1 per sample, at the query.
With `decoder=model.decoder` the bank also keeps every row's decoder-ENTRY tokens (bd_decoder_entry_tokens): the heat maps of a
reference are given once, `bank.add(ref_images, bbox_feat=ref_heatmaps)`, and a forward over such a bank reads the query crop and
nothing else -- `bbox_feat` may be absent from the batch dict (bd_decoder_forward_entry).
With `keep_poses=True` the bank also keeps every row's pose, `bank.add(ref_images, poses=ref_poses)`: the object's whole database --
features, match summaries, entry tokens, poses -- over which `dense_cfg.multi_round` runs (dense.process_multi_round_bank).
"""
from __future__ import annotations

import warnings

import torch

from . import _lib, features, hip_ops, operand

_WARNED_STALE = False
_WARNED_STALE_BANK = False


def _init_last_stale():
    merge_cached_features.last_stale = False


def take_views(feats: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """feats (B, T, P, C) fp32 from the HIP encoder; idx (B, T') long, -1 = an all-zero view -> (B, T', P, C) with
    out[b, j] = feats[b, idx[b, j]], its operand-dtype copy re-packed the same way and attached (features.attach): what the dense-reference
    helpers (dense.py: view selection, sub-batches of references) need so that BETR does not re-cast on every forward.  Features that carry
    no operand copy come back plain (BETR then re-casts, as before)."""
    B, T, P, C = feats.shape
    dev = feats.device
    idx = idx.to(dev).long()
    Tn = idx.shape[1]
    valid = (idx >= 0).reshape(-1)
    flat = (torch.arange(B, device=dev)[:, None] * T + idx.clamp_min(0)).reshape(-1)
    out32 = feats.reshape(B * T, P, C)[flat]
    out32[~valid] = 0
    out32 = out32.reshape(B, Tn, P, C)
    tag = features.tag_of(feats)
    if tag is None:
        return out32
    f16, pid = tag
    out16 = operand.empty(pid, B * Tn * P, C, dev, zero=True)
    for dst, src in zip(operand.row_planes(out16, pid, B * Tn * P), operand.row_planes(f16, pid, B * T * P)):
        g = src.reshape(B * T, P, C)[flat]
        g[~valid] = 0
        dst.copy_(g.reshape(-1, C))
    return features.attach(out32, out16, pid, features.stamp_of(feats))


class RefFeatureCache:
    def __init__(self, encoder):
        self.encoder = encoder                                 # a DinoV2Wrapper

    def encode(self, images: torch.Tensor) -> torch.Tensor:
        """(B, R, 3, H, W) -> (B, R, P, C) fp32 features tagged with their operand-dtype copy."""
        return self.encoder.predict(images)

    def place(self, ref_feats: torch.Tensor, query_idx: torch.Tensor, T: int):
        """Scatter R = T-1 cached reference features into a (B, T, P, C) layout leaving the query slot empty.
        Returns (features, valid_mask (B, T) bool)."""
        B, R, P, C = ref_feats.shape
        assert R == T - 1
        f16, pid = features.require_tag(ref_feats)
        dev = ref_feats.device
        valid = torch.ones((B, T), dtype=torch.bool, device=dev)
        valid[torch.arange(B, device=dev), query_idx.to(dev).long()] = False
        full32 = torch.zeros((B, T, P, C), dtype=torch.float32, device=dev)
        full32[valid] = ref_feats.reshape(B * R, P, C)
        full16 = operand.empty(pid, B * T * P, C, dev, zero=True)
        for dst, src in zip(operand.row_planes(full16, pid, B * T * P), operand.row_planes(f16, pid, B * R * P)):
            dst.reshape(B, T, P, C)[valid] = src.reshape(B * R, P, C)
        return features.attach(full32, full16, pid, features.stamp_of(ref_feats)), valid


class RefFeatureBank:
    """Device-resident store of reference features in the decoder's operand format, addressed by row (one row = one view).

    add() runs crops through the encoder once and appends their operand copy; the fp32 copy is dropped (the decoder never reads it).
    All rows live in one tensor that grows geometrically; row ids never change, whatever is added later.  `stamp` is the encoder state
    (encoder.state_stamp: operand class + per-Linear promotion) plus the operand class the rows are in.  When the encoder's state has
    moved on since (the load-time calibration ran, calibrate.set_state was applied), the bank is stale: with keep_images=True it
    re-encodes every row from the crops it kept (in the dtype they came in) -- once, with one warning -- and with keep_images=False it
    raises RuntimeError; rows of two promotion states are never mixed.

    `match_threshold` (None: none kept, today's bank byte for byte; 0.05 is dense.match_views' luminance threshold, the reference's):
    every row also gets its dense-reference match summary -- the foreground feature sum (C floats) and the foreground patch count of
    bd_match_view_sums, computed from the encoder's fp32 output and the crop before that copy is dropped: 3 KB per view against the
    operand row's ~590 KB.  With them a dense-reference forward (dense_cfg.enable + ref_bank) scores and selects among a sample's
    whole database without its features or crops (select).

    `keep_poses` (False: none kept, today's bank byte for byte): every row also gets its view's pose, given in add(..., poses=...), as
    fp32 [rows, 4, 4] in a store that grows with the others (same row ids): 64 bytes per view.  With them the bank is an object's whole
    database and a dense MULTI-ROUND forward (dense_cfg.multi_round + ref_bank) runs over it: the fine level picks the references
    nearest to the coarse pose from these rows (bd_pose_select_rows), and the short last round is padded with `zero_row`.

    `decoder` (None: none kept, today's bank byte for byte; a betr.BETR): every row also gets its decoder-entry tokens
    x = bbox_emb(patchify(bbox_feat)) + pos + adapter(feat) (bd_decoder_entry_tokens), computed in add() from the heat maps given there
    while the encoder's output still exists, in a second store that grows with the first (same row ids): fp32 [rows, P, D],
    P * D * 4 = 786 432 bytes per view at P = 256, D = 768, on top of the operand row's ~590 KB (the feature rows stay: the refresh
    path and the dense selection use them).  A decoder then runs on these rows (BETR.forward_entry) without patchifying or embedding
    a heat map.  The entry rows carry a second stamp -- what they depend on in the decoder: its weights (_signature), precision
    mode and the promotion of the Linears outside the blocks -- and a mismatch of either stamp makes the bank stale; with
    keep_images=True the heat maps are kept too, in the dtype they came in, and a refresh re-encodes and re-embeds."""

    def __init__(self, encoder, keep_images: bool = True, match_threshold: float | None = None, decoder=None, keep_poses: bool = False):
        self.encoder = encoder                                 # a DinoV2Wrapper
        self.decoder = decoder                                 # a betr.BETR, or None: no entry tokens
        self.keep_images = bool(keep_images)
        self.keep_poses = bool(keep_poses)
        self.match_threshold = None if match_threshold is None else float(match_threshold)
        self.refresh_count = 0
        self._tables = {}       # (ref_rows of the valid slots, counts, T_max, device) -> device tables of one gather launch
        self._dense_tables = {}  # (reference rows, n_refs, N_max, device) -> device tables of one select launch
        self.clear()

    def clear(self) -> None:
        """Drop every row (ids start again at 0), the kept crops and the kept poses."""
        self._t16, self._cap, self._n = None, 0, 0
        self._pid, self._P, self._C, self._stamp = None, 0, 0, None
        self._images = []       # [(first row, crops (N, 3, S, S))] when keep_images
        self._msums, self._mcounts = None, None                # [cap, C] / [cap] fp32 match summaries (match_threshold)
        self._x32, self._entry_stamp, self._entry_shape = None, None, None   # [cap, P, D] fp32 decoder-entry tokens, their stamp (decoder)
        self._heat = []         # [(first row, heat maps (N, 8, S, S))] when keep_images and decoder
        self._poses = None      # [>= cap, 4, 4] fp32 object-to-camera poses of the rows (keep_poses)
        self._zero_row = None   # the row of the all-zero view, once a multi-round forward asked for it (zero_row)

    def __len__(self) -> int:
        return self._n

    @property
    def stamp(self):
        """(encoder.state_stamp under which the rows were encoded, operand class), None while the bank is empty."""
        return self._stamp

    @property
    def operand_class(self):
        return self._pid

    @property
    def has_match_summaries(self) -> bool:
        """Whether every row carries its dense-reference match summary (the bank was built with a match_threshold)."""
        return self.match_threshold is not None

    @property
    def has_entry_tokens(self) -> bool:
        """Whether every row carries its decoder-entry tokens (the bank was built with a decoder)."""
        return self.decoder is not None

    @property
    def has_poses(self) -> bool:
        """Whether every row carries its view's pose (the bank was built with keep_poses=True): what the dense multi-round mode
        needs, whose fine level picks the references nearest to the coarse pose (bd_pose_select_rows)."""
        return self.keep_poses

    @property
    def poses(self):
        """The pose store: fp32 (>= capacity, 4, 4), rows [0, len(bank)) in use (None while the bank is empty or keeps none)."""
        return self._poses

    def poses_of(self, row: int) -> torch.Tensor:
        """The kept pose of a row, fp32 (4, 4) on the device (keep_poses=True)."""
        if not self.has_poses or not 0 <= int(row) < self._n:
            raise KeyError(f"row {row}: no pose kept")
        return self._poses[int(row)]

    @property
    def zero_row(self) -> int:
        """The bank row of the all-zero view that pads the last round of a multi-round decode (dense.sub_batchify pads with views whose
        features AND heat maps are zero): zero bytes in every plane of the operand class, a zero match summary, a zero pose and, in an
        entry-token bank, bd_decoder_entry_tokens of zero features and zero heat maps.  Made on first use, once per bank (clear()
        forgets it); an ordinary row to every kernel, but never re-encoded from a crop -- a zero IMAGE does not encode to zero
        features -- so a refresh re-makes it in place (ensure_fresh)."""
        if self._zero_row is None:
            if self._n == 0:
                raise ValueError("an empty reference bank has no operand class yet: add() references before asking for its zero view")
            self.ensure_fresh()
            self._append_zero()
        return self._zero_row

    def _append_zero(self) -> None:
        dev, P, C, z = self._t16.device, self._P, self._C, self._n
        self._reserve(z + 1, dev)
        for plane in operand.row_planes(self._t16, self._pid, (z + 1) * P):
            plane[z * P:].zero_()
        if self.has_match_summaries:
            self._msums[z].zero_()
            self._mcounts[z].zero_()
        if self.has_poses:
            self._poses[z].zero_()
        if self.has_entry_tokens:
            d = self.decoder
            zeros = features.OperandOnly((1, P, C), operand.empty(self._pid, P, C, dev, zero=True), self._pid, self._stamp[0])
            d.entry_tokens(torch.zeros((1, d.box_dim, d.img_size, d.img_size), dtype=torch.float32, device=dev), zeros, out=self._x32[z:z + 1])
        self._zero_row = z
        self._n += 1

    @property
    def entry_tokens(self):
        """The entry store: fp32 (capacity, P, D), rows [0, len(bank)) in use (None while the bank is empty or keeps none)."""
        return self._x32

    @property
    def entry_stamp(self):
        """(decoder._signature(), precision mode, promotion of its Linears outside the blocks) the entry rows were made under."""
        return self._entry_stamp

    @property
    def tokens_per_view(self) -> int:
        """P: patch tokens of one view (0 while the bank is empty)."""
        return self._P

    @property
    def feature_dim(self) -> int:
        """C: feature channels (0 while the bank is empty)."""
        return self._C

    @property
    def bytes_per_view(self) -> int:
        """Bytes of one row in the bank (all planes)."""
        return 0 if self._pid is None else self._P * operand.row_bytes(self._pid, self._C)

    @property
    def entry_bytes_per_view(self) -> int:
        """Bytes of one row's decoder-entry tokens (0 when the bank keeps none, or is empty)."""
        return 0 if self._entry_shape is None else self._entry_shape[0] * self._entry_shape[1] * 4

    def _now(self):
        return (self.encoder.model.state_stamp(self.encoder.prec), int(self.encoder.model.feats_class(self.encoder.prec)))

    def _entry_now(self):
        d = self.decoder
        misc = int(d.hip_promote_misc)
        return (d._signature(), str(d.hip_precision), misc | (_lib.PROMOTE_ADAPTER_FC2 if misc & _lib.PROMOTE_ADAPTER_FC1 else 0))

    def is_stale(self) -> bool:
        return self._n > 0 and (self._stamp != self._now() or (self.has_entry_tokens and self._entry_stamp != self._entry_now()))

    def _reserve(self, need: int, dev) -> None:
        self._reserve_poses(need, dev)
        if self._t16 is not None and need <= self._cap and self._t16.device == dev:
            return
        cap = max(need, 2 * self._cap, 8)
        new = operand.empty(self._pid, cap * self._P, self._C, dev, zero=True)
        if self._t16 is not None:       # growth re-lays the planes out: plane 1 starts at the new capacity
            operand.copy_rows(new, 0, self._t16.to(dev), self._n * self._P, self._pid)
        if self.has_match_summaries:
            msums = torch.zeros((cap, self._C), dtype=torch.float32, device=dev)
            mcounts = torch.zeros((cap,), dtype=torch.float32, device=dev)
            if self._msums is not None:
                msums[:self._n].copy_(self._msums[:self._n])
                mcounts[:self._n].copy_(self._mcounts[:self._n])
            self._msums, self._mcounts = msums, mcounts
        if self.has_entry_tokens:
            x32 = torch.empty((cap,) + self._entry_shape, dtype=torch.float32, device=dev)
            if self._x32 is not None:
                x32[:self._n].copy_(self._x32[:self._n])
            self._x32 = x32
        self._t16, self._cap = new, cap

    def _reserve_poses(self, need: int, dev) -> None:
        """The pose store has a capacity of its own (a refresh rebuilds the other stores and leaves this one alone)."""
        if not self.has_poses or (self._poses is not None and need <= self._poses.shape[0] and self._poses.device == dev):
            return
        poses = torch.zeros((max(need, 2 * (0 if self._poses is None else self._poses.shape[0]), 8), 4, 4), dtype=torch.float32, device=dev)
        if self._poses is not None:
            poses[:self._n].copy_(self._poses[:self._n])
        self._poses = poses

    ENTRY_CHUNK = 64            # views per bd_decoder_entry_tokens call (its workspace is ~4 MB per view; rows do not depend on the chunking)

    def _append(self, images: torch.Tensor, bbox_feat: torch.Tensor | None = None) -> None:
        if images.device != self.encoder.get_device():
            self.encoder.to_device(images.device)
        feats = self.encoder.predict(images)                   # (N, P, C) fp32, tagged; only the operand copy is kept
        f16, pid = features.require_tag(feats)
        n, P, C = feats.shape
        if self.has_match_summaries and P > 1024:
            raise ValueError(f"match summaries cover views of at most 1024 patch tokens (bd_match_view_sums); these have {P}")
        if self._n == 0:
            self._pid, self._P, self._C, self._stamp = _lib.operand_prec(pid), int(P), int(C), self._now()
            self._t16, self._cap, self._msums, self._mcounts = None, 0, None, None
            if self.has_entry_tokens:
                self._x32, self._entry_stamp, self._entry_shape = None, self._entry_now(), (int(P), int(self.decoder.d_model))
        elif (_lib.operand_prec(pid), int(P), int(C)) != (self._pid, self._P, self._C):
            raise ValueError(f"the bank holds ({self._P}, {self._C}) views of operand class {self._pid}; got ({P}, {C}) of class {pid}")
        self._reserve(self._n + n, images.device)
        operand.copy_rows(self._t16, self._n * P, f16, n * P, self._pid)
        if self.has_match_summaries:       # straight into the rows' place, while the fp32 features still exist
            hip_ops.match_view_sums(feats, images.contiguous(), self.match_threshold, self._msums[self._n:self._n + n],
                                    self._mcounts[self._n:self._n + n])
        if self.has_entry_tokens:          # straight into the rows' place too, from the encoder's tagged output
            for i in range(0, n, self.ENTRY_CHUNK):
                j = min(n, i + self.ENTRY_CHUNK)
                # (a slice of the tagged features carries no operand copy: the whole output goes in when one call covers it)
                self.decoder.entry_tokens(bbox_feat[i:j], feats if (i, j) == (0, n) else _slice_views(feats, i, j),
                                          out=self._x32[self._n + i:self._n + j])
        if self.keep_images:
            self._images.append((self._n, images))
            if self.has_entry_tokens:
                self._heat.append((self._n, bbox_feat))
        self._n += n

    def add(self, images: torch.Tensor, bbox_feat: torch.Tensor | None = None, poses: torch.Tensor | None = None) -> torch.Tensor:
        """images (R, 3, S, S) or (B, R, 3, S, S) in [0, 1] -> CPU int64 row ids of the same leading shape.  Earlier ids stay valid.
        bbox_feat: the views' corner heat maps, (R, 8, S, S) or (B, R, 8, S, S) -- required by a bank that keeps decoder-entry tokens
        (built with decoder=), refused by one that does not.  poses: the views' poses, (R, 4, 4) or (B, R, 4, 4) of any float dtype
        (kept as fp32) -- required by a bank that keeps poses (keep_poses=True), refused by one that does not."""
        if images.dim() not in (4, 5):
            raise ValueError(f"expected (R, 3, S, S) or (B, R, 3, S, S), got {tuple(images.shape)}")
        lead = tuple(images.shape[:-3])
        if self.has_poses and poses is None:
            raise ValueError("this reference bank keeps poses (it was built with keep_poses=True): add(images, poses=...) needs the "
                             "references' poses")
        if poses is not None and not self.has_poses:
            raise ValueError("poses given to a reference bank that keeps none: build it with RefFeatureBank(encoder, keep_poses=True)")
        if poses is not None and (not isinstance(poses, torch.Tensor) or not poses.dtype.is_floating_point
                                  or tuple(poses.shape) != lead + (4, 4)):
            raise ValueError(f"poses must be a float tensor of shape {lead + (4, 4)} for images {tuple(images.shape)}, got "
                             f"{tuple(poses.shape) if isinstance(poses, torch.Tensor) else type(poses).__name__}"
                             f"{' ' + str(poses.dtype) if isinstance(poses, torch.Tensor) else ''}")
        if self.has_entry_tokens and bbox_feat is None:
            raise ValueError("this reference bank keeps decoder-entry tokens (it was built with decoder=): add(images, bbox_feat=...) "
                             "needs the references' heat maps")
        if bbox_feat is not None and not self.has_entry_tokens:
            raise ValueError("bbox_feat given to a reference bank that keeps no decoder-entry tokens: build it with "
                             "RefFeatureBank(encoder, decoder=model.decoder)")
        if bbox_feat is not None and (tuple(bbox_feat.shape[:-3]) != lead or tuple(bbox_feat.shape[-3:]) != (8,) + tuple(images.shape[-2:])):
            raise ValueError(f"bbox_feat must be {lead + (8,) + tuple(images.shape[-2:])} for images {tuple(images.shape)}, got "
                             f"{tuple(bbox_feat.shape)}")
        flat = images.reshape(-1, *images.shape[-3:])
        heat = bbox_feat.reshape(-1, *bbox_feat.shape[-3:]) if bbox_feat is not None else None
        self.ensure_fresh()                                    # never append rows of a new encoder state to rows of an old one
        n0 = self._n
        if flat.shape[0]:
            keep = self.keep_images
            self._append(flat.clone() if keep else flat, None if heat is None else (heat.clone() if keep else heat.contiguous()))
            if poses is not None:
                self._poses[n0:self._n].copy_(poses.reshape(-1, 4, 4))
        return torch.arange(n0, self._n, dtype=torch.int64).reshape(lead)

    def ensure_fresh(self) -> bool:
        """Bring a stale bank up to the encoder's state.  Returns True when the rows were re-encoded.  RuntimeError when they cannot be."""
        if not self.is_stale():
            return False
        if not self.keep_images:
            raise RuntimeError("RefFeatureBank: the rows were encoded under another precision / promotion state of the encoder (the load-time "
                               "calibration ran, or calibrate.set_state was applied, after add()) and the bank kept no crops to re-encode "
                               "them from (keep_images=False): clear() and add() the references again")
        global _WARNED_STALE_BANK
        if not _WARNED_STALE_BANK:
            _WARNED_STALE_BANK = True
            warnings.warn("BoxDreamer HIP path: the reference bank was filled under another precision / promotion state of the encoder (the "
                          "load-time calibration ran, or calibrate.set_state was applied, after RefFeatureBank.add); re-encoding its rows "
                          "from the kept crops, once." + (" (An entry-token bank: or under other decoder weights / another promotion "
                          "state of the decoder; its entry rows are re-embedded from the kept heat maps.)" if self.has_entry_tokens else ""),
                          stacklevel=3)
        # the new store is built on the side and swapped in when every row is there: a re-encode that fails part-way (out of memory,
        # say) leaves the rows and the kept crops as they were, and the failure is what the caller sees
        new = RefFeatureBank(self.encoder, keep_images=True, match_threshold=self.match_threshold, decoder=self.decoder)
        heat = self._heat if self.has_entry_tokens else [(None, None)] * len(self._images)
        for (_, img), (_, hm) in zip(self._images, heat):      # in row order: ids are unchanged
            if self._zero_row == new._n:                       # the zero view keeps its row: zero features, its entry tokens re-made
                new._append_zero()
            new._append(img, hm)
        if self._zero_row == new._n:
            new._append_zero()
        # (the poses are no function of the encoder or the decoder: the store stays as it is, under the same row ids)
        for k in ("_zero_row", "_t16", "_cap", "_n", "_pid", "_P", "_C", "_stamp", "_images", "_msums", "_mcounts", "_x32", "_entry_stamp", "_entry_shape", "_heat"):
            setattr(self, k, getattr(new, k))
        self.refresh_count += 1
        return True

    def real_crops(self, images: torch.Tensor, rows, n: int) -> torch.Tensor:
        """images[:n] of a banked batch ((B, T, 3, S, S); `rows`: its validated host table) with every banked slot -- whose image is never
        read and may hold anything -- replaced by the crop the bank kept: what the precision self-check measures on.  Only those
        samples are sliced out and copied."""
        images = images[:n]
        banked = [(b, t, rows[b][t]) for b in range(images.shape[0]) for t in range(images.shape[1]) if rows[b][t] >= 0]
        if banked:
            if not self.keep_images:
                raise RuntimeError("the precision self-check needs the reference crops of the samples it measures on, and the reference "
                                   "bank kept none (keep_images=False): run model.calibrate(data) on a batch with real images (or one "
                                   "plain forward) first")
            images = images.clone()
            for b, t, r in banked:
                images[b, t] = self.image_of(r).to(images.dtype)
        return images

    def real_heatmaps(self, rows, n: int, like: torch.Tensor) -> torch.Tensor:
        """(n, T, 8, S, S) heat maps that go with real_crops' images `like` (n, T, 3, S, S) in the precision self-check of an entry-token
        bank's batch: every banked slot holds the heat maps the bank kept, in their dtype; the other slots -- the queries, whose heat
        maps no decoder reads (their token rows are the query token's) -- hold zeros, whatever the batch dict has there."""
        if not self.keep_images:
            raise RuntimeError("the precision self-check needs the reference heat maps of the samples it measures on, and the reference "
                               "bank kept none (keep_images=False): run model.calibrate(data) on a batch with real images (or one "
                               "plain forward) first")
        t = like.shape[1]
        dtype = self._heat[0][1].dtype if self._heat else like.dtype
        out = torch.zeros((n, t, 8) + tuple(like.shape[-2:]), dtype=dtype, device=like.device)
        for b in range(n):
            for s in range(t):
                if rows[b][s] >= 0:
                    out[b, s] = self.heatmaps_of(rows[b][s]).to(out.device)
        return out

    def heatmaps_of(self, row: int) -> torch.Tensor:
        """The kept heat maps of a row (8, S, S) (keep_images=True, an entry-token bank)."""
        for r0, hm in self._heat:
            if r0 <= row < r0 + hm.shape[0]:
                return hm[row - r0]
        raise KeyError(f"row {row}: no heat maps kept")

    def image_of(self, row: int) -> torch.Tensor:
        """The kept crop of a row (3, S, S) (keep_images=True)."""
        for r0, img in self._images:
            if r0 <= row < r0 + img.shape[0]:
                return img[row - r0]
        raise KeyError(f"row {row}: no crop kept")

    def tables(self, rows, counts, t_max: int, dev):
        """(src int32 [n_views], encode index int64 [n_fresh] or None, n_fresh) on `dev` for a validated host table: built on the host,
        uploaded once per distinct (rows of the valid slots, counts, T_max) and kept, like BETR.ragged_index."""
        key = (tuple(tuple(r[:c]) for r, c in zip(rows, counts)), tuple(counts), int(t_max), str(dev))
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= 64:
                self._tables.clear()
            src, encode = _lib.gather_sources(rows, counts, t_max)
            hit = (torch.tensor(src, dtype=torch.int32).to(dev),
                   torch.tensor(encode, dtype=torch.int64).to(dev) if encode else None, len(encode))
            self._tables[key] = hit
        return hit

    def dense_tables(self, ref_rows, n_refs, n_max: int, query, t_max: int, dev):
        """(rows int32 [B, N_max], n_refs int32 [B], query int64 [B], flat slot of every query int64 [B]) on `dev` for the host tables of
        _lib.dense_bank_tables: uploaded once per distinct table and kept, like tables()."""
        key = (tuple(tuple(r[:n]) for r, n in zip(ref_rows, n_refs)), tuple(query), int(n_max), int(t_max), str(dev))
        hit = self._dense_tables.get(key)
        if hit is None:
            if len(self._dense_tables) >= 64:
                self._dense_tables.clear()
            B = len(n_refs)
            hit = (torch.tensor(ref_rows, dtype=torch.int32).reshape(B, n_max).to(dev), torch.tensor(n_refs, dtype=torch.int32).to(dev),
                   torch.tensor(query, dtype=torch.int64).to(dev), torch.tensor([b * t_max + q for b, q in enumerate(query)], dtype=torch.int64).to(dev))
            self._dense_tables[key] = hit
        return hit

    def select(self, fresh: torch.Tensor, images: torch.Tensor, rows: torch.Tensor, n_refs: torch.Tensor, topk: int):
        """Dense-reference selection among banked rows: `fresh` (B, P, C) the encoder's output for the B query crops `images`
        (B, 3, S, S); rows / n_refs: dense_tables().  Two launches (bd_match_view_sums on the queries, bd_match_select_rows) ->
        (scores fp32 (B, N_max), sel int32 (B, topk) selected slots in ascending order, src int32 (B (topk + 1),): gather()'s source
        table of the (B, topk + 1) batch, the query last)."""
        if not self.has_match_summaries:
            raise ValueError("the reference bank keeps no match summaries: build it with RefFeatureBank(encoder, match_threshold=0.05)")
        if self._n == 0:
            raise ValueError("nothing to select from: the bank is empty")
        q_sums, q_counts = hip_ops.match_view_sums(fresh, images.contiguous(), self.match_threshold)
        return hip_ops.match_select_rows(self._msums, self._mcounts, self._n, q_sums, q_counts, rows, n_refs, self._P, topk)

    def gather(self, src: torch.Tensor, fresh, lead) -> "features.OperandOnly":
        """One bd_gather_view_rows launch: the operand of len(src) views from bank rows and `fresh` (the encoder's tagged output for
        the views encoded in this forward, or None) -> features.OperandOnly of the logical shape (*lead, P, C); `lead` is (B, T) for a
        uniform batch, (n_views,) for a packed ragged one."""
        n_views = int(src.numel())
        lead = tuple(int(x) for x in lead)
        if len(lead) not in (1, 2) or (lead[0] * lead[1] if len(lead) == 2 else lead[0]) != n_views:
            raise ValueError(f"src names {n_views} views, the leading shape {lead} does not")
        n_fresh, f16 = 0, None
        pid, P, C = self._pid, self._P, self._C
        if fresh is not None:
            f16, fpid = features.require_tag(fresh)
            n_fresh = int(fresh.shape[0])
            if pid is None:                                    # an empty bank: every view is fresh
                pid, P, C = _lib.operand_prec(fpid), int(fresh.shape[1]), int(fresh.shape[2])
            elif (_lib.operand_prec(fpid), tuple(fresh.shape[1:])) != (pid, (P, C)) or features.stamp_of(fresh) != self._stamp[0]:
                raise ValueError("the freshly encoded views and the bank's rows differ in operand class, shape or encoder state")
        if pid is None:
            raise ValueError("nothing to gather: the bank is empty and no view was encoded")
        out16 = operand.empty(pid, n_views * P, C, src.device)
        # (the plane offsets default to each tensor's own: the bank's is its capacity, operand.plane_offset)
        hip_ops.gather_view_rows(self._t16 if self._n else None, self._n, f16, n_fresh, src, out16, n_views, P, C, prec=pid)
        stamp = self._stamp[0] if self._stamp is not None else features.stamp_of(fresh)
        return features.OperandOnly(lead + (P, C), out16, pid, stamp)


def _slice_views(feats: torch.Tensor, i: int, j: int) -> torch.Tensor:
    """Views [i, j) of the encoder's tagged (N, P, C) output, with the same rows of its operand copy attached."""
    f16, pid = features.require_tag(feats)
    n, P, C = feats.shape
    out16 = operand.empty(pid, (j - i) * P, C, feats.device)
    for dst, src in zip(operand.row_planes(out16, pid, (j - i) * P), operand.row_planes(f16, pid, n * P)):
        dst.copy_(src[i * P:j * P])
    return features.attach(feats[i:j].contiguous(), out16, pid, features.stamp_of(feats))


def merge_cached_features(encoder, images: torch.Tensor, cached: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """Encode only the views with valid == False and write them into (a copy of) the cached layout.  `merge_cached_features.last_stale`
    says whether THIS call fell back to encoding every view (the facade records it per forward in data["hip_precision"]["cache_stale"]:
    the warning fires once per process, the fallback every time)."""
    B, T = images.shape[:2]
    f16, pid = features.require_tag(cached)
    stamp, now = features.stamp_of(cached), encoder.model.state_stamp(encoder.prec)
    # (a missing stamp -- an older producer, or a tag lost through .to() / .clone() -- counts as stale whenever the encoder's state carries
    # a promotion: such features cannot be told apart from ones computed under another state)
    promoted_now = any(getattr(encoder.model, "promote", ())) or bool(getattr(encoder.model, "promote_misc", 0))
    merge_cached_features.last_stale = bool((stamp is not None and stamp != now) or (stamp is None and promoted_now))
    if merge_cached_features.last_stale:
        global _WARNED_STALE
        if not _WARNED_STALE:
            _WARNED_STALE = True
            warnings.warn("BoxDreamer HIP path: the cached reference features were encoded under another precision / promotion state of the "
                          "encoder (the load-time calibration ran, or calibrate.set_state was applied, after RefFeatureCache.encode); "
                          "encoding every view afresh.  Re-encode the references after the first forward to keep the cache's saving.",
                          stacklevel=2)
        return encoder.predict(images)
    miss = ~valid
    new = encoder.predict(images[miss])                       # (n_miss, P, C), tagged
    n16, npid = features.require_tag(new)
    if npid != pid:
        raise ValueError("cached features were produced in a different precision mode")
    P, C = cached.shape[2:]
    out32 = cached.clone()
    out32[miss] = new
    out16 = f16.clone()
    n_miss = int(new.shape[0])
    for dst, src in zip(operand.row_planes(out16, pid, B * T * P), operand.row_planes(n16, pid, n_miss * P)):
        dst.reshape(B, T, P, C)[miss] = src.reshape(n_miss, P, C)
    return features.attach(out32, out16, pid, now)


_init_last_stale()
