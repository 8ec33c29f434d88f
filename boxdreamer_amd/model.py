"""Model facade: `BoxDreamer(config).forward(data: dict) -> dict`, the drop-in boundary
(/root/reference/src/models/BoxDreamerModel.py:21-384).  Same constructor input (`config["modules"]`),
same batch-dict keys in and out, same `decoder.*` state_dict, same encoder-plugin API -- the internals call
the gfx950 HIP library.  Only the released configuration (dino encoder, bb8 / heatmap) is implemented;
tracker / matcher / plucker rays are out of the hot path and raise; the dense-reference mode ("next" row
f4) is wired through boxdreamer_amd/dense.py.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple

import torch
import torch.nn as nn

from .betr import BETR
from . import _lib, calibrate, features, pnp
from .box_utils import recover_bb8_corners_chw, solve_poses_device, solve_poses_host
from .cache import merge_cached_features
from .config import setup_camera_params, validate_model_config
from .dense import _get, filter_by_view_index, process_dense_input, process_multi_round, process_multi_round_bank
from .encoder import DinoV2Wrapper


# What `BoxDreamer._plan` knows about one batch before any launch, host values only.  mode: the step that runs it ("graph", "banked_dense",
# "entry_bank" or "eager").  counts: a ragged batch's validated view_counts, None: the uniform batch; views_per_sample: counts, or T for
# every sample.  query_idx: host ints, or None: it lives on the device and is checked there.  bank / rows: the cache.RefFeatureBank and its
# validated host table (-1: encode this slot); entry: it keeps decoder-entry tokens (no heat map is read, bbox_feat may be absent), and
# entry_query is the table's query slot per sample.  The last five, the banked dense mode's (_lib.dense_bank_tables; k = filter_topk).
_Batch = namedtuple("_Batch", "mode B T counts views_per_sample query_idx dense multi_round bank rows entry entry_query "
                              "ref_rows n_refs n_max query k", defaults=(None,) * 5)

# What one mode's step hands to forward's common tail.  heat: the decoder's output for the query views (None: coarse prediction only, the
# dict is already written); qi, ar: query slot per sample and arange(B), after any re-pack of the dict; record: this forward's entries of
# data["hip_precision"]; decoded: (normalised, pixel) corners where the step decoded them itself (the graph); slots: device slots that
# travel with the corners' D2H (original_images is re-packed by them); bad: a 0-dim device verdict on query_idx, deferred to that D2H.
_Out = namedtuple("_Out", "heat qi ar record decoded slots bad", defaults=(None,) * 3)


def _host_query(query_idx):
    """query_idx as host ints when it lives on the host (absent or a device tensor: None -- that one is checked on the device)."""
    if isinstance(query_idx, torch.Tensor):
        return None if query_idx.is_cuda else query_idx.reshape(-1).tolist()
    return None if query_idx is None else list(query_idx)


def _cut(flat, fields):
    """{name: its view} of a flat host array that holds the ordered `fields` (name, shape) back to back."""
    views, at = {}, 0
    for name, shape in fields:
        views[name] = flat[at:at + math.prod(shape)].reshape(shape)
        at += math.prod(shape)
    return views


class BoxDreamer(nn.Module):
    """BoxDreamer model for predicting 3D object poses from multiple images (MI355X inference path)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        module_configs = dict(config["modules"])
        self.use_matching = module_configs["use_matching"]
        self.use_tracking = module_configs["use_tracking"]
        self.use_keypoints = module_configs["use_keypoints"]
        self.use_rgb = module_configs["use_rgb"]
        self.use_pp = module_configs["use_pp"]
        self.regression_intri = module_configs["regression_intri"]
        self.roatation_type = module_configs["rotation_type"]
        self.coordinate = module_configs["coordinate"]
        self.pose_representation = module_configs["pose_representation"]
        self.image_size = module_configs["decoder"]["img_size"]
        self.patch_size = module_configs["decoder"]["patch_size"]
        self.patchify_rays = module_configs["patchify_rays"]
        module_configs = validate_model_config(module_configs)
        self.bbox_representation = module_configs["bbox_representation"]
        self.dense_cfg = module_configs.get("dense_cfg", None)
        # False: host PnP (the default); True: bd_solve_pnp (one pose per thread); "wave": bd_solve_pnp_wave (one wavefront per pose)
        self.pnp_on_device = module_configs.get("pnp_on_device", False)
        if isinstance(self.pnp_on_device, str):
            if self.pnp_on_device != "wave":
                raise ValueError(f"config['modules']['pnp_on_device'] must be False, True or 'wave', got {self.pnp_on_device!r}")
        else:
            self.pnp_on_device = bool(self.pnp_on_device)
        module_configs, self.camera_dim, self.rotation_length = setup_camera_params(module_configs)
        self.module_configs = module_configs

        if self.use_tracking:
            raise NotImplementedError("Tracking is not supported yet")            # BoxDreamerModel.py:74-75
        if self.use_matching:
            raise NotImplementedError("LoFTR matching is outside the MI355X hot path")
        if self.pose_representation != "bb8" or self.roatation_type is not None:
            raise NotImplementedError("only pose_representation='bb8' (rotation_type null) is on the hot path")
        self.tracker = None
        self.matcher = None
        if self.use_rgb:
            name = module_configs["encoder"]["name"]
            if name != "dino":
                raise NotImplementedError(f"encoder '{name}' is not used by the released checkpoint; only 'dino'")
            dino = module_configs["encoder"]["dino"]
            self.rgb_encoder = DinoV2Wrapper(_get(dino, "ckpt_path"), dict(_get(dino, "cfg") or {}))
        else:
            raise NotImplementedError("use_rgb=False (from-scratch embeddings) is outside the hot path")
        dec_cfg = {k: v for k, v in dict(module_configs["decoder"]).items()}
        self.decoder = BETR(**dec_cfg)
        # Load-time self-check of the precision mode (boxdreamer_amd/calibrate.py): on the first forward the default mode is measured
        # against the most precise GPU mode on that batch's first sample and the Linears that need it are promoted to split-f16, so
        # that a real checkpoint's outlier channels cannot silently cost the 1e-3 parity bar.  `hip_calibrate: false` in
        # config["modules"] only measures and warns.  Re-armed whenever the decoder weights change (a checkpoint load).
        self.hip_calibrate = bool(module_configs.get("hip_calibrate", True))
        # optional: a JSON file that keeps the measured promotion state next to the checkpoint (stamped with a content fingerprint of
        # both weight sets): the first process measures and writes it, later ones load it instead of re-measuring
        self.hip_promotion_file = module_configs.get("hip_promotion_file", None)
        self._calibrated_for = None
        self._ranks_synced_for = None
        self._pending_save = False
        self.hip_precision_source = ("config" if "hip_precision" in dec_cfg else
                                     ("$BOXDREAMER_HIP_PREC" if "BOXDREAMER_HIP_PREC" in os.environ else "package default"))
        # `hip_graph: true` in config["modules"]: the plain path (no dense mode, no cached features) of an eval forward is captured as ONE
        # HIP graph per batch shape on first use and replayed afterwards (boxdreamer_amd/graph.py: ~300 launches per step; bit-identical
        # outputs, tests/test_gpu_facade.py).  One graph is kept: a new batch shape drops it and captures again.
        self.hip_graph = bool(module_configs.get("hip_graph", False))
        self._graph, self._graph_key = None, None
        # `hip_latency: true` in config["modules"]: opt into the latency forms for calls of one or two poses (the reference demo's per-frame
        # call, src/demo/demo.py:1501-1514): the residual Linears run split-K (bd_*_weights.latency_mode, ABI 9) -- one pose 4.6 -> 3.6 ms.
        # Deterministic and within the mode's tolerance, but a sample's bits then differ from the same sample inside a larger batch; off
        # by default, so that every row stays bit-identical across batch sizes, lanes and launch forms.
        if "hip_latency" in module_configs:
            self.decoder.hip_latency = bool(module_configs["hip_latency"])
            if hasattr(self.rgb_encoder, "model"):
                self.rgb_encoder.model.latency = bool(module_configs["hip_latency"])
        self.decoder.validate_inputs = "deferred"      # the one-hot check of camera_mask travels with the corners' D2H (no sync of its own)
        self.host_syncs_per_forward = None             # filled by forward(): what still waits for the device, for the record
        self._pose_pin = None
        self._d2h_pin, self._d2h_done = None, None
        self._aranges, self._query_tables = {}, {}

    def calibrate(self, data, plan=None) -> dict:
        """Run the precision self-check / promotion on (the first samples of) a batch dict now (forward() does it once by itself, and hands
        over the plan it made of the batch)."""
        images = data["images"]
        B, T = images.shape[:2]
        plan = self._plan(data, B, T) if plan is None else plan
        mask = torch.zeros((B, T), dtype=torch.bool, device=images.device)
        mask[torch.arange(B, device=images.device), data["query_idx"].to(images.device).long()] = True
        bank, counts = plan.bank, plan.counts
        bbox_feat = data.get("bbox_feat")                                      # (an entry-token bank's batch needs none)
        if counts is not None:       # ragged batch: the first sample with its own view count (its padded slots are never read)
            images, mask = images[:1, :counts[0]], mask[:1, :counts[0]]
            bbox_feat = bbox_feat[:1, :counts[0]] if bbox_feat is not None else None
        if bank is not None:
            # a banked batch: every sample the self-check measures on takes its references from the crops the bank kept (and, an
            # entry-token bank's, their heat maps from the ones it kept: the batch's own are never read and may be absent)
            n = min(calibrate.MAX_SAMPLES, images.shape[0])
            images, mask = bank.real_crops(images, plan.rows, n), mask[:n]
            bbox_feat = bank.real_heatmaps(plan.rows, n, images) if plan.entry else bbox_feat[:n]
        if images.device != self.rgb_encoder.get_device():
            self.rgb_encoder.to_device(images.device)
        if self.hip_promotion_file and self.hip_calibrate and calibrate.load_state(self.hip_promotion_file, self.rgb_encoder, self.decoder):
            self._calibrated_for = self.decoder._signature()
            return self.decoder.hip_calibration
        rep = calibrate.calibrate(self.rgb_encoder, self.decoder, images, bbox_feat, mask, promote=self.hip_calibrate)
        self._calibrated_for = self.decoder._signature()
        # (no collective in here: an explicit model.calibrate(data) on ONE rank must not wait for the others.  forward() adopts rank 0's
        # state in one place that every rank reaches, _sync_ranks_once, and rank 0 writes the promotion file there)
        self._pending_save = bool(self.hip_promotion_file and self.hip_calibrate and rep.get("applicable"))
        if self._pending_save and not self._multi_rank():
            calibrate.save_state(self.hip_promotion_file, self.rgb_encoder, self.decoder, rep)
            self._pending_save = False
        return rep

    @staticmethod
    def _multi_rank() -> bool:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _sync_ranks_once(self, failure: str | None = None) -> None:
        """One process per GPU: every rank measured (or loaded, or was handed) a promotion state on its own; rank 0's is the one all
        ranks run (same bits for the same sample on every rank).  Called from ONE place in forward(), after the calibrate / mark_calibrated
        branches, once per decoder signature: every rank reaches it whichever branch it took; a rank-0 failure is broadcast instead of a
        state, so the others raise instead of hanging.  Only rank 0 writes the promotion file."""
        import torch.distributed as dist
        sig = self.decoder._signature()
        if self._ranks_synced_for == sig or not self._multi_rank():
            self._ranks_synced_for = sig
            return
        if failure is not None:
            calibrate.broadcast_failure(failure)
            return
        if calibrate.sync_state_across_ranks(self.rgb_encoder, self.decoder):
            rep = dict(self.decoder.hip_calibration or {}, state=calibrate.get_state(self.rgb_encoder, self.decoder), synced_from_rank=0)
            # this rank's own measurement no longer describes the state it runs: say so instead of reporting its numbers
            for k in ("promoted", "delta_final", "ok"):
                rep[k] = None if k != "promoted" else []
            rep["measured_here"] = False
            self.decoder.hip_calibration = rep
            self._calibrated_for = self.decoder._signature()
        if getattr(self, "_pending_save", False) and dist.get_rank() == 0:
            calibrate.save_state(self.hip_promotion_file, self.rgb_encoder, self.decoder, self.decoder.hip_calibration or {})
        self._pending_save = False
        self._ranks_synced_for = sig

    @staticmethod
    def _view_counts(data, B: int, T: int):
        """The optional batch-dict key `view_counts` (a list or a CPU int tensor, one entry per sample: the sample's valid views are the
        slots [0, count) of its T_max = T slots) as validated host ints -- or None when the key is absent or every count equals T, which
        IS the uniform batch.  A device tensor raises TypeError (reading it would add a host sync per forward); counts outside [2, T] or
        a host-side `query_idx` that is not among the sample's views raise ValueError (a device-side `query_idx` is checked on the
        device and reported with the corners' D2H, like the one-hot check of camera_mask)."""
        if data.get("view_counts") is None:
            return None
        counts = _lib.view_counts_list(data["view_counts"], B)
        _lib.check_view_counts(counts, T, _host_query(data.get("query_idx")))
        return None if all(c == T for c in counts) else counts

    def _arange(self, n: int, dev) -> torch.Tensor:
        """arange(n) on `dev`, kept (read-only use): the host time between two batches is device idle time in an eval forward."""
        key = (int(n), str(dev))
        t = self._aranges.get(key)
        if t is None:
            t = self._aranges[key] = torch.arange(n, device=dev)
        return t

    def mark_calibrated(self) -> None:
        """Keep the promotion state that is in place (applied through `calibrate.set_state` / `calibrate.load_state`): the first forward
        will not measure and replace it."""
        self._calibrated_for = self.decoder._signature()

    def _precision_record(self) -> dict:
        rep = self.decoder.hip_calibration or {}
        return {"decoder": str(self.decoder.hip_precision), "encoder": str(self.rgb_encoder.prec), "source": self.hip_precision_source,
                "calibrated": bool(rep.get("applicable")), "promoted_units": len(rep.get("promoted", [])),
                "self_check_max_abs_dlogits": rep.get("delta_final"), "self_check_unpromoted": rep.get("delta_unpromoted"),
                "self_check_budget": rep.get("budget"), "self_check_ok": rep.get("ok")}

    def _images_from_frames(self, data) -> torch.Tensor:
        """`data["images"]` from raw frames (boxdreamer_amd/preprocess.py): uint8 `frames` [F, H, W, 3] + int32 `crop_boxes` [B, T, 4] on the
        device, optionally `frame_idx` [B, T] (default: view i reads frame i), `keep_boxes` [B, T, 4] (background masking),
        `frame_format` (the frames' layout when it is not packed RGB: "bgr", "rgba", "bgra", "nv12", or a dict) and `crop_size` (224) ->[B, T, 3, S, S] in bbox_feat's dtype, ONE launch on the current stream.  With `hip_graph` the launch stays
        outside the captured graph and writes straight into the graph's static image buffer when one exists for the shape (the replay's
        input copy of that tensor onto itself is a no-op); `data["images"]` then aliases that buffer until the next forward."""
        from .preprocess import crop_resize_frames, resolve_format
        missing = [k for k in ("frames", "crop_boxes") if k not in data]
        if missing:
            raise KeyError(f"the batch dict needs 'images', or 'frames' + 'crop_boxes' to make them on the device (missing: {missing})")
        boxes = data["crop_boxes"]
        if boxes.dim() != 3 or boxes.shape[-1] != 4:
            raise ValueError(f"crop_boxes must be int32 [B, T, 4], got {tuple(boxes.shape)}")
        B, T = boxes.shape[:2]
        S = int(data.get("crop_size", 224))
        feat = data.get("bbox_feat")
        dtype = feat.dtype if isinstance(feat, torch.Tensor) and feat.dtype.is_floating_point else torch.float32
        out = None
        g = self._graph if self.hip_graph else None
        if (g is not None and tuple(g.images.shape) == (B, T, 3, S, S) and g.images.dtype == dtype
                and g.images.device == data["frames"].device):
            out = g.images
        # `frame_format` (absent: packed RGB, the call as it was): a name, or a dict frame_format / colorspace / range, of the layout
        # the frames arrive in (preprocess.resolve_format); the kernel converts the pixels under the crops as it stages them
        fmt = {} if data.get("frame_format") is None else {"frame_format": resolve_format(data["frame_format"])}
        return crop_resize_frames(data["frames"], boxes, frame_idx=data.get("frame_idx"), keep_boxes=data.get("keep_boxes"),
                                  out_size=S, out=out, dtype=dtype, **fmt)

    def forward(self, data):
        if "images" not in data:      # opt-in: raw uint8 frames + crop windows in place of the dataset's float crops
            data["images"] = self._images_from_frames(data)
        images = data["images"]
        B, T = images.shape[:2]
        plan = self._plan(data, B, T)           # every refusal that needs no device, and the batch's mode
        # (a comparison on the device: an indexed assignment of the Python scalar True uploads it first -- a synchronising copy)
        dev = images.device
        qi = data["query_idx"].to(dev).long()
        camera_mask = self._arange(T, dev)[None, :] == qi[:, None]
        data["camera_mask"] = camera_mask.clone()
        sig = self._settle_precision(data, plan)
        step = {"graph": self._step_graph, "banked_dense": self._step_banked_dense, "entry_bank": self._step_entry_bank,
                "eager": self._step_eager}[plan.mode]
        out = step(data, plan, qi, self._arange(B, dev), camera_mask, sig)
        self._defer(out.bad)
        if sig is not None:
            data["hip_precision"].update(out.record)
        syncs = []
        if out.heat is None:        # coarse prediction only (dense_cfg.multi_round without fine_level): the dict is final, nothing is read back
            if plan.mode == "banked_dense":     # (the un-banked mirror of the reference leaves host_syncs_per_forward as the last forward did)
                if out.slots is not None:
                    self._repack_original_images(data, plan.query, out.slots, None, syncs)
                self.host_syncs_per_forward = syncs
            return data

        # BoxDreamerModel.py:341-344 (`pred_bbox[camera_mask] = query_ret`): the same write through (sample, view) indices -- a boolean-mask
        # assignment runs nonzero() and waits for the device.  In eval the copy (the largest device operation of the dict contract: bbox_feat's
        # 154 MB at configs[1]) is enqueued BEHIND the corners' D2H, so that the device has it to do while the host solves the poses.
        # Over an entry-token bank `bbox_feat` may be absent: nothing to clone, the decoder's output goes out as `pred_query_bbox`.
        def write_pred_bbox():
            if "bbox_feat" not in data:
                data["pred_query_bbox"] = out.heat
                return
            data["pred_bbox"] = data["bbox_feat"].clone()
            data["pred_bbox"][out.ar, out.qi] = out.heat.to(data["pred_bbox"].dtype)

        pred_poses, slots_host = data["poses"].clone(), None
        if not self.training:
            pred_poses, slots_host = self._process_evaluation(pred_poses, data, out, syncs, write_pred_bbox)
        else:
            write_pred_bbox()
        if out.slots is not None:
            self._repack_original_images(data, plan.query, out.slots, slots_host, syncs)
        data["pred_poses"] = pred_poses
        data["pred_intrinsics"] = data["intrinsics"]
        self.host_syncs_per_forward = syncs
        return data

    def _plan(self, data, B: int, T: int) -> _Batch:
        """One batch on the host, before any launch: every refusal that needs no device, in one order (view_counts, the mode, bbox_feat,
        the entry bank's table, the dense bank's table), then what the batch is and which of the four steps runs it."""
        images, query_idx = data["images"], data["query_idx"]
        counts = self._view_counts(data, B, T)
        views = counts if counts is not None else [T] * B
        dense = self.dense_cfg is not None and bool(_get(self.dense_cfg, "enable", False))
        multi_round = dense and bool(_get(self.dense_cfg, "multi_round", False))
        bank, rows = self._check_mode(data, counts, dense, multi_round)
        if bank is not None:
            rows = _lib.ref_rows_table(rows, B, T)
            _lib.check_ref_rows(rows, views, len(bank))
        entry = bank is not None and bank.has_entry_tokens
        if data.get("bbox_feat") is None and not entry:
            raise KeyError("bbox_feat")
        if entry and bank.decoder is not self.decoder:
            raise ValueError("ref_bank keeps the entry tokens of another decoder than this model's")
        # both tables name every reference by bank row and the query by its one -1; a host query_idx must agree with them (a device one is
        # compared on the device and reported with the corners' D2H)
        host_q = _host_query(query_idx)
        entry_query = _lib.entry_bank_queries(rows, views, host_q) if entry else None
        dense_plan = self._dense_bank_plan(bank, rows, views, host_q) if dense and bank is not None else ()
        # (a banked or a ragged batch takes an eager step -- capture of ragged shapes is a follow-up)
        graph = (self.hip_graph and bank is None and counts is None and not dense and "cached_rgb_feat" not in data and not self.training
                 and images.is_cuda and isinstance(self.decoder, BETR) and not torch.cuda.is_current_stream_capturing())
        mode = "graph" if graph else "banked_dense" if dense_plan else "entry_bank" if entry else "eager"
        return _Batch(mode, B, T, counts, views, host_q, dense, multi_round, bank, rows, entry, entry_query, *dense_plan)

    def _check_mode(self, data, counts, dense: bool, multi_round: bool):
        """One batch names its references ONE way: refuse, before any launch, the combinations that are not implemented.  Returns
        (cache.RefFeatureBank, the batch's table of its rows as given), or (None, None) without a bank."""
        bank, rows = data.get("ref_bank"), data.get("ref_rows")
        ragged, banked, cached, betr = counts is not None, bank is not None or rows is not None, "cached_rgb_feat" in data, isinstance(self.decoder, BETR)
        if ragged and cached:
            raise NotImplementedError("view_counts together with cached_rgb_feat (ragged feature cache) is not implemented")
        if ragged and dense and not banked:
            raise NotImplementedError("view_counts together with dense_cfg.enable needs a ref_bank: the ragged dense-reference mode is "
                                      "implemented over the reference bank only")
        if ragged and not betr:
            raise NotImplementedError("view_counts needs the BETR decoder")
        if banked and multi_round and not getattr(bank, "has_poses", False):
            raise NotImplementedError("ref_bank together with dense_cfg.multi_round (multi-round decode over the bank) needs a bank that "
                                      "keeps its views' poses: build it with RefFeatureBank(..., keep_poses=True) and add(..., poses=...)")
        if banked and dense and not (_get(self.dense_cfg, "filter") == "dino" and _get(self.dense_cfg, "filter_enable")):
            raise NotImplementedError("ref_bank together with dense_cfg.enable is implemented for the DINO filter only "
                                      "(dense_cfg.filter = 'dino' with dense_cfg.filter_enable)")
        if banked and cached:
            raise NotImplementedError("ref_bank together with cached_rgb_feat: give the references one way or the other")
        if banked and not betr:
            raise NotImplementedError("ref_bank needs the BETR decoder")
        if banked and (bank is None or rows is None):
            raise KeyError("the batch dict needs both 'ref_bank' (a cache.RefFeatureBank) and 'ref_rows' (its (B, T_max) host table)")
        if banked and bank.encoder is not self.rgb_encoder:
            raise ValueError("ref_bank was built on another encoder than this model's rgb_encoder")
        return (bank, rows) if banked else (None, None)

    def _dense_bank_plan(self, bank, rows, views, host_q):
        """Host side of the banked dense-reference mode: (reference rows [B][N_max], n_refs, N_max, query slot per sample, k), _Batch's
        last five fields."""
        if not bank.has_match_summaries:
            raise ValueError("dense_cfg.enable with a ref_bank needs the bank's match summaries: build it with "
                             "RefFeatureBank(encoder, match_threshold=0.05)")
        k = int(_get(self.dense_cfg, "filter_topk"))
        return _lib.dense_bank_tables(rows, views, k, host_q) + (k,)

    def _settle_precision(self, data, plan: _Batch):
        """Before the first launch of a forward: the encoder on the batch's device, the load-time self-check once per decoder signature,
        rank 0's state on every rank, data["hip_precision"].  Returns the decoder's signature (None: a test's stub decoder)."""
        images = data["images"]
        if images.device != self.rgb_encoder.get_device():
            self.rgb_encoder.to_device(images.device)                            # BoxDreamerModel.py:279-282
        if not isinstance(self.decoder, BETR):     # (tests swap the decoder for a stub: nothing to check then)
            return None
        sig = self.decoder._signature()            # (walks every parameter: computed once per forward and handed on)
        if (self._calibrated_for != sig and images.is_cuda and not torch.cuda.is_current_stream_capturing()
                and calibrate.applicable(self.rgb_encoder, self.decoder)):
            if self._calibrated_for is None and calibrate.has_state(self.rgb_encoder, self.decoder):
                self.mark_calibrated()       # a state the caller applied before the first forward is kept, not measured over
            else:
                try:
                    self.calibrate(data, plan)
                except Exception as e:       # noqa: BLE001 -- tell the other ranks before re-raising (they wait in _sync_ranks_once)
                    self._sync_ranks_once(failure=f"{type(e).__name__}: {e}")
                    raise
        if images.is_cuda and not torch.cuda.is_current_stream_capturing():
            self._sync_ranks_once()
        data["hip_precision"] = self._precision_record()
        return sig

    # ---- one step per mode: (data, plan, qi, arange(B), camera_mask, the decoder's signature) -> _Out
    def _step_graph(self, data, plan, qi, ar, camera_mask, sig) -> _Out:
        """The plain uniform batch under `hip_graph`: encoder -> decoder -> corner decode replayed as one captured graph."""
        heat, kp_px, kn, _ = self._graphed(data["images"], data["bbox_feat"], qi, sig)
        self.decoder.mask_error = None          # query_idx indexes one view per sample by construction
        # (static buffers the next replay overwrites: pred_bbox's query slot is written straight from the heat map, the corners are copied)
        return _Out(heat, qi, ar, self._lanes_record(plan.B, plan.T, None), decoded=(kn.clone(), kp_px.clone()))

    def _step_banked_dense(self, data, plan, qi, ar, camera_mask, sig) -> _Out:
        """Dense-reference mode over the bank: the query is the one view encoded, the references are scored and selected among the bank's
        rows; the decoder runs on the uniform (B, k + 1) batch in rounds, from the bank's entry rows, or on the gathered features."""
        bank, slots_key = plan.bank, "dense_ref_slots"
        feats, record, idx, bad = self._banked_dense_features(data, plan, qi)
        qi = filter_by_view_index(data, idx, ar)
        images, camera_mask = data["images"], data["camera_mask"]
        if plan.multi_round:
            # (feats: the queries' encoder output and the bank-row table of the selection, on the device)
            heat, fine_qi = process_multi_round_bank(data, bank, feats[0], feats[1], data["dense_ref_slots"], ar, self.decoder,
                                                     self.dense_cfg, pnp_on_device=self.pnp_on_device)
            if heat is not None:        # a fine level ran: the original slots of ITS choice -- both selections composed
                qi, slots_key = fine_qi, "dense_fine_slots"
        elif plan.entry:     # (feats: the queries' encoder output and the source table bd_match_select_rows wrote)
            heat = self.decoder.forward_entry(bank.entry_tokens, len(bank), feats[1], feats[0], camera_mask, images.shape[-1])
        else:
            heat = self.decoder(data.get("bbox_feat"), images, camera_mask, feats, None)
        # the selected slots travel with the corners' D2H when the host needs them (original_images is a host list)
        return _Out(heat, qi, ar, record, slots=data[slots_key] if "original_images" in data else None, bad=bad)

    def _step_entry_bank(self, data, plan, qi, ar, camera_mask, sig) -> _Out:
        """A plain banked batch, uniform or ragged, over an entry-token bank: the B query crops are the one thing encoded, BETR.forward_entry
        runs the adapter on their rows, assembles its token stream from the bank's entry rows (ONE bd_assemble_entry_tokens launch;
        bank.tables' source table) and runs the blocks.  No heat map, no image of a banked slot and no feature row of the bank is read."""
        images, bank = data["images"], plan.bank
        src, fresh, record = self._bank_sources(images, plan)
        heat = self.decoder.forward_entry(bank.entry_tokens, len(bank), src, fresh, camera_mask, images.shape[-1], view_counts=plan.counts)
        # (a device-side query_idx that is not the table's -1 slot -- a host one was checked in the plan)
        return _Out(heat, qi, ar, record, bad=(qi != self._query_table(plan.entry_query, qi.device)).any() if plan.query_idx is None else None)

    def _step_eager(self, data, plan, qi, ar, camera_mask, sig) -> _Out:
        """Everything else: the features from the ONE source the batch names (_eager_features), then the decoder -- once, or as the
        un-banked dense mode's mirror of the reference runs it (boxdreamer_amd/dense.py)."""
        images, pose_feat, bad = data["images"], data["bbox_feat"], None
        rgb_feature, record = self._eager_features(data, images, plan)
        if plan.dense:     # BoxDreamerModel.py:291-327
            data, pose_feat, images, camera_mask, rgb_feature, _ = process_dense_input(
                data, pose_feat, images, camera_mask, rgb_feature, None, self.dense_cfg)
            if plan.multi_round:
                heat = process_multi_round(data, pose_feat, images, camera_mask, rgb_feature, None, self.decoder,
                                           self.dense_cfg, self.bbox_representation, pnp_on_device=self.pnp_on_device)
            else:
                # .contiguous() returns a NEW tensor object when it has to copy; the operand-dtype copy of the features
                # follows only an alias of the same storage (features.carry), otherwise BETR re-casts explicitly
                heat = self.decoder(pose_feat.contiguous(), images.contiguous(), camera_mask,
                                    features.carry(rgb_feature, rgb_feature.contiguous()), None)
            if heat is not None:    # the dense helpers re-pack the batch dict: re-read the query position (BoxDreamerModel.py:150-158)
                ar, qi = torch.arange(data["images"].shape[0], device=qi.device), data["query_idx"].to(qi.device).long()
        elif plan.counts is None:
            heat = self.decoder(pose_feat, images, camera_mask, rgb_feature, None)
        else:       # (the keyword goes to a BETR only: _check_mode)
            heat = self.decoder(pose_feat, images, camera_mask, rgb_feature, None, view_counts=plan.counts)
            if plan.query_idx is None:      # a device-side query_idx: "is it one of the sample's views" (a host one was checked in the plan)
                view_start = self.decoder.ragged_index(plan.counts, plan.T, qi.device)[1]
                bad = (qi >= (view_start[1:] - view_start[:-1]).long()).any()
        return _Out(heat, qi, ar, record, bad=bad)

    def _defer(self, bad) -> None:
        """OR a 0-dim device verdict into the decoder's deferred mask verdict: it travels with the corners' D2H (no sync here)."""
        if bad is not None:
            err = self.decoder.mask_error
            self.decoder.mask_error = bad if err is None else (err | bad)

    def _query_table(self, query, dev) -> torch.Tensor:
        """A host table of query slots on `dev`, uploaded once per distinct table and kept."""
        key = (tuple(query), str(dev))
        q_d = self._query_tables.get(key)
        if q_d is None:
            if len(self._query_tables) >= 256:
                self._query_tables.clear()
            q_d = self._query_tables[key] = torch.tensor(query, dtype=torch.int64).to(dev)
        return q_d

    def _encode_slots(self, images, index):
        """(the encoder's output, the crops) of the (sample, view) slots of `images` (B, T, ...) that `index` names, flat: ONE predict call."""
        crops = images.reshape(images.shape[0] * images.shape[1], *images.shape[2:]).index_select(0, index)
        return self.rgb_encoder.predict(crops), crops

    @staticmethod
    def _bank_record(bank, refreshed, banked: int, encoded: int, **more) -> dict:
        """data["hip_precision"]["ref_bank"] of one forward over a bank."""
        return dict(banked_views=banked, encoded_views=encoded, refreshed=bool(refreshed), **more, **({"entry_tokens": True} if bank.has_entry_tokens else {}))

    def _bank_sources(self, images, plan: _Batch):
        """A plain banked batch: a stale bank is refreshed first (after the calibration: a bank filled before the first forward just works),
        then (the source table of its views, the encoder's output for the -1 slots among the valid views or None, this forward's record)."""
        bank, views = plan.bank, plan.views_per_sample
        refreshed = bank.ensure_fresh()
        src, encode, n_fresh = bank.tables(plan.rows, views, plan.T, images.device)
        fresh = self._encode_slots(images, encode)[0] if n_fresh else None
        record = self._lanes_record(plan.B, plan.T, plan.counts)
        record["ref_bank"] = self._bank_record(bank, refreshed, sum(views) - n_fresh, n_fresh)
        return src, fresh, record

    def _banked_dense_features(self, data, plan: _Batch, qi):
        """(features.OperandOnly of (B, k + 1, P, C), this forward's record, view indices (B, k + 1) of the kept views: the selected
        references in slot order, the query last; the verdict on a device-side query_idx or None).  The B query crops go through the
        encoder in ONE predict call; bd_match_view_sums summarises them, ONE bd_match_select_rows launch scores every reference against
        its query from the bank's summaries, picks the k best and writes the source table of ONE bd_gather_view_rows launch.  Images
        in banked slots are never read; nothing here waits for the device.  With dense_cfg.multi_round nothing is gathered here: the first
        item is (the queries' encoder output, the device table of bank rows per reference slot): dense.process_multi_round_bank's input."""
        bank, B, k, multi, images = plan.bank, plan.B, plan.k, plan.multi_round, data["images"]
        refreshed = bank.ensure_fresh()
        rows_d, n_refs_d, q_d, q_flat = bank.dense_tables(plan.ref_rows, plan.n_refs, plan.n_max, plan.query, plan.T, images.device)
        fresh, crops = self._encode_slots(images, q_flat)
        scores, sel, src = bank.select(fresh, crops, rows_d, n_refs_d, k)
        # (an entry-token bank: the decoder takes the source table itself, no feature row is gathered; multi-round: the rounds have a
        # source table of their own, bd_round_sources', made from the selection and the bank-row table)
        feats = (fresh, rows_d) if multi else (fresh, src) if plan.entry else bank.gather(src, fresh, (B, k + 1))
        data["dense_ref_slots"], data["dense_ref_scores"] = sel, scores
        sub = int(_get(self.dense_cfg, "sub_batch_size")) if multi else k
        rounds = (k + sub - 1) // sub
        at_once = 1 if multi and _get(self.dense_cfg, "dense_mem_friendly") else rounds      # rounds one decoder call covers
        record = self._lanes_record(B * at_once, sub + 1, None) if isinstance(self.decoder, BETR) else {}
        # (the zero views that pad a multi-round decode's last round are bank rows too, and are not counted as banked views)
        more = dict(rounds=rounds, padded_views=B * (rounds * sub - k)) if multi else {}
        record["ref_bank"] = self._bank_record(bank, refreshed, B * k, B, scored_views=sum(plan.n_refs), **more)
        ref = sel.long()
        ref = ref + (ref >= q_d[:, None]).long()                # reference slot -> view slot: the query's own slot is skipped
        return feats, record, torch.cat([ref, q_d[:, None]], dim=1), (qi != q_d).any() if plan.query_idx is None else None

    @staticmethod
    def _repack_original_images(data, query, slots, slots_host, syncs) -> None:
        """`original_images` ([T][B] host list) keeps the selected views, the query (slot `query[b]`) last (data_processing.py:150-176)
        -- on the host, from `slots_host`, the slots that came back with the corners' D2H (None: no such copy ran, one of their own)."""
        if slots_host is None:
            slots_host = slots.cpu().tolist()
            syncs.append(f"dense_ref_slots D2H ({slots.numel() * 4} bytes; original_images is re-packed on the host)")
        org, k = data["original_images"], len(slots_host[0])
        new = [[] for _ in range(k + 1)]
        for b, q in enumerate(query):
            for j, s in enumerate(slots_host[b]):
                new[j].append(org[int(s) + (int(s) >= q)][b])
            new[k].append(org[q][b])
        data["original_images"] = new

    def _lanes_record(self, B: int, T: int, counts) -> dict:
        """Sub-batch lanes this batch runs as (bit-identical for every value; `hip_lanes` in the decoder / encoder cfg, default "auto").  The
        ragged decoder call has no laned form yet: ONE lane (the encoder lanes its packed images as ever)."""
        if counts is not None:
            return {"sub_batch_lanes": 1, "ragged_views": sum(counts)}
        return {"sub_batch_lanes": _lib.resolve_lanes(self.decoder.hip_lanes, B * T, B, self.decoder.hip_precision)}

    def _eager_features(self, data, images, plan: _Batch):
        """(the decoder's features, this forward's entries of data["hip_precision"]) from the ONE source the batch names.  Bank
        (_bank_sources): ONE bd_gather_view_rows launch assembles the operand from its rows and the views encoded here; images in banked
        or padded slots are never read and no fp32 features exist (features.OperandOnly).  view_counts: the encoder sees the real views
        only, packed.  cached_rgb_feat: only the views the cache lacks are encoded (a stale cache re-encodes all, and says so every time)."""
        B, T, counts = plan.B, plan.T, plan.counts
        if plan.bank is not None:
            src, fresh, record = self._bank_sources(images, plan)
            return plan.bank.gather(src, fresh, (B, T) if counts is None else (sum(counts),)), record
        record = self._lanes_record(B, T, counts) if isinstance(self.decoder, BETR) else {}
        if counts is not None:
            return self._encode_slots(images, self.decoder.ragged_index(counts, T, images.device)[0])[0], record
        if "cached_rgb_feat" in data:
            feats = merge_cached_features(self.rgb_encoder, images, data["cached_rgb_feat"], data["cached_rgb_mask"])
            record["cache_stale"] = bool(merge_cached_features.last_stale)
            return feats, record
        return self.rgb_encoder.predict(images), record

    def _graphed(self, images, pose_feat, qi, sig=None):
        """Replay (capturing first, per batch shape) encoder -> decoder -> corner decode as one HIP graph; returns the graph's STATIC
        output tensors (heat, corners px, corners normalised, None)."""
        from .graph import GraphedPath
        B, T = images.shape[:2]
        key = (B, T, images.shape[-1], images.dtype, pose_feat.dtype, str(images.device), sig if sig is not None else self.decoder._signature(),
               self.rgb_encoder.model.state_stamp(self.rgb_encoder.prec), str(self.decoder.hip_precision),
               bool(self.decoder.hip_latency), bool(getattr(self.rgb_encoder.model, "latency", False)))
        if self._graph is None or self._graph_key != key:
            self._graph = None                      # lifts the modules' freeze before anything re-allocates
            if pose_feat.dtype != images.dtype:
                raise ValueError("hip_graph: images and bbox_feat must share a dtype (the dataset casts both to its precision)")
            self._graph = GraphedPath(self.rgb_encoder, self.decoder, B, T, images.shape[-1], images.dtype, images.device)
            self._graph_key = key
        return self._graph(images, pose_feat, qi)

    def _process_evaluation(self, pred_poses, data, out: _Out, syncs, behind_the_d2h):
        """prediction_utils.py:63-101 for bb8/heatmap: decode corners on the GPU, ONE D2H (corners + 3-D box + K + the decoder's deferred
        mask verdict, and the step's slots when it has some, in one buffer), host PnP.  Returns (pred_poses, those slots as host ints --
        None where they did not make the trip)."""
        ar, qi, slots, slots_host = out.ar, out.qi, out.slots, None
        B = out.heat.shape[0]
        norm_kp, kp_px = out.decoded if out.decoded is not None else recover_bb8_corners_chw(out.heat)[:2]           # [B,8,2] each
        bbox_3d = data["bbox_3d"][ar, qi].float()
        K = data["non_ndc_intrinsics"][ar, qi].float()
        err = getattr(self.decoder, "mask_error", None)
        flag = (err if err is not None else torch.zeros((), dtype=torch.bool, device=kp_px.device)).float().reshape(1)
        # PnP stays on the host CPU (north_star; box_utils.py:139-199): OpenCV's solvePnP when cv2 is importable, else this repo's
        # restatement of its ITERATIVE algorithm -- whose parity against OpenCV is UN-PINNED in this image;
        # `pose_solver` says which one produced `pred_poses`.  The HIP solver (row f3) is opt-in: config["modules"]["pnp_on_device"] =
        # True (bd_solve_pnp, one pose per thread) or "wave" (bd_solve_pnp_wave, one wavefront per pose, which also leaves each pose's
        # pixel reprojection RMS in data["pred_pose_rms_px"]); then only the mask verdict crosses to the host.
        def device_work_independent_of_the_poses():
            behind_the_d2h()
            data["regression_boxes"] = data["bbox_proj_crop"].clone()
            data["regression_boxes"][ar, qi] = norm_kp.to(data["regression_boxes"].dtype)
            data["pred_corners_px"] = kp_px

        if self.pnp_on_device:
            device_work_independent_of_the_poses()
            if self.pnp_on_device == "wave":
                poses, data["pred_pose_rms_px"] = solve_poses_device(kp_px, bbox_3d, K, form="wave", want_rms=True)
                data["pose_solver"] = "hip:bd_solve_pnp_wave (one wavefront per pose, DLT + LM; parity vs OpenCV un-pinned)"
            else:
                poses = solve_poses_device(kp_px, bbox_3d, K)
                data["pose_solver"] = "hip:bd_solve_pnp (DLT + LM, parity vs OpenCV un-pinned)"
            bad = bool(flag.item()) if err is not None else False
            if err is not None:
                syncs.append("mask verdict D2H (4 bytes; pnp_on_device)")
        else:
            # ONE D2H into a pinned buffer, asynchronously; everything the device can do without the poses is enqueued behind it, and only
            # then does the host wait (for the copy's event, not for the stream) -- round 6: the device used to idle through the host PnP
            parts = {"corners": kp_px, "box": bbox_3d, "K": K, "verdict": flag}
            if slots is not None:       # (small integers: exact in fp32)
                parts["slots"] = slots.float()
            packed = torch.cat([p.reshape(-1) for p in parts.values()])
            if packed.is_cuda:
                if self._d2h_pin is None or self._d2h_pin.numel() != packed.numel():
                    self._d2h_pin = torch.empty(packed.numel(), dtype=torch.float32, pin_memory=True)
                    self._d2h_done = torch.cuda.Event()
                self._d2h_pin.copy_(packed, non_blocking=True)
                self._d2h_done.record()
                device_work_independent_of_the_poses()
                self._d2h_done.synchronize()
                host = self._d2h_pin.numpy()
            else:
                device_work_independent_of_the_poses()
                host = packed.numpy()
            syncs.append(f"corners + 3-D box + K + mask verdict: ONE D2H of {host.size * 4} bytes, then the host PnP of {B} poses")
            got = _cut(host, [(name, tuple(p.shape)) for name, p in parts.items()])
            bad = bool(got["verdict"][0] != 0.0)
            if slots is not None:
                slots_host = got["slots"].astype("int64").tolist()
            poses = torch.from_numpy(solve_poses_host(got["corners"], got["box"], got["K"]))
            data["pose_solver"] = ("host:cv2.solvePnP" if pnp._HAVE_CV2
                                   else "host:bd_solve_pnp_host (native threads, DLT + LM; parity vs OpenCV un-pinned)")
        if bad:
            raise ValueError("camera_mask must mark exactly one query view per sample, among the sample's view_counts views when those "
                             "are given (reported with the corners' D2H; BETR.validate_inputs = True checks before the launch instead)")
        if not poses.is_cuda and pred_poses.is_cuda:
            # the solved poses go back through a pinned staging buffer: an asynchronous copy (from pageable memory it would wait for the
            # stream).  The buffer is rewritten only after the NEXT forward's D2H, which waits for everything enqueued before it.
            if self._pose_pin is None or self._pose_pin.shape[0] != B:
                self._pose_pin = torch.empty((B, 4, 4), dtype=torch.float32, pin_memory=True)
            self._pose_pin.copy_(poses)
            poses = self._pose_pin.to(pred_poses.device, non_blocking=True)
        pred_poses[ar, qi] = poses.to(pred_poses.device).to(pred_poses.dtype)
        return torch.nan_to_num(pred_poses, nan=0.0, posinf=0.0, neginf=0.0), slots_host
