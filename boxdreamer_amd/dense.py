"""Dense-reference mode: pick the best references out of a dense database view set, optionally in
several decoder rounds.  Host mirror of the reference's helpers, same names / arguments / dict side effects:

  dino_matching                     /root/reference/src/models/utils/matching.py:64-174
  filter_by_neighbor_mask           /root/reference/src/models/utils/data_processing.py:9-176
  process_dense_input               /root/reference/src/models/utils/data_processing.py:179-225
  sub_batchify                      /root/reference/src/models/utils/data_utils.py:5-94
  fetch_neighbors_by_pose_similarity /root/reference/src/models/utils/data_utils.py:97-135
  process_multi_round               /root/reference/src/models/utils/dense_processing.py:8-158

The arithmetic that scales with the database size -- the L x L patch-similarity of every (query, reference) pair -- runs in
HIP (csrc/match.hip: one pass over the patch features per view, closed form of the reference's masked mean) together with
the top-k selection; the decoder rounds reuse BETR unchanged.  View selection / re-packing of the batch tensors is torch
indexing on the device (plumbing).  Pose recovery inside the multi-round mode goes through the host RANSAC PnP (pnp.solve_pnp_ransac:
the reference's cv2.solvePnPRansac call where cv2 imports, a restatement of the scheme otherwise), whose parity against OpenCV is
un-pinned in this image.  With `pnp_on_device: "wave"` and at most 8 rounds the same scheme runs in HIP instead
(csrc/pnp.hip: bd_solve_pnp_ransac_wave, one wavefront per hypothesis): corners, box, K and the coarse pose stay on the device;
data["dense_pose_solver"] names what ran, data["dense_pose_inliers"] / data["dense_pose_rms_px"] say which rounds it kept.
Over a reference bank that keeps poses (cache.RefFeatureBank(keep_poses=True)) the multi-round decode runs from the bank's rows
(process_multi_round_bank; csrc/rounds.hip: bd_round_sources, bd_pose_select_rows, restated here for the CPU as round_sources_host /
pose_select_rows_host): only the query crops are encoded, the results are those of process_multi_round bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, pnp
from .box_utils import RANSAC_MAX_ROUNDS, recover_bb8_corners_chw, solve_poses_ransac_device


def _get(cfg, key, default=None):
    try:
        return cfg[key]
    except (KeyError, AttributeError, TypeError):
        return getattr(cfg, key, default)


# ------------------------------------------------------------------------------------------- reference selection

def match_views(rgb_feature: torch.Tensor, frames: torch.Tensor, query_idx: torch.Tensor, topk: int,
                threshold: float = 0.05):
    """rgb_feature (B, T, L, D) fp32 encoder output, frames (B, T, 3, H, W) RGB in [0, 1], query_idx (B,) ->
    (scores (B, T-1) fp32, neighbor_mask (B, T-1) bool), references in view order (query view skipped)."""
    _lib.require_gpu()
    lib = _lib.load()
    B, T, L, D = rgb_feature.shape
    H, W = frames.shape[-2:]
    feats = rgb_feature.contiguous()
    if feats.dtype != torch.float32:
        feats = feats.float()
    frames = frames.contiguous()
    dev = feats.device
    q = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    sums = torch.empty((B * T, D), dtype=torch.float32, device=dev)
    counts = torch.empty((B * T,), dtype=torch.float32, device=dev)
    scores = torch.empty((B, T - 1), dtype=torch.float32, device=dev)
    _lib.check(lib.bd_dino_match_scores(_lib.ptr(feats), _lib.ptr(frames), _lib.dtype_id(frames), _lib.ptr(q), B, T, L, D,
                                        H, W, float(threshold), _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(scores),
                                        _lib.stream()), "bd_dino_match_scores")
    mask = torch.empty((B, T - 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.bd_topk_mask(_lib.ptr(scores), B, T - 1, int(topk), _lib.ptr(mask), _lib.stream()), "bd_topk_mask")
    return scores, mask.bool()


def dino_matching(ref_features, query_features, ref_images, query_images, similarity_type="dot_product", topk=10,
                  similarity_params=None):
    """Same signature as the reference: ref_features (B, N, L, D), query_features (B, L, D), ref_images (B, N, 3, H, W),
    query_images (B, 3, H, W) -> bool top-k mask (B, N)."""
    if similarity_type != "dot_product":
        raise NotImplementedError("only the reference's default 'dot_product' similarity is implemented")
    B, N = ref_features.shape[:2]
    feats = torch.cat([ref_features, query_features.unsqueeze(1)], dim=1)
    frames = torch.cat([ref_images, query_images.unsqueeze(1)], dim=1)
    q = torch.full((B,), N, dtype=torch.int32, device=feats.device)
    return match_views(feats, frames, q, topk)[1]


def _filter(x, camera_mask, neighbor_mask):
    B, T = camera_mask.shape
    ref = x[~camera_mask].reshape(B, T - 1, *x.shape[2:])[neighbor_mask].reshape(B, -1, *x.shape[2:])
    return torch.cat([ref, x[camera_mask].unsqueeze(1)], dim=1)


def _filter_index(camera_mask, neighbor_mask):
    """The view indices `_filter` keeps, (B, k + 1): the selected references in their original order, the query last."""
    B, T = camera_mask.shape
    ar = torch.arange(T, device=camera_mask.device).expand(B, T)
    ref = ar[~camera_mask].reshape(B, T - 1)[neighbor_mask].reshape(B, -1)
    return torch.cat([ref, ar[camera_mask].reshape(B, 1)], dim=1)


def _filter_features(rgb_feature, camera_mask, neighbor_mask):
    """`_filter` for the encoder features: the same views, WITH their operand-dtype copy (cache.take_views) -- a plain index would drop
    it and BETR would re-cast the features on every forward (the dense path always ran that slow path)."""
    from .cache import take_views
    if rgb_feature.dim() != 4:
        return _filter(rgb_feature, camera_mask, neighbor_mask)
    return take_views(rgb_feature, _filter_index(camera_mask, neighbor_mask))


def _sub_index(camera_mask, sub):
    """View indices of `_sub`, (B, rounds, sub + 1): `sub` consecutive references per round (-1 where the last round runs out), query last."""
    B, T = camera_mask.shape
    ar = torch.arange(T, device=camera_mask.device).expand(B, T)
    ref, q = ar[~camera_mask].reshape(B, T - 1), ar[camera_mask].reshape(B)
    rounds = (T - 1 + sub - 1) // sub
    idx = torch.full((B, rounds, sub + 1), -1, dtype=torch.long, device=camera_mask.device)
    for i in range(rounds):
        end = min((i + 1) * sub, T - 1)
        idx[:, i, :end - i * sub] = ref[:, i * sub:end]
        idx[:, i, sub] = q
    return idx


def filter_by_neighbor_mask(data, neighbor_mask, pose_feat, frames, camera_mask, rgb_feature, image_masks):
    """Keep the selected references (original order) followed by the query view; updates the batch dict like the
    reference's update_filtered_data (bbox_feat, images, query_idx, camera_mask, poses and the per-view tensors)."""
    B = frames.shape[0]
    new_pose_feat = _filter(pose_feat, camera_mask, neighbor_mask)
    new_frames = _filter(frames, camera_mask, neighbor_mask)
    new_rgb = _filter_features(rgb_feature, camera_mask, neighbor_mask) if rgb_feature is not None else None
    new_masks = _filter(image_masks, camera_mask, neighbor_mask) if image_masks is not None else None
    T = new_frames.shape[1]
    new_camera_mask = torch.zeros(B, T, dtype=torch.bool, device=camera_mask.device)
    new_camera_mask[:, -1] = True
    data["bbox_feat"] = new_pose_feat.clone()
    data["images"] = new_frames.clone()
    data["query_idx"] = torch.tensor([T - 1], device=frames.device).repeat(B)
    data["camera_mask"] = new_camera_mask.clone()
    for key in ("poses", "original_poses", "intrinsics", "non_ndc_intrinsics", "original_intrinsics", "scale", "bbox_3d",
                "bbox_proj_crop"):
        if key in data:
            data[key] = _filter(data[key], camera_mask, neighbor_mask)
    if "original_images" in data:                              # list [T][B] -> keep the selected views (data_processing.py:150-176)
        nm = neighbor_mask.cpu().numpy()
        org = data["original_images"]
        n_keep = int(nm[0].sum())
        new = [[] for _ in range(n_keep + 1)]
        for b in range(B):
            r = 0
            for t in range(len(org) - 1):
                if nm[b, t]:
                    new[r].append(org[t][b]); r += 1
            new[-1].append(org[-1][b])
        data["original_images"] = new
    return data, new_pose_feat, new_frames, new_camera_mask, new_rgb, new_masks


def filter_by_view_index(data, idx, ar):
    """filter_by_neighbor_mask's update of the batch dict for a selection that exists as view indices on the device (the banked dense
    mode, model.py: bd_match_select_rows' slots): idx (B, k + 1) long, the selected references in their original order and the query
    last; ar = arange(B) on the same device.  The same keys get the same views, through integer indexing: no boolean mask, no
    nonzero(), nothing waits for the device.  Features are not re-packed here (the bank gathers them) and `original_images`, a host
    list, is left to the caller.  Returns the new query_idx (B,) long, all k."""
    B, T = idx.shape
    rows = ar[:, None]
    for key in ("bbox_feat", "images", "poses", "original_poses", "intrinsics", "non_ndc_intrinsics", "original_intrinsics", "scale",
                "bbox_3d", "bbox_proj_crop"):
        if key in data:
            data[key] = data[key][rows, idx]
    qi = torch.full((B,), T - 1, dtype=torch.long, device=idx.device)
    data["query_idx"] = qi
    data["camera_mask"] = torch.arange(T, device=idx.device)[None, :] == qi[:, None]
    return qi


def process_dense_input(data, pose_feat, frames, camera_mask, rgb_feature, image_masks, dense_cfg):
    if _get(dense_cfg, "filter") == "dino" and _get(dense_cfg, "filter_enable"):
        q = camera_mask.to(torch.int32).argmax(dim=1)
        _, neighbor_mask = match_views(rgb_feature, frames, q, int(_get(dense_cfg, "filter_topk")))
        return filter_by_neighbor_mask(data, neighbor_mask, pose_feat, frames, camera_mask, rgb_feature, image_masks)
    return data, pose_feat, frames, camera_mask, rgb_feature, image_masks


# ------------------------------------------------------------------------------------------- multi-round decode

def _sub(x, camera_mask, sub):
    B, T = camera_mask.shape
    q = x[camera_mask]
    ref = x[~camera_mask].reshape(B, T - 1, *x.shape[2:])
    rounds = (T - 1 + sub - 1) // sub
    out = torch.zeros(B, rounds, sub + 1, *x.shape[2:], dtype=x.dtype, device=x.device)
    for i in range(rounds):
        end = min((i + 1) * sub, T - 1)
        out[:, i, :end - i * sub] = ref[:, i * sub:end]
        out[:, i, sub] = q
    return out


def sub_batchify(pose_feat, frames, camera_mask, rgb_feature, image_masks, sub_batch_size):
    """(B, T, ...) -> (B, rounds, sub+1, ...): `sub` consecutive references per round (zero-padded at the end), query last."""
    B, T = camera_mask.shape
    rounds = (T - 1 + sub_batch_size - 1) // sub_batch_size
    new_camera_mask = torch.zeros(B, rounds, sub_batch_size + 1, dtype=torch.bool, device=camera_mask.device)
    new_camera_mask[:, :, sub_batch_size] = True
    return (_sub(pose_feat, camera_mask, sub_batch_size), _sub(frames, camera_mask, sub_batch_size), new_camera_mask,
            _sub(rgb_feature, camera_mask, sub_batch_size),
            _sub(image_masks, camera_mask, sub_batch_size) if image_masks is not None else None)


def fetch_neighbors_by_pose_similarity(gt_poses, pred_pose, topk=5):
    """gt_poses (B, N, 4, 4), pred_pose (B, 1, 4, 4) -> (B, topk) indices of the closest reference poses
    (geodesic rotation distance + translation distance)."""
    B, N = gt_poses.shape[:2]
    g = gt_poses.reshape(B * N, 4, 4).float()
    p = pred_pose.reshape(B, 1, 4, 4).repeat(1, N, 1, 1).reshape(B * N, 4, 4).float()
    Rd = torch.matmul(p[:, :3, :3], g[:, :3, :3].transpose(1, 2))
    tr = torch.diagonal(Rd, dim1=-2, dim2=-1).sum(-1)
    rot = torch.acos(torch.clamp((tr - 1) / 2, -1, 1))
    dist = (rot + torch.norm(p[:, :3, 3] - g[:, :3, 3], dim=-1)).reshape(B, N)
    return torch.topk(dist, k=topk, dim=1, largest=False)[1]


# ------------------------------------------------------------------------------------------- multi-round decode over a bank
# CPU restatements (plain Python / numpy fp64) of the two kernels of csrc/rounds.hip: what their tests compare against.

NO_VIEW = 0x7fffffff        # a source-table entry bd_gather_view_rows skips


def _candidate_row(rows_b, slot, n_bank):
    if not 0 <= slot < len(rows_b):
        return NO_VIEW
    r = int(rows_b[slot])
    return r if 0 <= r < n_bank else NO_VIEW


def round_sources_host(rows, cand, n_bank, sub, zero_row, per_round_query):
    """bd_round_sources on the host: rows [B][N_max], cand [B][k] (lists or tensors) -> (src, view), flat int lists of
    B * R * (sub + 1) entries, R = ceil(k / sub)."""
    rows, cand = torch.as_tensor(rows).tolist(), torch.as_tensor(cand).tolist()
    k = len(cand[0])
    R = -(-k // sub)
    src, view = [], []
    for b, (rb, cb) in enumerate(zip(rows, cand)):
        for r in range(R):
            for j in range(sub):
                c = r * sub + j
                src.append(_candidate_row(rb, int(cb[c]), n_bank) if c < k else int(zero_row))
                view.append(c if c < k else -1)
            src.append(-((b * R + r if per_round_query else b) + 1))
            view.append(k)
    return src, view


def pose_distance_host(pred, pose) -> float:
    """bd_pose_select_rows' distance of two (4, 4) poses in fp64, in the kernel's summation order (include/boxdreamer_hip.h)."""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    tr = np.float64(0.0)
    for i in range(3):
        for j in range(3):
            tr = tr + p[i, j] * g[i, j]
    x = (tr - 1.0) / 2.0
    x = np.float64(-1.0) if x < -1.0 else (np.float64(1.0) if x > 1.0 else x)
    ss = np.float64(0.0)
    for i in range(3):
        d = p[i, 3] - g[i, 3]
        ss = ss + d * d
    with np.errstate(invalid="ignore"):
        return float(np.arccos(x) + np.sqrt(ss))


def pose_select_rows_host(bank_poses, n_bank, pred, rows, cand, fk):
    """bd_pose_select_rows on the host: bank_poses (>= n_bank, 4, 4) and pred (B, 4, 4) fp32, rows [B][N_max], cand [B][k] ->
    (dist64 [B][k] the fp64 distances (inf: invalid candidate), fine_pos [B][fk], src flat [B * (fk + 1)]); the ranking is on the
    distances rounded to fp32, as the kernel's."""
    bank = torch.as_tensor(bank_poses).detach().cpu().float().numpy()
    pr = torch.as_tensor(pred).detach().cpu().float().numpy()
    rows, cand = torch.as_tensor(rows).tolist(), torch.as_tensor(cand).tolist()
    dist, fine_pos, src = [], [], []
    for b, (rb, cb) in enumerate(zip(rows, cand)):
        rws = [_candidate_row(rb, int(s), n_bank) for s in cb]
        d64 = [float("inf") if r == NO_VIEW else pose_distance_host(pr[b], bank[r]) for r in rws]
        d32 = [float(np.float32(d)) for d in d64]
        valid = [c for c, r in enumerate(rws) if r != NO_VIEW]
        order = sorted(valid, key=lambda c: (d32[c] != d32[c], 0.0 if d32[c] != d32[c] else d32[c], c))
        pos = sorted(order[:fk])
        pos += [-1] * (fk - len(pos))
        dist.append(d64)
        fine_pos.append(pos)
        src += [rws[c] if c >= 0 else NO_VIEW for c in pos] + [-(b + 1)]
    return dist, fine_pos, src


DENSE_SOLVER_HOST ="host:pnp.solve_pnp_ransac (cv2.solvePnPRansac where importable, else its scheme restated; parity vs OpenCV un-pinned)"
DENSE_SOLVER_WAVE = "hip:bd_solve_pnp_ransac_wave (one wavefront per hypothesis, DLT + LM; parity vs OpenCV un-pinned)"


def recover_pose_from_dense_bb8(query_rets, bbox_3d, K, pnp_on_device=False, n_trials=1000, record=None):
    """query_rets (B, R, 8, H, W) heatmaps of R decoder rounds; bbox_3d (B, 8, 3); K (B, 3, 3).  All R*8 decoded corners of
    a sample go into one RANSAC PnP (box_utils.py:202-300: solvePnPRansac at 2 px / 0.99 / 1000 trials, ITERATIVE on failure --
    pnp.solve_pnp_ransac: cv2's own call where importable, else this repo's restatement of the scheme): a round whose corners are off
    is rejected instead of pulling the coarse pose (and with it the fine level's neighbour choice).  Returns poses (B, 1, 4, 4),
    normalised corners (B, R, 8, 2).  pnp_on_device == "wave" with R <= 8: the HIP form of the scheme (bd_solve_pnp_ransac_wave), nothing
    leaves the device.  record (a dict, e.g. the batch dict): gets dense_pose_solver, dense_pose_inliers (B, R, 8) bool and
    dense_pose_rms_px (B,), both on the device."""
    B, R = query_rets.shape[:2]
    norm_kp, kp_px, _ = recover_bb8_corners_chw(query_rets.reshape(B * R, *query_rets.shape[2:]))
    dev = query_rets.device
    if pnp_on_device == "wave" and R <= RANSAC_MAX_ROUNDS:
        poses, inl, rms, _ = solve_poses_ransac_device(kp_px.reshape(B, R, 8, 2), bbox_3d, K, n_trials=n_trials, reproj_err=2.0,
                                                       confidence=0.99)
        if record is not None:
            record["dense_pose_solver"], record["dense_pose_inliers"], record["dense_pose_rms_px"] = DENSE_SOLVER_WAVE, inl, rms
        return poses.reshape(B, 1, 4, 4), norm_kp.reshape(B, R, 8, 2)
    kp = kp_px.reshape(B, R * 8, 2).cpu().numpy()
    b3 = bbox_3d.float().cpu().numpy()
    Kh = K.float().cpu().numpy()
    poses = np.zeros((B, 1, 4, 4), np.float32)
    inl = np.zeros((B, R * 8), bool)
    rms = np.zeros((B,), np.float32)
    for b in range(B):
        try:
            ok, Rm, t, m = pnp.solve_pnp_ransac(np.tile(b3[b], (R, 1)), kp[b], Kh[b], reproj_err=2.0, confidence=0.99, max_trials=n_trials, seed=b)
        except Exception as e:  # noqa: BLE001
            print(f"PnP failed due to exception: {e}")
            continue
        if ok:
            poses[b, 0, :3, :3] = Rm
            poses[b, 0, :3, 3] = t
            poses[b, 0, 3, 3] = 1.0
            inl[b] = m
            if record is not None and m.any():
                p3 = np.tile(b3[b], (R, 1)).astype(np.float64)
                err = pnp._reproj_px(Rm, t, p3[m], kp[b][m].astype(np.float64), Kh[b].astype(np.float64))
                rms[b] = np.sqrt(np.mean(err * err))
    if record is not None:
        record["dense_pose_solver"] = DENSE_SOLVER_HOST
        record["dense_pose_inliers"] = torch.from_numpy(inl.reshape(B, R, 8)).to(dev)
        record["dense_pose_rms_px"] = torch.from_numpy(rms).to(dev)
    return torch.from_numpy(poses).to(dev), norm_kp.reshape(B, R, 8, 2)


def process_multi_round(data, pose_feat, frames, camera_mask, rgb_feature, image_masks, decoder, dense_cfg,
                        bbox_representation="heatmap", pnp_on_device=False):
    """Decoder over sub-batches of the references (query appended to each), one PnP over all rounds' corners, optional
    fine round on the references nearest to that pose.  Returns the decoder output of the fine round or, without it, None: the
    coarse prediction is then written into the batch dict (_write_coarse; the reference returns the dict).  pnp_on_device: the model's setting; "wave" runs that PnP
    on the device when there are at most 8 rounds (recover_pose_from_dense_bb8).  dense_cfg.ransac_trials (optional): its trial count,
    default 1000 (the reference's iterationsCount)."""
    B = frames.shape[0]
    poses = data["poses"].clone()
    K = data["non_ndc_intrinsics"].clone()
    bbox_3d = data["bbox_3d"].clone()
    sub = int(_get(dense_cfg, "sub_batch_size"))
    from .cache import take_views
    npf, nfr, ncm, nrf, _ = sub_batchify(pose_feat, frames, camera_mask, rgb_feature, None, sub)
    R = npf.shape[1]
    # the rounds' features WITH their operand-dtype copies (same values as `nrf`; cache.take_views): BETR does not re-cast them
    sidx = _sub_index(camera_mask, sub)                                   # (B, R, sub + 1) view indices, -1 = zero padding
    tagged = rgb_feature.dim() == 4
    if _get(dense_cfg, "dense_mem_friendly"):
        outs = [decoder(npf[:, i].contiguous(), nfr[:, i].contiguous(), ncm[:, i],
                        take_views(rgb_feature, sidx[:, i]) if tagged else nrf[:, i].contiguous(), None).clone() for i in range(R)]
        query_rets = torch.stack(outs, dim=1)
    else:
        feats = (take_views(rgb_feature, sidx.reshape(B, R * (sub + 1))) if tagged else nrf)
        if tagged:      # (B, R (sub + 1), P, C) -> (B R, sub + 1, P, C): the same storage, the operand copy follows the alias
            from . import features as _features
            feats = _features.carry(feats, feats.reshape(B * R, sub + 1, *feats.shape[2:]))
        else:
            feats = feats.reshape(B * R, *nrf.shape[2:])
        flat = decoder(npf.reshape(B * R, *npf.shape[2:]), nfr.reshape(B * R, *nfr.shape[2:]), ncm.reshape(B * R, -1), feats, None)
        query_rets = flat.reshape(B, R, *flat.shape[1:])
    trials = _get(dense_cfg, "ransac_trials")
    query_poses, pred_proj = recover_pose_from_dense_bb8(query_rets, bbox_3d[camera_mask], K[camera_mask], pnp_on_device=pnp_on_device,
                                                         n_trials=1000 if trials is None else int(trials), record=data)
    if _get(dense_cfg, "fine_level"):
        idx = fetch_neighbors_by_pose_similarity(poses[~camera_mask].reshape(B, poses.shape[1] - 1, 4, 4), query_poses,
                                                 topk=int(_get(dense_cfg, "fine_topk")))
        neighbor_mask = torch.zeros(B, poses.shape[1] - 1, dtype=torch.bool, device=poses.device)
        neighbor_mask.scatter_(1, idx.to(poses.device), True)
        data, pose_feat, frames, camera_mask, rgb_feature, image_masks = filter_by_neighbor_mask(
            data, neighbor_mask, pose_feat, frames, camera_mask, rgb_feature, image_masks)
        from . import features as _features
        return decoder(pose_feat.contiguous(), frames.contiguous(), camera_mask, _features.carry(rgb_feature, rgb_feature.contiguous()), None)
    _write_coarse(data, camera_mask, pose_feat, query_rets, query_poses, pred_proj)     # (a boolean mask: each write waits for the device)
    return None


def _write_coarse(data, where, pose_feat, query_rets, query_poses, pred_proj) -> None:
    """The coarse prediction of a multi-round decode without a fine level, into the batch dict at the query view `[where]`: camera_mask
    (the reference's own write) or (arange(B), query_idx).  An entry-token bank's batch may carry no heat maps (pose_feat None): the
    decoder's output then goes out as it does from BoxDreamer.forward, in pred_query_bbox."""
    if pose_feat is not None:
        data["pred_bbox"] = pose_feat.clone()
        data["pred_bbox"][where] = query_rets[:, 0].to(pose_feat.dtype)
    else:
        data["pred_query_bbox"] = query_rets[:, 0]
    pred_poses = data["poses"].clone()
    pred_poses[where] = query_poses.squeeze(1).to(pred_poses.dtype)
    data["regression_boxes"] = data["bbox_proj_crop"].clone()
    data["regression_boxes"][where] = pred_proj[:, 0].to(data["regression_boxes"].dtype)
    data["pred_poses"] = pred_poses
    data["pred_intrinsics"] = data["intrinsics"].clone()


def _repeat_views(fresh, times: int):
    """The encoder's tagged (B, P, C) output with every view `times` times in a row, as the operand copy alone (features.OperandOnly of
    (B * times, P, C)): the multi-round batch's query features over an entry-token bank.  The bytes are copied, nothing is re-cast."""
    from . import features as _features, operand
    f16, pid = _features.require_tag(fresh)
    B, P, C = fresh.shape
    out16 = operand.empty(pid, B * times * P, C, fresh.device)
    for dst, src in zip(operand.row_planes(out16, pid, B * times * P), operand.row_planes(f16, pid, B * P)):
        dst.reshape(B, times, P, C).copy_(src.reshape(B, 1, P, C).expand(B, times, P, C))
    return _features.OperandOnly((B * times, P, C), out16, pid, _features.stamp_of(fresh))


def process_multi_round_bank(data, bank, fresh, rows, cand, ar, decoder, dense_cfg, pnp_on_device=False):
    """process_multi_round over a reference bank that keeps poses (cache.RefFeatureBank(keep_poses=True)), after the banked dense
    selection re-packed the batch dict to (B, k + 1): `fresh` the encoder's tagged output for the B query crops, rows (B, N_max) /
    cand (B, k) the device tables of that selection (bank rows per reference slot; the kept slots, ascending), ar = arange(B).
    ONE bd_round_sources launch names the views of the (B * R, sub + 1) rounds -- the short last round padded with bank.zero_row --
    and the decoder runs on them from the bank: bank.gather for a feature bank (bbox_feat re-packed by integer indexing with the
    kernel's `view` table, zeros where it pads), BETR.forward_entry for an entry-token bank (the query's features repeated per
    round; bbox_feat may be absent).  recover_pose_from_dense_bb8 runs as it is.  Without dense_cfg.fine_level the coarse dict is
    written as process_multi_round writes it (_write_coarse) and (None, None) returned.  With it ONE bd_pose_select_rows launch picks the fine_topk
    kept references nearest to the coarse pose by the BANK's poses (the dict's are not read), the dict is re-packed to
    (B, fine_topk + 1) and (the fine round's decoder output, the new query_idx) returned; the dict gains dense_fine_slots
    (B, fine_topk) -- original reference slots, ascending -- and dense_fine_dist (B, k).  Nothing here waits for the device unless
    the host RANSAC runs.  The results are bit-identical to process_multi_round on the same crops."""
    from . import hip_ops
    B, k = cand.shape
    sub = int(_get(dense_cfg, "sub_batch_size"))
    R = (k + sub - 1) // sub
    entry, friendly = bank.has_entry_tokens, bool(_get(dense_cfg, "dense_mem_friendly"))
    dev = fresh.device
    pose_feat, frames = data.get("bbox_feat"), data["images"]
    size = frames.shape[-1]
    zero_row = bank.zero_row if k % sub else -1
    # (forward_entry takes one fresh view per pseudo-sample, in order: the round-by-round form decodes B samples at a time)
    src, view = hip_ops.round_sources(rows, cand, len(bank), sub, zero_row, per_round_query=entry and not friendly)
    src = src.reshape(B, R, sub + 1)
    masks = (torch.arange(sub + 1, device=dev) == sub).expand(B * R, sub + 1).contiguous()
    npf = nfr = None
    if not entry:
        v = view.reshape(B, R * (sub + 1)).long()
        npf = pose_feat[ar[:, None], v.clamp_min(0)]
        npf.masked_fill_((v < 0).reshape(B, -1, 1, 1, 1), 0)
        npf = npf.reshape(B, R, sub + 1, *pose_feat.shape[2:])
        # (BETR reads the shape of the crops and nothing else: a view of the right shape, no copy)
        nfr = frames[:1, :1].expand(B * R, sub + 1, *frames.shape[2:])

    def decode(s, n, heat):
        if entry:
            return decoder.forward_entry(bank.entry_tokens, len(bank), s, fresh if n == B else _repeat_views(fresh, R), masks[:n], size)
        return decoder(heat, nfr[:n], masks[:n], bank.gather(s, fresh, (n, sub + 1)), None)

    if friendly:
        outs = [decode(src[:, i].reshape(-1).contiguous(), B, None if entry else npf[:, i].contiguous()).clone() for i in range(R)]
        query_rets = torch.stack(outs, dim=1)
    else:
        flat = decode(src.reshape(-1), B * R, None if entry else npf.reshape(B * R, sub + 1, *pose_feat.shape[2:]))
        query_rets = flat.reshape(B, R, *flat.shape[1:])
    qi = data["query_idx"]
    trials = _get(dense_cfg, "ransac_trials")
    query_poses, pred_proj = recover_pose_from_dense_bb8(query_rets, data["bbox_3d"][ar, qi], data["non_ndc_intrinsics"][ar, qi],
                                                         pnp_on_device=pnp_on_device, n_trials=1000 if trials is None else int(trials),
                                                         record=data)
    if _get(dense_cfg, "fine_level"):
        fk = int(_get(dense_cfg, "fine_topk"))
        dist, fine_pos, fsrc = hip_ops.pose_select_rows(bank.poses, len(bank), query_poses.reshape(B, 4, 4).float().contiguous(), rows, cand, fk)
        pos = fine_pos.long().clamp_min(0)
        data["dense_fine_dist"], data["dense_fine_slots"] = dist, cand.gather(1, pos)
        qi = filter_by_view_index(data, torch.cat([pos, torch.full((B, 1), k, dtype=torch.long, device=dev)], dim=1), ar)
        if entry:
            return decoder.forward_entry(bank.entry_tokens, len(bank), fsrc, fresh, data["camera_mask"], size), qi
        return decoder(data["bbox_feat"], data["images"], data["camera_mask"], bank.gather(fsrc, fresh, (B, fk + 1)), None), qi
    _write_coarse(data, (ar, qi), pose_feat, query_rets, query_poses, pred_proj)
    return None, None
