"""Corner decode + pose recovery with the reference's function names
(/root/reference/src/models/utils/box_utils.py:14-199, heatmap branch only).

`recover_bb8_corners` runs the HIP top-20 decode (bd_decode_topk); `recover_pose_from_bb8` moves the 8 corners,
the 3-D box and K to the host ONCE per batch and solves PnP there (the reference does a D2H + two OpenCV
calls per sample inside a Python loop, box_utils.py:139-199)."""
from __future__ import annotations


import numpy as np
import torch

from . import _lib, hip_ops, pnp



def recover_bb8_corners(bbox_feat: torch.Tensor, bbox_representation: str = "heatmap"):
    """bbox_feat: [B, T, H, W, 8] in [-1, 1] (the reference's layout, prediction_utils.py:65) ->
    (normalised [B,T,8,2] in [-1,1], pixel [B,T,8,2])."""
    if bbox_representation != "heatmap":
        raise NotImplementedError("the MI355X path implements the heatmap representation only")
    B, T, H, W, C = bbox_feat.shape
    heat = bbox_feat.permute(0, 1, 4, 2, 3).contiguous().float()      # [B,T,8,H,W]
    kp, kn, _ = hip_ops.decode_topk(heat, k=20, want_idx=False)
    return kn, kp


def recover_bb8_corners_chw(heat: torch.Tensor, want_idx: bool = False):
    """Same decode on the decoder's native [B, 8, H, W] output (no permute round trip)."""
    kp, kn, idx = hip_ops.decode_topk(heat, k=20, want_idx=want_idx)
    return kn, kp, idx


def _host_workers() -> int:
    """Threads of the native host solver: the CPUs this process may use (affinity and cgroup quota), at most 16."""
    global _WORKERS
    if _WORKERS is None:
        import os
        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        try:
            q, p = open("/sys/fs/cgroup/cpu.max").read().split()
            if q != "max":
                n = min(n, max(1, int(int(q) / int(p))))
        except Exception:  # noqa: BLE001
            pass
        _WORKERS = max(1, min(16, n))
    return _WORKERS


_WORKERS = None


def solve_poses_host(kp_px: np.ndarray, bbox_3d: np.ndarray, K: np.ndarray, workers: int | None = None) -> np.ndarray:
    """kp_px [N,8,2], bbox_3d [N,8,3], K [N,3,3] (host) -> poses [N,4,4] ([R|t], zeros on failure).
    One batched solve for all N poses ("next" row f3: no per-sample Python loop; pnp.solve_pnp_batched)."""
    n = kp_px.shape[0]
    out = np.zeros((n, 4, 4), np.float32)
    if n == 0:
        return out
    if not pnp._HAVE_CV2:
        # native host solver of the HIP library (csrc/pnp.hip: bd_solve_pnp_host, `workers` threads): the algorithm of
        # pnp.solve_pnp_batched step by step (which stays as its numpy cross-check, tests/test_host_logic.py)
        # The PnP post-solve is HOST work (north_star); on a host-only box without the built library (the GPU path itself has raised
        # long before) or when the native solver rejects its arguments, the batched numpy form below solves the same problem.
        try:
            lib = _lib.load()
            kp32, p32, K32 = (np.ascontiguousarray(a, np.float32) for a in (kp_px, bbox_3d, K))
            rc = lib.bd_solve_pnp_host(kp32.ctypes.data, p32.ctypes.data, K32.ctypes.data, n, kp32.shape[1], pnp.LM_MAX_ITERS, out.ctypes.data,
                                       _host_workers() if workers is None else workers)
            if rc == 0:
                return out
            out[:] = 0.0
        except (_lib.HipLibraryError, OSError):
            pass
    try:
        ok, R, t = pnp.solve_pnp_batched(bbox_3d, kp_px, K)
    except Exception as e:  # noqa: BLE001  (reference: print and leave zeros, box_utils.py:192-195)
        print(f"PnP failed due to exception: {e}")
        return out
    out[ok, :3, :3] = R[ok]
    out[ok, :3, 3] = t[ok]
    out[ok, 3, 3] = 1.0
    return out


PNP_DEVICE_FORMS = ("thread", "wave")


def solve_poses_device(kp_px: torch.Tensor, bbox_3d: torch.Tensor, K: torch.Tensor, iters: int = pnp.LM_MAX_ITERS, form: str = "thread",
                       want_rms: bool = False):
    """kp_px [N,n,2], bbox_3d [N,n,3], K [N,3,3] on the GPU -> poses [N,4,4] on the GPU ([R|t], zeros on failure) -- the corners never
    leave the device ("next" row f3).  form="thread": `bd_solve_pnp`, one pose per thread in fp64.  form="wave": `bd_solve_pnp_wave`, one
    wavefront per pose (same algorithm, same minimum); with want_rms=True it returns (poses, rms_px), rms_px [N] fp32 = root mean square
    of the pixel reprojection error of each returned pose (0 where the solve failed)."""
    if form not in PNP_DEVICE_FORMS:
        raise ValueError(f"solve_poses_device: form must be one of {PNP_DEVICE_FORMS}, got {form!r}")
    if want_rms and form != "wave":
        raise ValueError("solve_poses_device: want_rms=True needs form='wave' (bd_solve_pnp has no rms_px output)")
    _lib.require_gpu()
    lib = _lib.load()
    kp = kp_px.float().contiguous()
    p3 = bbox_3d.to(kp.device).float().contiguous()
    Kd = K.to(kp.device).float().contiguous()
    n, npts = kp.shape[0], kp.shape[1]
    out = torch.empty((n, 4, 4), dtype=torch.float32, device=kp.device)
    if form == "wave":
        rms = torch.empty((n,), dtype=torch.float32, device=kp.device) if want_rms else None
        _lib.check(lib.bd_solve_pnp_wave(_lib.ptr(kp), _lib.ptr(p3), _lib.ptr(Kd), n, npts, iters, _lib.ptr(out), _lib.ptr(rms),
                                         _lib.stream()), "bd_solve_pnp_wave")
        return (out, rms) if want_rms else out
    _lib.check(lib.bd_solve_pnp(_lib.ptr(kp), _lib.ptr(p3), _lib.ptr(Kd), n, npts, iters, _lib.ptr(out), _lib.stream()),
               "bd_solve_pnp")
    return out


RANSAC_MAX_ROUNDS = 8                  # 64 observations: MAXPTS of csrc/pnp.hip
_PICKS = {}                            # (n_rounds, n_trials, seed, device) -> int32 [n_trials, 6] on that device


def ransac_picks_device(n_rounds: int, n_trials: int, seed: int, device) -> torch.Tensor:
    """pnp.ransac_picks on `device`, built once per (n_rounds, n_trials, seed, device)."""
    key = (int(n_rounds), int(n_trials), int(seed), str(torch.device(device)))
    if key not in _PICKS:
        _PICKS[key] = torch.from_numpy(pnp.ransac_picks(n_rounds, n_trials, seed)).to(device)
    return _PICKS[key]


def solve_poses_ransac_device(kp_px: torch.Tensor, bbox_3d: torch.Tensor, K: torch.Tensor, n_trials: int = 1000, reproj_err: float = 2.0,
                              confidence: float = 0.99, seed: int = 0):
    """RANSAC PnP of the dense multi-round mode on the GPU (`bd_solve_pnp_ransac_wave`: one wavefront per hypothesis, then one per sample).
    kp_px [N, R, 8, 2] pixels (R <= 8 rounds of the same 8 corners), bbox_3d [N, 8, 3], K [N, 3, 3] ->
    (poses [N, 4, 4] fp32, zeros on failure; inliers [N, R, 8] bool; rms_px [N] fp32 over the observations used; info [N, 4] int32 =
    trials used, best hypothesis or -1, entries of the mask, path 0 = inliers / 1 = all observations / 2 = failed), all on the device.
    Every sample runs the hypotheses of the same sampling table (pnp.ransac_picks(R, n_trials, seed)), kept on the device."""
    kp = kp_px.float().contiguous()
    if kp.dim() != 4 or kp.shape[2:] != (8, 2) or not 1 <= kp.shape[1] <= RANSAC_MAX_ROUNDS:
        raise ValueError(f"solve_poses_ransac_device: kp_px must be [N, R, 8, 2] with 1 <= R <= {RANSAC_MAX_ROUNDS}, got {tuple(kp.shape)}")
    dev = kp.device
    N, R = kp.shape[:2]
    b3 = bbox_3d.to(dev).float().contiguous()
    Kd = K.to(dev).float().contiguous()
    if b3.shape != (N, 8, 3) or Kd.shape != (N, 3, 3):
        raise ValueError(f"solve_poses_ransac_device: bbox_3d {tuple(b3.shape)} / K {tuple(Kd.shape)} do not match {N} samples")
    _lib.require_gpu()
    lib = _lib.load()
    picks = ransac_picks_device(R, n_trials, seed, dev)
    poses = torch.empty((N, 4, 4), dtype=torch.float32, device=dev)
    inl = torch.empty((N, R * 8), dtype=torch.uint8, device=dev)
    rms = torch.empty((N,), dtype=torch.float32, device=dev)
    info = torch.empty((N, 4), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.bd_solve_pnp_ransac_workspace_bytes(N, int(n_trials)))
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.bd_solve_pnp_ransac_wave(_lib.ptr(kp), _lib.ptr(b3), _lib.ptr(Kd), _lib.ptr(picks), N, R, int(n_trials), float(reproj_err),
                                            float(confidence), 5, pnp.LM_MAX_ITERS, _lib.ptr(poses), _lib.ptr(inl), _lib.ptr(rms), _lib.ptr(info),
                                            _lib.ptr(ws), ws_bytes, _lib.stream()), "bd_solve_pnp_ransac_wave")
    return poses, inl.bool().reshape(N, R, 8), rms, info


def recover_pose_from_bb8(bbox_feat, bbox_3d, K, bbox_representation="heatmap"):
    """box_utils.py:113-199: (poses [B,T,4,4], normalised corners [B,T,8,2])."""
    B, T = bbox_feat.shape[:2]
    normalized_keypoints_2d, keypoints_2d = recover_bb8_corners(bbox_feat, bbox_representation)
    kp = keypoints_2d.reshape(B * T, 8, 2).cpu().numpy()              # ONE device->host sync per batch
    b3 = bbox_3d.float().reshape(B * T, 8, 3).cpu().numpy()
    Kh = K.float()
    Kh = (Kh.reshape(B * T, 3, 3) if Kh.dim() == 4 else Kh.reshape(1, 3, 3).expand(B * T, 3, 3)).cpu().numpy()
    poses = torch.from_numpy(solve_poses_host(kp, b3, Kh)).reshape(B, T, 4, 4).to(bbox_feat.device)
    return poses, normalized_keypoints_2d
