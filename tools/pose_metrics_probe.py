"""Time the device pose metrics (bd_pose_metrics) next to the host form the reference runs (profiles/pose_metrics.md).

    python tools/pose_metrics_probe.py [--out FILE]

GPU: B = 32 poses at N in {1k, 10k, 50k} model points, one object; median of 20 timed calls (HIP events) after 3 warm-up calls,
plus the achieved ADD-S pair rate (B N^2 / time) against the fp32 VALU issue peak (non-packed) at the compiled loop's 6.5 VALU ops per pair.
Host: the reference-equivalent form on this machine's CPUs -- per pose a scipy cKDTree over the pred-transformed points and a query
of the gt-transformed ones, on a 16-thread pool (skipped without scipy), plus the batch copies of the reference's test_step at
configs[1] (B = 32, T = 6): a ~370 MB device-to-host copy (`back_to_cpu`) and three host copies of it (`copy.deepcopy`).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from boxdreamer_amd import metrics as pm  # noqa: E402

# a SIMD issues a wave64 fp32 VALU op over 2 cycles (32 lanes / cycle): 256 CUs x 4 SIMDs x 32 x 2.4 GHz = 78.6 T lane-ops / s
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
# the compiled pair loop (4 candidates x 4 queries per iteration): 3 v_sub_f32 + 1 v_mul_f32 + 2 v_fmac_f32 per pair, one v_min3_f32
# per two pairs
OPS_PER_PAIR = 6.5


def make(rng, B, n):
    def rot(v):
        th = np.linalg.norm(v); k = v / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    gt, pred = np.tile(np.eye(4), (2, B, 1, 1))
    for b in range(B):
        gt[b, :3, :3] = rot(rng.normal(size=3)); gt[b, :3, 3] = [0.05, -0.02, 0.8]
        pred[b, :3, :3] = gt[b, :3, :3] @ rot(rng.normal(size=3) * 0.05); pred[b, :3, 3] = gt[b, :3, 3] + rng.normal(size=3) * 0.01
    K = np.tile(np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]]), (B, 1, 1))
    pts = (rng.uniform(-1, 1, (n, 3)) * [0.05, 0.035, 0.03]).astype(np.float32)
    return pred.astype(np.float32), gt.astype(np.float32), K.astype(np.float32), pts


def time_gpu(B, n, rng):
    pred, gt, K, pts = make(rng, B, n)
    d = lambda a: torch.from_numpy(a).cuda()
    args = (d(pred), d(gt), torch.ones(B, 3, device="cuda"), torch.eye(4, device="cuda").expand(B, 4, 4).contiguous(), d(K), d(pts),
            [0] * B, [n] * B)
    for _ in range(3):
        pm.pose_metrics(*args, t_scale="m")
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); pm.pose_metrics(*args, t_scale="m"); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    rate = B * n * n / (ms * 1e-3)
    return {"B": B, "N": n, "gpu_ms": round(ms, 4), "gpu_ms_min": round(min(ts), 4), "pairs_per_s": rate,
            "valu_peak_fraction": round(rate * OPS_PER_PAIR / VALU_LANE_OPS, 3)}


def time_host(B, n, rng):
    try:
        from scipy import spatial
    except ImportError:
        return {"B": B, "N": n, "host_ms": None, "note": "scipy not importable"}
    pred, gt, K, pts = make(rng, B, n)

    def one(b):
        mp = pts @ pred[b, :3, :3].T + pred[b, :3, 3]
        mg = pts @ gt[b, :3, :3].T + gt[b, :3, 3]
        dist, _ = spatial.cKDTree(mp).query(mg, k=1)
        return np.mean(dist), np.mean(np.linalg.norm(mp - mg, axis=-1))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as ex:
        list(ex.map(one, range(B)))
    return {"B": B, "N": n, "host_ms": round((time.perf_counter() - t0) * 1e3, 2)}


def time_copies():
    nbytes = 370 * 2 ** 20
    dev = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").fill_(1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = dev.cpu()
    d2h = (time.perf_counter() - t0) * 1e3
    a = host.numpy()
    t0 = time.perf_counter()
    for _ in range(3):
        a = a.copy()
    copies = (time.perf_counter() - t0) * 1e3
    return {"d2h_370MB_ms": round(d2h, 1), "three_host_copies_ms": round(copies, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = {"gpu": [time_gpu(32, n, rng) for n in (1000, 10000, 50000)],
            "host": [time_host(32, n, rng) for n in (1000, 10000, 50000)], "copies": time_copies()}
    for k, v in rows.items():
        for r in (v if isinstance(v, list) else [v]):
            print(k, json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
