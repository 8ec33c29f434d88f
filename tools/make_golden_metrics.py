"""Write tests/golden/pose_metrics_vectors.npz: the reference's own eval metrics on seeded inputs.

    python tools/make_golden_metrics.py [--reference PATH]

Runs the REAL `Metrics.compute_metrics` + `aggregate_metrics` of the reference (src/lightning/utils/metrics/metric_utils.py), loaded
from its file with stand-ins for the modules this image lacks (loguru, plyfile / open3d / trimesh behind sample_points_on_cad,
torchmetrics), on three small point clouds -- one of them symmetric under a 90-degree turn about z, where ADD-S << ADD -- and three
runs: (`cat`, t_scale 'm'), (no `cat`, 'mm'), (`cat`, null), two batches each.  `get_cached_points` is patched to return the clouds
(the files the reference checks for are created empty in a temporary directory).  The inputs are float32 values handed to the
reference as float64 tensors, so its per-sample values carry no float32 rounding of their own; no ADD / ADD-S / proj2D value lies
within 1e-3 (relative) of its threshold.

Stored: per run the clouds in the run's unit (`r{r}_pts_{k}`), and batch the inputs (`r{r}_b{i}_{key}`) and the model index of each sample, and per run
the reference's `metrics_result` and aggregate dict as JSON (`r{r}_result`, `r{r}_agg`).  Test infrastructure only: nothing on the
GPU path imports this file.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pose_metrics_vectors.npz")
RUNS = [("m", True), ("mm", False), (None, True)]     # (t_scale, cat)
UNIT = {"m": 1.0, "mm": 1000.0, None: 10.0}           # length unit of the run's geometry
B, T, NB = 8, 3, 2
THRESHOLDS = [1, 3, 5, 10, 15, 20, 30]


def clouds(rng):
    """obj 0: anisotropic box surface (500), obj 1: 4-fold symmetric about z (4 x 150), obj 2: ellipsoid surface (1500); metres."""
    a = rng.uniform(-1, 1, (500, 3)) * [0.06, 0.04, 0.025]
    face = rng.integers(0, 3, 500)
    a[np.arange(500), face] = np.sign(a[np.arange(500), face]) * np.array([0.06, 0.04, 0.025])[face]
    base = np.stack([rng.uniform(0.005, 0.04, 150), rng.uniform(-0.04, 0.04, 150), rng.uniform(-0.05, 0.05, 150)], -1)
    x, y, z = base.T
    sym = np.concatenate([base, np.stack([-y, x, z], -1), np.stack([-x, -y, z], -1), np.stack([y, -x, z], -1)])   # exact 90-degree turns
    e = rng.normal(size=(1500, 3))
    e = e / np.linalg.norm(e, axis=1, keepdims=True) * [0.05, 0.035, 0.03]
    return [a.astype(np.float32), sym.astype(np.float32), e.astype(np.float32)]


def rodrigues(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_batch(rng, unit, model_of):
    """Float32-valued inputs of one batch (query view only is meaningful; the other views hold noise poses)."""
    f = np.float32
    query = rng.integers(0, T, B)
    gt = np.tile(np.eye(4), (B, T, 1, 1))
    pred = np.tile(np.eye(4), (B, T, 1, 1))
    scale = rng.uniform(0.9, 1.1, (B, T, 3))
    ct = np.tile(np.eye(4), (B, 1, 1))
    K = np.tile(np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]]), (B, T, 1, 1))
    for b in range(B):
        for v in range(T):
            gt[b, v, :3, :3] = rodrigues(rng.normal(size=3))
            gt[b, v, :3, 3] = [rng.normal() * 0.1 * unit, rng.normal() * 0.1 * unit, (0.6 + 0.4 * rng.random()) * unit]
            pred[b, v] = gt[b, v]
        q = query[b]
        G = gt[b, q]
        P = G.copy()
        if model_of[b] == 1 and b % 2 == 0:        # the symmetric object under its symmetry: ADD-S ~ small, ADD large
            P[:3, :3] = G[:3, :3] @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]) @ rodrigues(rng.normal(size=3) * 0.01)
        else:
            P[:3, :3] = G[:3, :3] @ rodrigues(rng.normal(size=3) * rng.choice([0.01, 0.05, 0.2]))
        P[:3, 3] = G[:3, 3] + rng.normal(size=3) * rng.choice([0.002, 0.01, 0.05]) * unit
        C = np.eye(4)
        C[:3, :3] = rodrigues(rng.normal(size=3))
        C[:3, 3] = rng.normal(size=3) * 0.05 * unit
        S = pred[b, q] = P @ np.linalg.inv(C)        # stored so that (S with t * scale) @ C == P
        pred[b, q, :3, 3] = S[:3, 3] / scale[b, q]
        ct[b] = C
    return {"query_idx": query.astype(np.int64), "original_poses": gt.astype(f), "pred_poses": pred.astype(f),
            "scale": scale.astype(f), "coordinate_transform": ct.astype(f), "original_intrinsics": K.astype(f)}


def scaled(p, unit):
    return (p.astype(np.float64) * unit).astype(np.float32)


def model_path(root, k):
    return f"{root}/lm/models_eval/obj_{k:02d}/obj_{k:02d}.ply"


def to_data(arrs, root, model_of, cat):
    """The reference's batch dict (host tensors, float64 values of the float32 inputs)."""
    d = {k: torch.from_numpy(v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in arrs.items()}
    d["model_path"] = [[model_path(root, int(model_of[b])) for b in range(B)] for _ in range(T)]
    d["original_images"] = [[f"{root}/img/b{b}_v{v}.png" for b in range(B)] for v in range(T)]
    if cat:
        d["cat"] = [f"obj_{int(model_of[b]):02d}" for b in range(B)]
    return d


def jsonable(x):
    if isinstance(x, dict):
        return {str(k): jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist() if x.dtype.kind != "U" else str(x)
    if isinstance(x, (np.floating, float)):
        return float(x)
    if isinstance(x, (np.integer, int)):
        return int(x)
    if isinstance(x, np.str_):
        return str(x)
    return x


def load_reference(ref):
    for name in ("loguru",):
        m = types.ModuleType(name); m.logger = types.SimpleNamespace(**{k: (lambda *a, **kw: None) for k in
                                                                          ("info", "debug", "warning", "error", "critical")})
        sys.modules[name] = m
    for name in ("src", "src.utils", "src.utils.customize", "torchmetrics"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spc = types.ModuleType("src.utils.customize.sample_points_on_cad")
    spc.get_all_points_on_model = None
    sys.modules["src.utils.customize.sample_points_on_cad"] = spc
    log = types.ModuleType("src.utils.log"); log.INFO = log.ERROR = lambda *a, **k: None
    sys.modules["src.utils.log"] = log
    tmi = types.ModuleType("torchmetrics.image"); tmi.PeakSignalNoiseRatio = object
    sys.modules["torchmetrics.image"] = tmi
    spec = importlib.util.spec_from_file_location("ref_metric_utils", os.path.join(ref, "src/lightning/utils/metrics/metric_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BOXDREAMER_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    mu = load_reference(args.reference)
    rng = np.random.default_rng(20261016)
    pts = clouds(rng)
    out = {}
    out["runs"] = np.array(json.dumps([[t, c] for t, c in RUNS]))
    with tempfile.TemporaryDirectory() as root:
        for k in range(len(pts)):
            for sub in ("models_eval", "models"):
                p = model_path(root, k).replace("models_eval", sub)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                open(p, "w").close()
        cur = {}
        mu.Metrics.get_cached_points = lambda self, p: cur[os.path.realpath(p)]
        cwd = os.getcwd()
        os.chdir(root)                              # the cat branch writes path_*_dict_{id}.npy into the working directory
        try:
            for r, (t_scale, cat) in enumerate(RUNS):
                unit = UNIT[t_scale]
                cur.clear()
                for k in range(len(pts)):
                    cur[os.path.realpath(model_path(root, k).replace("models_eval", "models"))] = out[f"r{r}_pts_{k}"] = scaled(pts[k], unit)
                cfg = types.SimpleNamespace(metrics_list=["pose_error", "ADD", "proj2d"], t_scale=t_scale,
                                            pose_error=types.SimpleNamespace(pose_thresholds=THRESHOLDS),
                                            proj2d=types.SimpleNamespace(proj2d_thres=5))
                m = mu.Metrics(cfg)
                for i in range(NB):
                    while True:                     # redraw a batch until no raw value sits near its threshold
                        model_of = rng.integers(0, len(pts), B)
                        model_of[0], model_of[2] = 1, 1
                        arrs = make_batch(rng, unit, model_of)
                        probe = mu.Metrics(cfg)
                        probe.compute_metrics(to_data(arrs, root, model_of, cat))
                        flat = lambda k: np.array(probe.metrics_result[k]["all"] if cat else probe.metrics_result[k])
                        thr = np.array([np.linalg.norm(out[f"r{r}_pts_{j}"].max(0) - out[f"r{r}_pts_{j}"].min(0)) * 0.1 for j in model_of])
                        near = [np.abs(flat("ADD_raw_0") - thr) / thr, np.abs(flat("ADDs_raw_0") - thr) / thr,
                                np.abs(flat("proj2D_metric_0") - 5) / 5]
                        near += [np.abs(flat(k)[:, None] - np.array(THRESHOLDS)[None]) / np.array(THRESHOLDS)[None]
                                 for k in ("R_errs_0", "t_errs_0")]
                        if min(float(np.min(n)) for n in near) > 1e-3:
                            break
                    m.compute_metrics(to_data(arrs, root, model_of, cat))
                    for k, v in arrs.items():
                        out[f"r{r}_b{i}_{k}"] = v
                    out[f"r{r}_b{i}_model"] = model_of.astype(np.int64)
                res = jsonable(m.metrics_result)
                agg = jsonable(m.aggregate_metrics())
                out[f"r{r}_result"] = np.array(json.dumps(res).replace(root, "<root>"))
                out[f"r{r}_agg"] = np.array(json.dumps(agg))
        finally:
            os.chdir(cwd)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
