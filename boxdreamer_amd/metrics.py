"""Eval-step pose metrics on the device: a drop-in for the reference's `Metrics`
(src/lightning/utils/metrics/metric_utils.py of the reference).

The reference copies the whole batch to the host (`back_to_cpu`), deep-copies it three times and runs R / t errors, proj2D and
ADD / ADD-S per sample on thread pools, ADD-S through a scipy cKDTree per pose.  Here the six per-sample values of a batch come
out of one library call (`bd_pose_metrics`, csrc/metrics.hip) on the device; the host receives B x 6 values plus the composed
query poses it records, in one copy.  The bookkeeping (`metrics_result` keys and layout, `aggregate_metrics`) restates the
reference key for key, so the Lightning module's gather (`get_metrics` / `set_metrics`) and its JSON dump work unchanged.

No CPU fallback for the compute: without the library or a GPU the call raises HipLibraryError.
"""
from __future__ import annotations

import os
import types

import numpy as np
import torch

from . import _lib

T_SCALE = {None: 0, "m": 1, "mm": 2}
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


# ------------------------------------------------------------------------------------------------------------------------------
# model points
# ------------------------------------------------------------------------------------------------------------------------------
def _read_ply_vertices(path: str) -> np.ndarray:
    """x / y / z of the first element of a PLY file (ascii, binary_little_endian, binary_big_endian), in the stored dtype --
    what plyfile's `PlyData.read(path).elements[0].data[['x', 'y', 'z']]` gives the reference.  Other properties are skipped."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header without end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "end_header":
                break
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: property before any element")
                if tok[1] == "list":
                    elements[-1][2].append((tok[4], ("list", tok[2], tok[3])))
                else:
                    elements[-1][2].append((tok[2], tok[1]))
        if not elements:
            raise ValueError(f"{path}: PLY without elements")
        name, count, props = elements[0]
        if any(isinstance(t, tuple) for _, t in props):
            raise ValueError(f"{path}: list properties in the vertex element are not supported")
        names = [p for p, _ in props]
        for axis in ("x", "y", "z"):
            if axis not in names:
                raise ValueError(f"{path}: element {name!r} has no property {axis!r}")
        if fmt == "ascii":
            rows = []
            for _ in range(count):
                rows.append(f.readline().split())
            cols = {p: np.array([r[k] for r in rows], dtype=_PLY_TYPES[t]) for k, (p, t) in enumerate(props)}
            return np.stack([cols["x"], cols["y"], cols["z"]], axis=-1)
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unknown PLY format {fmt!r}")
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(p, end + _PLY_TYPES[t]) for p, t in props])
        data = np.frombuffer(f.read(dt.itemsize * count), dtype=dt, count=count)
        return np.stack([data["x"], data["y"], data["z"]], axis=-1).astype(data["x"].dtype.newbyteorder("="))


def load_model_points(path: str) -> np.ndarray:
    """`get_all_points_on_model` (src/utils/customize/sample_points_on_cad.py:148-177) for `.ply` and `.xyz`: (N, 3) points in the
    file's dtype (float32 for `float` PLY properties, float64 for `double` and for `.xyz`, which numpy.loadtxt reads)."""
    if path.endswith(".ply"):
        return _read_ply_vertices(path)
    if path.endswith(".glb") or path.endswith(".obj"):
        raise NotImplementedError(f"mesh sampling of {path} (.glb / .obj) is not provided; convert the model to .ply or .xyz")
    if path.endswith(".xyz"):
        return np.loadtxt(path)
    raise NotImplementedError(f"Model format {path} not implemented")


def gt_model_path(model_path: str) -> str:
    """The reference's rewrite (metric_utils.py:269-270, :351-352): xxx/models_suffix/obj_id/obj_id.ply -> the `models` tree."""
    suffix = model_path.split("/")[-3]
    return model_path.replace(suffix, "models")


class ModelBank:
    """Model points resident on one device, each object uploaded once, keyed by its resolved path.  All objects live in one packed
    fp32 (N, 3) buffer; `diameter_thres[key]` is the reference's 0.1 d (:387-390) computed on the host in the file's dtype."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.points = torch.zeros(0, 3, dtype=torch.float32, device=self.device)
        self.slots = {}                 # key -> (offset, count)
        self.diameter_thres = {}

    def add(self, key: str, pts: np.ndarray) -> tuple:
        if key in self.slots:
            return self.slots[key]
        pts = np.asarray(pts)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError(f"{key}: model points must be a non-empty (N, 3) array, got {pts.shape}")
        diameter = np.linalg.norm(np.max(pts, axis=0) - np.min(pts, axis=0))
        self.diameter_thres[key] = diameter * 0.1
        dev = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(self.device)
        self.slots[key] = (self.points.shape[0], pts.shape[0])
        self.points = torch.cat([self.points, dev], 0)
        return self.slots[key]

    def load(self, model_path: str) -> str:
        key = os.path.realpath(gt_model_path(model_path))
        if key not in self.slots:
            if not os.path.exists(key):
                raise FileNotFoundError(f"Model path does not exist: {key}")
            self.add(key, load_model_points(key))
        return key


# ------------------------------------------------------------------------------------------------------------------------------
# the op
# ------------------------------------------------------------------------------------------------------------------------------
def pose_metrics(pred_poses, original_poses, scale, coordinate_transform, original_intrinsics, points, pt_offset, pt_count,
                 t_scale=None, max_points=None) -> torch.Tensor:
    """Per pose b: (R_err deg, t_err, inplane_R_err deg, proj2d px, add, adds) as a float64 (B, 6) device tensor.

    pred_poses / original_poses (B, 4, 4), scale (B, 3) (or (B,) / (B, 1), broadcast), coordinate_transform (B, 4, 4),
    original_intrinsics (B, 3, 3): the QUERY view of each sample, on one device; cast to contiguous fp32.  points: fp32 (P, 3) on
    the device; pose b uses rows pt_offset[b] : pt_offset[b] + pt_count[b] (sequences or tensors).  t_scale: None / 'm' / 'mm'."""
    lib = _lib.load()
    _lib.require_gpu()
    dev = _lib.same_device(points)
    if dev is None:
        raise _lib.HipLibraryError("pose_metrics needs the model points on a HIP device")
    f32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
    pred, gt, ct, K = f32(pred_poses), f32(original_poses), f32(coordinate_transform), f32(original_intrinsics)
    B = pred.shape[0]
    if pred.shape != (B, 4, 4) or gt.shape != (B, 4, 4) or ct.shape != (B, 4, 4) or K.shape != (B, 3, 3):
        raise ValueError(f"pose_metrics: shapes {tuple(pred.shape)}, {tuple(gt.shape)}, {tuple(ct.shape)}, {tuple(K.shape)}")
    if t_scale not in T_SCALE:
        raise ValueError(f"t_scale must be None, 'm' or 'mm', got {t_scale!r}")
    sc = f32(scale).reshape(B, -1).expand(B, 3).contiguous()
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError("pose_metrics: points must be a contiguous fp32 (P, 3) tensor")
    off_h = np.asarray(torch.as_tensor(pt_offset).cpu(), dtype=np.int64).reshape(-1)
    cnt_h = np.asarray(torch.as_tensor(pt_count).cpu(), dtype=np.int64).reshape(-1)
    if off_h.shape != (B,) or cnt_h.shape != (B,) or (cnt_h <= 0).any() or (off_h < 0).any() or (off_h + cnt_h > points.shape[0]).any():
        raise ValueError("pose_metrics: every pose needs 1.. points inside the packed buffer")
    mp = int(cnt_h.max()) if max_points is None else int(max_points)
    if mp < cnt_h.max():
        raise ValueError(f"pose_metrics: max_points {mp} < the largest count {int(cnt_h.max())}")
    off = torch.from_numpy(off_h).to(dev)
    cnt = torch.from_numpy(cnt_h.astype(np.int32)).to(dev)
    ws_bytes = lib.bd_pose_metrics_workspace_bytes(B, mp)
    if ws_bytes == 0:
        raise ValueError(f"pose_metrics: unsupported batch {B} x {mp} points")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 6, dtype=torch.float64, device=dev)
    p = _lib.ptr
    rc = lib.bd_pose_metrics(p(pred), p(gt), p(sc), p(ct), p(K), p(points), p(off), p(cnt), B, mp, T_SCALE[t_scale], p(ws), ws_bytes, p(out),
                             _lib.stream())
    _lib.check(rc, "bd_pose_metrics")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the Metrics drop-in
# ------------------------------------------------------------------------------------------------------------------------------
def _attr(cfg):
    """DictConfig or plain (nested) dict -> attribute access, as the reference reads its config."""
    if isinstance(cfg, dict):
        return types.SimpleNamespace(**{k: _attr(v) for k, v in cfg.items()})
    return cfg


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _trapezoid_auc(X, Y):
    """sklearn.metrics.auc on an increasing X: the trapezoid rule."""
    return float(np.trapezoid(Y, X))


def auc_add(metrics):
    """metric_utils.py:770-776."""
    thresholds = np.linspace(0.0, 0.10, 1000)
    x_range = thresholds.max() - thresholds.min()
    accuracies = [(metrics <= t).sum() / len(metrics) for t in thresholds]
    return _trapezoid_auc(thresholds, accuracies) / x_range


def auc_proj2d(metrics):
    """metric_utils.py:779-785."""
    thresholds = np.linspace(0, 40.0, 1000)
    x_range = thresholds.max() - thresholds.min()
    accuracies = [(metrics <= t).sum() / len(metrics) for t in thresholds]
    return _trapezoid_auc(thresholds, accuracies) / x_range


def compute_auc_sklearn(errs, max_val=0.1, step=0.001):
    """metric_utils.py:788-800, including the early break that leaves the remaining Y at 1."""
    errs = np.sort(np.array(errs))
    X = np.arange(0, max_val + step, step)
    Y = np.ones(len(X))
    for i, x in enumerate(X):
        y = (errs <= x).sum() / len(errs)
        Y[i] = y
        if y >= 1:
            break
    return _trapezoid_auc(X, Y) / (max_val * 1)


class PoseMetrics:
    """Drop-in for the reference's `Metrics` (same constructor, `compute_metrics`, `get_metrics` / `set_metrics`, `reset` /
    `reset_config` / `set_data`, `aggregate_metrics`, and the same `metrics_result` keys and layout, with and without `cat`).

    `compute_metrics(data)` reads the batch where it lies (device or host) and makes no copy of it: the query view of every sample is
    gathered, the six per-sample values come from `bd_pose_metrics` on the model bank's device, and one B x 22 copy brings them and the
    composed query poses to the host.  Rows are appended in batch order (the reference appends from threads, in any order; no
    aggregate depends on it).  The `"image"` metric (PSNR) is not provided.

    `aggregate_metrics` writes the reference's `path_pose_dict_{id}.npy` / `path_error_dict_{id}.npy` into the working directory
    (the `cat` layout) only with `save_path_dicts=True`; by default it writes no file."""

    def __init__(self, metrics_config=None, device=None, save_path_dicts: bool = False):
        assert metrics_config is not None, "Metrics config is None!"
        self.metrics_config = _attr(metrics_config)
        if "image" in self.metrics_config.metrics_list:
            raise NotImplementedError("the 'image' metric (PSNR) is not provided by boxdreamer_amd.metrics")
        self.metrics_result = {}
        self.data = None
        self.dataloader_id = 0
        self.dataloader_id_set = set()
        self.save_path_dicts = save_path_dicts
        self._device = torch.device(device) if device is not None else None
        self._bank = None

    # --- the reference's small API -----------------------------------------------------------------------------------------
    def reset(self):
        self.metrics_result = {}
        self.data = None
        self.dataloader_id_set = set()

    def reset_config(self, metrics_config):
        self.metrics_config = _attr(metrics_config)

    def set_data(self, data):
        self.data = data

    def get_metrics(self):
        return self.metrics_result

    def set_metrics(self, metrics):
        self.metrics_result = metrics

    def bank(self, device=None) -> ModelBank:
        """The device-resident model points: on `device=` of the constructor, else on the device of the first batch's
        predictions, else on the current HIP device."""
        if self._bank is None:
            _lib.require_gpu()
            if self._device is not None:
                dev = self._device
            elif device is not None and torch.device(device).type == "cuda":
                dev = torch.device(device)
            else:
                dev = torch.device("cuda", torch.cuda.current_device())
            self._bank = ModelBank(dev)
        return self._bank

    # --- per batch -----------------------------------------------------------------------------------------------------------
    def compute_metrics(self, data, dataloader_id=0):
        self.dataloader_id = dataloader_id
        self.dataloader_id_set.add(dataloader_id)
        mlist = self.metrics_config.metrics_list
        if "pose_error" not in mlist:
            self.reset()
            return None
        want_2d, want_add = "proj2d" in mlist, "ADD" in mlist
        qidx = _np(data["query_idx"]).astype(np.int64).reshape(-1)
        B = len(qidx)
        src = data["pred_poses"]
        bank = self.bank(src.device if torch.is_tensor(src) else None)
        dev = bank.device
        bi = torch.arange(B, device=dev)
        qi = torch.from_numpy(qidx).to(dev)

        def q(key):                         # the query view of every sample, fp32 on the bank's device
            return torch.as_tensor(data[key]).to(dev)[bi, qi].to(torch.float32)

        pred, gt, K = q("pred_poses"), q("original_poses"), q("original_intrinsics")
        scale = q("scale").reshape(B, -1).expand(B, 3)
        ct = torch.as_tensor(data["coordinate_transform"]).to(dev)[bi].to(torch.float32)
        keys, off, cnt = [], [], []
        for b in range(B):
            key = bank.load(data["model_path"][qidx[b]][b])
            o, c = bank.slots[key]
            keys.append(key); off.append(o); cnt.append(c)
        vals = pose_metrics(pred, gt, scale, ct, K, bank.points, off, cnt, t_scale=self.metrics_config.t_scale)
        composed = pred.clone()
        composed[:, :3, 3] *= scale
        composed = composed @ ct
        host = torch.cat([vals, composed.reshape(B, 16).to(torch.float64)], 1).cpu().numpy()     # the one copy of the batch
        R_errs, t_errs, in_errs = host[:, 0], host[:, 1], host[:, 2]
        composed = host[:, 6:].reshape(B, 4, 4).astype(np.float32)
        original_paths = np.array(data["original_images"])[qidx, np.arange(B)]
        cat = data.get("cat", None)
        did = dataloader_id
        res = self.metrics_result
        names = (f"R_errs_{did}", f"t_errs_{did}", f"inplane_R_errs_{did}", f"pred_poses_{did}", f"original_paths_{did}")
        rows = [[float(R_errs[b]), float(t_errs[b]), float(in_errs[b]), composed[b], original_paths[b]] for b in range(B)]
        if cat is not None:
            for k in names:
                res.setdefault(k, {}).setdefault("all", [])
            for b, category in enumerate(cat):
                for k, v in zip(names, rows[b]):
                    res[k].setdefault(category, []).append(v)
                for k, v in zip(names[:3], rows[b][:3]):
                    res[k]["all"].append(v)
        else:
            for k in names:
                res.setdefault(k, [])
            for b in range(B):
                for k, v in zip(names, rows[b]):
                    res[k].append(v)

        def put(key, b, v):
            if cat is not None:
                res.setdefault(key, {}).setdefault(cat[b], []).append(v)
                res[key].setdefault("all", []).append(v)
            else:
                res.setdefault(key, []).append(v)

        for b in range(B):
            if want_2d:
                put(f"proj2D_metric_{did}", b, float(host[b, 3]))
            if want_add:
                add, adds = float(host[b, 4]), float(host[b, 5])
                thres = bank.diameter_thres[keys[b]]
                put(f"ADD_0.1d_{did}", b, 1.0 if add < thres else 0.0)
                put(f"ADD_raw_{did}", b, add)
                put(f"ADDs_0.1d_{did}", b, 1.0 if adds < thres else 0.0)
                put(f"ADDs_raw_{did}", b, adds)
        return {"R_err": tuple(rows[b][0] for b in range(B)), "t_err": tuple(rows[b][1] for b in range(B)),
                "inplane_R_err": tuple(rows[b][2] for b in range(B))}

    # --- aggregation (metric_utils.py:556-718) -------------------------------------------------------------------------------
    def aggregate_metrics(self):
        agg_metric = {}
        cfg = self.metrics_config
        for dataloader_id in self.dataloader_id_set:
            prefix = f"_{dataloader_id}"
            R_key, t_key, inplane_R_key = f"R_errs{prefix}", f"t_errs{prefix}", f"inplane_R_errs{prefix}"
            ADD_key, ADDs_key = f"ADD_0.1d_{dataloader_id}", f"ADDs_0.1d_{dataloader_id}"
            ADD_raw_key, ADDs_raw_key = f"ADD_raw_{dataloader_id}", f"ADDs_raw_{dataloader_id}"
            proj2D_key, psnr_key = f"proj2D_metric_{dataloader_id}", f"psnr_{dataloader_id}"
            eval_size_key = f"eval size_{dataloader_id}"
            pred_pose_key, original_paths_key = f"pred_poses_{dataloader_id}", f"original_paths_{dataloader_id}"
            res = self.metrics_result
            unit = "cm" if cfg.t_scale else "degree"
            if isinstance(res[R_key], dict):
                path_pose_dict, path_error_dict = {}, {}
                for cat, R_errs in res[R_key].items():
                    t_errs = np.array(res[t_key][cat])
                    R_errs = np.array(R_errs)
                    inplane_R_errs = np.array(res[inplane_R_key][cat])
                    eval_length = len(R_errs)
                    for threshold in cfg.pose_error.pose_thresholds:
                        condition = ((R_errs < threshold) & (t_errs < threshold)).astype(np.float32)
                        agg_metric.setdefault(f"{threshold}{unit}@{threshold}degree_{dataloader_id}", {})[cat] = np.mean(condition)
                    if ADD_key in res:
                        agg_metric.setdefault(f"ADD-0.1d {dataloader_id}", {})[cat] = np.mean(np.array(res[ADD_key][cat]))
                        agg_metric.setdefault(f"ADDs-0.1d {dataloader_id}", {})[cat] = np.mean(np.array(res[ADDs_key][cat]))
                        ADD_raw = np.array(res[ADD_raw_key][cat])
                        agg_metric.setdefault(f"ADD-AUC(10cm) {dataloader_id}", {})[cat] = auc_add(ADD_raw)
                        agg_metric.setdefault(f"ADD-AUC {dataloader_id}", {})[cat] = compute_auc_sklearn(ADD_raw)
                        adds_raw = np.array(res[ADDs_raw_key][cat])
                        agg_metric.setdefault(f"ADDs-AUC(10cm) {dataloader_id}", {})[cat] = auc_add(adds_raw)
                        agg_metric.setdefault(f"ADDs-AUC {dataloader_id}", {})[cat] = compute_auc_sklearn(adds_raw)
                    if proj2D_key in res:
                        proj2D_metric = np.array(res[proj2D_key][cat])
                        condition_2d = (proj2D_metric < cfg.proj2d.proj2d_thres).astype(np.float32)
                        agg_metric.setdefault(f"proj2D@5px {dataloader_id}", {})[cat] = np.mean(condition_2d)
                        agg_metric.setdefault(f"proj2D-AUC(40px) {dataloader_id}", {})[cat] = auc_proj2d(proj2D_metric)
                    if psnr_key in res:
                        agg_metric.setdefault(f"psnr_{dataloader_id}", {})[cat] = np.mean(np.array(res[psnr_key][cat]))
                    agg_metric.setdefault(eval_size_key, {})[cat] = eval_length
                    agg_metric.setdefault(f"avg_err_R_{dataloader_id}", {})[cat] = np.mean(R_errs)
                    agg_metric.setdefault(f"avg_err_t_{dataloader_id}", {})[cat] = np.mean(t_errs)
                    agg_metric.setdefault(f"avg_err_inplane_R_{dataloader_id}", {})[cat] = np.mean(inplane_R_errs)
                    pred_poses = res[pred_pose_key][cat]
                    original_paths = res[original_paths_key][cat]
                    path_pose_dict[cat], path_error_dict[cat] = {}, {}
                    for i, path in enumerate(original_paths):
                        path_pose_dict[cat][np.asarray(path).item()] = pred_poses[i]
                        path_error_dict[cat][np.asarray(path).item()] = R_errs[i]
                if self.save_path_dicts:
                    np.save(f"path_pose_dict_{dataloader_id}.npy", path_pose_dict)
                    np.save(f"path_error_dict_{dataloader_id}.npy", path_error_dict)
            else:
                R_errs = np.array(res[R_key])
                t_errs = np.array(res[t_key])
                inplane_R_errs = np.array(res[inplane_R_key])
                eval_length = len(R_errs)
                for threshold in cfg.pose_error.pose_thresholds:
                    condition = ((R_errs < threshold) & (t_errs < threshold)).astype(np.float32)
                    agg_metric[f"{threshold}{unit}@{threshold}degree_{dataloader_id}"] = np.mean(condition)
                if ADD_key in res:
                    agg_metric[f"ADD metric_{dataloader_id}"] = np.mean(np.array(res[ADD_key]))
                if proj2D_key in res:
                    condition_2d = (np.array(res[proj2D_key]) < cfg.proj2d.proj2d_thres).astype(np.float32)
                    agg_metric[f"proj2D metric_{dataloader_id}"] = np.mean(condition_2d)
                if psnr_key in res:
                    agg_metric[f"psnr_{dataloader_id}"] = np.mean(np.array(res[psnr_key]))
                agg_metric[eval_size_key] = eval_length
                agg_metric[f"avg_err_R_{dataloader_id}"] = np.mean(R_errs)
                agg_metric[f"avg_err_t_{dataloader_id}"] = np.mean(t_errs)
                agg_metric[f"avg_err_inplane_R_{dataloader_id}"] = np.mean(inplane_R_errs)
        return agg_metric
