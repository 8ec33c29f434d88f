"""CPU: the host side of boxdreamer_amd.metrics -- the model-point reader, the reference's aggregation restated key for key against the
reference's own output (tests/golden/pose_metrics_vectors.npz, tools/make_golden_metrics.py), the sharded gather, and the C entry
points' argument checks (no launch)."""
import ctypes
import json
import os
from itertools import chain

import numpy as np
import pytest

from boxdreamer_amd import _lib
from boxdreamer_amd import metrics as pm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_metrics_vectors.npz")
CFG = {"metrics_list": ["pose_error", "ADD", "proj2d"], "pose_error": {"pose_thresholds": [1, 3, 5, 10, 15, 20, 30]},
       "proj2d": {"proj2d_thres": 5}}


def write_ply(path, pts, fmt="binary_little_endian", dtype="float", extra=True):
    """A PLY vertex element with x / y / z (and, with `extra`, a leading uchar and a trailing double property), then a face element."""
    n = len(pts)
    props = ([("uchar", "red", "u1")] if extra else []) + [(dtype, a, "f4" if dtype == "float" else "f8") for a in "xyz"] + \
            ([("double", "nx", "f8")] if extra else [])
    head = ["ply", f"format {fmt} 1.0", "comment written by a test", f"element vertex {n}"]
    head += [f"property {t} {name}" for t, name, _ in props]
    head += ["element face 1", "property list uchar int vertex_indices", "end_header"]
    end = {"binary_little_endian": "<", "binary_big_endian": ">", "ascii": "<"}[fmt]
    dt = np.dtype([(name, end + c) for _, name, c in props])
    rec = np.zeros(n, dt)
    for k, a in enumerate("xyz"):
        rec[a] = pts[:, k]
    if extra:
        rec["red"] = np.arange(n) % 256
        rec["nx"] = -1.5
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if fmt == "ascii":
            for r in rec:
                f.write((" ".join(repr(v.item()) for v in r) + "\n").encode())
            f.write(b"3 0 1 2\n")
        else:
            f.write(rec.tobytes())
            f.write(np.array([3], "u1").tobytes() + np.array([0, 1, 2], end + "i4").tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_ply_reader_round_trips(tmp_path, fmt, dtype):
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(37, 3)).astype(np.float32 if dtype == "float" else np.float64)
    p = str(tmp_path / "m.ply")
    write_ply(p, pts, fmt, dtype)
    got = pm.load_model_points(p)
    assert got.dtype == pts.dtype and got.shape == (37, 3)
    assert np.array_equal(got, pts)
    write_ply(p, pts, fmt, dtype, extra=False)
    assert np.array_equal(pm.load_model_points(p), pts)


def test_xyz_and_unsupported_formats(tmp_path):
    pts = np.random.default_rng(2).normal(size=(5, 3))
    np.savetxt(tmp_path / "m.xyz", pts)
    assert np.array_equal(pm.load_model_points(str(tmp_path / "m.xyz")), np.loadtxt(tmp_path / "m.xyz"))
    for ext in (".glb", ".obj"):
        with pytest.raises(NotImplementedError):
            pm.load_model_points(str(tmp_path / ("m" + ext)))
    assert pm.gt_model_path("/d/lm/models_eval/obj_01/obj_01.ply") == "/d/lm/models/obj_01/obj_01.ply"


def _golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["runs"]))


def _result_from_json(s):
    """The reference's metrics_result from the fixture: lists of floats, poses as float arrays, paths as numpy strings."""
    res = json.loads(s)

    def fix(key, v):
        if key.startswith("pred_poses"):
            return [np.array(p) for p in v]
        if key.startswith("original_paths"):
            return [np.str_(p) for p in v]
        return list(v)
    return {k: ({c: fix(k, l) for c, l in v.items()} if isinstance(v, dict) else fix(k, v)) for k, v in res.items()}


def _config(t_scale):
    return dict(CFG, t_scale=t_scale)


def _assert_agg_equal(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, dict):
            assert set(got[k]) == set(v), k
            for c in v:
                assert abs(float(got[k][c]) - v[c]) <= 1e-12, (k, c, got[k][c], v[c])
        else:
            assert abs(float(got[k]) - v) <= 1e-12, (k, got[k], v)


def test_aggregate_restates_the_reference_on_its_own_per_sample_values(tmp_path, monkeypatch):
    z, runs = _golden()
    monkeypatch.chdir(tmp_path)
    for r, (t_scale, cat) in enumerate(runs):
        m = pm.PoseMetrics(_config(t_scale))
        m.set_metrics(_result_from_json(str(z[f"r{r}_result"])))
        m.dataloader_id_set = {0}
        _assert_agg_equal(m.aggregate_metrics(), json.loads(str(z[f"r{r}_agg"])))
    assert os.listdir(tmp_path) == []                  # the path dicts are opt-in
    m.save_path_dicts = True
    m.aggregate_metrics()
    assert sorted(os.listdir(tmp_path)) == ["path_error_dict_0.npy", "path_pose_dict_0.npy"]


def flatten(data):
    """The harness's gather (DataProcessor.flatten_data, src/lightning/utils/data_utils/data_utils.py:61-85)."""
    if isinstance(data[0], dict):
        return {k: flatten([d[k] for d in data]) for k in data[0]}
    if isinstance(data[0], np.ndarray):
        return np.concatenate(data, axis=0)
    if isinstance(data[0], list):
        return list(chain(*data))
    return data


def _split(res, n_first):
    """Cut a metrics_result after the first batch: `n_first` = per list key the number of entries the first batch appended."""
    a, b = {}, {}
    for k, v in res.items():
        if isinstance(v, dict):
            a[k] = {c: l[:n_first[c]] for c, l in v.items()}
            b[k] = {c: l[n_first[c]:] for c, l in v.items()}
        else:
            a[k], b[k] = v[:n_first[None]], v[n_first[None]:]
    return a, b


def test_two_shards_gathered_aggregate_like_one_process(tmp_path, monkeypatch):
    z, runs = _golden()
    monkeypatch.chdir(tmp_path)
    for r, (t_scale, cat) in enumerate(runs):
        res = _result_from_json(str(z[f"r{r}_result"]))
        model0 = z[f"r{r}_b0_model"]
        n_first = {None: len(model0), "all": len(model0)}
        n_first.update({f"obj_{k:02d}": int((model0 == k).sum()) for k in range(3)})
        s0, s1 = _split(res, n_first)
        if cat:                                          # pred_poses / original_paths keep an empty "all" list, as the reference's
            for k in ("pred_poses_0", "original_paths_0"):
                assert res[k]["all"] == []
        gathered = flatten([s0, s1])
        one, two = pm.PoseMetrics(_config(t_scale)), pm.PoseMetrics(_config(t_scale))
        one.set_metrics(res); one.dataloader_id_set = {0}
        two.set_metrics(gathered); two.dataloader_id_set = {0}
        _assert_agg_equal(two.aggregate_metrics(), {k: (dict(v) if isinstance(v, dict) else v)
                                                    for k, v in json.loads(json.dumps(one.aggregate_metrics(), default=float)).items()})


def test_config_forms_and_unsupported_metrics():
    m = pm.PoseMetrics(_config("m"))
    assert m.metrics_config.pose_error.pose_thresholds[0] == 1 and m.metrics_config.proj2d.proj2d_thres == 5
    with pytest.raises(NotImplementedError):
        pm.PoseMetrics(dict(CFG, t_scale="m", metrics_list=["pose_error", "image"]))
    with pytest.raises(AssertionError):
        pm.PoseMetrics(None)
    m.set_metrics({"x": [1.0]})
    assert m.get_metrics() == {"x": [1.0]}
    m.reset()
    assert m.get_metrics() == {} and m.dataloader_id_set == set()


def test_auc_helpers_restate_the_reference_formulas():
    errs = np.array([0.0005, 0.02, 0.0999, 0.5])
    X = np.arange(0, 0.1 + 0.001, 0.001)
    Y = np.array([(errs <= x).sum() / len(errs) for x in X])
    assert pm.compute_auc_sklearn(errs) == pytest.approx(float(np.trapezoid(Y, X)) / 0.1, abs=1e-15)
    small = np.array([0.0005, 0.001])                    # reaches 1 at x = 0.001: the rest of Y stays 1 (the early break)
    assert pm.compute_auc_sklearn(small) == pytest.approx(float(np.trapezoid(np.r_[0.0, np.ones(len(X) - 1)], X)) / 0.1, abs=1e-15)
    assert pm.auc_add(np.array([0.0])) == pytest.approx(1.0)
    assert pm.auc_proj2d(np.array([np.inf, np.nan])) == 0.0


def test_pose_metrics_entry_points_reject_bad_arguments_without_launching():
    lib = _lib.load()
    assert lib.bd_pose_metrics_workspace_bytes(0, 10) == 0 and lib.bd_pose_metrics_workspace_bytes(4, 0) == 0
    assert lib.bd_pose_metrics_workspace_bytes(70000, 10) == 0
    ws = lib.bd_pose_metrics_workspace_bytes(32, 10000)
    assert ws >= 32 * 10000 * 4 and ws % (32 * 10000 * 4) == 0
    fake = ctypes.c_void_p(0x1000)                       # never dereferenced: every call below fails its checks first
    args = [fake] * 8
    assert lib.bd_pose_metrics(None, *args[1:], 4, 100, 1, fake, ws, fake, None) == -5
    assert lib.bd_pose_metrics(*args, 4, 100, 1, None, ws, fake, None) == -5
    assert lib.bd_pose_metrics(*args, 4, 100, 1, fake, ws, None, None) == -5
    assert lib.bd_pose_metrics(*args, 0, 100, 1, fake, ws, fake, None) == -1
    assert lib.bd_pose_metrics(*args, 4, 0, 1, fake, ws, fake, None) == -1
    assert lib.bd_pose_metrics(*args, 4, 100, 3, fake, ws, fake, None) == -1
    assert lib.bd_pose_metrics(*args, 4, 100, -1, fake, ws, fake, None) == -1
    need = lib.bd_pose_metrics_workspace_bytes(4, 100)
    assert lib.bd_pose_metrics(*args, 4, 100, 1, fake, need - 1, fake, None) == -4
