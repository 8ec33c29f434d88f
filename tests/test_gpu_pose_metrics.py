"""GPU: the eval-step pose metrics (boxdreamer_amd.metrics, csrc/metrics.hip) against the reference's own values
(tests/golden/pose_metrics_vectors.npz), against an fp64 brute-force restatement, for determinism, and end to end after
`BoxDreamer.forward`."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from boxdreamer_amd import metrics as pm
from boxdreamer_amd import synth
from boxdreamer_amd.model import BoxDreamer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = {"metrics_list": ["pose_error", "ADD", "proj2d"], "pose_error": {"pose_thresholds": [1, 3, 5, 10, 15, 20, 30]},
       "proj2d": {"proj2d_thres": 5}}
NAMES = ("R_err", "t_err", "inplane_R_err", "proj2d", "add", "adds")


def write_ply(path, pts):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.ascontiguousarray(pts, dtype="<f4").tobytes())


def reference_fp64(pred, gt, scale, ct, K, pts, t_scale):
    """The reference's per-sample formulas (metric_utils.py:162-211, :224-306, :331-424) in fp64 on the host; ADD-S by brute force."""
    pred, gt, ct, K = (torch.as_tensor(x).double().cpu() for x in (pred, gt, ct, K))
    sc = torch.as_tensor(scale).double().cpu().reshape(-1)
    x = torch.as_tensor(pts).double().cpu()
    P = pred.clone()
    P[:3, 3] *= sc.expand(3)
    P = P @ ct
    Rp, tp, Rg, tg = P[:3, :3], P[:3, 3], gt[:3, :3], gt[:3, 3]
    t_err = torch.linalg.norm(tp - tg).item() * {"m": 100.0, "mm": 0.1, None: 1.0}[t_scale]
    D = Rp @ Rg.T
    tr = float(np.clip(torch.trace(D).item(), -1.0, 3.0))
    r_err = float(np.rad2deg(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))))
    inpl = abs(float(np.rad2deg(np.arctan2(D[1, 0].item(), D[0, 0].item()))))
    yp, yg = x @ Rp.T + tp, x @ Rg.T + tg
    add = torch.linalg.norm(yp - yg, dim=-1).mean().item()
    up, ug = yp @ K.T, yg @ K.T
    with np.errstate(all="ignore"):
        d = (up[:, :2] / up[:, 2:3]) - (ug[:, :2] / ug[:, 2:3])
        proj = float(np.mean(np.linalg.norm(d.numpy(), axis=1)))
    best = torch.empty(len(x), dtype=torch.float64)
    for i in range(0, len(x), 512):
        best[i:i + 512] = torch.cdist(yg[i:i + 512], yp, compute_mode="use_mm_for_euclid_dist").min(1)[0]
    return np.array([r_err, t_err, inpl, proj, add, best.mean().item()])


def check_close(got, want, radius, what=""):
    got = np.asarray(got, np.float64)
    assert abs(got[0] - want[0]) <= 2e-4 + 1e-5 * abs(want[0]), (what, "R_err", got[0], want[0])     # arccos conditioning near 0
    assert abs(got[2] - want[2]) <= 2e-4 + 1e-5 * abs(want[2]), (what, "inplane", got[2], want[2])
    for k in (1, 3, 4):
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-12, (what, NAMES[k], got[k], want[k])
    assert abs(got[5] - want[5]) <= 1e-5 * abs(want[5]) + 4e-7 * radius, (what, "adds", got[5], want[5])


def rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_poses(rng, B, noise=0.1):
    gt, pred, ct = np.tile(np.eye(4), (3, B, 1, 1))
    for b in range(B):
        gt[b, :3, :3] = rodrigues(rng.normal(size=3))
        gt[b, :3, 3] = [rng.normal() * 0.1, rng.normal() * 0.1, 0.6 + 0.4 * rng.random()]
        pred[b, :3, :3] = gt[b, :3, :3] @ rodrigues(rng.normal(size=3) * noise)
        pred[b, :3, 3] = gt[b, :3, 3] + rng.normal(size=3) * 0.02
        ct[b, :3, :3] = rodrigues(rng.normal(size=3) * 0.3)
        ct[b, :3, 3] = rng.normal(size=3) * 0.01
    K = np.tile(np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]]), (B, 1, 1))
    scale = rng.uniform(0.95, 1.05, (B, 3))
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    return f(pred), f(gt), f(scale), f(ct), f(K)


def run(pred, gt, scale, ct, K, clouds, which, t_scale="m"):
    pts = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).cuda()
    starts = np.cumsum([0] + [len(c) for c in clouds])
    off = [int(starts[w]) for w in which]
    cnt = [len(clouds[w]) for w in which]
    out = pm.pose_metrics(pred.cuda(), gt.cuda(), scale.cuda(), ct.cuda(), K.cuda(), pts, off, cnt, t_scale=t_scale)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def cloud(rng, n, ext=(0.05, 0.035, 0.03)):
    return (rng.uniform(-1, 1, (n, 3)) * ext).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------------------------
def _golden_batch(z, r, i, root, cat, dev):
    arr = {k: torch.from_numpy(z[f"r{r}_b{i}_{k}"]).to(dev) for k in
           ("query_idx", "original_poses", "pred_poses", "scale", "coordinate_transform", "original_intrinsics")}
    model = z[f"r{r}_b{i}_model"]
    B, T = arr["pred_poses"].shape[:2]
    arr["model_path"] = [[f"{root}/lm/models_eval/obj_{int(model[b]):02d}/obj_{int(model[b]):02d}.ply" for b in range(B)] for _ in range(T)]
    arr["original_images"] = [[f"<root>/img/b{b}_v{v}.png" for b in range(B)] for v in range(T)]
    if cat:
        arr["cat"] = [f"obj_{int(model[b]):02d}" for b in range(B)]
    return arr


@pytest.mark.parametrize("on_device", [True, False])
def test_against_the_reference_fixture(tmp_path, monkeypatch, on_device):
    z = np.load(os.path.join(HERE, "golden", "pose_metrics_vectors.npz"))
    runs = json.loads(str(z["runs"]))
    monkeypatch.chdir(tmp_path)
    for r, (t_scale, cat) in enumerate(runs):
        root = str(tmp_path / f"run{r}")
        for k in range(3):
            write_ply(f"{root}/lm/models/obj_{k:02d}/obj_{k:02d}.ply", z[f"r{r}_pts_{k}"])
        m = pm.PoseMetrics(dict(CFG, t_scale=t_scale))
        for i in range(2):
            m.compute_metrics(_golden_batch(z, r, i, root, cat, "cuda" if on_device else "cpu"))
        want = json.loads(str(z[f"r{r}_result"]))
        got = m.get_metrics()
        assert set(got) == set(want)
        flat = lambda d, k: (d[k]["all"] if cat else d[k])
        # R / t / in-plane rows are in batch order in both; the reference appends proj2D and ADD rows from a thread pool, in any
        # order (metric_utils.py:308-329, :426-447), so those lists are compared as sorted multisets
        for k, rel, ab, order in (("t_errs_0", 1e-5, 0, False), ("R_errs_0", 1e-5, 2e-4, False), ("inplane_R_errs_0", 1e-5, 2e-4, False),
                                  ("ADD_raw_0", 1e-5, 0, True), ("ADDs_raw_0", 1e-5, 0, True), ("proj2D_metric_0", 1e-5, 0, True)):
            for c in (list(want[k]) if cat else [None]):
                g = np.array(got[k][c] if cat else got[k])
                w = np.array(want[k][c] if cat else want[k])
                if order:
                    g, w = np.sort(g), np.sort(w)
                assert np.all(np.abs(g - w) <= rel * np.abs(w) + ab), (r, k, c, g, w)
        for k in ("ADD_0.1d_0", "ADDs_0.1d_0"):
            for c in (list(want[k]) if cat else [None]):
                assert sorted(got[k][c] if cat else got[k]) == sorted(want[k][c] if cat else want[k]), (r, k, c)
        if cat:
            for c, poses in want["pred_poses_0"].items():
                assert np.allclose(np.array(got["pred_poses_0"][c]), np.array(poses), atol=1e-5)
        agg, wagg = m.aggregate_metrics(), json.loads(str(z[f"r{r}_agg"]))
        assert set(agg) == set(wagg)
        for k, v in wagg.items():
            for c in (v if isinstance(v, dict) else [None]):
                g, w = (agg[k][c], v[c]) if c is not None else (agg[k], v)
                tol = 2e-3 if "AUC" in k else 1e-5 * max(1.0, abs(w))      # an AUC step is 1 / (1000 n); the others are exact or averages
                assert abs(float(g) - w) <= tol, (r, k, c, g, w)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 10007, 50000])
def test_against_fp64_brute_force(n):
    rng = np.random.default_rng(n)
    B = 1 if n == 50000 else 3
    pred, gt, scale, ct, K = random_poses(rng, B)
    c = cloud(rng, n)
    got = run(pred, gt, scale, ct, K, [c], [0] * B)
    for b in range(B):
        check_close(got[b], reference_fp64(pred[b], gt[b], scale[b], ct[b], K[b], c, "m"), 0.07, (n, b))


def test_mixed_models_in_one_batch_of_64():
    rng = np.random.default_rng(64)
    clouds = [cloud(rng, 100), cloud(rng, 2500, (0.1, 0.02, 0.02)), cloud(rng, 777)]
    which = rng.integers(0, 3, 64)
    pred, gt, scale, ct, K = random_poses(rng, 64)
    got = run(pred, gt, scale, ct, K, clouds, which, t_scale="mm")
    for b in range(64):
        check_close(got[b], reference_fp64(pred[b], gt[b], scale[b], ct[b], K[b], clouds[which[b]], "mm"), 0.1, b)


def test_identical_poses_and_a_symmetric_object():
    rng = np.random.default_rng(5)
    c = cloud(rng, 3000)
    pred, gt, scale, ct, K = random_poses(rng, 4)
    ones, eye = torch.ones(4, 3), torch.eye(4).expand(4, 4, 4).contiguous()
    got = run(gt, gt, ones, eye, K, [c], [0] * 4)
    assert (got[:, 3] == 0).all() and (got[:, 4] == 0).all()
    radius = float(np.linalg.norm(c, axis=1).max())
    assert (np.abs(got[:, 5]) <= 4 * np.finfo(np.float32).eps * radius).all()
    assert (got[:, 0] <= 0.05).all() and (got[:, 1] == 0).all()
    base = cloud(rng, 500)
    x, y, zz = base.T
    sym = np.concatenate([base, np.stack([-y, x, zz], -1), np.stack([-x, -y, zz], -1), np.stack([y, -x, zz], -1)]).astype(np.float32)
    turned = gt.clone()
    turned[:, :3, :3] = gt[:, :3, :3] @ torch.tensor([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    got = run(turned, gt, ones, eye, K, [sym], [0] * 4)
    assert (got[:, 5] <= 1e-6).all() and (got[:, 4] > 0.01).all()
    for b in range(4):
        check_close(got[b], reference_fp64(turned[b], gt[b], ones[b], eye[b], K[b], sym, "m"), 0.07, b)


def test_point_on_the_camera_plane_gives_numpys_non_finite_proj2d(tmp_path, monkeypatch):
    rng = np.random.default_rng(9)
    c = cloud(rng, 200)
    c[17] = [0.01, 0.02, 0.0]
    gt = torch.eye(4).expand(2, 4, 4).contiguous()                      # the gt camera sees point 17 at depth 0
    pred = gt.clone()
    pred[:, :3, 3] = torch.tensor([[0.01, 0, 0.5], [0, 0.02, 0.3]])
    ones, eye = torch.ones(2, 3), torch.eye(4).expand(2, 4, 4).contiguous()
    K = torch.tensor([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]]).expand(2, 3, 3).contiguous()
    got = run(pred, gt, ones, eye, K, [c], [0, 0])
    for b in range(2):
        want = reference_fp64(pred[b], gt[b], ones[b], eye[b], K[b], c, "m")
        assert not np.isfinite(want[3]) and not np.isfinite(got[b, 3])
        assert (np.isnan(got[b, 3]) and np.isnan(want[3])) or got[b, 3] == want[3], (got[b, 3], want[3])
    monkeypatch.chdir(tmp_path)
    m = pm.PoseMetrics(dict(CFG, t_scale="m"))
    m.set_metrics({"R_errs_0": [0.0, 0.0], "t_errs_0": [0.0, 0.0], "inplane_R_errs_0": [0.0, 0.0],
                   "proj2D_metric_0": [float(got[0, 3]), 1.0]})
    m.dataloader_id_set = {0}
    assert m.aggregate_metrics()["proj2D metric_0"] == 0.5


def test_deterministic_across_calls_and_batch_composition():
    rng = np.random.default_rng(11)
    clouds = [cloud(rng, 4000), cloud(rng, 1500)]
    which = rng.integers(0, 2, 64)
    pred, gt, scale, ct, K = random_poses(rng, 64)
    a = run(pred, gt, scale, ct, K, clouds, which)
    b2 = run(pred, gt, scale, ct, K, clouds, which)
    assert np.array_equal(a, b2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run(pred, gt, scale, ct, K, clouds, which)
    assert np.array_equal(a, c)
    for b in (0, 13, 63):
        one = run(pred[b:b + 1], gt[b:b + 1], scale[b:b + 1], ct[b:b + 1], K[b:b + 1], clouds, which[b:b + 1])
        assert np.array_equal(one[0], a[b]), b


# -------------------------------------------------------------------------------------------------------------------------------
def _model_config():
    path = os.path.join(HERE, "golden", "model_modules_config.json")
    mods = copy.deepcopy(json.load(open(path))["modules"])
    mods["decoder"].update(num_decoder_layers=2, hip_precision="bf16")
    mods["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=2, hip_precision="bf16")
    return {"modules": mods}


def _posed_batch(B, T, seed=3):
    """Per sample a box, intrinsics and a known query pose; the query view's true corner projections (for a stub decoder)."""
    from boxdreamer_amd import pnp
    rng = np.random.default_rng(seed)
    data = synth.make_batch(seed=seed, B=B, T=T)
    f = 1.2 * 224
    K = np.array([[f, 0, 112.0], [0, f, 112.0], [0, 0, 1.0]])
    box = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * [0.45, 0.35, 0.3]
    poses = np.tile(np.eye(4), (B, T, 1, 1))
    proj = np.zeros((B, 8, 2))
    for b in range(B):
        R = pnp.rodrigues(rng.normal(size=3) * 0.6)
        t = np.array([rng.normal() * 0.1, rng.normal() * 0.1, 2.6 + rng.random() * 0.6])
        pc = box @ R.T + t
        proj[b] = pc[:, :2] / pc[:, 2:3] * f + 112.0
        poses[b, T - 1, :3, :3], poses[b, T - 1, :3, 3] = R, t
    data["bbox_3d"] = torch.from_numpy(np.tile(box, (B, T, 1, 1))).float()
    data["non_ndc_intrinsics"] = torch.from_numpy(np.tile(K, (B, T, 1, 1))).float()
    data["intrinsics"] = data["non_ndc_intrinsics"].clone()
    data["poses"] = torch.from_numpy(poses).float()
    return data, torch.from_numpy(proj).float(), box


def test_end_to_end_after_the_forward(tmp_path, monkeypatch):
    from boxdreamer_amd.bbox_features import make_bbox_features
    monkeypatch.chdir(tmp_path)
    model = BoxDreamer(_model_config()).cuda().eval()
    B, T = 5, 3
    data, proj, box = _posed_batch(B, T)
    gt = data["poses"].clone()
    data["poses"][:, T - 1] = torch.eye(4)
    heat = make_bbox_features(proj.cuda(), "heatmap", (224, 224), group=1)

    class Stub(torch.nn.Module):
        def forward(self, *a, **k):
            return heat.float()
    model.decoder = Stub()
    rng = np.random.default_rng(4)
    pts = (rng.uniform(-1, 1, (5000, 3)) * box.max(0)).astype(np.float32)
    write_ply(str(tmp_path / "lm/models/obj_01/obj_01.ply"), pts)
    data["original_poses"] = gt
    data["scale"] = torch.ones(B, T, 3)
    data["coordinate_transform"] = torch.eye(4).expand(B, 4, 4).contiguous()
    data["original_intrinsics"] = data["non_ndc_intrinsics"].clone()
    data["model_path"] = [[str(tmp_path / "lm/models_test/obj_01/obj_01.ply")] * B for _ in range(T)]
    data["original_images"] = [[f"img_{b}_{v}.png" for b in range(B)] for v in range(T)]
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    out = dict(dev, **model(dev))
    m = pm.PoseMetrics(dict(CFG, t_scale="m"))
    m.compute_metrics(out)
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    res = m.get_metrics()
    for b in range(B):
        q = int(host["query_idx"][b])
        want = reference_fp64(host["pred_poses"][b, q].float(), host["original_poses"][b, q], host["scale"][b, q],
                              host["coordinate_transform"][b], host["original_intrinsics"][b, q], pts, "m")
        got = [res[k][b] for k in ("R_errs_0", "t_errs_0", "inplane_R_errs_0", "proj2D_metric_0", "ADD_raw_0", "ADDs_raw_0")]
        check_close(got, want, 0.6, b)
        # the facade's pose accuracy on exact corner maps (test_gpu_facade.py): R to ~0.03 per entry, t to 3 % of the depth
        assert got[0] <= 5.0 and got[1] <= 100 * 0.03 * 3.2 and got[4] <= 0.15
    assert res["ADD_0.1d_0"] and len(res["ADDs_raw_0"]) == B
