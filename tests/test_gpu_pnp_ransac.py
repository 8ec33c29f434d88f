"""GPU: the device RANSAC PnP of the dense multi-round mode (csrc/pnp.hip: pnp_ransac_hyp_kernel, one wavefront per hypothesis, and
pnp_ransac_final_kernel, one per sample -- bd_solve_pnp_ransac_wave) against its HOST twins on the same sampling table: the same
two-stage code run through the loop runner on one thread (bd_solve_pnp_ransac_host) and the numpy form (pnp.solve_pnp_ransac(picks=...)).
Never against the kernels' own output.  Scenes, margins and twins are those of tests/test_pnp_ransac_host.py (5 samples, R in {1, 3, 8},
1000 trials: at most 5000 workgroups), built once and never modified."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, pnp
from boxdreamer_amd.box_utils import solve_poses_device, solve_poses_ransac_device
from boxdreamer_amd.model import BoxDreamer
from test_gpu_pnp_wave import _config, _posed_batch, f32
from test_pnp_ransac_host import CONF, N, THR, TOL, assert_same_result, case, twin

pytestmark = pytest.mark.gpu

_DEVICE = {}


def run(kp, box, K, n_trials=1000):
    out = solve_poses_ransac_device(f32(kp), f32(box), f32(K), n_trials=n_trials, reproj_err=THR, confidence=CONF, seed=0)
    poses, inl, rms, info = (o.cpu().numpy() for o in out)
    return poses, inl.reshape(len(kp), -1), rms, info


def device(name, n_trials=1000):
    """The launch on case `name`, once."""
    key = (name, n_trials)
    if key not in _DEVICE:
        c = case(name, n_trials)
        _DEVICE[key] = run(c["kp"], c["box"], c["K"], n_trials)
    return _DEVICE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype in (np.bool_, np.uint8) else np.int32)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def wave_on_the_mask(c, inl):
    """bd_solve_pnp_wave per sample on the observations the mask keeps, in index order, the box corners tiled to match, under the
    iteration cap of the RANSAC's final solve (solve_poses_ransac_device passes pnp.LM_MAX_ITERS)."""
    R = c["rounds"]
    poses, rms = np.zeros((N, 4, 4), np.float32), np.zeros((N,), np.float32)
    for s in range(N):
        m = inl[s].astype(bool)
        kp, p3 = c["kp"][s].reshape(-1, 2)[m], np.tile(c["box"][s], (R, 1))[m]
        p, r = solve_poses_device(f32(kp[None]), f32(p3[None]), f32(c["K"][s:s + 1]), iters=pnp.LM_MAX_ITERS, form="wave", want_rms=True)
        poses[s], rms[s] = p[0].cpu().numpy(), r[0].item()
    return poses, rms


def pixel_rms(pose, c, inl):
    """fp64 pixel RMS of the fp32 pose over the inliers."""
    R, out = c["rounds"], np.zeros(N)
    for s in range(N):
        m = inl[s].astype(bool)
        kp, p3 = c["kp"][s].reshape(-1, 2)[m].astype(np.float64), np.tile(c["box"][s], (R, 1))[m].astype(np.float64)
        P, K = pose[s].astype(np.float64), c["K"][s].astype(np.float64)
        pc = p3 @ P[:3, :3].T + P[:3, 3]
        uv = pc[:, :2] / pc[:, 2:] * [K[0, 0], K[1, 1]] + K[:2, 2]
        out[s] = np.sqrt(((kp - uv) ** 2).sum(-1).mean())
    return out


@pytest.mark.parametrize("name", ["R1", "R3", "R8"])
def test_bad_rounds_are_rejected_like_the_host_twins(hip, name):
    """One bad round at R = 3, three at R = 8 (none at R = 1): mask and trials used equal both twins', the pose is within 1e-4 of them,
    rms_px is the fp64 pixel RMS of the returned pose over the inliers (1e-4 relative), and the pose IS bd_solve_pnp_wave's on the
    observations the mask keeps, bit for bit."""
    c, got = case(name), device(name)
    poses, inl, rms, info = got
    assert_same_result(got, c, f"device, {name}")
    hp, hi, hr, hinfo = c["native"]
    assert np.array_equal(inl, hi) and np.array_equal(info, hinfo), (info, hinfo)
    assert np.abs(poses - hp).max() < TOL
    mine = pixel_rms(poses, c, inl)
    rel = np.abs(rms - mine) / mine
    print(f"[pnp_ransac] {name}: rms_px {rms.min():.4f} .. {rms.max():.4f}, vs recomputed {rel.max():.3g} (relative)")
    assert rel.max() <= 1e-4
    wp, wr = wave_on_the_mask(c, inl)
    assert np.array_equal(bits(poses), bits(wp)) and np.array_equal(bits(rms), bits(wr))


@pytest.mark.parametrize("name", ["R3_clean", "R8_clean", "R3_all_bad", "R8_all_bad"])
def test_final_solve_on_all_observations(hip, name):
    """Clean rounds: every observation is an inlier after one batch (path 0).  Every round bad: no hypothesis qualifies, path 1.  Either
    way the pose is bd_solve_pnp_wave's on all R * 8 observations bit for bit, and everything equals the host twin."""
    c, got = case(name), device(name)
    poses, inl, rms, info = got
    assert inl.all() and (info[:, 3] == (1 if "bad" in name else 0)).all() and (info[:, 0] == (1000 if "bad" in name else 32)).all()
    hp, hi, hr, hinfo = c["native"]
    assert np.array_equal(inl, hi) and np.array_equal(info[:, [0, 2, 3]], hinfo[:, [0, 2, 3]]) and np.abs(poses - hp).max() < TOL
    assert np.array_equal(info[:, 0], c["twin"][3])
    if "clean" in name:
        assert_same_result(got, c, f"device, {name}")
    wp, wr = wave_on_the_mask(c, inl)
    assert np.array_equal(bits(poses), bits(wp)) and np.array_equal(bits(rms), bits(wr))


def test_batch_shape_does_not_change_a_sample(hip):
    c, full = case("R8"), device("R8")
    for n in (1, 3):
        assert same_bits(run(c["kp"][:n], c["box"][:n], c["K"][:n]), [o[:n] for o in full]), n
    assert same_bits(run(c["kp"], c["box"], c["K"]), full)


def test_failure_stays_in_its_sample(hip):
    c, full = case("R3"), device("R3")
    kp = c["kp"].copy()
    kp[2, 1, 3, 0] = np.nan
    poses, inl, rms, info = got = run(kp, c["box"], c["K"])
    assert (poses[2] == 0).all() and not inl[2].any() and rms[2] == 0 and info[2, 3] == 2
    keep = np.arange(N) != 2
    assert same_bits([o[keep] for o in got], [o[keep] for o in full])
    assert not twin(kp[2:3], c["box"][2:3], c["K"][2:3], c["picks"])[0][0]                  # the numpy twin fails that sample too
    nan = lambda *s: np.full(s, np.nan, np.float32)
    for rounds in (1, 8):
        poses, inl, rms, info = run(nan(3, rounds, 8, 2), nan(3, 8, 3), nan(3, 3, 3))
        assert (poses == 0).all() and not inl.any() and (rms == 0).all() and (info[:, 3] == 2).all()


@pytest.mark.parametrize("n_trials", [70, 1])
def test_short_tables(hip, n_trials):
    """70 trials: the last batch has 6.  One trial: a single hypothesis -- whatever it finds, the host twins find the same (where one
    trial falls back to the plain solve of a scene WITH bad rounds, the pose is held to the native host twin alone:
    test_pnp_ransac_host.assert_same_result says why)."""
    for name in ("R3", "R8", "R8_clean"):
        c, got = case(name, n_trials), device(name, n_trials)
        assert_same_result(got, c, f"device, {name}, {n_trials} trials")
        assert same_bits(got[1:2], c["native"][1:2]) and np.array_equal(got[3], c["native"][3]) and np.abs(got[0] - c["native"][0]).max() < TOL
        assert (got[3][:, 0] <= n_trials).all()


def test_guard_bands_and_null_outputs(hip):
    """Outputs are rows [1 : N + 1] of pattern-filled tensors: the rows around them keep their patterns; rms_px = info = NULL change no pose."""
    c, full = case("R3"), device("R3")
    lib = _lib.load()
    kp, box, K, picks = f32(c["kp"]), f32(c["box"]), f32(c["K"]), torch.from_numpy(c["picks"]).cuda()
    n_obs = c["rounds"] * 8
    ws_bytes = lib.bd_solve_pnp_ransac_workspace_bytes(N, 1000)
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda").fill_(0xA5)

    def fresh():
        p = torch.full((N + 2, 4, 4), float("nan"), device="cuda")
        r = torch.full((N + 2,), float("nan"), device="cuda")
        p.view(torch.int32)[[0, N + 1]] = 0x7FC01234
        r.view(torch.int32)[[0, N + 1]] = 0x7FC01234
        return p, torch.full((N + 2, n_obs), 0x5A, dtype=torch.uint8, device="cuda"), r, torch.full((N + 2, 4), 0x12345678, dtype=torch.int32, device="cuda")

    def launch(p, i, r, f):
        _lib.check(lib.bd_solve_pnp_ransac_wave(_lib.ptr(kp), _lib.ptr(box), _lib.ptr(K), _lib.ptr(picks), N, c["rounds"], 1000, THR, CONF, 5, 30,
                                                _lib.ptr(p[1:N + 1]), _lib.ptr(i[1:N + 1]), _lib.ptr(r[1:N + 1]) if r is not None else C.c_void_p(0),
                                                _lib.ptr(f[1:N + 1]) if f is not None else C.c_void_p(0), _lib.ptr(ws), ws_bytes, _lib.stream()),
                   "bd_solve_pnp_ransac_wave")
        torch.cuda.synchronize()

    p, i, r, f = fresh()
    launch(p, i, r, f)
    assert (p.view(torch.int32)[[0, N + 1]] == 0x7FC01234).all() and (r.view(torch.int32)[[0, N + 1]] == 0x7FC01234).all()
    assert (i[[0, N + 1]] == 0x5A).all() and (f[[0, N + 1]] == 0x12345678).all() and (ws[ws_bytes:] == 0xA5).all()
    got = [t[1:N + 1].cpu().numpy() for t in (p, i, r, f)]
    assert same_bits(got, full)
    p2, i2, r2, f2 = fresh()
    launch(p2, i2, None, None)
    assert torch.equal(p2[1:N + 1], p[1:N + 1]) and torch.equal(i2, i)
    assert torch.isnan(r2).all() and (f2 == 0x12345678).all()                     # untouched


# ---------------------------------------------------------------------------------------------------------------- the facade

R_ROUNDS, SUB = 3, 2
DENSE = {"enable": True, "filter": "dino", "filter_enable": False, "filter_topk": 4, "multi_round": True, "sub_batch_size": SUB,
         "dense_mem_friendly": False, "fine_level": False, "fine_topk": 2}


def _multi_round_batch(B):
    """tests/test_gpu_pnp_wave.py's posed batch with T = 1 + SUB * R_ROUNDS views, the query last; the references' poses are the
    query's TRUE pose turned about the camera's z axis by 0.2 rad x a per-sample permutation of 1 .. T - 1: the two nearest to any pose
    within 0.1 rad of the true one are known.  -> data, true projections (B, 8, 2), true pose (B, 4, 4), the two nearest views (B, 2)."""
    T = 1 + SUB * R_ROUNDS
    data, proj = _posed_batch(B, T)
    data["query_idx"] = torch.full((B,), T - 1)
    gt = data["poses"][:, T - 1].clone()
    rng = np.random.default_rng(17)
    nearest = np.zeros((B, 2), int)
    for b in range(B):
        order = rng.permutation(T - 1) + 1
        for t in range(T - 1):
            a = 0.2 * order[t]
            Rz = torch.tensor([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
            data["poses"][b, t] = Rz @ gt[b]
            data["poses"][b, t, :3, 3] = gt[b, :3, 3]
        nearest[b] = np.sort(np.argsort(order)[:2])
    data["poses"][:, T - 1] = torch.eye(4)
    return data, proj, gt, nearest


def _forwards(dense_cfg, B=3):
    """The same batch through pnp_on_device "wave" and False, a stub decoder in place of BETR: in the multi-round call it emits heat maps
    peaked at the query's true projections in rounds 0 and 1 and at random pixels in round 2, in any other call the true ones."""
    from boxdreamer_amd.bbox_features import make_bbox_features
    data, proj, gt, nearest = _multi_round_batch(B)
    rng = np.random.default_rng(23)
    rounds = proj[:, None].repeat(1, R_ROUNDS, 1, 1).clone()
    rounds[:, 2] = torch.from_numpy(rng.uniform(30, 194, (B, 8, 2))).float()
    heat_true = make_bbox_features(proj.cuda(), "heatmap", (224, 224), group=1).float()
    heat_rounds = make_bbox_features(rounds.reshape(B * R_ROUNDS, 8, 2).cuda(), "heatmap", (224, 224), group=1).float()

    class Stub(torch.nn.Module):
        def forward(self, pose_feat, *a, **k):
            return heat_rounds if pose_feat.shape[0] == B * R_ROUNDS else heat_true

    outs = {}
    for solver in ("wave", False):
        model = BoxDreamer(_config(pnp_on_device=solver, dense_cfg=dense_cfg)).cuda().eval()
        model.decoder = Stub()
        outs[solver] = model({k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in data.items()})
    return outs["wave"], outs[False], gt, nearest


def test_facade_coarse_pose_rejects_the_bad_round_on_the_device(hip):
    """multi_round, fine_level False, R = 3: the known pose within test_facade_pose_values_with_the_wave_solver's bounds (0.03 on R, 3 % of
    the depth on t), within 1e-4 of the host-RANSAC forward, the third round rejected, and the batch dict says what ran."""
    B = 3
    out, host, gt, _ = _forwards(DENSE, B)
    T = out["pred_poses"].shape[1]
    assert "bd_solve_pnp_ransac_wave" in out["dense_pose_solver"] and "un-pinned" in out["dense_pose_solver"]
    assert "bd_solve_pnp_ransac_wave" not in host["dense_pose_solver"] and "solve_pnp_ransac" in host["dense_pose_solver"]
    pp = out["pred_poses"][:, T - 1].float().cpu()
    assert (pp[:, :3, :3] - gt[:, :3, :3]).abs().max().item() <= 0.03
    assert ((pp[:, :3, 3] - gt[:, :3, 3]).abs() / gt[:, 2:3, 3]).max().item() <= 0.03
    assert torch.equal(pp[:, 3], torch.tensor([0.0, 0, 0, 1]).expand(B, 4))
    d = (out["pred_poses"].float() - host["pred_poses"].float()).abs().max().item()
    print(f"[pnp_ransac] facade, coarse: |wave - host RANSAC| {d:.3g}")
    assert d < TOL
    for o in (out, host):
        inl, rms = o["dense_pose_inliers"], o["dense_pose_rms_px"]
        assert inl.is_cuda and inl.dtype == torch.bool and inl.shape == (B, R_ROUNDS, 8)
        assert rms.is_cuda and rms.shape == (B,) and (rms > 0).all() and (rms < THR).all()
        assert inl[:, :2].all() and (inl[:, 2].sum(1) <= 1).all()
    assert torch.equal(out["dense_pose_inliers"], host["dense_pose_inliers"])
    assert torch.equal(out["regression_boxes"], host["regression_boxes"]) and torch.equal(out["pred_bbox"], host["pred_bbox"])


def test_facade_fine_level_keeps_the_same_references(hip):
    B = 3
    out, host, gt, nearest = _forwards(dict(DENSE, fine_level=True), B)
    assert "bd_solve_pnp_ransac_wave" in out["dense_pose_solver"]
    assert out["images"].shape[1] == 3 and torch.equal(out["images"], host["images"]) and torch.equal(out["poses"], host["poses"])
    full, _, _, _ = _multi_round_batch(B)
    for b in range(B):                                           # ... and they are the two references nearest to the true pose
        assert torch.equal(out["poses"][b, :2].cpu(), full["poses"][b, nearest[b]])
