"""GPU: the wave form of the device PnP (csrc/pnp.hip: pnp_wave_kernel, bd_solve_pnp_wave -- one wavefront per pose) against the HOST form
of the same solver (bd_solve_pnp_host on one thread, the cv2 branch forced off): never against the thread kernel, never against itself.
Box, intrinsics and noise are those of tests/test_gpu_ops.py::test_gpu_pnp_matches_host_form; points beyond the 8 corners are drawn
normal * (0.1, 0.07, 0.05).  1e-4 is the tolerance the forms of this solver are already held to among each other."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, pnp, synth
from boxdreamer_amd.box_utils import solve_poses_device, solve_poses_host
from boxdreamer_amd.model import BoxDreamer

pytestmark = pytest.mark.gpu

EXT = np.array([0.1, 0.07, 0.05])
BOX = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * EXT
TOL = 1e-4


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host_form(kp, p3, K, iters=30):
    """The reference of every comparison: bd_solve_pnp_host, one thread.  (solve_poses_host runs 30 iterations; any other count goes to
    the same entry point directly.)"""
    kp, p3, K = (np.ascontiguousarray(a, np.float32) for a in (kp, p3, K))
    if iters == 30:
        have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
        try:
            return solve_poses_host(kp, p3, K, workers=1)
        finally:
            pnp._HAVE_CV2 = have
    out = np.zeros((kp.shape[0], 4, 4), np.float32)
    rc = _lib.load().bd_solve_pnp_host(kp.ctypes.data, p3.ctypes.data, K.ctypes.data, kp.shape[0], kp.shape[1], iters, out.ctypes.data, 1)
    assert rc == 0
    return out


def wave(kp, p3, K, iters=30):
    poses, rms = solve_poses_device(f32(kp), f32(p3), f32(K), iters=iters, form="wave", want_rms=True)
    return poses.cpu().numpy(), rms.cpu().numpy()


def scene(rng, N, npts, rvec=None, t=None, fx=600.0, fy=600.0, cx=112.0, cy=112.0, noise=0.7):
    """-> (exact pixels, noisy pixels, p3, K, R, t), float64."""
    extra = rng.normal(size=(N, npts - 8, 3)) * EXT if npts > 8 else np.zeros((N, 0, 3))
    p3 = np.concatenate([np.tile(BOX, (N, 1, 1)), extra], 1)[:, :npts]
    K = np.tile(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), (N, 1, 1))
    R = pnp._rodrigues_b(rng.normal(size=(N, 3)) * 0.9 if rvec is None else np.tile(np.asarray(rvec, float), (N, 1)))
    tt = (np.stack([rng.normal(size=N) * 0.05, rng.normal(size=N) * 0.05, 0.6 + rng.random(N) * 0.4], 1) if t is None
          else np.tile(np.asarray(t, float), (N, 1)))
    pc = p3 @ np.swapaxes(R, 1, 2) + tt[:, None]
    exact = pc[..., :2] / pc[..., 2:] * [fx, fy] + [cx, cy]
    return exact, exact + rng.normal(size=exact.shape) * noise, p3, K, R, tt


def pixel_rms(pose, kp, p3, K):
    """Root mean square of the pixel reprojection error of `pose` (fp32 [N,4,4]) over the points, in fp64 from the fp32 inputs."""
    pose, kp, p3, K = (np.asarray(np.asarray(a, np.float32), np.float64) for a in (pose, kp, p3, K))
    pc = p3 @ np.swapaxes(pose[:, :3, :3], 1, 2) + pose[:, None, :3, 3]
    uv = pc[..., :2] / pc[..., 2:] * np.stack([K[:, 0, 0], K[:, 1, 1]], 1)[:, None] + K[:, None, :2, 2]
    return np.sqrt(((kp - uv) ** 2).sum(-1).mean(-1))


def close_to_host(got, ref, what):
    """Every pose: solved by both, R and t within 1e-4, last row exactly (0, 0, 0, 1).  -> (max |dR|, max |dt|)."""
    assert (ref[:, 3, 3] == 1.0).all(), f"{what}: the host form failed on {np.nonzero(ref[:, 3, 3] != 1.0)[0].tolist()}"
    dR, dt = np.abs(got[:, :3, :3] - ref[:, :3, :3]).max(), np.abs(got[:, :3, 3] - ref[:, :3, 3]).max()
    print(f"[pnp_wave] {what}: max |dR| {dR:.3g}, max |dt| {dt:.3g}")
    assert dR < TOL and dt < TOL, (what, dR, dt)
    assert np.array_equal(got[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (got.shape[0], 1))), what
    return dR, dt


@pytest.fixture(scope="module")
def batch40():
    """40 poses on the 8 corners: noisy pixels, the launch's poses / rms_px and the host form's poses (computed once, never modified)."""
    exact, noisy, p3, K, R, t = scene(np.random.default_rng(3), 40, 8)
    poses, rms = wave(noisy, p3, K)
    return {"exact": exact, "noisy": noisy, "p3": p3, "K": K, "R": R, "t": t, "poses": poses, "rms": rms, "host": host_form(noisy, p3, K)}


@pytest.mark.parametrize("npts", [6, 7, 8, 9, 16, 24, 63, 64])
def test_point_counts_pose_and_rms(hip, npts):
    """Fewer points than a chunk of 8, one chunk, one past it, several, MAXPTS - 1 and MAXPTS.  The pose is the host form's; rms_px is the
    pixel RMS of the returned pose (recomputed in fp64: within 1e-4 relative to max(rms, 1e-3)) and does not exceed the host form's by
    more than 1e-6 relative: the wave form sits ON the minimum, not merely near the pose."""
    exact, noisy, p3, K, _, _ = scene(np.random.default_rng(100 + npts), 5, npts)
    got, rms = wave(noisy, p3, K)
    ref = host_form(noisy, p3, K)
    close_to_host(got, ref, f"n_points = {npts}")
    mine, theirs = pixel_rms(got, noisy, p3, K), pixel_rms(ref, noisy, p3, K)
    rel = np.abs(rms - mine) / np.maximum(mine, 1e-3)
    excess = rms / theirs - 1.0
    print(f"[pnp_wave] n_points = {npts}: rms_px {rms.min():.4f} .. {rms.max():.4f} px, vs recomputed {rel.max():.3g} (relative), "
          f"excess over the host form's rms {excess.max():.3g} (relative)")
    assert rel.max() <= 1e-4
    assert (rms <= theirs * (1 + 1e-6)).all(), excess
    got, rms = wave(exact, p3, K)                                   # exact corners: the true pose, no residual left
    assert (got[:, 3, 3] == 1.0).all() and (rms < 1e-3).all(), rms


def test_batch_shape_does_not_change_a_pose(hip, batch40):
    """A pose's bits depend neither on n_poses nor on its row: rows [0] and [0:3] of the launch of 40 are the launches of 1 and of 3 on
    those rows' inputs, bit for bit; and a launch repeats itself bit for bit."""
    b = batch40
    close_to_host(b["poses"], b["host"], "40 poses, 8 points")
    for n in (1, 3):
        poses, rms = wave(b["noisy"][:n], b["p3"][:n], b["K"][:n])
        assert np.array_equal(poses.view(np.int32), b["poses"][:n].view(np.int32)), n
        assert np.array_equal(rms.view(np.int32), b["rms"][:n].view(np.int32)), n
    poses, rms = wave(b["noisy"], b["p3"], b["K"])
    assert np.array_equal(poses.view(np.int32), b["poses"].view(np.int32)) and np.array_equal(rms.view(np.int32), b["rms"].view(np.int32))


def test_failure_stays_in_its_pose(hip, batch40):
    """One NaN corner in pose 7 of 40: that pose is zeros with rms 0, every other pose keeps its bits.  A NaN in K fails its pose alone;
    a launch of nothing but NaN returns, all zeros."""
    b = batch40
    kp = b["noisy"].copy()
    kp[7, 3, 0] = np.nan
    poses, rms = wave(kp, b["p3"], b["K"])
    assert (poses[7] == 0).all() and rms[7] == 0
    keep = np.arange(40) != 7
    assert np.array_equal(poses[keep].view(np.int32), b["poses"][keep].view(np.int32))
    assert np.array_equal(rms[keep].view(np.int32), b["rms"][keep].view(np.int32))
    assert (host_form(kp, b["p3"], b["K"])[7] == 0).all()
    K = b["K"].copy()
    K[11, 0, 0] = np.nan
    poses, rms = wave(b["noisy"], b["p3"], K)
    assert (poses[11] == 0).all() and rms[11] == 0
    keep = np.arange(40) != 11
    assert np.array_equal(poses[keep].view(np.int32), b["poses"][keep].view(np.int32))
    for npts in (8, 64):
        nan = lambda *s: np.full(s, np.nan)
        poses, rms = wave(nan(6, npts, 2), nan(6, npts, 3), nan(6, 3, 3))
        assert (poses == 0).all() and (rms == 0).all()


@pytest.mark.parametrize("noise", [0.0, 0.7])
@pytest.mark.parametrize("short_of_pi", [1e-2, 1e-5, 0.0])
def test_rotations_near_pi(hip, short_of_pi, noise):
    """rvec_from_R's near-pi branch (angle within 1e-4 of pi) and its neighbourhood: axis (0.6, 0, 0.8), t = (0.01, 0.02, 0.7)."""
    angle = np.pi - short_of_pi
    exact, noisy, p3, K, R, t = scene(np.random.default_rng(11), 1, 8, rvec=np.array([0.6, 0.0, 0.8]) * angle, t=[0.01, 0.02, 0.7], noise=noise)
    got, rms = wave(noisy, p3, K)
    close_to_host(got, host_form(noisy, p3, K), f"angle pi - {short_of_pi:g}, noise {noise}")
    if noise == 0.0:
        assert np.abs(got[0, :3, :3] - R[0]).max() < TOL and np.abs(got[0, :3, 3] - t[0]).max() < TOL and rms[0] < 1e-3


def test_identity_nonsquare_pixels_and_iteration_counts(hip):
    rng = np.random.default_rng(12)
    exact, _, p3, K, R, t = scene(rng, 1, 8, rvec=[0.0, 0.0, 0.0], t=[0.01, 0.02, 0.7])
    got, rms = wave(exact, p3, K)
    close_to_host(got, host_form(exact, p3, K), "identity rotation, exact corners")
    assert np.abs(got[0, :3, :3] - np.eye(3)).max() < TOL and rms[0] < 1e-3
    # pixel weights (wx, wy) != 1
    _, noisy, p3, K, _, _ = scene(rng, 5, 8, fx=640.0, fy=480.0, cx=100.0, cy=120.0)
    got, rms = wave(noisy, p3, K)
    ref = host_form(noisy, p3, K)
    close_to_host(got, ref, "fx 640, fy 480, cx 100, cy 120")
    assert (rms <= pixel_rms(ref, noisy, p3, K) * (1 + 1e-6)).all()
    # iters = 0: the DLT estimate alone; iters = 1: one LM step -- against the host form at the same count
    _, noisy, p3, K, _, _ = scene(rng, 5, 8)
    for iters in (0, 1):
        got, _ = wave(noisy, p3, K, iters=iters)
        close_to_host(got, host_form(noisy, p3, K, iters=iters), f"iters = {iters}")


def test_degenerate_input_terminates(hip):
    """All eight corners on one pixel, and planar 3-D points: the call returns with the host form's verdict (zeros where it fails,
    otherwise finite)."""
    rng = np.random.default_rng(13)
    _, noisy, p3, K, _, _ = scene(rng, 2, 8)
    kp = np.full_like(noisy, 112.0)
    got, rms = wave(kp, p3, K)
    ref = host_form(kp, p3, K)
    assert np.isfinite(got).all() and np.isfinite(rms).all()
    assert np.array_equal(got[:, 3, 3] == 1.0, ref[:, 3, 3] == 1.0)
    assert (got[ref[:, 3, 3] != 1.0] == 0).all()
    flat = p3.copy()
    flat[..., 2] = 0.0
    assert (host_form(noisy, flat, K) == 0).all()                 # constructed to fail: the DLT needs non-planar points
    got, rms = wave(noisy, flat, K)
    assert (got == 0).all() and (rms == 0).all()


def test_guard_bands_and_null_rms(hip, batch40):
    """Outputs are rows [1 : N + 1] of NaN-filled tensors: the rows around them keep their bit patterns; rms_px = NULL changes no pose."""
    b, N = batch40, 40
    lib = _lib.load()
    kp, p3, K = f32(b["noisy"]), f32(b["p3"]), f32(b["K"])
    big_p = torch.full((N + 2, 4, 4), float("nan"), device="cuda")
    big_r = torch.full((N + 2,), float("nan"), device="cuda")
    big_p.view(torch.int32)[[0, N + 1]] = 0x7FC01234
    big_r.view(torch.int32)[[0, N + 1]] = 0x7FC01234
    _lib.check(lib.bd_solve_pnp_wave(_lib.ptr(kp), _lib.ptr(p3), _lib.ptr(K), N, 8, 30, _lib.ptr(big_p[1:N + 1]), _lib.ptr(big_r[1:N + 1]),
                                     _lib.stream()), "bd_solve_pnp_wave")
    torch.cuda.synchronize()
    assert (big_p.view(torch.int32)[[0, N + 1]] == 0x7FC01234).all() and (big_r.view(torch.int32)[[0, N + 1]] == 0x7FC01234).all()
    assert np.array_equal(big_p[1:N + 1].cpu().numpy().view(np.int32), b["poses"].view(np.int32))
    assert np.array_equal(big_r[1:N + 1].cpu().numpy().view(np.int32), b["rms"].view(np.int32))
    big_p2 = torch.full((N + 2, 4, 4), float("nan"), device="cuda")
    _lib.check(lib.bd_solve_pnp_wave(_lib.ptr(kp), _lib.ptr(p3), _lib.ptr(K), N, 8, 30, _lib.ptr(big_p2[1:N + 1]), C.c_void_p(0),
                                     _lib.stream()), "bd_solve_pnp_wave")
    torch.cuda.synchronize()
    assert torch.isnan(big_p2[[0, N + 1]]).all()
    assert np.array_equal(big_p2[1:N + 1].cpu().numpy().view(np.int32), b["poses"].view(np.int32))
    assert torch.equal(solve_poses_device(kp, p3, K, form="wave"), big_p2[1:N + 1])          # want_rms=False passes NULL


# ---------------------------------------------------------------------------------------------------------------- the facade

def _config(prec="bf16", depth=2, **mods):
    import json, os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_modules_config.json")
    m = copy.deepcopy(json.load(open(path))["modules"])
    m["decoder"].update(num_decoder_layers=depth, hip_precision=prec)
    m["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=depth, hip_precision=prec)
    m.update(mods)
    return {"modules": m}


def _posed_batch(B, T, seed=3):
    """tests/test_gpu_facade.py's recipe: per sample a box, intrinsics and a known query pose; the query view's TRUE corner projections
    are returned so that a stub decoder can emit heat maps peaked exactly there."""
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
    return data, torch.from_numpy(proj).float()


def test_facade_pose_values_with_the_wave_solver(hip):
    """test_pose_values_from_exact_corner_heatmaps with pnp_on_device: "wave": a stub decoder emits heat maps peaked at the query view's
    true corner projections; decode + PnP must return the known pose (0.03 on R, 3 % of the depth on t: that test's bounds), the same
    corners as the host-PnP forward bit for bit and its poses to 1e-4, plus a per-pose pixel RMS below one pixel."""
    from boxdreamer_amd.bbox_features import make_bbox_features
    B, T = 5, 3
    data, proj = _posed_batch(B, T)
    gt = data["poses"][:, T - 1].clone()
    data["poses"][:, T - 1] = torch.eye(4)
    heat = make_bbox_features(proj.cuda(), "heatmap", (224, 224), group=1)

    class Stub(torch.nn.Module):
        def forward(self, *a, **k):
            return heat.float()

    outs = {}
    for solver in ("wave", False):
        model = BoxDreamer(_config(pnp_on_device=solver)).cuda().eval()
        model.decoder = Stub()
        outs[solver] = model({k: (v.clone().cuda() if torch.is_tensor(v) else v) for k, v in data.items()})
    out, host = outs["wave"], outs[False]
    assert out["pose_solver"] == "hip:bd_solve_pnp_wave (one wavefront per pose, DLT + LM; parity vs OpenCV un-pinned)"
    assert "pred_pose_rms_px" not in host and "bd_solve_pnp_wave" not in host["pose_solver"]
    pp = out["pred_poses"][:, T - 1].float().cpu()
    assert (pp[:, :3, :3] - gt[:, :3, :3]).abs().max().item() <= 0.03
    assert ((pp[:, :3, 3] - gt[:, :3, 3]).abs() / gt[:, 2:3, 3]).max().item() <= 0.03
    assert torch.equal(pp[:, 3], torch.tensor([0.0, 0, 0, 1]).expand(B, 4))
    rms = out["pred_pose_rms_px"]
    assert rms.is_cuda and rms.dtype == torch.float32 and rms.shape == (B,) and (rms < 1.0).all() and (rms > 0).all()
    assert torch.equal(out["pred_corners_px"], host["pred_corners_px"])
    assert (out["pred_poses"].float() - host["pred_poses"].float()).abs().max().item() < TOL
    assert torch.equal(out["pred_poses"][:, : T - 1].cpu(), data["poses"][:, : T - 1])


def test_facade_wave_solver_under_hip_graph_waits_for_nothing(hip):
    """`hip_graph: true` with the wave solver: every output equals the eager forward's bit for bit, and the graphed forward
    records no host synchronisation at all (the corners never leave the device, and the captured path has no mask verdict to fetch)."""
    def build(graph):
        m = BoxDreamer(_config(hip_graph=graph, pnp_on_device="wave"))
        m.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(1234, 2).items()}, strict=True)
        return m.cuda().eval()
    eager, graphed = build(False), build(True)
    batch = synth.make_batch(seed=8, B=2, T=3)
    batch["query_idx"] = torch.tensor([2, 0])
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    a, b = eager(dict(dev)), graphed(dict(dev))
    assert graphed._graph is not None
    for k in ("pred_bbox", "pred_poses", "regression_boxes", "pred_corners_px", "pred_pose_rms_px"):
        assert torch.equal(a[k], b[k]), k
    assert "bd_solve_pnp_wave" in b["pose_solver"] and b["pred_pose_rms_px"].shape == (2,)
    assert list(graphed.host_syncs_per_forward) == []
    # (the eager forward still fetches the decoder's 4-byte mask verdict, as with pnp_on_device: True)
    assert all("mask verdict" in s for s in eager.host_syncs_per_forward)
