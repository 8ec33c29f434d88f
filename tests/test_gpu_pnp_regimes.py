"""GPU: the three device solvers (csrc/pnp.hip: pnp_kernel, pnp_wave_kernel, the two RANSAC kernels) over the regimes of
tests/test_pnp_regimes_host.py, held to the same criteria against the same independent reference (reference_minimum: fp64 numpy, no
scipy) -- the first comparison of these kernels with anything but their own host twins.  Forms:
  thread    solve_poses_device(form="thread")                      bd_solve_pnp, one pose per thread
  wave      solve_poses_device(form="wave", want_rms=True)         bd_solve_pnp_wave, one wavefront per pose
  ransac1   solve_poses_ransac_device on one round of the corners  (pts64: 8 rounds of the 8 corners, the interface takes box corners only)
  ransac3   the same on three rounds of the same corners under independent noise (pts64 left out: its three rounds ARE base's)
The RANSAC forms run a 4-trial table with a threshold no observation in front of the camera can miss, so their last stage is the wave
solver on every observation (asserted on `info`).  Every case is launched once per form and shared by the tests below."""
import numpy as np
import pytest
import torch

from boxdreamer_amd import pnp
from boxdreamer_amd.box_utils import solve_poses_device, solve_poses_ransac_device
from test_pnp_regimes_host import (ALL_CASES, HARD, N, RANSAC_PICKS, RANSAC_THR, REGIMES, SHIFT, TOL32, TOL_FORMS, WELL_POSED, _f64, case, check_hard,
                                   check_well_posed, classify, classify_forms, form_native, form_ransac_native, make_case, pose_distance, ransac_case,
                                   take)

pytestmark = pytest.mark.gpu

FORMS = ("thread", "wave", "ransac1", "ransac3")
BITS_CASE = ("noise8", 22)                       # the hard case that is also launched as N = 1 and N = 3
_RUNS = {}


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def launch(form, c):
    """-> (poses [n, 4, 4] fp32, rms_px [n] fp32 or None)."""
    if form == "thread":
        return solve_poses_device(f32(c["kp"]), f32(c["p3"]), f32(c["K"]), form="thread").cpu().numpy(), None
    if form == "wave":
        poses, rms = solve_poses_device(f32(c["kp"]), f32(c["p3"]), f32(c["K"]), form="wave", want_rms=True)
        return poses.cpu().numpy(), rms.cpu().numpy()
    kp, box = (c["kp_rounds"], c["box"]) if "kp_rounds" in c else (c["kp"][:, None], c["p3"])
    poses, inl, rms, info = (o.cpu().numpy() for o in solve_poses_ransac_device(f32(kp), f32(box), f32(c["K"]), n_trials=RANSAC_PICKS,
                                                                                 reproj_err=RANSAC_THR, confidence=0.99, seed=0))
    solved = info[:, 3] != 2
    assert (info[solved, 2] == kp.shape[1] * 8).all() and inl.reshape(len(kp), -1)[solved].all(), (c["name"], info)     # the all-inlier path ran
    assert (poses[~solved] == 0).all() and (rms[~solved] == 0).all()
    return poses, rms


def case_of(form, name, seed):
    if form == "ransac3":
        return case(name, seed, rounds=3)
    return ransac_case(name, seed) if form == "ransac1" else case(name, seed)


def forms_of(name):
    return [f for f in FORMS if not (f == "ransac3" and REGIMES[name]["npts"] != 8)]


def device_results(name, seed):
    """Every device form on (name, seed), launched once: {form: (case, poses, classification, rms_px)}."""
    key = (name, seed)
    if key not in _RUNS:
        runs = {f: case_of(f, name, seed) for f in forms_of(name)}
        out = {f: launch(f, runs[f]) for f in runs}
        cls = classify_forms(runs, {f: out[f][0] for f in runs})
        _RUNS[key] = {f: (*cls[f], out[f][1]) for f in runs}
    return _RUNS[key]


def host_twin(form, c):
    """The same code on the host, on the same case: bd_solve_pnp_host (solve_one_pose, one thread) for the thread kernel;
    bd_solve_pnp_ransac_host (pnp_wave_solve through the loop runner) for the RANSAC kernels and, where the case is 8 corners, for the
    wave kernel too -- with every observation an inlier its last stage is the wave solver on those 8 points.  (pts64's 64 distinct
    points do not fit the RANSAC interface: there the wave kernel is held to solve_one_pose.)"""
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    try:
        if form.startswith("ransac") or (form == "wave" and c["kp"].shape[1] == 8):
            return form_ransac_native(c)
        return form_native(c)
    finally:
        pnp._HAVE_CV2 = have


@pytest.mark.parametrize("name", WELL_POSED)
def test_well_posed_regimes_reach_the_reference(hip, name):
    """Every pose of every device form is at the reference minimum and within 2e-6 of the reference pose, and within 1e-4 of its host twin."""
    for seed in REGIMES[name]["seeds"]:
        for form, (c, poses, cls, _) in device_results(name, seed).items():
            what = f"{name} seed {seed}, device {form}"
            check_well_posed(poses, cls, c, TOL32, what)
            d = np.abs(poses.astype(np.float64) - host_twin(form, c))
            d[:, :3, 3] /= np.maximum(1.0, np.abs(c["t"]).max(1))[:, None]
            print(f"[pnp_regimes] {what}: max difference to the host twin {d.max():.3g}")
            assert d.max() < TOL_FORMS, (what, d.max())
            assert np.array_equal(poses[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (len(poses), 1))), what


@pytest.mark.parametrize("name,seed", HARD)
def test_hard_regimes_stop_on_a_minimum_in_front_of_the_camera(hip, name, seed):
    """No pose not_stationary, none behind the camera, at most 5 % in another minimum or failed: per device form.  Disagreements with the
    host twin are printed, not asserted."""
    for form, (c, poses, cls, _) in device_results(name, seed).items():
        what = f"{name} seed {seed}, device {form}"
        check_hard(cls, what)
        d = np.abs(poses.astype(np.float64) - host_twin(form, c)).max((1, 2))
        print(f"[pnp_regimes] {what}: differs from the host twin by more than {TOL_FORMS:g} on {int((d > TOL_FORMS).sum())} of {N} poses")


@pytest.mark.parametrize("name,seed", ALL_CASES)
def test_rms_px_is_the_pixel_rms_of_the_returned_pose(hip, name, seed):
    """rms_px of the wave and RANSAC forms against the fp64 recomputation from the returned fp32 pose (as returned, no projection onto
    SO(3)): within 1e-4 relative to max(rms, 1e-3) in every regime; 0 where the pose is zeros."""
    for form, (c, poses, cls, rms) in device_results(name, seed).items():
        if rms is None:
            continue
        kp, p3, K = _f64(c)
        P = poses.astype(np.float64)
        solved = P[:, 3, 3] == 1.0
        assert (rms[~solved] == 0).all()
        pc = p3 @ np.swapaxes(P[:, :3, :3], 1, 2) + P[:, None, :3, 3]
        with np.errstate(all="ignore"):
            uv = pc[..., :2] / pc[..., 2:] * np.stack([K[:, 0, 0], K[:, 1, 1]], 1)[:, None] + K[:, None, :2, 2]
        mine = np.sqrt(((kp - uv) ** 2).sum(-1).mean(-1))[solved]
        rel = np.abs(rms[solved] - mine) / np.maximum(mine, 1e-3)
        print(f"[pnp_regimes] {name} seed {seed}, device {form}: rms_px {rms[solved].min():.4g} .. {rms[solved].max():.4g} px, "
              f"against the recomputation {rel.max():.3g} relative")
        assert rel.max() <= 1e-4, (name, seed, form, rel.max())


def test_batch_shape_does_not_change_a_row(hip):
    """A hard case launched as N = 40, N = 1 and N = 3: the same rows come back bit for bit, pose and rms_px, in every form."""
    for form, (c, poses, cls, rms) in device_results(*BITS_CASE).items():
        for n in (1, 3):
            p, r = launch(form, take(c, slice(0, n)))
            assert np.array_equal(p.view(np.int32), poses[:n].view(np.int32)), (form, n)
            if rms is not None:
                assert np.array_equal(r.view(np.int32), rms[:n].view(np.int32)), (form, n)


def test_millimetres_give_the_same_pose_as_metres(hip):
    """`mm` against `base`, pose by pose, per device form: same R to 1e-6, t / 1000 to 1e-6 relative."""
    for form in FORMS:
        (ca, Pa, _, _), (cb, Pb, _, _) = device_results("base", 1)[form], device_results("mm", 1)[form]
        assert np.array_equal(ca["kp"], cb["kp"])
        Pa, Pb = Pa.astype(np.float64), Pb.astype(np.float64)
        dR = np.abs(Pa[:, :3, :3] - Pb[:, :3, :3]).max()
        dt = (np.abs(Pa[:, :3, 3] - Pb[:, :3, 3] / 1000.0).max(1) / np.abs(Pa[:, :3, 3]).max(1)).max()
        print(f"[pnp_regimes] mm against base, device {form}: |dR| {dR:.3g}, relative |dt| {dt:.3g}")
        assert dR < 1e-6 and dt < 1e-6, (form, dR, dt)


def test_a_shifted_image_gives_the_same_pose(hip):
    """Every pixel and the principal point moved by (1000, -700), per device form: within 1e-6 of the unshifted result and within the
    well-posed tolerance of the reference of the shifted inputs."""
    for form in FORMS:
        c = make_case("base", 1, rounds=3, shift=SHIFT) if form == "ransac3" else make_case("base", 1, shift=SHIFT)
        poses, _ = launch(form, c)
        check_well_posed(poses, classify(poses, c), c, TOL32, f"base shifted by {SHIFT}, device {form}")
        base = device_results("base", 1)[form][1].astype(np.float64)
        P = poses.astype(np.float64)
        d = pose_distance(P[:, :3, :3], P[:, :3, 3], base[:, :3, :3], base[:, :3, 3])
        print(f"[pnp_regimes] shifted against unshifted, device {form}: {d.max():.3g}")
        assert d.max() < 1e-6, (form, d.max())
