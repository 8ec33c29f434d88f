"""Host side of the device RANSAC PnP of the dense multi-round mode (csrc/pnp.hip: bd_solve_pnp_ransac_wave / _host): the exports and
their argument checks (which return before any launch), the sampling table (pnp.ransac_picks), and the two-stage code itself run on the
HOST through the loop runner (bd_solve_pnp_ransac_host = pnp.solve_pnp_ransac_native) against its numpy twin on the same hypotheses
(pnp.solve_pnp_ransac(picks=...)).  Nothing here needs a GPU.

Scenes (shared with tests/test_gpu_pnp_ransac.py): the box, intrinsics (fx = fy = 600, c = 112) and pose distribution of
tests/test_gpu_pnp_wave.py; a clean round is the exact projections + 0.3 px normal noise, a bad round 8 uniform pixels in [30, 194].
The inputs are rounded to fp32 (what the native forms take) before EITHER form sees them.  Every scene must keep every scored pixel
error of every hypothesis at least 1e-6 px away from the 2 px threshold (`margin`, asserted where the scene is built): the two forms
differ at the 1e-9 level and must not be able to flip an inlier.  No seed had to be left out for that."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from boxdreamer_amd import _lib, pnp
from boxdreamer_amd.box_utils import solve_poses_host
from test_gpu_pnp_wave import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BD_ERR_SHAPE, BD_ERR_NULL = -1, -5
TOL = 1e-4                      # the tolerance the forms of this solver are already held to among each other
THR = 2.0
CONF = float(np.float32(0.99))  # the native forms take the confidence as a float
N = 5
# (rounds, bad rounds): the GPU tests use the same list
SHAPES = {"R1": (1, ()), "R3": (3, (1,)), "R8": (8, (1, 4, 6)), "R3_clean": (3, ()), "R8_clean": (8, ()), "R3_all_bad": (3, (0, 1, 2)),
          "R1_all_bad": (1, (0,)), "R8_all_bad": (8, tuple(range(8)))}


def ransac_scene(seed, n, rounds, bad=()):
    """-> kp [n, rounds, 8, 2], box [n, 8, 3], K [n, 3, 3] fp32, and the true (R, t)."""
    rng = np.random.default_rng(seed)
    exact, _, p3, K, Rm, t = scene(rng, n, 8, noise=0.0)
    kp = exact[:, None] + rng.normal(size=(n, rounds, 8, 2)) * 0.3
    for r in bad:
        kp[:, r] = rng.uniform(30, 194, (n, 8, 2))
    return kp.astype(np.float32), p3.astype(np.float32), K.astype(np.float32), Rm, t


def margin(kp, box, K, picks):
    """Smallest |pixel error - threshold| over every (hypothesis, observation) pair of one sample, by the numpy form."""
    R = kp.shape[0]
    p3, p2, K = np.tile(box.astype(np.float64), (R, 1)), kp.reshape(-1, 2).astype(np.float64), K.astype(np.float64)
    ok, Rm, t = pnp.solve_pnp_batched(p3[picks], p2[picks], np.broadcast_to(K, (len(picks), 3, 3)), iters=5)
    err = pnp._reproj_px(Rm, t, p3[None], p2[None], K)[ok]
    return np.abs(err[np.isfinite(err)] - THR).min()


def twin(kp, box, K, picks):
    """pnp.solve_pnp_ransac(picks=...) per sample, the cv2 branch off -> (ok [n], poses [n,4,4] fp64, masks [n, R*8], trials [n])."""
    n, R = kp.shape[:2]
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    try:
        oks, poses, masks, trials = np.zeros(n, bool), np.zeros((n, 4, 4)), np.zeros((n, R * 8), bool), np.zeros(n, int)
        for s in range(n):
            ok, Rm, t, m, tr = pnp.solve_pnp_ransac(np.tile(box[s].astype(np.float64), (R, 1)), kp[s].reshape(-1, 2).astype(np.float64),
                                                    K[s].astype(np.float64), reproj_err=THR, confidence=CONF, max_trials=len(picks),
                                                    picks=picks, want_trials=True)
            oks[s], masks[s], trials[s] = ok, m, tr
            if ok:
                poses[s, :3, :3], poses[s, :3, 3], poses[s, 3, 3] = Rm, t, 1.0
        return oks, poses, masks, trials
    finally:
        pnp._HAVE_CV2 = have


_CASES = {}


def case(name, n_trials=1000):
    """One scene with everything the comparisons need, computed once and never modified: inputs, picks, the native host form on ONE
    thread and the numpy twin.  Asserts the scene's margin."""
    key = (name, n_trials)
    if key not in _CASES:
        rounds, bad = SHAPES[name]
        kp, box, K, Rm, t = ransac_scene(1000 + 10 * rounds + len(bad), N, rounds, bad)
        picks = pnp.ransac_picks(rounds, n_trials, 0)
        mg = min(margin(kp[s], box[s], K[s], picks) for s in range(N))
        print(f"[pnp_ransac] {name}, {n_trials} trials: smallest |error - {THR}| = {mg:.3g} px")
        assert mg > 1e-6, (name, n_trials, mg)
        poses, inl, rms, info = pnp.solve_pnp_ransac_native(kp, box, K, picks, THR, CONF, workers=1)
        _CASES[key] = {"kp": kp, "box": box, "K": K, "R": Rm, "t": t, "picks": picks, "rounds": rounds, "bad": bad,
                       "native": (poses, inl, rms, info), "twin": twin(kp, box, K, picks)}
    return _CASES[key]


def assert_same_result(got, c, what):
    """got = (poses, inl, rms, info) of a native form against the numpy twin of case c: mask and trials identical, R and t within TOL.
    The poses of samples whose host twin (bd_solve_pnp_ransac_host) fell back to ALL observations of a scene with bad rounds are left
    out of the comparison with the NUMPY form: a least-squares fit through a third of random pixels has no well-conditioned minimum (its
    pixel RMS is in the hundreds), the DLT start of numpy's SVD and of the native Jacobi sweep differ in the last bits and the 30
    iterations end in different places.  Those poses are held to the native host forms instead (the callers compare with c["native"],
    test_every_round_bad_falls_back_to_all_observations with bd_solve_pnp_host)."""
    poses, inl, rms, info = got
    oks, tposes, masks, trials = c["twin"]
    assert oks.all(), what
    assert np.array_equal(inl.reshape(masks.shape), masks), what
    assert np.array_equal(info[:, 0], trials), (what, info[:, 0], trials)
    defined = ~((c["native"][3][:, 3] == 1) & (len(c["bad"]) > 0))
    d = np.abs(poses.astype(np.float64) - tposes)[defined] if defined.any() else np.zeros((1, 4, 4))
    print(f"[pnp_ransac] {what}: max |dR| {d[:, :3, :3].max():.3g}, max |dt| {d[:, :3, 3].max():.3g}, trials {trials.tolist()}")
    assert d[:, :3, :3].max() < TOL and d[:, :3, 3].max() < TOL, what
    assert np.array_equal(poses[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (len(poses), 1))), what
    assert np.array_equal(info[:, 2], masks.sum(1)), what


# ------------------------------------------------------------------------------------------------------------------- exports

def test_exports_header_and_abi():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "boxdreamer_hip.h")).read()
    for name, decl in (("bd_solve_pnp_ransac_workspace_bytes", "size_t bd_solve_pnp_ransac_workspace_bytes(int n_samples, int n_trials);"),
                       ("bd_solve_pnp_ransac_wave", "int bd_solve_pnp_ransac_wave("), ("bd_solve_pnp_ransac_host", "int bd_solve_pnp_ransac_host(")):
        assert name in _lib.EXPORTS and hasattr(lib, name) and decl in hdr, name
    assert "box_utils.py:202-300" in hdr[hdr.index("RANSAC PnP over the n_rounds x 8"):hdr.index("size_t bd_solve_pnp_ransac_workspace_bytes(")]
    assert "box_utils.py:202-300" in hdr[hdr.index("int bd_solve_pnp_ransac_wave("):hdr.index("int bd_solve_pnp_ransac_host(")]
    assert lib.bd_abi_version() == 9
    assert lib.bd_solve_pnp_ransac_workspace_bytes(3, 1000) >= 3 * 1000 * 20          # count, error sum and a 64-bit mask per hypothesis
    assert lib.bd_solve_pnp_ransac_workspace_bytes(0, 1000) == 0 and lib.bd_solve_pnp_ransac_workspace_bytes(3, -1) == 0


def test_argument_checks_return_before_a_launch():
    """A null pointer -> BD_ERR_NULL, a bad count or a short workspace -> BD_ERR_SHAPE, all before anything touches a device (the
    non-null pointers below are host buffers that no kernel may ever see); rms_px and info may be NULL."""
    lib = _lib.load()
    kp, box, K, picks = (C.c_float * 128)(), (C.c_float * 24)(), (C.c_float * 9)(), (C.c_int32 * 60)()
    poses, inl, rms, info, ws = (C.c_float * 16)(), (C.c_ubyte * 64)(), (C.c_float * 1)(), (C.c_int32 * 4)(), (C.c_double * 64)()
    a = lambda x: C.cast(x, C.c_void_p)
    need = lib.bd_solve_pnp_ransac_workspace_bytes(1, 10)
    assert 0 < need <= C.sizeof(ws)
    #       0      1       2     3         4  5  6   7    8     9  10  11        12      13      14       15     16    17
    good = [a(kp), a(box), a(K), a(picks), 1, 3, 10, 2.0, 0.99, 5, 30, a(poses), a(inl), a(rms), a(info), a(ws), need, None]
    host = lambda args: args[:15] + [1]
    for i in (0, 1, 2, 3, 11, 12, 15):
        args = list(good)
        args[i] = None
        assert lib.bd_solve_pnp_ransac_wave(*args) == BD_ERR_NULL, i
        if i != 15:
            assert lib.bd_solve_pnp_ransac_host(*host(args)) == BD_ERR_NULL, i
    for field, value in ((5, 0), (5, 9), (6, 0), (4, 0), (9, -1), (10, -1), (16, need - 1), (16, 0)):
        args = list(good)
        args[field] = value
        assert lib.bd_solve_pnp_ransac_wave(*args) == BD_ERR_SHAPE, (field, value)
        args[13] = args[14] = None                                   # rms_px / info may be NULL: still the shape error
        assert lib.bd_solve_pnp_ransac_wave(*args) == BD_ERR_SHAPE, (field, value)
        if field != 16:
            assert lib.bd_solve_pnp_ransac_host(*host(args)) == BD_ERR_SHAPE, (field, value)


# ------------------------------------------------------------------------------------------------------------------- sampling table

def test_ransac_picks():
    for rounds, trials in ((1, 1), (3, 70), (8, 1000)):
        p = pnp.ransac_picks(rounds, trials, seed=0)
        assert p.dtype == np.int32 and p.shape == (trials, 6) and p.flags.c_contiguous
        assert np.array_equal(p, pnp.ransac_picks(rounds, trials, seed=0))                      # deterministic
        assert p.min() >= 0 and p.max() < rounds * 8
        assert all(len(set(row % 8)) == 6 for row in p)                                        # 6 distinct corners per trial
        if trials > 1:
            assert not np.array_equal(p, pnp.ransac_picks(rounds, trials, seed=1))
    assert (pnp.ransac_picks(1, 200) // 8 == 0).all()
    p = pnp.ransac_picks(8, 1000)
    assert set(np.unique(p // 8)) == set(range(8)) and set(np.unique(p % 8)) == set(range(8))   # every round and corner is drawn
    with pytest.raises(ValueError):
        pnp.ransac_picks(0, 10)


def test_picks_argument_leaves_the_default_draws_alone():
    """picks=None is the function as it was (same stream, same result); picks=... runs exactly those samples."""
    kp, box, K, _, _ = ransac_scene(5, 1, 3, (2,))
    p3, p2, Kd = np.tile(box[0].astype(np.float64), (3, 1)), kp[0].reshape(-1, 2).astype(np.float64), K[0].astype(np.float64)
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    try:
        a = pnp.solve_pnp_ransac(p3, p2, Kd, seed=4)
        b = pnp.solve_pnp_ransac(p3, p2, Kd, seed=4, picks=None, want_trials=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b[:4])) and b[4] % 32 == 0 and len(a) == 4
        picks = pnp.ransac_picks(3, 1000, 0)
        c = pnp.solve_pnp_ransac(p3, p2, Kd, seed=4, picks=picks)
        d = pnp.solve_pnp_ransac(p3, p2, Kd, seed=9, picks=picks)                              # the seed no longer matters
        assert all(np.array_equal(x, y) for x, y in zip(c, d))
        assert np.array_equal(c[3].reshape(3, 8).sum(1), [8, 8, 0])
    finally:
        pnp._HAVE_CV2 = have


# ------------------------------------------------------------------------------------------------------------------- the host form

@pytest.mark.parametrize("n_trials", [1000, 70])
@pytest.mark.parametrize("name", ["R1", "R3", "R8"])
def test_host_form_against_the_numpy_twin(name, n_trials):
    """R = 1 (clean), 3 (one bad round), 8 (three bad rounds); at 70 trials the last batch has 6.  The bad rounds are rejected whole."""
    c = case(name, n_trials)
    assert_same_result(c["native"], c, f"{name}, {n_trials} trials")
    poses, inl, rms, info = c["native"]
    per_round = inl.reshape(N, c["rounds"], 8).sum(2)
    for r in range(c["rounds"]):
        assert (per_round[:, r] <= 1).all() if r in c["bad"] else (per_round[:, r] == 8).all(), per_round
    assert (info[:, 3] == 0).all() and (info[:, 1] >= 0).all() and (info[:, 1] < info[:, 0]).all()
    assert (info[:, 0] <= n_trials).all() and (rms > 0).all() and (rms < THR).all()
    # the scene's pose, loosely: 0.3 px of noise on a box ~75 px across is ~1e-3 in R and in t / depth per 16 points
    assert np.abs(poses[:, :3, :3] - c["R"]).max() < 0.02 and np.abs(poses[:, :3, 3] - c["t"]).max() < 0.02
    again = pnp.solve_pnp_ransac_native(c["kp"], c["box"], c["K"], c["picks"], THR, CONF, workers=4)               # threads change no bit
    assert all(np.array_equal(x, y) for x, y in zip(again, c["native"]))


@pytest.mark.parametrize("name", ["R1", "R3", "R8", "R8_clean"])
def test_a_single_trial(name):
    """n_trials = 1: one hypothesis, one short batch.  Clean rounds: it takes everything.  With bad rounds it either hits clean corners
    only (path 0) or the plain solve of all observations runs (path 1), as in the numpy twin."""
    c = case(name, 1)
    assert_same_result(c["native"], c, f"{name}, 1 trial")
    poses, inl, rms, info = c["native"]
    assert (info[:, 0] == 1).all() and (info[:, 1] == 0).all() and (info[:, 3] <= 1).all()
    if not c["bad"]:
        assert inl.all() and (info[:, 3] == 0).all()


@pytest.mark.parametrize("name", ["R3_clean", "R8_clean"])
def test_clean_rounds_take_every_observation_after_one_batch(name):
    c = case(name)
    assert_same_result(c["native"], c, name)
    poses, inl, rms, info = c["native"]
    assert inl.all() and (info[:, 0] == 32).all() and (info[:, 3] == 0).all() and (info[:, 2] == c["rounds"] * 8).all()


@pytest.mark.parametrize("name", ["R1_all_bad", "R3_all_bad", "R8_all_bad"])
def test_every_round_bad_falls_back_to_all_observations(name):
    """No hypothesis finds 6 inliers on 6 corners: path 1, every trial used, and the pose is the plain solve of all observations --
    bd_solve_pnp_host on the tiled box."""
    c = case(name)
    poses, inl, rms, info = c["native"]
    R = c["rounds"]
    assert (info[:, 3] == 1).all() and inl.all() and (info[:, 0] == 1000).all() and (info[:, 2] == R * 8).all()
    assert np.array_equal(info[:, 0], c["twin"][3]) and c["twin"][2].all()
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    try:
        ref = solve_poses_host(c["kp"].reshape(N, R * 8, 2), np.tile(c["box"], (1, R, 1)), c["K"], workers=1)
    finally:
        pnp._HAVE_CV2 = have
    assert (ref[:, 3, 3] == 1.0).all()
    d = np.abs(poses - ref)
    print(f"[pnp_ransac] {name}: max |dR| {d[:, :3, :3].max():.3g}, max |dt| {d[:, :3, 3].max():.3g} vs bd_solve_pnp_host")
    assert d.max() < TOL


def test_a_nan_corner_fails_its_sample_alone():
    c = case("R3")
    kp = c["kp"].copy()
    kp[2, 1, 3, 0] = np.nan
    poses, inl, rms, info = pnp.solve_pnp_ransac_native(kp, c["box"], c["K"], c["picks"], THR, CONF, workers=1)
    assert (poses[2] == 0).all() and not inl[2].any() and rms[2] == 0 and info[2, 3] == 2 and info[2, 2] == 0
    keep = np.arange(N) != 2
    for got, ref in zip((poses, inl, rms, info), c["native"]):
        assert np.array_equal(got[keep], ref[keep])
    ok, _, _, _ = twin(kp[2:3], c["box"][2:3], c["K"][2:3], c["picks"])
    assert not ok[0]


def test_an_out_of_range_pick_is_clamped():
    c = case("R3", 70)
    picks = c["picks"].copy()
    picks[3, 2], picks[5, 0] = 10 ** 6, -7
    clamped = picks.copy()
    clamped[3, 2], clamped[5, 0] = 23, 0
    a = pnp.solve_pnp_ransac_native(c["kp"], c["box"], c["K"], picks, THR, CONF, workers=1)
    b = pnp.solve_pnp_ransac_native(c["kp"], c["box"], c["K"], clamped, THR, CONF, workers=1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------- the model

def _mods(**kw):
    mods = copy.deepcopy(json.load(open(os.path.join(ROOT, "tests", "golden", "model_modules_config.json")))["modules"])
    mods["decoder"].update(num_decoder_layers=1, hip_precision="bf16")
    mods["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=1, hip_precision="bf16")
    mods.update(kw)
    return {"modules": mods}


def test_model_accepts_multi_round_with_the_wave_solver_and_still_refuses_the_bank():
    import torch
    from boxdreamer_amd.model import BoxDreamer
    from test_dense_bank_host import _bank, _batch
    dense_cfg = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": 3, "multi_round": True, "sub_batch_size": 2,
                 "ransac_trials": 200}
    model = BoxDreamer(_mods(pnp_on_device="wave", dense_cfg=dense_cfg)).eval()
    assert model.pnp_on_device == "wave"
    data, table = _batch()
    with pytest.raises(NotImplementedError, match="multi_round"):
        model(dict(data, ref_bank=_bank(model, match_threshold=0.05), ref_rows=table))


def test_device_wrapper_checks_shapes_before_the_gpu():
    import torch
    from boxdreamer_amd.box_utils import RANSAC_MAX_ROUNDS, solve_poses_ransac_device
    assert RANSAC_MAX_ROUNDS == 8
    for shape in ((1, 9, 8, 2), (1, 3, 7, 2), (1, 24, 2)):
        with pytest.raises(ValueError, match="kp_px"):
            solve_poses_ransac_device(torch.zeros(shape), torch.zeros(1, 8, 3), torch.eye(3)[None])
    with pytest.raises(ValueError, match="bbox_3d"):
        solve_poses_ransac_device(torch.zeros(2, 3, 8, 2), torch.zeros(1, 8, 3), torch.eye(3)[None])
