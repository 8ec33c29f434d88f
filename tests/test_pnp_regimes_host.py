"""The pose solvers outside the one scene family every other test draws from, against an INDEPENDENT minimiser of the objective.

Every form of the solver (pnp.solve_pnp_iterative, pnp.solve_pnp_batched, bd_solve_pnp_host, the wave code through
bd_solve_pnp_ransac_host; the GPU kernels in tests/test_gpu_pnp_regimes.py, which imports this file) is one algorithm: DLT start, then
Levenberg-Marquardt on the pixel reprojection error.  Here they are run over a table of REGIMES -- other units, a tight crop's intrinsics,
a close-up, large rotations, heavy noise, a thin box, a far box -- and every returned pose is CLASSIFIED against `reference_minimum`: a
plain fp64 numpy LM with an analytic Jacobian on SO(3) x R^3, written for this file (it shares no code with boxdreamer_amd/pnp.py: another
parametrisation, another Jacobian, another damping schedule), started at the true pose and at the form's own output.  That reference is
itself pinned against scipy's MINPACK LM (test_reference_minimum_is_minpacks_minimum), so the GPU tests can use it without scipy.

A CASE is one (regime, seed): N = 40 poses.  Inputs are rounded to fp32 (what the native forms take) before ANY form or the reference
sees them.  The classes, per pose (`classify`):
  failed          the form returned zeros
  behind          some point has z <= 0 under the returned pose
  at_reference    cost <= reference * (1 + 1e-6) + 1e-9 (the margin of test_host_logic's minimiser test), cost = sum of squared pixel errors;
                  on EXACT corners (regime `exact`), for an fp32 pose, plus what rounding the reference pose to fp32 can cost
                  (fp32_rounding_cost, ~1e-8 px^2)
  other_minimum   stationary (the reference started there lowers the cost by no more than 1e-6 relative) at a higher cost
  not_stationary  the reference started there lowers the cost by more than 1e-6 relative: the form stopped on a slope
WELL-POSED regimes: every pose of every form is at_reference and within 5e-7 (fp64 forms) / 2e-6 (fp32 outputs) of the reference pose.
HARD regimes: no pose is not_stationary or behind; at most 5 % are other_minimum or failed (local minima of a DLT start on nearly planar
or very noisy corners: OpenCV switches to a planar start there, which this solver does not reproduce).
"""
import numpy as np
import pytest

from boxdreamer_amd import pnp
from boxdreamer_amd.box_utils import solve_poses_host

N = 40
EXT = (0.1, 0.07, 0.05)
TOL64, TOL32, TOL_FORMS = 5e-7, 2e-6, 1e-4          # the tolerances the existing tests hold the forms to
CAP = 0.05                                          # hard regimes: share of poses that may be other_minimum or failed
SIGNS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float)


def _regime(**kw):
    r = dict(ext=EXT, depth=(0.55, 1.05), f=(600.0, 600.0), c=(112.0, 112.0), place=None, rot=0.9, noise=0.7, scale=1.0, npts=8, seeds=(1,),
             hard=False)
    r.update(kw)
    return r


# ext: box half-extents (m); depth: range of t_z (m); f, c: intrinsics; place: range of the pixel the box centre projects to (None: t_xy
# normal * 0.0625 t_z, i.e. +- 37 px at f = 600); rot: spread of the rotation vector; noise: px; scale: model units per metre.
# No regime needs a wider tolerance than TOL64 / TOL32: the reference's own two starts (the truth, a form's pose) never differ by more than a
# tenth of it -- the measured spread is the comment at the end of each line -- and check_well_posed asserts that.
REGIMES = {
    "base": _regime(),                                                                                     # spread 2e-12
    "mm": _regime(scale=1000.0),                                                                           # spread 2e-12
    "tele_crop": _regime(f=(6000.0, 6000.0), c=(-2500.0, 3100.0), depth=(4.0, 8.0), place=(60.0, 164.0)),  # spread 3e-11
    "close": _regime(f=(300.0, 300.0), depth=(0.16, 0.22)),                                                # spread 1e-12
    "big_rot": _regime(rot=3.0),                                                                           # spread 2e-12
    "noise3": _regime(noise=3.0),                                                                          # spread 3e-12
    "aniso": _regime(f=(600.0, 450.0)),                                                                    # spread 2e-12
    "pts64": _regime(npts=64),                                                                             # spread 1e-12
    "exact": _regime(noise=0.0),                                                                           # spread 1e-12
    "thin": _regime(ext=(0.075, 0.035, 0.004), depth=(0.4, 0.7), seeds=(12, 18), hard=True),
    "noise5": _regime(noise=5.0, seeds=(4, 11), hard=True),
    "noise8": _regime(noise=8.0, seeds=(8, 22), hard=True),
    # far seed 16 holds the pose that pins the cap: its start overshoots to four times the depth, LM needs ~800 iterations to come back, and
    # under the cap of 400 every form must return it as FAILED (inside the 5 %), not as a pose from the slope
    "far": _regime(depth=(4.0, 8.0), seeds=(2, 11, 16), hard=True),
}
WELL_POSED = [k for k, v in REGIMES.items() if not v["hard"]]
HARD = [(k, s) for k, v in REGIMES.items() if v["hard"] for s in v["seeds"]]
ALL_CASES = [(k, s) for k, v in REGIMES.items() for s in v["seeds"]]


# ------------------------------------------------------------------------------------------------------------------- scenes

def _rotation(w):
    """exp of the skew matrix of w [.., 3] -> [.., 3, 3] (this file's own: cos I + sin [k]x + (1 - cos) k k^T)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    k = w / np.where(th[..., 0] == 0, 1.0, th[..., 0])
    hat = np.zeros(w.shape[:-1] + (3, 3))
    hat[..., 0, 1], hat[..., 0, 2], hat[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    hat[..., 1, 2], hat[..., 2, 0], hat[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.cos(th) * np.eye(3) + np.sin(th) * hat + (1 - np.cos(th)) * (k[..., :, None] * k[..., None, :])


def make_case(name, seed, rounds=None, n=N, shift=(0.0, 0.0)):
    """One case of regime `name`: the fp32 arrays the solvers receive (kp [n, P, 2] pixels, p3 [n, P, 3], K [n, 3, 3]) and the fp64 truth
    (R, t).  rounds=None: the regime's own points (the 8 box corners, plus npts - 8 points normal * extents).  rounds=R: R observations of
    the 8 corners under independent noise (P = 8 R; kp also as [n, R, 8, 2] under "kp_rounds", the corners under "box"), round 0 carrying
    the noise of the rounds=None case.  The poses depend on (name, seed) only; `mm` is `base` times 1000 on the same seeds.  shift: added
    to every pixel and to the principal point before the rounding to fp32."""
    g = REGIMES[name]
    rng = np.random.default_rng([20261020, seed])
    noise_rng = np.random.default_rng([20261021, seed])
    ext, (fx, fy), (cx, cy) = np.asarray(g["ext"], float), g["f"], g["c"]
    R = _rotation(rng.normal(size=(n, 3)) * g["rot"])
    z = g["depth"][0] + rng.random(n) * (g["depth"][1] - g["depth"][0])
    if g["place"] is None:
        t = np.stack([rng.normal(size=n) * 0.0625 * z, rng.normal(size=n) * 0.0625 * z, z], 1)
    else:
        u0 = g["place"][0] + rng.random((n, 2)) * (g["place"][1] - g["place"][0])
        t = np.stack([(u0[:, 0] - cx) / fx * z, (u0[:, 1] - cy) / fy * z, z], 1)
    extra = rng.normal(size=(n, max(g["npts"] - 8, 0), 3)) * ext
    box = np.tile(SIGNS * ext, (n, 1, 1))
    p3 = np.concatenate([box, extra], 1) if rounds is None else np.tile(box, (1, rounds, 1))
    pc = p3 @ np.swapaxes(R, 1, 2) + t[:, None]
    assert (pc[..., 2] > 0).all()
    exact = pc[..., :2] / pc[..., 2:] * [fx, fy] + [cx, cy]
    noise = np.concatenate([noise_rng.normal(size=(n, 8, 2)), noise_rng.normal(size=(n, p3.shape[1] - 8, 2))], 1) * g["noise"]
    K = np.tile(np.array([[fx, 0, cx + shift[0]], [0, fy, cy + shift[1]], [0, 0, 1]]), (n, 1, 1))
    c = {"name": name, "seed": seed, "kp": (exact + noise + np.asarray(shift)).astype(np.float32), "p3": (p3 * g["scale"]).astype(np.float32),
         "K": K.astype(np.float32), "R": R, "t": t * g["scale"], "hard": g["hard"]}
    if rounds is not None:
        c["kp_rounds"], c["box"] = c["kp"].reshape(n, rounds, 8, 2), np.ascontiguousarray(c["p3"][:, :8])
    return c


def take(c, rows):
    """The case restricted to `rows` (a slice)."""
    return {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in c.items() if k != "ref_truth"}


# ------------------------------------------------------------------------------------------------------------------- the reference

def _f64(c):
    return c["kp"].astype(np.float64), c["p3"].astype(np.float64), c["K"].astype(np.float64)


def pixel_residuals(R, t, c):
    """-> (residuals [n, 2 P] in pixels (u0, v0, u1, ..), camera-frame points [n, P, 3]), fp64 from the case's fp32 inputs."""
    kp, p3, K = _f64(c)
    pc = np.einsum("nij,npj->npi", R, p3) + t[:, None]
    f, pp = np.stack([K[:, 0, 0], K[:, 1, 1]], 1)[:, None], K[:, None, :2, 2]
    with np.errstate(all="ignore"):
        r = pc[..., :2] / pc[..., 2:] * f + pp - kp
    return r.reshape(len(kp), -1), pc


def cost_of(R, t, c):
    r, pc = pixel_residuals(R, t, c)
    return (r * r).sum(1), pc[..., 2].min(1)


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    d = np.sign(np.linalg.det(U @ Vt))
    U = U.copy()
    U[..., :, 2] *= d[..., None]
    return U @ Vt


def reference_minimum(c, start=None, max_iter=400):
    """fp64 Levenberg-Marquardt on the pixel residuals over SO(3) x R^3 with the analytic Jacobian of the left perturbation
    R <- exp(d) R, t <- t + e, all poses of the case at once, run to convergence (at most max_iter steps).  start: poses [n, 4, 4] (their
    rotation part is projected onto SO(3)); rows that are zeros, not finite, or put a point behind the camera start at the true pose, like
    start=None.  -> (R [n, 3, 3], t [n, 3], cost [n] = sum of squared pixel errors, iterations [n])."""
    kp, p3, K = _f64(c)
    n = len(kp)
    R, t = c["R"].copy(), c["t"].copy()
    if start is not None:
        s = np.asarray(start, np.float64)
        good = np.isfinite(s).all((1, 2)) & (s[:, 3, 3] == 1.0)
        Rs = np.where(good[:, None, None], s[:, :3, :3], np.eye(3))
        Rs, ts = nearest_rotation(Rs), s[:, :3, 3]
        good &= cost_of(Rs, ts, c)[1] > 0
        R[good], t[good] = Rs[good], ts[good]
    fx, fy = K[:, 0, 0][:, None], K[:, 1, 1][:, None]
    r, pc = pixel_residuals(R, t, c)
    cost = (r * r).sum(1)
    lam = np.full(n, 1e-3)
    active = np.ones(n, bool)
    iters = np.zeros(n, int)
    for _ in range(max_iter):
        if not active.any():
            break
        x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
        q = pc - t[:, None]                                          # R p: d(pc) / d(rotation) = -[q]x, d(pc) / d(t) = I
        du = np.stack([fx / z, np.zeros_like(z), -fx * x / z ** 2], -1)          # [n, P, 3]: d u / d pc
        dv = np.stack([np.zeros_like(z), fy / z, -fy * y / z ** 2], -1)
        J = np.empty((n, r.shape[1], 6))
        J[:, 0::2, :3], J[:, 1::2, :3] = np.cross(q, du), np.cross(q, dv)       # row^T (-[q]x) = q x row
        J[:, 0::2, 3:], J[:, 1::2, 3:] = du, dv
        H, g = np.swapaxes(J, 1, 2) @ J, np.einsum("nij,ni->nj", J, r)
        D = np.einsum("nii->ni", H)
        A = H + (lam[:, None] * D)[:, :, None] * np.eye(6)
        A[~active] = np.eye(6)
        d = np.linalg.solve(A, -g[:, :, None])[:, :, 0]
        Rn, tn = _rotation(d[:, :3]) @ R, t + d[:, 3:]
        rn, pcn = pixel_residuals(Rn, tn, c)
        cn = (rn * rn).sum(1)
        # (within 1e-13 of the minimum's cost the comparison is rounding noise: the step is taken, it contracts towards the stationary point)
        better = active & np.isfinite(cn) & (cn <= cost * (1 + 1e-13)) & (pcn[..., 2].min(1) > 0)
        tiny = np.maximum(np.abs(d[:, :3]).max(1), np.abs(d[:, 3:]).max(1) / np.maximum(1.0, np.abs(t).max(1))) < 1e-14
        R[better], t[better], r[better], pc[better], cost[better] = Rn[better], tn[better], rn[better], pcn[better], cn[better]
        lam = np.where(better, np.maximum(lam / 5.0, 1e-12), lam * 4.0)
        iters[active] += 1
        active &= ~tiny & (lam < 1e12)
    return nearest_rotation(R), t, cost, iters


def pose_distance(Ra, ta, Rb, tb):
    """max(|dR|, |dt| / max(1, |t_b|_inf)) per pose."""
    return np.maximum(np.abs(Ra - Rb).max((1, 2)), np.abs(ta - tb).max(1) / np.maximum(1.0, np.abs(tb).max(1)))


def fp32_rounding_cost(c):
    """What the fp32 OUTPUT alone may add to the cost of the reference minimum, per pose: every entry of [R | t] off by half an fp32 ulp
    (<= 2^-24 of its magnitude), all with the worst sign: sum over the residuals of (sum over the entries of |d residual / d entry| *
    2^-24 |entry|)^2.  (The first-order term vanishes at the minimum.)  It is ~1e-8 px^2: nothing against the 1e-6 relative margin on noisy
    corners (~1e-5 px^2), but all there is on exact ones, where the cost is ~1e-10 px^2 and the margin 1e-9."""
    if "ref_truth" not in c:
        c["ref_truth"] = reference_minimum(c)
    R, t = c["ref_truth"][:2]
    kp, p3, K = _f64(c)
    pc = np.einsum("nij,npj->npi", R, p3) + t[:, None]
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
    fx, fy = K[:, 0, 0][:, None], K[:, 1, 1][:, None]
    du = np.abs(np.stack([fx / z, np.zeros_like(z), fx * x / z ** 2], -1))            # [n, P, 3]: |d u / d pc|
    dv = np.abs(np.stack([np.zeros_like(z), fy / z, fy * y / z ** 2], -1))
    dpc = (np.einsum("nij,npj->npi", np.abs(R), np.abs(p3)) + np.abs(t)[:, None]) * 2.0 ** -24      # [n, P, 3]: what the entries move pc by
    return ((du * dpc).sum(-1) ** 2 + (dv * dpc).sum(-1) ** 2).sum(1)


LABELS = ("at_reference", "other_minimum", "failed", "behind", "not_stationary")


def classify(poses, c, ref_cost=None):
    """poses [n, 4, 4] as a form returned them (fp32 or fp64) -> per pose a dict: label, cost (of the pose, rotation part projected onto
    SO(3)), ref (the reference cost: the lowest of ref_cost, the reference from the truth and the reference from this pose), polished (the
    cost the reference reaches from this pose)."""
    P = np.asarray(poses, np.float64)
    n = len(P)
    failed = ~np.isfinite(P).all((1, 2)) | (P[:, 3, 3] != 1.0)
    Rp = nearest_rotation(np.where(failed[:, None, None], np.eye(3), P[:, :3, :3]))
    tp = np.where(failed[:, None], c["t"], P[:, :3, 3])
    cost, zmin = cost_of(Rp, tp, c)
    behind = ~failed & ~(zmin > 0)
    if "ref_truth" not in c:
        c["ref_truth"] = reference_minimum(c)
    polished = reference_minimum(c, P)[2]
    # (only where the corners are exact: every regime with noise keeps the margin as it is, there the 1e-6 relative term covers it)
    fp32 = fp32_rounding_cost(c) if np.asarray(poses).dtype == np.float32 and REGIMES[c["name"]]["noise"] == 0 else np.zeros(n)
    ref = np.minimum(c["ref_truth"][2], polished)
    if ref_cost is not None:
        ref = np.minimum(ref, ref_cost)
    out = []
    for i in range(n):
        if failed[i]:
            label = "failed"
        elif behind[i]:
            label = "behind"
        elif cost[i] <= ref[i] * (1 + 1e-6) + 1e-9 + fp32[i]:
            label = "at_reference"
        elif cost[i] - polished[i] <= 1e-6 * cost[i]:
            label = "other_minimum"
        else:
            label = "not_stationary"
        out.append({"label": label, "cost": float(cost[i]), "ref": float(ref[i]), "polished": float(polished[i])})
    return out


def counts(cls):
    return {k: sum(1 for x in cls if x["label"] == k) for k in LABELS}


def check_hard(cls, what):
    """The hard-regime conditions on one form's classification of one case; prints every pose that is not at the reference."""
    for i, x in enumerate(cls):
        if x["label"] != "at_reference":
            print(f"[pnp_regimes] {what} pose {i}: {x['label']}, cost {x['cost']:.6g} px^2, reference {x['ref']:.6g} px^2, "
                  f"reference started there reaches {x['polished']:.6g}")
    k = counts(cls)
    print(f"[pnp_regimes] {what}: {k}")
    assert k["not_stationary"] == 0, (what, k)
    assert k["behind"] == 0, (what, k)
    assert k["other_minimum"] + k["failed"] <= CAP * len(cls), (what, k)
    return k


def check_well_posed(poses, cls, c, tol, what):
    """Every pose at_reference and within tol of the reference pose (the reference from the truth; its spread against the reference
    started at the form's pose is printed and must stay below a tenth of tol)."""
    k = counts(cls)
    assert k["at_reference"] == len(cls), (what, k, [(i, x) for i, x in enumerate(cls) if x["label"] != "at_reference"])
    P = np.asarray(poses, np.float64)
    Rr, tr = c["ref_truth"][:2]
    d = pose_distance(P[:, :3, :3], P[:, :3, 3], Rr, tr)
    Rs, ts = reference_minimum(c, P)[:2]
    spread = pose_distance(Rs, ts, Rr, tr).max()
    print(f"[pnp_regimes] {what}: max distance to the reference pose {d.max():.3g} (tolerance {tol:g}), reference's own spread {spread:.3g}")
    assert spread <= tol / 10, (what, spread)
    assert d.max() < tol, (what, d.max(), int(d.argmax()))
    return d.max(), spread


# ------------------------------------------------------------------------------------------------------------------- the host forms

def as44(ok, R, t):
    P = np.zeros((len(R), 4, 4))
    P[ok, :3, :3], P[ok, :3, 3], P[ok, 3, 3] = R[ok], t[ok], 1.0
    return P


def form_scalar(c):
    kp, p3, K = _f64(c)
    res = [pnp.solve_pnp_iterative(p3[i], kp[i], K[i]) for i in range(len(kp))]
    return as44(np.array([r[0] for r in res], bool), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]))


def form_batched(c):
    kp, p3, K = _f64(c)
    return as44(*pnp.solve_pnp_batched(p3, kp, K))


def form_native(c):
    return solve_poses_host(c["kp"], c["p3"], c["K"], workers=1)


def ransac_inputs(c):
    """The RANSAC forms take R rounds of the 8 box corners: a case of 8 points is one round of itself; a regime with more points runs
    as P / 8 rounds of the corners (make_case(rounds=...)), which the caller passes in as `c`."""
    if "kp_rounds" in c:
        return c["kp_rounds"], c["box"]
    assert c["kp"].shape[1] == 8
    return c["kp"][:, None], c["p3"]


RANSAC_PICKS, RANSAC_THR = 4, 1e9          # a short table; every observation in front of the camera is an inlier


def form_ransac_native(c):
    """The wave code on the host: bd_solve_pnp_ransac_host, all observations inliers, so its last stage is pnp_wave_solve on all of them."""
    kp, box = ransac_inputs(c)
    poses, inl, rms, info = pnp.solve_pnp_ransac_native(kp, box, c["K"], pnp.ransac_picks(kp.shape[1], RANSAC_PICKS, 0), RANSAC_THR, 0.99, workers=1)
    solved = info[:, 3] != 2
    assert (info[solved, 2] == kp.shape[1] * 8).all() and inl[solved].all(), (c["name"], info)       # the all-inlier path ran
    assert (poses[~solved] == 0).all() and (rms[~solved] == 0).all()
    return poses


HOST_FORMS = {"scalar": (form_scalar, TOL64), "batched": (form_batched, TOL64), "native": (form_native, TOL32),
              "ransac_native": (form_ransac_native, TOL32)}
_CACHE = {}


def ransac_case(name, seed):
    """The case the RANSAC forms run for (name, seed): the case itself at 8 points, else its rounds variant."""
    P = REGIMES[name]["npts"]
    return case(name, seed) if P == 8 else case(name, seed, rounds=P // 8)


def case(name, seed, rounds=None):
    key = (name, seed, rounds)
    if key not in _CACHE:
        _CACHE[key] = make_case(name, seed, rounds)
    return _CACHE[key]


def host_results(name, seed):
    """Every host form on (name, seed), computed once and never modified: {form: (case it ran on, poses, classification)}.  The reference
    cost of a pose is the lowest any start reached: the truth, and every form's output on the same case."""
    key = ("host", name, seed)
    if key not in _CACHE:
        have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
        try:
            runs = {f: (ransac_case(name, seed) if f == "ransac_native" else case(name, seed)) for f in HOST_FORMS}
            poses = {f: HOST_FORMS[f][0](runs[f]) for f in HOST_FORMS}
        finally:
            pnp._HAVE_CV2 = have
        _CACHE[key] = classify_forms(runs, poses)
    return _CACHE[key]


def classify_forms(runs, poses):
    """{form: case}, {form: poses} -> {form: (case, poses, classification)} with the reference cost shared among the forms of a case."""
    first = {f: classify(poses[f], runs[f]) for f in poses}
    out = {}
    for f in poses:
        same = [g for g in poses if runs[g] is runs[f]]
        best = np.min([[x["ref"] for x in first[g]] for g in same], 0)
        out[f] = (runs[f], poses[f], classify(poses[f], runs[f], best) if len(same) > 1 else first[f])
    return out


# ------------------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("name,seed", ALL_CASES)
def test_reference_minimum_is_minpacks_minimum(name, seed):
    """reference_minimum from the true pose against scipy.optimize.least_squares(method="lm") at 1e-15 tolerances from the true pose: cost to
    1e-9 relative, pose to 1e-8.  MINPACK works in its own parametrisation (rotation vector, scipy's Rotation, its own column scaling) with
    the EXACT Jacobian of that parametrisation, d(R p)/dv = -R [p]x Jr(v), Jr the right Jacobian of SO(3); the first pose of each case
    checks it against central differences.  (A differenced Jacobian will not do: its ~1e-10 of noise is enough to make MINPACK's gain
    ratio collapse the trust region on the nearly planar box, 1.1e-8 short of the minimum, and its own forward differences leave 5e-8.)
    MEASURED over the 16 cases (640 poses): cost within 7e-13 relative; pose within 7.4e-9, but for thin seed 18 pose 30 at 9.7e-9,
    where MINPACK's ftol test (a relative cost decrease of 1e-15) ends it that far out along the flat direction of the thin box."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    c = case(name, seed)
    kp, p3, K = _f64(c)
    Rr, tr, cr, iters = reference_minimum(c)
    assert iters.max() < 400, (name, seed, iters.max())          # it converged, the cap did not end it

    def skew(a):
        return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])

    worst_c = worst_p = 0.0
    for i in range(N):
        f = np.array([K[i, 0, 0], K[i, 1, 1]])

        def fun(v):
            pc = p3[i] @ Rotation.from_rotvec(v[:3]).as_matrix().T + v[3:]
            return (pc[:, :2] / pc[:, 2:3] * f + K[i, :2, 2] - kp[i]).reshape(-1)

        def jac(v):
            R, th, W = Rotation.from_rotvec(v[:3]).as_matrix(), np.linalg.norm(v[:3]), skew(v[:3])
            Jr = np.eye(3) - (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * (W @ W) if th > 1e-8 else np.eye(3) - 0.5 * W
            pc = p3[i] @ R.T + v[3:]
            J = np.zeros((2 * len(pc), 6))
            for k, (p, q) in enumerate(zip(p3[i], pc)):
                du = np.array([[f[0] / q[2], 0.0, -f[0] * q[0] / q[2] ** 2], [0.0, f[1] / q[2], -f[1] * q[1] / q[2] ** 2]])
                J[2 * k:2 * k + 2] = du @ np.concatenate([-R @ skew(p) @ Jr, np.eye(3)], 1)
            return J

        v0 = np.concatenate([Rotation.from_matrix(c["R"][i]).as_rotvec(), c["t"][i]])
        if i == 0:
            h = 1e-6 * np.r_[1.0, 1.0, 1.0, [max(1.0, np.abs(v0[3:]).max())] * 3]
            Jn = np.stack([(fun(v0 + h[j] * e) - fun(v0 - h[j] * e)) / (2 * h[j]) for j, e in enumerate(np.eye(6))], 1)
            assert np.abs(Jn - jac(v0)).max() < 1e-8 * np.abs(Jn).max(), (name, seed)
        s = least_squares(fun, v0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac")
        cs = float(s.fun @ s.fun)
        dc = max(abs(cs - cr[i]) - 1e-16, 0.0) / cs       # (1e-16 px^2: on exact corners the cost is 16 residuals of ~1e-6 px, each the
                                                          # difference of two ~200 px numbers and so good to 5e-14: 2 * 16 * 1e-6 * 5e-14 is 1.6e-18)
        dp = pose_distance(Rr[i:i + 1], tr[i:i + 1], Rotation.from_rotvec(s.x[:3]).as_matrix()[None], s.x[None, 3:])[0]
        worst_c, worst_p = max(worst_c, dc), max(worst_p, dp)
        assert dc < 1e-9 and dp < 1e-8, (name, seed, i, cs, cr[i], dp)
    print(f"[pnp_regimes] {name} seed {seed}: reference vs MINPACK, cost {worst_c:.3g} relative, pose {worst_p:.3g}; "
          f"at most {iters.max()} reference iterations")


def test_classify_tells_the_classes_apart():
    """classify on constructed poses of a base case: the reference pose, zeros, a pose turned to face away, the reference pose nudged
    off the minimum, and the truth (which noisy corners make a non-stationary point)."""
    c = make_case("base", 3, n=5)
    Rr, tr, cr, _ = reference_minimum(c)
    P = as44(np.ones(5, bool), Rr, tr)
    P[1] = 0.0
    P[2, :3, 3] = -P[2, :3, 3]
    P[3, :3, 3] += [0.0, 0.0, 0.01]
    P[4, :3, :3], P[4, :3, 3] = c["R"][4], c["t"][4]
    got = [x["label"] for x in classify(P.astype(np.float32), c)]
    assert got == ["at_reference", "failed", "behind", "not_stationary", "not_stationary"], got
    assert [x["label"] for x in classify(P[:1], take(c, slice(0, 1)))] == ["at_reference"]


@pytest.mark.parametrize("form", list(HOST_FORMS))
@pytest.mark.parametrize("name", WELL_POSED)
def test_well_posed_regimes_reach_the_reference(name, form):
    for seed in REGIMES[name]["seeds"]:
        c, poses, cls = host_results(name, seed)[form]
        check_well_posed(poses, cls, c, HOST_FORMS[form][1], f"{name} seed {seed}, {form}")


def test_the_cap_is_not_a_budget():
    """Two ends of the stop rule on the native host form.  Exact corners (`exact`: the error is the fp32 rounding of the pixels) converge
    well inside the cap: with iters = LM_STRICT_ITERS, where a solve that has not converged has no pose, all 40 are solved, as are the
    `base` poses.  And the far seed 16 pose that needs ~800 iterations is zeros at the default cap, while a budget (iters below
    LM_STRICT_ITERS) returns its iterate as it stands."""
    from boxdreamer_amd import _lib
    lib = _lib.load()

    def native(c, iters):
        out = np.zeros((len(c["kp"]), 4, 4), np.float32)
        assert lib.bd_solve_pnp_host(c["kp"].ctypes.data, c["p3"].ctypes.data, c["K"].ctypes.data, len(c["kp"]), c["kp"].shape[1], iters,
                                     out.ctypes.data, 1) == 0
        return out
    for name in ("exact", "base"):
        assert (native(case(name, 1), pnp.LM_STRICT_ITERS)[:, 3, 3] == 1.0).all(), name
        have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
        try:
            kp, p3, K = _f64(case(name, 1))
            assert pnp.solve_pnp_batched(p3, kp, K, iters=pnp.LM_STRICT_ITERS)[0].all(), name
        finally:
            pnp._HAVE_CV2 = have
    c = case("far", 16)
    full, budget = native(c, pnp.LM_MAX_ITERS), native(c, pnp.LM_STRICT_ITERS - 1)
    unfinished = np.nonzero(full[:, 3, 3] != 1.0)[0]
    assert len(unfinished) == 1 and (full[unfinished] == 0).all(), unfinished
    assert (budget[:, 3, 3] == 1.0).all()


@pytest.mark.parametrize("name", WELL_POSED)
def test_well_posed_regimes_forms_agree(name):
    """The forms that ran on the same inputs agree with each other within 1e-4 (pts64: the RANSAC form runs another case)."""
    for seed in REGIMES[name]["seeds"]:
        res = host_results(name, seed)
        forms = [f for f in res if res[f][0] is res["native"][0]]
        for a in forms:
            for b in forms:
                d = np.abs(np.asarray(res[a][1], np.float64) - np.asarray(res[b][1], np.float64))
                d[:, :3, 3] /= np.maximum(1.0, np.abs(res[b][0]["t"]).max(1))[:, None]
                assert d.max() < TOL_FORMS, (name, a, b, d.max())


@pytest.mark.parametrize("form", list(HOST_FORMS))
def test_millimetres_give_the_same_pose_as_metres(form):
    """`mm` is `base` times 1000 on the same seeds and the same pixels: same R to 1e-6, t / 1000 to 1e-6 relative, pose by pose."""
    a, b = host_results("base", 1)[form], host_results("mm", 1)[form]
    assert np.array_equal(a[0]["kp"], b[0]["kp"])
    Pa, Pb = np.asarray(a[1], np.float64), np.asarray(b[1], np.float64)
    dR = np.abs(Pa[:, :3, :3] - Pb[:, :3, :3]).max()
    dt = (np.abs(Pa[:, :3, 3] - Pb[:, :3, 3] / 1000.0).max(1) / np.abs(Pa[:, :3, 3]).max(1)).max()
    print(f"[pnp_regimes] mm against base, {form}: |dR| {dR:.3g}, relative |dt| {dt:.3g}")
    assert dR < 1e-6 and dt < 1e-6, (form, dR, dt)


SHIFT = (1000.0, -700.0)


@pytest.mark.parametrize("form", list(HOST_FORMS))
def test_a_shifted_image_gives_the_same_pose(form):
    """Every pixel and the principal point moved by (1000, -700): R and t stay within 1e-6 of the unshifted result, and within the
    well-posed tolerance of the reference OF THE SHIFTED INPUTS (fp32 pixels near 1100 carry 1.2e-4 px of rounding, which moves the minimum
    itself by ~1e-7)."""
    base = host_results("base", 1)[form]
    c = make_case("base", 1, shift=SHIFT)
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    try:
        poses = HOST_FORMS[form][0](c)
    finally:
        pnp._HAVE_CV2 = have
    check_well_posed(poses, classify(poses, c), c, HOST_FORMS[form][1], f"base shifted by {SHIFT}, {form}")
    d = pose_distance(np.asarray(poses, np.float64)[:, :3, :3], np.asarray(poses, np.float64)[:, :3, 3],
                      np.asarray(base[1], np.float64)[:, :3, :3], np.asarray(base[1], np.float64)[:, :3, 3])
    print(f"[pnp_regimes] shifted against unshifted, {form}: {d.max():.3g}")
    assert d.max() < 1e-6, (form, d.max())


@pytest.mark.parametrize("form", list(HOST_FORMS))
@pytest.mark.parametrize("name,seed", HARD)
def test_hard_regimes_stop_on_a_minimum_in_front_of_the_camera(name, seed, form):
    c, poses, cls = host_results(name, seed)[form]
    check_hard(cls, f"{name} seed {seed}, {form}")


@pytest.mark.parametrize("name,seed", HARD)
def test_hard_regimes_report_disagreements(name, seed):
    """Forms may settle in different minima here (a last-bit difference decides an accept / reject): the count is printed, not asserted."""
    res = host_results(name, seed)
    forms = [f for f in res if res[f][0] is res["native"][0]]
    for i, a in enumerate(forms):
        for b in forms[i + 1:]:
            d = np.abs(np.asarray(res[a][1], np.float64) - np.asarray(res[b][1], np.float64)).max((1, 2))
            print(f"[pnp_regimes] {name} seed {seed}: {a} and {b} differ by more than {TOL_FORMS:g} on {int((d > TOL_FORMS).sum())} of {N} poses")
