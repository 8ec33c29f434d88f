"""Two builds of the library on the same pose problems, bit for bit: the device forms of csrc/pnp.hip (bd_solve_pnp, bd_solve_pnp_wave,
bd_solve_pnp_ransac_wave) of build A against build B, for a change that must not change what the solvers compute.

    python tools/pnp_forms_ab.py --a /path/to/A/libboxdreamer_hip.so --b boxdreamer_amd/libboxdreamer_hip.so [--out DIR] [--report FILE.md]

This process never opens the device.  It starts one child per library ($BOXDREAMER_HIP_LIB names it), each under its own
`timeout -k 10`, one after the other, and stops at the first that fails.  A child runs the regime table of
tests/test_pnp_regimes_host.py (every (regime, seed): 40 poses of 8 points, `pts64` of 64; the RANSAC form on the rounds variant), at
most 32 poses per launch, and stores what came back as it is:
  thread   bd_solve_pnp                                       poses
  wave     bd_solve_pnp_wave                                  poses, rms_px
  ransac   bd_solve_pnp_ransac_wave, 64 trials at 2 px        poses, inliers, rms_px, info
  host     bd_solve_pnp_host, one thread (the thread form's source, compiled for the CPU)
Device code is compiled with FMA contraction, so statements that moved can move a last bit.  Per form and regime the page gives the
number of 32-bit words that differ and the largest |A - B| of a pose entry or rms_px; next to it, measured in the same run, the largest
|thread - host| of build A: the same source on the same inputs, differing by contraction only.  A difference passes only where, in every
well-posed regime, the solved / zeros verdicts are equal and max |A - B| does not exceed that figure; in the hard regimes the caps of
tests/test_gpu_pnp_regimes.py decide.  Exit status 1 where it does not pass, 2 where a child failed."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CHILD_LIMIT = 420            # seconds per child: the import of torch, 16 cases of 40 poses in three device forms and one host form
CHUNK = 32
FORMS = ("thread", "wave", "ransac")


def child(path):
    import numpy as np
    import torch
    from boxdreamer_amd import _lib, pnp
    from boxdreamer_amd.box_utils import solve_poses_device, solve_poses_host, solve_poses_ransac_device
    import test_pnp_regimes_host as T
    _lib.require_gpu()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    out = {}
    pnp._HAVE_CV2 = False
    for name, seed in T.ALL_CASES:
        c, cr = T.case(name, seed), T.ransac_case(name, seed)
        kpr, box = T.ransac_inputs(cr)
        got = {}
        for lo in range(0, T.N, CHUNK):
            rows = slice(lo, min(lo + CHUNK, T.N))
            kp, p3, K = dev(c["kp"][rows]), dev(c["p3"][rows]), dev(c["K"][rows])
            part = {"thread.poses": solve_poses_device(kp, p3, K, form="thread")}
            part["wave.poses"], part["wave.rms"] = solve_poses_device(kp, p3, K, form="wave", want_rms=True)
            r = solve_poses_ransac_device(dev(kpr[rows]), dev(box[rows]), dev(cr["K"][rows]), n_trials=64, reproj_err=2.0, confidence=0.99, seed=0)
            part["ransac.poses"], part["ransac.inliers"], part["ransac.rms"], part["ransac.info"] = r[0], r[1].to(torch.uint8), r[2], r[3]
            for k, v in part.items():
                got.setdefault(k, []).append(v.cpu().numpy())
        for k, v in got.items():
            out[f"{name}/{seed}/{k}"] = np.concatenate(v)
        out[f"{name}/{seed}/host.poses"] = solve_poses_host(c["kp"], c["p3"], c["K"], workers=1)
        print(f"[pnp_forms_ab] {name} seed {seed}: done", flush=True)
    np.savez(path, **out)


def words(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1) if a.dtype.itemsize == 1 else a.view(np.uint32).reshape(-1)


def compare(A, B):
    """-> (rows of the page, passed)."""
    import numpy as np
    import test_pnp_regimes_host as T
    lines = ["| regime | hard | form | words that differ / words | verdicts equal | max abs(A - B) | max abs(thread - host) of A | passes |", "|---|---|---|---|---|---|---|---|"]
    passed, identical = True, True
    for name, g in T.REGIMES.items():
        keys = [k for k in A.files if k.startswith(name + "/")]
        tp = np.concatenate([A[f"{name}/{s}/thread.poses"] for s in g["seeds"]]).astype(np.float64)
        hp = np.concatenate([A[f"{name}/{s}/host.poses"] for s in g["seeds"]]).astype(np.float64)
        both = (tp[:, 3, 3] == 1) & (hp[:, 3, 3] == 1)
        ref = float(np.abs(tp[both] - hp[both]).max()) if both.any() else 0.0
        for form in FORMS:
            diff = total = 0
            dmax, same_verdict = 0.0, True
            for k in keys:
                if k.split("/")[2].split(".")[0] != form:
                    continue
                a, b = A[k], B[k]
                wa, wb = words(a), words(b)
                diff, total = diff + int((wa != wb).sum()), total + wa.size
                if k.endswith(".poses"):
                    same_verdict = same_verdict and np.array_equal(a[:, 3, 3] == 1, b[:, 3, 3] == 1)
                if a.dtype == np.float32:
                    dmax = max(dmax, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
            within = same_verdict and dmax <= ref
            ok = diff == 0 or within or g["hard"]
            passed, identical = passed and ok, identical and diff == 0
            verdict = "identical" if diff == 0 else ("within contraction" if within else ("the tests decide" if g["hard"] else "NO"))
            lines.append(f"| {name} | {g['hard']} | {form} | {diff} / {total} | {same_verdict} | {dmax:.3g} | {ref:.3g} | {verdict} |")
    lines += ["", "Every form in every regime: identical bits." if identical else
              ("Bits differ; every well-posed regime is within what contraction alone moves." if passed else "NOT PASSED: see the rows above.")]
    return lines, passed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="library A (the parent build)")
    ap.add_argument("--b", help="library B (the build under test)")
    ap.add_argument("--out", default=None, help="directory for the two dumps (default: a temporary one)")
    ap.add_argument("--report", default=None)
    ap.add_argument("--child", default=None, help="(internal) dump this process's library into the named .npz")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    if not a.a or not a.b:
        ap.error("--a and --b are required")
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        out = a.out or tmp
        os.makedirs(out, exist_ok=True)
        dumps = []
        for tag, lib in (("a", a.a), ("b", a.b)):
            path = os.path.join(out, f"pnp_forms_{tag}.npz")
            env = dict(os.environ, BOXDREAMER_HIP_LIB=os.path.abspath(lib))
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", path], env=env).returncode
            if rc != 0:
                print(f"the child for library {tag} ({lib}) ended with status {rc}: nothing further is started on the device", file=sys.stderr)
                sys.exit(2)
            dumps.append(np.load(path))
        lines, passed = compare(*dumps)
    text = "\n".join([f"A = `{a.a}`, B = `{a.b}`", ""] + lines) + "\n"
    print(text)
    if a.report:
        with open(a.report, "w") as f:
            f.write(text)
    sys.exit(0 if passed else 1)


if __name__ == "__main__":
    main()
