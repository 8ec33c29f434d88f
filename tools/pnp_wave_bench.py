"""The wave form of the device PnP (bd_solve_pnp_wave, one wavefront per pose), measured against the thread form (bd_solve_pnp, one
pose per thread) and, through the facade, against the host PnP round trip.

    python tools/pnp_wave_bench.py [--out profiles/pnp_wave.md] [--repeats 7] [--inner 3]

One visit to the GPU: the steps below run one after the other, each as a child process of its own under `timeout -k 10`, and a step
that fails ends the visit (this process itself never opens the device, so one GPU process exists at a time).
  launch     bd_solve_pnp and bd_solve_pnp_wave alone: device events around single launches, median of `--launches` after warm-up,
             n_points = 8 at N = 1, 32, 256 and n_points = 40 at N = 32, and N = 32 on corners that belong to no pose; plus the parity of the wave form against the host form
             (bd_solve_pnp_host, one thread) on tests/test_gpu_pnp_wave.py's inputs: max |dR|, max |dt|, max relative rms_px excess.
  facade32   BoxDreamer(config)(batch), default mode, full depth, B = 32, T = 6: pnp_on_device in {False, True, "wave"}, eager and
             hip_graph.  The False leg runs TWICE (two models), so its own run-to-run spread is on the page.  The legs alternate inside
             every repeat; host clock around `inner` forwards ending in a device synchronise; median over the repeats.
  facade1    the same at B = 1, T = 6, without and with `hip_latency: true`.
The compiler's resource usage of both kernels is read from the build's record (boxdreamer_amd/csrc/_obj/resources.json)."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("launch", 240), ("facade32", 480), ("facade1", 480))      # (step, its time limit in seconds)
SOLVERS = (("host (a)", False), ("thread", True), ("wave", "wave"), ("host (b)", False))


# ------------------------------------------------------------------------------------------------------------------ the steps
def scene(rng, N, npts, fx=600.0, fy=600.0, cx=112.0, cy=112.0, noise=0.7):
    """tests/test_gpu_pnp_wave.py's inputs: the 0.1 / 0.07 / 0.05 box, f = 600, c = 112, z in [0.6, 1.0], rvec ~ normal * 0.9."""
    import numpy as np
    from boxdreamer_amd import pnp
    ext = np.array([0.1, 0.07, 0.05])
    box = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * ext
    extra = rng.normal(size=(N, max(npts - 8, 0), 3)) * ext
    p3 = np.concatenate([np.tile(box, (N, 1, 1)), extra], 1)[:, :npts]
    K = np.tile(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), (N, 1, 1))
    R = pnp._rodrigues_b(rng.normal(size=(N, 3)) * 0.9)
    t = np.stack([rng.normal(size=N) * 0.05, rng.normal(size=N) * 0.05, 0.6 + rng.random(N) * 0.4], 1)
    pc = p3 @ np.swapaxes(R, 1, 2) + t[:, None]
    kp = pc[..., :2] / pc[..., 2:] * [fx, fy] + [cx, cy] + rng.normal(size=(N, npts, 2)) * noise
    return kp.astype(np.float32), p3.astype(np.float32), K.astype(np.float32)


def step_launch(a):
    import numpy as np
    import torch
    from boxdreamer_amd import _lib, pnp
    from boxdreamer_amd.box_utils import solve_poses_device, solve_poses_host
    _lib.require_gpu()
    rng = np.random.default_rng(a.seed)
    rows = []
    for npts, N, posed in ((8, 1, True), (8, 32, True), (8, 256, True), (40, 32, True), (8, 32, False)):
        kp, p3, K = scene(rng, N, npts)
        if not posed:          # corners that belong to no pose (what an untrained decoder's heat maps give the facade legs below)
            kp = (rng.random(kp.shape) * 224).astype(np.float32)
        kp, p3, K = (torch.from_numpy(x).cuda() for x in (kp, p3, K))
        row = {"n_points": npts, "n_poses": N, "corners": "a pose's projections + 0.7 px noise" if posed else "uniform random pixels"}
        for form in ("thread", "wave"):
            fn = lambda: solve_poses_device(kp, p3, K, form=form)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            row[form] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}
            print(f"[launch] n_points {npts} N {N} {form}: median {row[form]['median_us']:.1f} us", flush=True)
        rows.append(row)
    # parity against the host form on the tests' inputs
    have, pnp._HAVE_CV2 = pnp._HAVE_CV2, False
    dR = dt = 0.0
    excess = -1.0
    try:
        for npts in (6, 7, 8, 9, 16, 24, 63, 64):
            kp, p3, K = scene(np.random.default_rng(100 + npts), 5, npts)
            ref = solve_poses_host(kp, p3, K, workers=1)
            got, rms = solve_poses_device(*(torch.from_numpy(x).cuda() for x in (kp, p3, K)), form="wave", want_rms=True)
            got, rms = got.cpu().numpy(), rms.cpu().numpy().astype(np.float64)
            assert (ref[:, 3, 3] == 1).all() and (got[:, 3, 3] == 1).all()
            dR = max(dR, float(np.abs(got[:, :3, :3] - ref[:, :3, :3]).max()))
            dt = max(dt, float(np.abs(got[:, :3, 3] - ref[:, :3, 3]).max()))
            pc = p3.astype(np.float64) @ np.swapaxes(ref[:, :3, :3].astype(np.float64), 1, 2) + ref[:, None, :3, 3]
            uv = pc[..., :2] / pc[..., 2:] * np.stack([K[:, 0, 0], K[:, 1, 1]], 1)[:, None] + K[:, None, :2, 2]
            theirs = np.sqrt(((kp - uv) ** 2).sum(-1).mean(-1))
            excess = max(excess, float((rms / theirs - 1.0).max()))
    finally:
        pnp._HAVE_CV2 = have
    return {"rows": rows, "launches": a.launches, "parity": {"max_dR": dR, "max_dt": dt, "max_rms_excess": excess, "poses": 40},
            "device": torch.cuda.get_device_name(0), "torch": torch.__version__}


def step_facade(a, B, latency_settings):
    import warnings
    import torch
    import bench
    from boxdreamer_amd import _lib, synth
    from boxdreamer_amd.model import BoxDreamer
    _lib.require_gpu()
    dev = torch.device("cuda")
    bsd, dsd = bench.state_dicts("plain")
    one = synth.make_batch(seed=100, B=B, T=6)
    batch = {k: ((v.to(torch.bfloat16) if v.is_floating_point() else v).to(dev) if torch.is_tensor(v) else v) for k, v in one.items()}
    path = os.path.join(ROOT, "tests", "golden", "model_modules_config.json")
    out = []
    for lat in latency_settings:
        for graph in (False, True):
            legs, solver_of, syncs = {}, {}, {}
            for name, solver in SOLVERS:
                mods = copy.deepcopy(json.load(open(path))["modules"])
                mods["decoder"].update(num_decoder_layers=12, hip_precision=a.prec)
                mods["encoder"]["dino"]["cfg"].update(state_dict=dsd, hip_precision=a.prec)
                mods["hip_graph"], mods["pnp_on_device"] = graph, solver
                if lat:
                    mods["hip_latency"] = True
                m = BoxDreamer({"modules": mods})
                m.load_state_dict({"decoder." + k: v for k, v in bsd.items()}, strict=True)
                m = m.to(dev).eval()
                legs[name] = (lambda m=m: m(dict(batch)))
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    for _ in range(max(2, a.warmup)):      # (the first forward calibrates; with hip_graph it also captures)
                        ret = legs[name]()
                solver_of[name], syncs[name] = ret["pose_solver"], list(m.host_syncs_per_forward or [])
                print(f"[facade] B {B} latency {lat} graph {graph} {name}: built", flush=True)
            torch.cuda.synchronize()
            times = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.inner):
                        fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
            res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "pose_solver": solver_of[k], "host_syncs": syncs[k]}
                   for k, v in times.items()}
            out.append({"B": B, "T": 6, "hip_latency": bool(lat), "hip_graph": graph, "legs": res})
            print(f"[facade] B {B} latency {lat} graph {graph}: " + ", ".join(f"{k} {v['median_ms']:.3f} ms" for k, v in res.items()), flush=True)
            del legs
            torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------------------------ the page
def resources():
    try:
        rec = json.load(open(os.path.join(ROOT, "boxdreamer_amd", "csrc", "_obj", "resources.json")))
    except OSError:
        return {}
    return {("wave" if "pnp_wave_kernel" in k else "thread"): v for k, v in rec.items() if "pnp_kernel" in k or "pnp_wave_kernel" in k}


def page(a, res, cmd):
    la, commit = res["launch"], a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lines = ["# Device PnP, one wavefront per pose (`bd_solve_pnp_wave`) against one thread per pose (`bd_solve_pnp`) and the host round trip",
             "",
             f"`{cmd}` on {la['device']}, torch {la['torch']}; parent commit of the measured tree: `{commit}`.  One visit; every step a process "
             "of its own.",
             "",
             "## Launch time",
             "",
             f"Device events around ONE launch (output allocation included), median of {la['launches']} after 3 warm-up launches; noisy corners of "
             "the tests' box, 30 LM iterations allowed.  The last row's corners are uniform random pixels: no pose projects onto them, which is what the "
             "facade legs below solve (their decoder has synthetic weights).",
             "",
             "| n_points | n_poses | corners | `bd_solve_pnp` us (median, min .. max) | `bd_solve_pnp_wave` us (median, min .. max) | thread / wave |",
             "|---|---|---|---|---|---|"]
    for r in la["rows"]:
        t, w = r["thread"], r["wave"]
        lines.append(f"| {r['n_points']} | {r['n_poses']} | {r['corners']} | {t['median_us']:.1f} ({t['min_us']:.1f} .. {t['max_us']:.1f}) | "
                     f"{w['median_us']:.1f} ({w['min_us']:.1f} .. {w['max_us']:.1f}) | {t['median_us'] / w['median_us']:.1f}x |")
    key = next(r for r in la["rows"] if r["n_points"] == 8 and r["n_poses"] == 32 and r["corners"].startswith("a pose"))
    faster = key["wave"]["median_us"] < key["thread"]["median_us"]
    lines += ["", f"Acceptance (N = 32, n_points = 8): the wave launch is faster than the thread launch of the same run: **{faster}**.", ""]
    lines += ["## Facade: ms per forward", "",
              f"`BoxDreamer(config)(batch)`, mode `{a.prec}`, DINOv2 ViT-B/14 + 12 BETR layers, T = 6, bf16 inputs on the device; {a.repeats} repeats x "
              f"{a.inner} forwards per leg, the legs alternating inside each repeat, host clock around forwards that end in a device synchronise.  "
              "`host (a)` and `host (b)` are two models with the same configuration (`pnp_on_device: false`): their difference is the spread "
              "the `wave` leg is judged against.", "",
              "| B | hip_latency | hip_graph | host (a) | host (b) | spread | thread (`true`) | wave (`\"wave\"`) | wave - host | wave not slower than host + spread | host syncs, wave leg |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = {}
    for blk in res.get("facade32", []) + res.get("facade1", []):
        L = blk["legs"]
        ha, hb = L["host (a)"]["median_ms"], L["host (b)"]["median_ms"]
        host, spread, w = (ha + hb) / 2, abs(ha - hb), L["wave"]["median_ms"]
        ok = w <= host + spread
        verdicts[(blk["B"], blk["hip_latency"], blk["hip_graph"])] = ok
        lines.append(f"| {blk['B']} | {blk['hip_latency']} | {blk['hip_graph']} | {ha:.3f} | {hb:.3f} | {spread:.3f} | {L['thread']['median_ms']:.3f} | {w:.3f} | "
                     f"{w - host:+.3f} | **{ok}** | `{L['wave']['host_syncs']}` |")
    lines += ["", "All figures in ms per forward (median).  `wave - host` is against the mean of the two host legs.", ""]
    if verdicts:
        slower = sorted(k for k, ok in verdicts.items() if not ok)
        lines += [("Through the facade the wave form is not slower than the host round trip in any leg: it is the faster option." if not slower else
                   f"Through the facade the wave form is SLOWER than the host round trip, beyond the spread of the two host legs, in {len(slower)} of "
                   f"{len(verdicts)} legs (B, hip_latency, hip_graph): {slower}.  It is opt-in; the host solver remains the faster default.  What "
                   "the wave form buys is a forward with no host synchronisation under `hip_graph`, and it is several times cheaper than the thread "
                   "form for a caller who wants that."), ""]
    rs = resources()
    lines += ["## Resource usage (the compiler's kernel-resource-usage remarks, gfx950)", "",
              "| kernel | scratch bytes / lane | VGPRs | SGPRs | LDS bytes / workgroup | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
    for form, name in (("thread", "`pnp_kernel`"), ("wave", "`pnp_wave_kernel`")):
        r = rs.get(form)
        lines.append(f"| {name} | {r.get('ScratchSize')} | {r.get('VGPRs')} | {r.get('TotalSGPRs')} | {r.get('LDS Size')} | {r.get('Occupancy')} |" if r
                     else f"| {name} | not recorded in this tree (run `python -m boxdreamer_amd.build --force`) | | | | |")
    p = la["parity"]
    lines += ["", "## Parity with the host form (`bd_solve_pnp_host`, one thread)", "",
              f"On the {p['poses']} poses of tests/test_gpu_pnp_wave.py's point-count case (n_points = 6, 7, 8, 9, 16, 24, 63, 64, five noisy poses each): "
              f"max |dR| = {p['max_dR']:.3g}, max |dt| = {p['max_dt']:.3g} (bound: 1e-4); max relative excess of `rms_px` over the host pose's pixel "
              f"RMS = {p['max_rms_excess']:.3g} (bound: 1e-6).", ""]
    return "\n".join(lines) + "\n", faster, verdicts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--prec", default="f16c8_qk16")
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and write its JSON to --json")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.launches < 20 or a.repeats * a.inner < 20:
        ap.error("at least 20 launches and repeats x inner >= 20 forwards")
    if a.step:
        res = {"launch": lambda: step_launch(a), "facade32": lambda: step_facade(a, 32, (False,)),
               "facade1": lambda: step_facade(a, 1, (False, True))}[a.step]()
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    passthrough = ["--prec", a.prec, "--seed", str(a.seed), "--launches", str(a.launches), "--repeats", str(a.repeats), "--inner", str(a.inner),
                   "--warmup", str(a.warmup)]
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:
            js = os.path.join(tmp, step + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--json", js,
                                 *passthrough]).returncode
            if rc != 0:
                sys.exit(f"step {step} ended with status {rc}: nothing further is started on the device")
            res[step] = json.load(open(js))
    text, faster, verdicts = page(a, res, "python tools/pnp_wave_bench.py " + " ".join(passthrough))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if not faster:
        sys.exit("bd_solve_pnp_wave is not faster than bd_solve_pnp at N = 32, n_points = 8: the wave form is mis-built")


if __name__ == "__main__":
    main()
