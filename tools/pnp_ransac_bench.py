"""The device RANSAC PnP of the dense multi-round mode (bd_solve_pnp_ransac_wave: one wavefront per hypothesis, then one per sample),
measured against the host forms and, through the facade, against the host RANSAC round trip.

    python tools/pnp_ransac_bench.py [--out profiles/pnp_ransac.md] [--launches 20] [--repeats 5]

One visit to the GPU: the steps below run one after the other, each as a child process of its own under `timeout -k 10`, and a step
that fails ends the visit (this process itself never opens the device, so one GPU process exists at a time).
  launch   n_samples = 1, 8, 32 at R = 3 (one bad round) and R = 7 (two bad rounds), 1000 trials, tests/test_pnp_ransac_host.py's scene
           recipe (clean round: exact projections + 0.3 px; bad round: uniform pixels in [30, 194]):
             (a) device events around solve_poses_ransac_device (both launches and the output allocations), median of `--launches`;
             (b) the host clock around the per-sample loop the dense mode ran before the device form existed: corners, box and K
                 copied to the host, pnp.solve_pnp_ransac once per sample with seed = sample, the poses copied back;
             (c) the host clock around the native host form (bd_solve_pnp_ransac_host on the worker pool), host arrays in and out.
  facade   BoxDreamer(config)(batch), dense multi-round, B = 8, 21 references, sub_batch_size 3 (R = 7), fine_level off, full depth:
           pnp_on_device False twice (two models: their difference is the spread) and "wave"; the legs alternate inside every repeat;
           host clock around a forward that ends in a device synchronise; median over the repeats.
The compiler's resource usage of the two kernels is read from the build's record (boxdreamer_amd/csrc/_obj/resources.json)."""
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

STEPS = (("launch", 420), ("facade", 540))      # (step, its time limit in seconds)
LEGS = (("host (a)", False), ("wave", "wave"), ("host (b)", False))
SHAPES = ((3, (1,)), (7, (2, 5)))
TRIALS = 1000


def scene(rng, n, rounds, bad):
    import numpy as np
    from boxdreamer_amd import pnp
    box = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * [0.1, 0.07, 0.05]
    R = pnp._rodrigues_b(rng.normal(size=(n, 3)) * 0.9)
    t = np.stack([rng.normal(size=n) * 0.05, rng.normal(size=n) * 0.05, 0.6 + rng.random(n) * 0.4], 1)
    pc = np.tile(box, (n, 1, 1)) @ np.swapaxes(R, 1, 2) + t[:, None]
    exact = pc[..., :2] / pc[..., 2:] * 600.0 + 112.0
    kp = exact[:, None] + rng.normal(size=(n, rounds, 8, 2)) * 0.3
    for r in bad:
        kp[:, r] = rng.uniform(30, 194, (n, 8, 2))
    K = np.tile(np.array([[600.0, 0, 112.0], [0, 600.0, 112.0], [0, 0, 1]]), (n, 1, 1))
    return kp.astype(np.float32), np.tile(box, (n, 1, 1)).astype(np.float32), K.astype(np.float32)


def step_launch(a):
    import numpy as np
    import torch
    from boxdreamer_amd import _lib, pnp
    from boxdreamer_amd.box_utils import _host_workers, solve_poses_ransac_device
    _lib.require_gpu()
    rng = np.random.default_rng(a.seed)
    rows = []

    def host_loop(kp_d, box_d, K_d):          # the dense mode's pose step without the device form (dense.recover_pose_from_dense_bb8)
        B, R = kp_d.shape[:2]
        kp, b3, Kh = kp_d.reshape(B, R * 8, 2).cpu().numpy(), box_d.float().cpu().numpy(), K_d.float().cpu().numpy()
        poses = np.zeros((B, 1, 4, 4), np.float32)
        for b in range(B):
            ok, Rm, t, _ = pnp.solve_pnp_ransac(np.tile(b3[b], (R, 1)), kp[b], Kh[b], reproj_err=2.0, confidence=0.99, max_trials=TRIALS, seed=b)
            if ok:
                poses[b, 0, :3, :3], poses[b, 0, :3, 3], poses[b, 0, 3, 3] = Rm, t, 1.0
        return torch.from_numpy(poses).to(kp_d.device)

    for rounds, bad in SHAPES:
        for n in (1, 8, 32):
            kp, box, K = scene(rng, n, rounds, bad)
            dkp, dbox, dK = (torch.from_numpy(x).cuda() for x in (kp, box, K))
            picks = pnp.ransac_picks(rounds, TRIALS, 0)
            row = {"n_samples": n, "rounds": rounds, "bad_rounds": len(bad)}
            fn = lambda: solve_poses_ransac_device(dkp, dbox, dK, n_trials=TRIALS)
            for _ in range(3):
                out = fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            row["device_us"] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
            info = out[3].cpu().numpy()
            row["trials_used"], row["paths"] = [int(info[:, 0].min()), int(info[:, 0].max())], sorted(set(info[:, 3].tolist()))
            for key, call, reps in (("host_loop_ms", lambda: host_loop(dkp, dbox, dK), a.repeats),
                                    ("native_host_ms", lambda: pnp.solve_pnp_ransac_native(kp, box, K, picks, workers=_host_workers()), a.repeats)):
                call()
                ms = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                row[key] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
            print(f"[launch] R {rounds} n {n}: device {row['device_us']['median']:.1f} us, host loop {row['host_loop_ms']['median']:.2f} ms, "
                  f"native host {row['native_host_ms']['median']:.2f} ms", flush=True)
            rows.append(row)
    return {"rows": rows, "launches": a.launches, "repeats": a.repeats, "workers": _host_workers(), "device": torch.cuda.get_device_name(0),
            "torch": torch.__version__}


def step_facade(a):
    import warnings
    import torch
    import bench
    from boxdreamer_amd import _lib, synth
    from boxdreamer_amd.model import BoxDreamer
    _lib.require_gpu()
    dev = torch.device("cuda")
    bsd, dsd = bench.state_dicts("plain")
    B, T = 8, 22
    one = synth.make_batch(seed=100, B=B, T=T)
    one["query_idx"] = torch.full((B,), T - 1)
    batch = {k: ((v.to(torch.bfloat16) if v.is_floating_point() else v).to(dev) if torch.is_tensor(v) else v) for k, v in one.items()}
    path = os.path.join(ROOT, "tests", "golden", "model_modules_config.json")
    legs, solver_of = {}, {}
    for name, solver in LEGS:
        mods = copy.deepcopy(json.load(open(path))["modules"])
        mods["decoder"].update(num_decoder_layers=12, hip_precision=a.prec)
        mods["encoder"]["dino"]["cfg"].update(state_dict=dsd, hip_precision=a.prec)
        mods["pnp_on_device"] = solver
        mods["dense_cfg"] = {"enable": True, "filter": "dino", "filter_enable": False, "filter_topk": 4, "multi_round": True, "sub_batch_size": 3,
                             "dense_mem_friendly": False, "fine_level": False, "fine_topk": 5}
        m = BoxDreamer({"modules": mods})
        m.load_state_dict({"decoder." + k: v for k, v in bsd.items()}, strict=True)
        m = m.to(dev).eval()
        legs[name] = (lambda m=m: m(dict(batch)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(max(2, a.warmup)):
                ret = legs[name]()
        solver_of[name] = ret["dense_pose_solver"]
        inl = ret["dense_pose_inliers"]
        print(f"[facade] {name}: built, rounds {inl.shape[1]}, inliers per sample {inl.reshape(B, -1).sum(1).tolist()}", flush=True)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "solver": solver_of[k]} for k, v in times.items()}
    print("[facade] " + ", ".join(f"{k} {v['median_ms']:.2f} ms" for k, v in res.items()), flush=True)
    return {"B": B, "T": T, "rounds": int(inl.shape[1]), "legs": res}


def resources():
    try:
        rec = json.load(open(os.path.join(ROOT, "boxdreamer_amd", "csrc", "_obj", "resources.json")))
    except OSError:
        return {}
    return {name: v for k, v in rec.items() for name in ("pnp_ransac_hyp_kernel", "pnp_ransac_final_kernel") if name in k}


def page(a, res, cmd):
    la, fa, commit = res["launch"], res["facade"], a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lines = ["# Device RANSAC PnP of the dense multi-round mode (`bd_solve_pnp_ransac_wave`) against the host forms", "",
             f"`{cmd}` on {la['device']}, torch {la['torch']}; parent commit of the measured tree: `{commit}`.  One visit; every step a process of "
             "its own.", "",
             "## The pose step alone", "",
             f"{TRIALS} trials, 2 px, confidence 0.99; R = 3 with one bad round, R = 7 with two.  (a) device events around "
             f"`solve_poses_ransac_device` (both launches and the output allocations), median of {la['launches']} after 3 warm-up calls.  (b) host "
             "clock around the per-sample loop the dense mode runs without the device form: corners, box and K to the host, "
             f"`pnp.solve_pnp_ransac` per sample, poses back; median of {la['repeats']}.  (c) host clock around `bd_solve_pnp_ransac_host` on "
             f"{la['workers']} worker threads (all {TRIALS} hypotheses, like the device), median of {la['repeats']}.", "",
             "| n_samples | R | bad rounds | (a) device us (median, min .. max) | trials used | paths | (b) host loop ms (median, min .. max) | (c) native host ms | (b) / (a) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in la["rows"]:
        d, h, n = r["device_us"], r["host_loop_ms"], r["native_host_ms"]
        lines.append(f"| {r['n_samples']} | {r['rounds']} | {r['bad_rounds']} | {d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f}) | "
                     f"{r['trials_used'][0]} .. {r['trials_used'][1]} | {r['paths']} | {h['median']:.2f} ({h['min']:.2f} .. {h['max']:.2f}) | "
                     f"{n['median']:.2f} ({n['min']:.2f} .. {n['max']:.2f}) | {h['median'] * 1e3 / d['median']:.0f}x |")
    key = next(r for r in la["rows"] if r["n_samples"] == 8 and r["rounds"] == 7)
    shorter = key["device_us"]["median"] < key["host_loop_ms"]["median"] * 1e3
    lines += ["", f"Acceptance (n_samples = 8, R = 7): (a) is shorter than (b) in the same run: **{shorter}** "
              f"({key['device_us']['median']:.1f} us against {key['host_loop_ms']['median'] * 1e3:.0f} us).",
              "The device always scores all 1000 hypotheses; the host loop stops at the adaptive trial count (`trials used`).", ""]
    L = fa["legs"]
    ha, hb, w = L["host (a)"]["median_ms"], L["host (b)"]["median_ms"], L["wave"]["median_ms"]
    host, spread = (ha + hb) / 2, abs(ha - hb)
    ok = w <= host + spread
    lines += ["## Facade: ms per multi-round forward", "",
              f"`BoxDreamer(config)(batch)`, mode `{a.prec}`, DINOv2 ViT-B/14 + 12 BETR layers, dense multi-round, B = {fa['B']}, {fa['T'] - 1} references, "
              f"sub_batch_size 3 (R = {fa['rounds']}), fine_level off, bf16 inputs on the device; {a.repeats} repeats, the legs alternating inside "
              "each repeat, host clock around a forward that ends in a device synchronise.  `host (a)` and `host (b)` are two models with "
              "`pnp_on_device: false`: their difference is the spread the `wave` leg is judged against.  The decoder has synthetic weights: its "
              "corners belong to no pose, so the host RANSAC finds no consensus and runs all 1000 trials per sample -- its worst case, not the "
              "few ms per sample of posed corners in the table above.", "",
              "| host (a) | host (b) | spread | wave | wave - host | wave not slower than host + spread |", "|---|---|---|---|---|---|",
              f"| {ha:.2f} | {hb:.2f} | {spread:.2f} | {w:.2f} | {w - host:+.2f} | **{ok}** |", "",
              "All figures in ms per forward (median); `wave - host` is against the mean of the two host legs.", "",
              f"Solvers as the batch dict names them: host legs `{L['host (a)']['solver']}`; wave leg `{L['wave']['solver']}`.", ""]
    rs = resources()
    lines += ["## Resource usage (the compiler's kernel-resource-usage remarks, gfx950)", "",
              "| kernel | scratch bytes / lane | VGPRs | SGPRs | LDS bytes / workgroup | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
    for name in ("pnp_ransac_hyp_kernel", "pnp_ransac_final_kernel"):
        r = rs.get(name)
        lines.append(f"| `{name}` | {r.get('ScratchSize')} | {r.get('VGPRs')} | {r.get('TotalSGPRs')} | {r.get('LDS Size')} | {r.get('Occupancy')} |" if r
                     else f"| `{name}` | not recorded in this tree (run `python -m boxdreamer_amd.build --force`) | | | | |")
    return "\n".join(lines) + "\n", shorter, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--prec", default="f16c8_qk16")
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and write its JSON to --json")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.launches < 20 or a.repeats < 5:
        ap.error("at least 20 launches and 5 repeats")
    if a.step:
        res = {"launch": lambda: step_launch(a), "facade": lambda: step_facade(a)}[a.step]()
        with open(a.json, "w") as f:
            json.dump(res, f)
        return
    passthrough = ["--prec", a.prec, "--seed", str(a.seed), "--launches", str(a.launches), "--repeats", str(a.repeats), "--warmup", str(a.warmup)]
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:
            js = os.path.join(tmp, step + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--json", js,
                                 *passthrough]).returncode
            if rc != 0:
                sys.exit(f"step {step} ended with status {rc}: nothing further is started on the device")
            res[step] = json.load(open(js))
    text, shorter, ok = page(a, res, "python tools/pnp_ransac_bench.py " + " ".join(passthrough))
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if not shorter:
        sys.exit("the device RANSAC is not shorter than the host loop at n_samples = 8, R = 7")


if __name__ == "__main__":
    main()
