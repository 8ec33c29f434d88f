#!/usr/bin/env python
"""bench.py -- poses/s of the corner-heatmap inference path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--prec bf16|fp16|bf16x3|fp8] [--batch B] [--views T]
                    [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of synthetic input already resident in HBM:
DINOv2 ViT-B/14-reg encoder on all B*T crops -> BETR decoder -> corner decode (top-20 mean), plus for
N > 1 the RCCL all-gather of predicted corners.  Default workload = BASELINE.json configs[1]:
1 query + 5 refs, 224x224, batch 32 per GPU.  One process per GPU, batch sharded across ranks
(independent samples -> weak scaling, no data-path collective besides the corner gather).

Launch: `python bench.py --gpus N` with no torch.distributed environment re-executes itself under
`python -m torch.distributed.run --nproc-per-node N` (one rank per GPU, backend "nccl" = RCCL); started
by torch.distributed.run directly (the driver's form) it reads RANK / LOCAL_RANK / WORLD_SIZE and
asserts WORLD_SIZE == --gpus.  `--backend gloo --cpu-plumbing` runs ONLY the launcher / barrier /
gather plumbing on CPU (tests/test_bench_launcher.py) -- the data path itself has no CPU form.

Rank 0 prints ONE JSON line.  `value` is the headline mode (--prec, default: the package default f16c8_qk16, the mode
that meets north_star's 1e-3 heatmap-logit tolerance).  A plain run sets up, warms up, times the K steps and reports
them, nothing else.  `--full` adds everything else the line has carried: the other mode of record, rooflines, parity
against the CPU oracle, the one-lane record, side measurements, other batch sizes / view counts / precisions, the CPU
baseline and the in-run counters.  `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import threading
import time

# Rank 0 of a multi-rank launch must be able to report a failure even while its main thread is blocked inside a C++ call (process-group
# rendezvous, an NCCL collective, a device synchronise) -- Python runs signal handlers only between bytecodes.  So SIGTERM (what
# torch.distributed.run sends the survivors when a rank dies) is BLOCKED here, before `import torch` creates any thread (threads inherit
# the mask), and a dedicated thread picks it up with sigwait() and prints the failure line (see _sigterm_watcher below).
_WATCH_SIGTERM = int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("RANK", "0") == "0" and hasattr(signal, "pthread_sigmask")
if _WATCH_SIGTERM:
    signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM})

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# peaks from /opt/skills/guides/MI355X_MICROARCH.md (dense, no sparsity)
PEAK_MFMA_16BIT, PEAK_MFMA_FP8 = 2500.0, 5000.0      # TFLOP/s; every mode but "fp8" is priced against the 16-bit peak
PEAK_HBM_GBS = 8000.0
DINO_FLOP_PER_IMAGE = 47_078_313_984          # BASELINE.md §4 / SURVEY.md §8(d)
TRAINED_LIKE = "outliers_g0.5"                  # the trained-like weight set of the strict_trained_like leg (tests/golden/case_outliers_g0.5_T2.npz)
STRICT_PREC = "f16c8_qk16"                      # the package default: meets the 1e-3 bar with a 4x margin
DTYPE_LABEL = {"bf16": "bf16", "fp16": "f16", "bf16x3": "bf16x3", "bf16x3_attn_x3": "bf16x3", "f16c8": "f16 + e4m3 corrections",
               "f16c8_qk16": "f16 + e4m3 corrections (BETR q, k columns: f16)", "fp8": "fp8-e4m3 (Linears) + bf16 (attention)",
               "fp8_mixed": "fp8-e4m3 (MLPs, DINOv2 QKV) + bf16 (proj, BETR QKV, adapter, head, attention)",
               "f16x3": "f16x3 (split-f16 Linears)", "f16x3_attn_x3": "f16x3 (split-f16 Linears, split-bf16 attention)"}
MFMA_PASSES = {"f16x3": 3.0, "f16x3_attn_x3": 3.0, "bf16x3": 3.0, "bf16x3_attn_x3": 3.0, "f16c8": 2.0, "f16c8_qk16": 1.93}
_PRECS = tuple(DTYPE_LABEL)


def betr_flops(T: int) -> int:
    S = 256 * T
    return S * (4 * 768 ** 2 + 2 * 1568 * 768) + 12 * (S * 14_155_776 + 3072 * S * S) + 2 * 256 * 768 * 1568


def flops_per_pose(T: int) -> int:
    return T * DINO_FLOP_PER_IMAGE + betr_flops(T)


def state_dicts(weights: str = "plain"):
    """(betr_sd, dino_sd) of the bench: "plain" = seeded random init; "outliers_g<gain>" = the trained-like grafts (synth.py)."""
    from boxdreamer_amd import synth
    if weights.startswith("outliers_g"):
        g = float(weights[len("outliers_g"):])
        return synth.betr_state_dict_outliers(1234, 12, g), synth.dino_state_dict_outliers(4321, 12, g)
    return synth.betr_state_dict(seed=1234, depth=12), synth.dino_state_dict(seed=4321, depth=12)


def build_models(prec, device, weights: str = "plain"):
    from boxdreamer_amd.betr import BETR
    from boxdreamer_amd.encoder import DinoV2Wrapper
    bsd, dsd = state_dicts(weights)
    enc = DinoV2Wrapper(None, {"model_type": "dinov2_vitb14_reg", "state_dict": dsd, "hip_precision": prec})
    enc.to_device(device)
    dec = BETR(d_model=768, nhead=8, num_decoder_layers=12, decoder_only=True, patch_size=14, img_size=224,
               diff_emb=False, nvs_supervision=False, ray_supervision=True, use_mask=False, use_pretrained=True,
               patchify_rays=True, pose_representation="bb8", bbox_representation="heatmap", hip_precision=prec)
    dec.load_state_dict(bsd, strict=True)
    dec.validate_inputs = False         # the one-hot mask check is a device sync per forward: not inside a timed step
    return enc, dec.to(device).eval()


def usable_cpus() -> int:
    """CPUs this process may actually use: min(affinity, cgroup cpu.max quota).  (The GPU box shows 256 logical
    CPUs but a 16-CPU cgroup quota; 256 torch threads there run 100x slower than 16.)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(T: int, budget_s: float = 24.0) -> dict:
    """SURVEY §8d protocol: the oracle (CPU restatement of the reference arithmetic) on this box's host cores, same seeded
    inputs/weights as the GPU parity probe, 2 warm-up + median of >= 5 timed single-pose forwards, fp32 (primary, `value`)
    and CPU bf16-autocast (secondary: the reference's own `precision: bf16` on a CPU).  Bounded to ~budget_s."""
    from boxdreamer_amd import synth
    from oracle import boxdreamer_oracle as orc
    cores = usable_cpus()
    torch.set_num_threads(cores)
    bsd, dsd = synth.betr_state_dict(1234, 12), synth.dino_state_dict(4321, 12)
    data = synth.make_batch(seed=11, B=1, T=T)

    def leg(autocast: bool, budget: float):
        ts = []
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            t_begin = time.perf_counter()
            for i in range(2 + 64):
                t0 = time.perf_counter()
                orc.boxdreamer_forward(data, bsd, dsd)
                if i >= 2:
                    ts.append(time.perf_counter() - t0)
                if len(ts) >= 5 and time.perf_counter() - t_begin > budget:
                    break
                if len(ts) >= 9:
                    break
        return statistics.median(ts), len(ts)

    m32, n32 = leg(False, budget_s * 0.6)
    m16, n16 = leg(True, budget_s * 0.4)
    return {"value": round(1.0 / m32, 3), "unit": "poses/s", "cores": torch.get_num_threads(), "kind": "port",
            "bf16_autocast_value": round(1.0 / m16, 3),
            "sample": f"single-pose forwards (B=1, T={T}, 224x224, full depth) of oracle/boxdreamer_oracle.py: 2 warm-up + "
                      f"median of {n32} (fp32) / {n16} (CPU bf16 autocast) timed runs, torch {torch.__version__} CPU, "
                      f"{torch.get_num_threads()} threads"}


def parity_probe(prec, T: int, device, models=None, weights: str = "plain", B: int = 2) -> dict:
    """Max-abs error of the heatmap logits vs the CPU oracle on full-depth poses (outside the timed region): B = 2 samples
    with different inputs, the same weights as the timed step."""
    from boxdreamer_amd import hip_ops, synth
    from oracle import boxdreamer_oracle as orc
    enc, dec = models if models is not None else build_models(prec, device, weights)
    data = synth.make_batch(seed=11, B=B, T=T)
    mask = torch.zeros(B, T, dtype=torch.bool); mask[:, T - 1] = True
    img, bf = data["images"].to(device), data["bbox_feat"].to(device)
    heat = dec(bf, img, mask.to(device), enc.predict(img), None)
    kp, _, idx = hip_ops.decode_topk(heat)
    with torch.no_grad():
        o = orc.boxdreamer_forward(data, *state_dicts(weights))
    same = (idx.cpu().long().sort(-1)[0] == o["topk_idx"].sort(-1)[0]).all(-1).float().mean().item()
    return {"mode": prec, "logits_max_abs_err": float((dec.last_logits.cpu() - o["logits"]).abs().max()),
            "heat_max_abs_err": float((heat.cpu() - o["heat"]).abs().max()),
            "top20_sets_equal_frac": same,
            "corner_px_max_err": float((kp.cpu() - o["corners_px"]).abs().max()),
            "tolerance": 1e-3, "meets_tolerance": bool((dec.last_logits.cpu() - o["logits"]).abs().max() <= 1e-3),
            "case": f"B={B},T={T} full depth vs CPU oracle (fp32), " + ("random-init weights" if weights == "plain" else
                    f"trained-like outlier weights ({weights}: logits max {float(o['logits'].abs().max()):.1f})")}


# ------------------------------------------------------------------------------------------------ launcher

def dist_env():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def free_port() -> int:
    """A TCP port nobody listens on right now (two launches on one node -- the driver's N = 1, 2, 4, 8 sweep back to back, or a
    test suite running in parallel -- must not collide on a pid-derived number)."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return int(sk.getsockname()[1])


def launch_plan(args, argv) -> dict:
    """The exact command and environment `python bench.py --gpus N` turns into (also what `--dry-run` prints)."""
    port = os.environ.get("MASTER_PORT") or str(free_port())
    rest = [a for a in argv if a != "--dry-run"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__), *rest]
    env = {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),   # dmabuf IPC only on this host driver (RCCL needs it)
           "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": port}
    return {"cmd": cmd if args.gpus > 1 else [sys.executable, os.path.abspath(__file__), *rest], "env": env,
            "ranks": args.gpus, "backend": args.backend,
            "note": "one rank per GPU (LOCAL_RANK -> cuda:LOCAL_RANK), batch sharded across ranks, weights replicated, one "
                    "all_gather_into_tensor of the corners per step"}


def maybe_respawn(args) -> None:
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: become the launcher."""
    if args.dry_run:
        print(json.dumps(launch_plan(args, sys.argv[1:])), flush=True)
        raise SystemExit(0)
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    plan = launch_plan(args, sys.argv[1:])
    os.environ.update(plan["env"])
    os.execvp(plan["cmd"][0], plan["cmd"])


def init_dist(args):
    """Returns (world, rank, local_rank, dist-or-None).  World size must equal --gpus."""
    world, rank, local_rank = dist_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}; launch with "
                         f"`python bench.py --gpus {world}` (it spawns the ranks itself) or matching torchrun arguments")
    dist = None
    PROGRESS["line"].update(n_gpus=world)
    if world > 1 or getattr(args, "force_dist", False):
        # (--force-dist: the SAME process-group / collective path at world size 1 -- the one-GPU box's only way to execute RCCL)
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1"); os.environ.setdefault("LOCAL_RANK", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # a finite collective timeout: a rank that died must surface as an error on the others, not as a hang
        to = datetime.timedelta(seconds=args.dist_timeout)
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank), timeout=to)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world, timeout=to)
        if rank == 0 and not _WATCH_SIGTERM:
            signal.signal(signal.SIGTERM, _on_sigterm)      # torch.distributed.run terminates the survivors when a rank fails
    return world, rank, local_rank, dist


def rccl_probe(args) -> None:
    """Child of `rccl_world1_block` (under torch.distributed.run, one rank): the N > 1 sweep's process-group path executed on RCCL at
    world size 1 -- init_process_group("nccl", device_id=...), the polled barrier, the corner all-gather on a device tensor, the
    float64 timing gather -- and ONE JSON line with what the collective layer saw.  Replaces the reference's pickle + gloo gather
    (/root/reference/src/utils/comm.py:84-92, 179-219)."""
    from boxdreamer_amd.dist import gather_corners, gather_corners_ragged
    args.force_dist, args.backend = True, "nccl"
    _, _, local_rank = dist_env()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    t0 = time.perf_counter()
    world, rank, _, dist = init_dist(args)
    kp = torch.arange(32 * 16, dtype=torch.float32, device=device).reshape(32, 8, 2)
    out = gather_corners(kp, world)                 # the first collective creates the communicator
    torch.cuda.synchronize()
    init_s = time.perf_counter() - t0
    ok = bool(torch.equal(out, kp))
    ragged_ok = bool(torch.equal(gather_corners_ragged(kp[:29].clone(), 29), kp[:29]))
    lat = gather_latency_ms(kp, world, dist, gather_corners, reps=200)
    dt, per_rank, _ = timed_steps(lambda: gather_corners(kp, world), 20, 3, world, dist, interruptible_sync(device), device)
    if rank == 0:
        print(json.dumps({"rccl_probe": True, "backend": dist.get_backend(), "world_size_seen_by_the_collective": dist.get_world_size(),
                          "nccl_version": ".".join(str(v) for v in torch.cuda.nccl.version()),
                          "device": torch.cuda.get_device_name(device), "gather_ok": ok, "ragged_gather_ok": ragged_ok,
                          "corner_allgather_ms": round(lat, 4), "init_plus_first_collective_s": round(init_s, 3),
                          "timed_steps_ms_per_step": round(dt / 20 * 1e3, 4), "per_rank": len(per_rank),
                          "hsa_enable_ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def rccl_world1_block(timeout_s: float = 240.0) -> dict:
    """Run `rccl_probe` under the launcher the N > 1 sweep uses (torch.distributed.run, --nproc-per-node 1) and return its line."""
    port = str(free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__), "--rccl-probe"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"executed": False, "error": f"timed out after {timeout_s:.0f} s"}
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and "rccl_probe" in l]
    if r.returncode != 0 or not lines:
        return {"executed": False, "rc": r.returncode, "error": (r.stderr or r.stdout)[-600:]}
    j = json.loads(lines[-1])
    j.update(executed=True, wall_s=round(time.perf_counter() - t0, 1),
             what="the sweep's process-group path on RCCL at world size 1 (one GPU per box here): same launcher, backend, device_id, "
                  "barrier and all_gather_into_tensor calls as --gpus N; not a scaling figure")
    return j


# ------------------------------------------------------------------------------------------------ failure reporting
# What rank 0 knows so far (filled stage by stage).  If any rank fails -- its own exception, a collective timeout, or the
# launcher's SIGTERM after ANOTHER rank died -- rank 0 still prints ONE JSON line carrying n_gpus and whatever of
# per_rank_ms_per_step / corner_allgather_ms was measured, plus `error`, and exits non-zero.
PROGRESS = {"line": {"n_gpus": int(os.environ.get("WORLD_SIZE", "1"))}, "stage": "start", "printed": False}


def emit_failure(reason: str) -> None:
    if PROGRESS["printed"]:
        return
    PROGRESS["printed"] = True
    line = dict(PROGRESS["line"])
    line.setdefault("value", None)
    line.update(error=reason, failed_stage=PROGRESS["stage"])
    print(json.dumps(line), flush=True)


def _on_sigterm(signum, frame):
    emit_failure("terminated by the launcher: another rank failed (see its traceback above)")
    os._exit(1)


def _sigterm_watcher():
    signal.sigwait({signal.SIGTERM})
    emit_failure("terminated by the launcher: another rank failed (see its traceback above)")
    sys.stdout.flush()
    os._exit(1)


if _WATCH_SIGTERM:
    threading.Thread(target=_sigterm_watcher, daemon=True, name="bench-sigterm-watcher").start()


def interruptible_sync(device):
    """torch.cuda.synchronize() that keeps returning to the interpreter: Python runs signal handlers only between bytecodes, and
    rank 0 must be able to print its failure line when the launcher SIGTERMs it while a peer's death has its stream stuck in a
    collective.  Multi-rank runs only (adds <= 0.2 ms to a timed region of hundreds of ms)."""
    def sync():
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        while not ev.query():
            time.sleep(0.0002)
        torch.cuda.synchronize(device)            # (other streams: returns at once on the healthy path)
    return sync


def barrier(dist, device=None):
    """dist.barrier() whose wait polls from Python (see interruptible_sync)."""
    t = torch.zeros(1, dtype=torch.int32, device=device if device is not None else "cpu")
    work = dist.all_reduce(t, async_op=True)
    if device is None or torch.device(device).type != "cuda":
        work.wait()
        return
    while not work.is_completed():
        time.sleep(0.0002)
    work.wait()
    interruptible_sync(device)()


def timed_steps(step, steps: int, warmup: int, world: int, dist, sync, device=None):
    """W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize pairs; returns (max-over-ranks seconds,
    per-rank seconds list on rank 0, last output)."""
    out = None
    for _ in range(warmup):
        out = step()
    if dist is not None:
        barrier(dist, device)
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    if dist is not None:
        barrier(dist, device)
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if dist is not None:
        on_host = device is None or dist.get_backend() == "gloo"      # (gloo gathers host tensors only: CPU plumbing / --single-device-test)
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if on_host else device)
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        per_rank = [float(g.item()) for g in gathered]
        dt = max(per_rank)
    return dt, per_rank, out


def cpu_plumbing(args) -> None:
    """Launcher / barrier / corner-gather plumbing on CPU (gloo).  NOT the data path: the corners are a fixed pattern.  Walks the
    same stages as the GPU sweep: per-rank seeded shard, the lane-count agreement (all_reduce MIN), timed steps with the corner
    all-gather, the gather-latency probe, optionally a ragged global batch -- and `--plumbing-fail-rank` kills one rank at a chosen
    stage to exercise the failure report."""
    from boxdreamer_amd import synth
    from boxdreamer_amd.dist import gather_corners, gather_corners_ragged, shard_range
    world, rank, _, dist = init_dist(args)
    B = args.batch

    def maybe_fail(stage):
        PROGRESS["stage"] = stage
        if args.plumbing_fail_rank == rank and args.plumbing_fail_stage == stage:
            raise RuntimeError(f"injected failure on rank {rank} at stage {stage}")

    # per-rank seeds: every rank's shard must differ (seed = 100 + rank, as in the GPU sweep)
    mine = synth.make_batch(seed=100 + rank, B=1, T=1, size=56)["images"]      # (16-px zero border: 24 x 24 random pixels)
    chk = torch.tensor([float(mine.double().sum())], dtype=torch.float64)
    lanes = torch.tensor([1 if rank == args.plumbing_short_rank else 2], dtype=torch.int32)
    if world > 1:
        allc = [torch.zeros_like(chk) for _ in range(world)]
        dist.all_gather(allc, chk)
        distinct = len({round(float(c), 6) for c in allc}) == world
        dist.all_reduce(lanes, op=dist.ReduceOp.MIN)          # every rank must time the same number of in-flight lanes
    else:
        distinct = True
    maybe_fail("before_timed")
    kp = (torch.arange(B * 16, dtype=torch.float32).reshape(B, 8, 2) + 1000.0 * rank)

    def step():
        return gather_corners(kp, world) if world > 1 else kp
    dt, per_rank, out = timed_steps(step, args.steps, args.warmup, world, dist, lambda: None)
    ok = all(torch.equal(out[r * B:(r + 1) * B], torch.arange(B * 16, dtype=torch.float32).reshape(B, 8, 2) + 1000.0 * r)
             for r in range(world))
    PROGRESS["line"].update(per_rank_ms_per_step=[round(t / args.steps * 1e3, 4) for t in per_rank])
    maybe_fail("after_timed")
    lat = None
    if world > 1:
        lat = gather_latency_ms(kp, world, dist, gather_corners, reps=10, sync=lambda: None)
        PROGRESS["line"].update(corner_allgather_ms=round(lat, 4))
    ragged_ok = None
    if args.plumbing_global_batch and world > 1:           # a global batch that does not divide by the world size
        G = args.plumbing_global_batch
        full = torch.arange(G * 16, dtype=torch.float32).reshape(G, 8, 2)
        lo, hi = shard_range(G, rank, world)
        ragged_ok = bool(torch.equal(gather_corners_ragged(full[lo:hi].clone(), G), full))
    maybe_fail("before_report")
    if rank == 0:
        PROGRESS["printed"] = True
        print(json.dumps({"plumbing_only": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "backend": args.backend, "gathered_rows": int(out.shape[0]), "gather_ok": bool(ok),
                          "per_rank_seeds_distinct": bool(distinct), "lanes_agreed": int(lanes.item()), "ragged_ok": ragged_ok,
                          "corner_allgather_ms": None if lat is None else round(lat, 4),
                          "per_rank_ms_per_step": [round(t / args.steps * 1e3, 4) for t in per_rank]}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ PMC counters
# HBM traffic and MFMA-busy come from hardware counters, which only rocprofv3 can read: `python bench.py --measure-counters
# --prec P` runs the three PMC passes over THIS script (one counter group per pass, --kernel-trace only -- the combination the
# MI355X guide prescribes) and writes profiles/counters_<P>.json stamped with a hash of the kernel sources; a default run reports
# those figures as roofline.traffic / mfma_busy ONLY while the stamp matches the sources it is running (else null + why).

def kernel_source_sha() -> str:
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "boxdreamer_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def algorithmic_gemm_bytes(prec: str, B: int, T: int) -> tuple[int, int]:
    """(bytes, bd_gemm calls) of one step if every GEMM read each operand ONCE and wrote its result once: A, W, fp32 residual in /
    result out, in the storage formats of the mode."""
    a = {"bf16": 2, "fp16": 2, "fp8": 1, "f16c8": 3, "f16c8_qk16": 3}.get(prec, 4)           # activation operand bytes / element
    w = {"bf16": 2, "fp16": 2, "fp8": 1, "f16c8": 4, "f16c8_qk16": 4}.get(prec, 4)           # weight bytes / element (F16C8: f16 + [q8|lo8])
    strict = prec not in ("bf16", "fp16", "fp8")
    total, calls = 0, 0

    def gemm(M, N, K, a_b, w_b, out_b, resid=False):
        nonlocal total, calls
        total += M * K * a_b + N * K * w_b + M * N * out_b + (M * N * (resid if resid > 1 else 4) if resid else 0)
        calls += 1

    # Round 6, F16C8 family: LayerNorms folded, the residual stream in the 3-byte operand form between them (csrc/forward.hip: plan_resid).
    # A residual Linear then reads 3 bytes / element of residual and writes the 3-byte copy (+ 8 bytes of row statistics per 96 columns);
    # fp32 rows are read only by block 0's proj (nothing was folded in front of it) and written where someone reads fp32 next.
    from boxdreamer_amd import pack as _pack
    fold = prec in ("f16c8", "f16c8_qk16") and _pack.ln_fold_enabled()
    r3 = fold and os.environ.get("BOXDREAMER_HIP_RESID3", "1") != "0"

    def resid_gemm(M, K, first, f32_out, emits=True):
        # (first: the residual comes in as fp32; f32_out: fp32 rows go out next to / instead of the copy)
        rin = 4 if (first or not r3) else 3
        rout = (3 if emits else 0) + (4 if (f32_out or first or not r3) else 0)
        gemm(M, 768, K, a, w, rout, rin)

    def block(M, Mtail, qkv_a, qkv_w, qkv_o, i=0, last=False):
        gemm(M, 2304, 768, qkv_a, qkv_w, qkv_o)
        if fold:
            resid_gemm(Mtail, 768, i == 0, last)                # proj (the last block's fc2 reads fp32: its proj writes it)
            gemm(Mtail, 3072, 768, a, w, a)
            resid_gemm(Mtail, 3072, False, last, emits=not last) if not last else gemm(Mtail, 768, 3072, a, w, 4, True)
            return
        gemm(Mtail, 768, 768, a, w, 4, True)
        gemm(Mtail, 3072, 768, a, w, a)
        gemm(Mtail, 768, 3072, a, w, 4, True)

    n = B * T
    c8 = prec in ("f16c8", "f16c8_qk16")          # (the F16C8 family pads the embeddings' K to 192s: pack.embed_k_multiple)
    gemm(n * 256, 768, 768 if c8 else 640, a, w, 4)                                             # patch embed (+ positional table)
    for i in range(12):                                       # DINOv2: q, k not normalised -> split-bf16 attention in the strict modes
        block(n * 261, n * 261, a, w, 4 if strict else (2 if prec != "fp8" else 2), i, i == 11)
    M, Mq = n * 256, B * 256
    gemm(M, 768, 768, a, w, a); gemm(M, 768, 768, a, w, 4)                                     # adapter
    gemm(M, 768, 1728 if c8 else (1600 if prec != "fp8" else 1664), a, w, 4, True)                                # heatmap patch embedding + rgb + pos
    for i in range(12):                                       # BETR: f16 attention in the strict modes (q, k RMS-normalised)
        Mt = M if i < 11 else Mq
        if prec == "f16c8_qk16":                              # QKV split by column: q, k one f16 pass on the f16 plane, v full F16C8
            gemm(M, 1536, 768, 2, 2, 2)
            gemm(M, 768, 768, a, w, 2)
            if fold and i < 11:
                resid_gemm(Mt, 768, i == 0, False)
                gemm(Mt, 3072, 768, a, w, a)
                resid_gemm(Mt, 3072, False, i == 10)          # (block 10 writes fp32 rows too: the last block gathers its query rows from them)
            elif fold:                                        # the last block's compact rows: gathered fp32 stream in, fp32 out
                gemm(Mt, 768, 768, a, w, 7, True)
                gemm(Mt, 3072, 768, a, w, a)
                gemm(Mt, 768, 3072, a, w, 4, True)
            else:
                gemm(Mt, 768, 768, a, w, 4, True)
                gemm(Mt, 3072, 768, a, w, a)
                gemm(Mt, 768, 3072, a, w, 4, True)
        else:
            block(M, Mt, a, w, 2, i, i == 11)
    gemm(Mq, 1568, 768, a, w, 4)                                                               # head
    return total, calls


def _rocprof_pass(counters, child_args, timeout_s=600):
    import glob, subprocess, tempfile
    out = tempfile.mkdtemp(prefix="bd_pmc_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--pmc", *counters, "--output-format", "csv", "-d", out, "--",
           sys.executable, os.path.abspath(__file__), *child_args]
    env = dict(os.environ, TMPDIR="/tmp")
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
    files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
    if r.returncode != 0 or not files:
        raise RuntimeError(f"rocprofv3 pass {counters} failed (rc {r.returncode}): {r.stderr[-800:]}")
    return files[0]


# LDS pass (SQ block, 8 slots): instruction count, cycles the LDS pipe is busy / stalls issue, conflict cycles, all LDS-array cycles,
# next to the wave / busy cycle bases they are read against (MI355X_MICROARCH.md: PMC slots, LDS section)
LDS_COUNTERS = ("SQ_INSTS_LDS", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_ADDR_CONFLICT",
                "SQ_LDS_IDX_ACTIVE", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU_MFMA_MOPS_F16")


# stall pass: where the waves' cycles go (MI355X_MICROARCH.md: WAIT_ANY = parked at s_waitcnt / barrier, WAIT_INST_ANY = issue stall,
# ACTIVE_INST_ANY = issuing; the three are disjoint and add up to ~WAVE_CYCLES)
STALL_COUNTERS = ("SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_MISC",
                  "SQ_INSTS_MFMA", "SQ_VALU_MFMA_COEXEC_CYCLES")


# request-size pass (TCC block): the L2 -> fabric read requests by size.  FETCH_SIZE's expression tallies every request that is not a
# 32-byte one at 64 bytes (rocprofv3 -L: "(TCC_BUBBLE*128 + (RDREQ - BUBBLE - RDREQ_32B)*64 + RDREQ_32B*32) / 1024", BUBBLE = 0 on this
# part), which is what the guide's "x 2" correction repairs for streams of 128-byte requests; summing the sizes themselves needs no correction
# and is kept NEXT to the corrected figure as a check of it on this access pattern (MI355X_MICROARCH.md: "calibrate ... in your own
# access pattern").  `traffic` stays the guide's figure.
REQSIZE_COUNTERS = ("TCC_EA0_RDREQ_32B_sum", "TCC_EA0_RDREQ_64B_sum", "TCC_EA0_RDREQ_128B_sum", "TCC_EA0_RDREQ_sum")


def _available_counters(names):
    """The subset of `names` this rocprofv3 / device lists (`rocprofv3 -L`); [] when the listing itself fails."""
    import subprocess
    try:
        r = subprocess.run(["rocprofv3", "-L"], capture_output=True, text=True, timeout=120, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"))
    except Exception:                                            # noqa: BLE001
        return []
    text = r.stdout + r.stderr
    import re as _re
    return [n for n in names if _re.search(r"\b" + n + r"\b", text)]


def _kclass(name: str) -> str:
    for key, c in (("gemm_kernel", "gemm"), ("attn_kernel", "attention"), ("layernorm", "layernorm"), ("rmsnorm", "rmsnorm")):
        if key in name:
            return c
    # torch / runtime kernels in the profiled process are one-off harness work (weight packing at load time, input upload, the
    # bench's own bookkeeping), not launches of the step: kept out of the per-step figures
    if "at::native" in name or "rocclr" in name:
        return "harness (one-off torch / runtime kernels: weight packing, uploads)"
    return "other"


MARKER = "erfinv"        # a torch kernel nothing else in this process launches: brackets the measured steps of each mode in the counter child


def counter_child(args) -> None:
    """(hidden: what the rocprofv3 passes profile.)  One process, one or more modes: per mode the step's modules are built exactly as
    the timed run builds them (load-time calibration included), then 1 warm-up + `--steps` un-graphed ONE-LANE steps run between two
    marker kernels, so that the parent attributes exactly the measured steps' dispatches to the mode -- no weight packing, no
    calibration forwards, no warm-up in the figures."""
    from boxdreamer_amd import synth
    torch.set_num_threads(usable_cpus())
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tiny = torch.full((64,), 0.25, device=device)
    B, T = args.batch, args.views
    one = synth.make_batch(seed=100, B=B, T=T)
    images, bbox = one["images"].to(torch.bfloat16).to(device), one["bbox_feat"].to(torch.bfloat16).to(device)
    mask = torch.zeros(B, T, dtype=torch.bool, device=device); mask[:, T - 1] = True
    a1 = argparse.Namespace(**{**vars(args), "graph": False, "in_flight": 1, "lanes": "1", "cache_refs": False})
    for mode in args.counter_child.split(","):
        run = ModeRun(mode, a1, device, 1, 0, None, images, bbox, mask)
        run.eager()
        torch.cuda.synchronize()
        tiny.erfinv()
        for _ in range(args.steps):
            run.eager()
        torch.cuda.synchronize()
        tiny.erfinv()
        torch.cuda.synchronize()
        run.close()
        del run
        torch.cuda.empty_cache()
    print(json.dumps({"counter_child": args.counter_child, "steps": args.steps}), flush=True)


BASIC_GROUPS = (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES"))


def collect_counters(modes, B: int, T: int, groups, steps: int = 2, deadline: float | None = None, log=None) -> dict:
    """rocprofv3 PMC passes (one counter group per pass, --kernel-trace only: the combination MI355X_MICROARCH.md prescribes) over
    `bench.py --counter-child <modes>`; returns {mode: figures per step and per kernel class}.  Stops launching passes once
    `deadline` (time.monotonic()) has gone by and raises TimeoutError -- a partial set of passes is not reported."""
    import collections, csv
    child = ["--counter-child", ",".join(modes), "--batch", str(B), "--views", str(T), "--steps", str(steps)]
    names = sorted({c for g in groups for c in g})
    acc = {m: {c: collections.defaultdict(float) for c in names + ["stall:SQ_WAVE_CYCLES"]} for m in modes}
    launches = {m: collections.defaultdict(int) for m in modes}
    dur_ns = {m: collections.defaultdict(float) for m in modes}
    pass_seconds = []
    for group in groups:
        if deadline is not None and time.monotonic() > deadline:
            raise TimeoutError(f"counter budget spent after {len(pass_seconds)} of {len(groups)} passes ({pass_seconds} s)")
        t0 = time.monotonic()
        left = None if deadline is None else max(20.0, deadline - t0 + 30.0)
        path = _rocprof_pass(group, child, timeout_s=600 if left is None else left)
        pass_seconds.append(round(time.monotonic() - t0, 1))
        if log:
            log(f"counter pass {group}: {pass_seconds[-1]} s")
        rows = list(csv.DictReader(open(path)))
        # dispatch order; the marker kernel brackets the measured steps of mode k between its (2k+1)-th and (2k+2)-th launch
        disp = {}
        for r in rows:
            disp.setdefault(int(r["Dispatch_Id"]), []).append(r)
        seen_markers, is_stall = 0, "SQ_WAIT_ANY" in group
        for did in sorted(disp):
            rs = disp[did]
            if MARKER in rs[0]["Kernel_Name"]:
                seen_markers += 1
                continue
            if seen_markers % 2 == 0 or seen_markers // 2 >= len(modes):
                continue                                   # outside a measured window: packing, calibration, warm-up
            m = modes[seen_markers // 2]
            k = _kclass(rs[0]["Kernel_Name"])
            for r in rs:
                c = r["Counter_Name"]
                if is_stall and c == "SQ_WAVE_CYCLES":
                    c = "stall:SQ_WAVE_CYCLES"
                if c in acc[m]:
                    acc[m][c][k] += float(r["Counter_Value"])
            if group[0] == "SQ_VALU_MFMA_BUSY_CYCLES":
                launches[m][k] += 1
                dur_ns[m][k] += int(rs[0]["End_Timestamp"]) - int(rs[0]["Start_Timestamp"])
        if seen_markers != 2 * len(modes):
            raise RuntimeError(f"counter child: {seen_markers} marker launches in the profile, expected {2 * len(modes)}")
    lds_group = [c for c in LDS_COUNTERS if c in names]
    stall_group = [c for c in STALL_COUNTERS if c in names and "SQ_WAIT_ANY" in names]
    result = {}
    for m in modes:
        A = acc[m]
        alg_bytes, calls = algorithmic_gemm_bytes(m, B, T)
        per = {}
        for k in sorted(launches[m], key=lambda k: -dur_ns[m][k]):
            fetch = 2.0 * A["FETCH_SIZE"][k] * 1024.0 / steps if "FETCH_SIZE" in A else 0.0      # KB -> bytes; x2: gfx950 tallies 128-B requests at 64 B
            write = A["WRITE_SIZE"][k] * 1024.0 / steps if "WRITE_SIZE" in A else 0.0
            cyc = A["SQ_BUSY_CYCLES"][k] / 32.0                             # summed over the 32 shader engines
            per[k] = {"launches_per_step": round(launches[m][k] / steps, 2), "ms_per_step": round(dur_ns[m][k] / steps / 1e6, 3),
                      "fetch_bytes_per_step": round(fetch), "write_bytes_per_step": round(write),
                      "hbm_gb_per_s": round((fetch + write) / max(dur_ns[m][k] / steps, 1), 1),
                      "mfma_busy": round(A["SQ_VALU_MFMA_BUSY_CYCLES"][k] / max(cyc * 1024.0, 1.0), 4),
                      "delivered_clock_ghz": round(cyc / max(dur_ns[m][k], 1), 3)}
            if all(c in A for c in REQSIZE_COUNTERS):
                n32, n64, n128, nall = (A[c][k] / steps for c in REQSIZE_COUNTERS)
                exact = 32.0 * n32 + 64.0 * n64 + 128.0 * n128
                per[k]["fetch_by_request_size"] = {"requests_32B": round(n32), "requests_64B": round(n64), "requests_128B": round(n128),
                                                   "requests_all": round(nall), "bytes_per_step": round(exact),
                                                   "over_corrected_FETCH_SIZE": round(exact / fetch, 4) if fetch else None}
            if lds_group:
                wc = A["SQ_WAVE_CYCLES"][k]
                per[k]["lds"] = {c: round(A[c][k] / steps) for c in lds_group}
                per[k]["lds"]["wait_inst_lds_over_wave_cycles"] = round(A["SQ_WAIT_INST_LDS"][k] / wc, 4) if wc else None
                per[k]["lds"]["active_inst_lds_over_wave_cycles"] = round(A["SQ_ACTIVE_INST_LDS"][k] / wc, 4) if wc else None
                ia = A["SQ_LDS_IDX_ACTIVE"][k]
                per[k]["lds"]["bank_conflict_over_idx_active"] = round(A["SQ_LDS_BANK_CONFLICT"][k] / ia, 4) if ia else None
                per[k]["lds"]["lds_array_busy"] = round(ia / max(cyc * 256.0, 1.0), 4) if ia else None
            if stall_group:
                wc = A["stall:SQ_WAVE_CYCLES"][k]
                st = {c: round(A[c][k] / steps) for c in stall_group if c != "SQ_WAVE_CYCLES"}
                st["SQ_WAVE_CYCLES"] = round(wc / steps)
                for c, nm in (("SQ_WAIT_ANY", "parked_at_waitcnt_or_barrier"), ("SQ_WAIT_INST_ANY", "issue_stalled"), ("SQ_ACTIVE_INST_ANY", "issuing"),
                              ("SQ_ACTIVE_INST_VALU", "issuing_valu_incl_mfma"), ("SQ_ACTIVE_INST_MISC", "issuing_misc")):
                    if c in stall_group:
                        st[nm + "_frac_of_wave_cycles"] = round(A[c][k] / wc, 4) if wc else None
                per[k]["stall"] = st
        step_classes = [k for k in launches[m] if not k.startswith("harness")]
        tb = sum(A["SQ_VALU_MFMA_BUSY_CYCLES"][k] for k in step_classes)
        tc = sum(A["SQ_BUSY_CYCLES"][k] for k in step_classes) / 32.0
        g = per.get("gemm", {})
        result[m] = {"prec": m, "batch": B, "views": T, "kernel_source_sha": kernel_source_sha(), "steps_profiled": steps,
                     "gemm_calls_per_step": calls, "gemm_kernel_launches_per_step": g.get("launches_per_step"),
                     "gemm_hbm_bytes_per_call": round((g.get("fetch_bytes_per_step", 0) + g.get("write_bytes_per_step", 0)) / calls),
                     "gemm_algorithmic_bytes_per_call": round(alg_bytes / calls),
                     "gemm_traffic_over_algorithmic": round((g.get("fetch_bytes_per_step", 0) + g.get("write_bytes_per_step", 0)) / alg_bytes, 3),
                     "mfma_busy_whole_step": round(tb / max(tc * 1024.0, 1.0), 4), "per_kernel_class": per,
                     "lds_counters": list(lds_group), "stall_counters": list(stall_group), "pass_seconds": pass_seconds,
                     "how": "rocprofv3 --kernel-trace --pmc <one group per pass: " + " | ".join(" ".join(g) for g in groups) + "> over `bench.py "
                            + " ".join(child) + "` (un-graphed, one batch at a time as ONE lane; only the dispatches between the child's "
                            "marker kernels count: no packing, calibration or warm-up); bytes = counter KB x 1024, FETCH_SIZE x 2 (gfx950 "
                            "correction, MI355X_MICROARCH.md HBM section: L2 -> fabric requests, MALL hits included, i.e. an UPPER bound on "
                            "HBM bytes), WRITE_SIZE as is; MFMA busy = MFMA-busy SIMD-cycles / (SQ_BUSY_CYCLES / 32 x 1024 SIMDs)"
                            + ("; fetch_by_request_size = 32 / 64 / 128-byte read requests summed at their own sizes (no correction needed), the check "
                               "of the corrected FETCH_SIZE on this access pattern" if all(c in names for c in REQSIZE_COUNTERS) else "")}
    return result


def measure_counters(args) -> None:
    """`--measure-counters --prec P`: all counter groups (traffic, MFMA busy, LDS, stalls) for ONE mode -> profiles/counters_<P>.json."""
    prec, B, T = args.prec, args.batch, args.views
    lds_group = _available_counters(LDS_COUNTERS)
    stall_group = _available_counters(STALL_COUNTERS)
    req_group = _available_counters(REQSIZE_COUNTERS)
    groups = list(BASIC_GROUPS) + ([tuple(lds_group)] if lds_group else []) + ([tuple(stall_group)] if stall_group else [])
    if len(req_group) == len(REQSIZE_COUNTERS):
        groups.append(tuple(req_group))
    out = collect_counters([prec], B, T, groups)[prec]
    path = os.path.join(ROOT, "profiles", f"counters_{prec}.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "how"}), flush=True)


def inline_counters(modes, B: int, T: int, budget_s: float):
    """The default single-GPU run re-measures MFMA-busy and HBM traffic for the headline and the default mode IN THIS RUN (VERDICT r4
    item 4): three PMC passes over one child process that runs both modes, bounded by `budget_s`.  ({mode: figures} or None, why-not)."""
    import shutil
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 is not on PATH"
    t0 = time.monotonic()
    try:
        res = collect_counters(list(modes), B, T, BASIC_GROUPS, steps=2, deadline=t0 + budget_s,
                               log=lambda msg: print("bench: " + msg, file=sys.stderr, flush=True))
    except Exception as e:                                   # noqa: BLE001 -- the stamped file is the fall-back, never a failed bench
        return None, f"in-run counter measurement failed ({type(e).__name__}: {str(e)[:300]})"
    for m in res.values():
        m["measured_in_this_run"] = True
        m["seconds"] = round(time.monotonic() - t0, 1)
    return res, None


def load_counters(prec: str, B: int, T: int):
    """(counters dict or None, why-not).  Only counters measured on the kernel sources now in the tree count."""
    path = os.path.join(ROOT, "profiles", f"counters_{prec}.json")
    if not os.path.exists(path):
        return None, f"no profiles/counters_{prec}.json (run `python bench.py --measure-counters --prec {prec}`)"
    c = json.load(open(path))
    if (c.get("batch"), c.get("views")) != (B, T):
        return None, f"profiles/counters_{prec}.json was measured at batch {c.get('batch')}, views {c.get('views')}"
    if c.get("kernel_source_sha") != kernel_source_sha():
        return None, (f"profiles/counters_{prec}.json is STALE: measured on kernel sources {c.get('kernel_source_sha')}, this tree is "
                      f"{kernel_source_sha()} (re-run --measure-counters)")
    return c, None


# ------------------------------------------------------------------------------------------------ one precision mode

class ModeRun:
    """Everything needed to time one precision mode on this rank: models, resident inputs, the (graphed) step."""

    def __init__(self, prec, args, device, world, rank, dist, images, bbox, mask, weights: str = "plain"):
        from boxdreamer_amd import calibrate, hip_ops
        from boxdreamer_amd.dist import gather_corners
        self.prec, self.args, self.device, self.world, self.rank, self.dist = prec, args, device, world, rank, dist
        self.images, self.bbox, self.mask = images, bbox, mask
        self.hip_ops, self.gather = hip_ops, gather_corners
        if getattr(args, "single_device_test", False) and world > 1:
            def host_staged_gather(kp, w):          # TEST mode only (gloo): the product's gather is dist.gather_corners on RCCL
                parts = [torch.zeros(kp.shape, dtype=kp.dtype) for _ in range(w)]
                dist.all_gather(parts, kp.detach().cpu())
                return torch.cat(parts, 0).to(kp.device)
            self.gather = host_staged_gather
        self.enc, self.dec = build_models(prec, device, weights)
        if getattr(args, "latency_forms", False):      # opt-in latency forms (split-K residual Linears for calls of one or two poses; ABI 9)
            self.enc.model.latency, self.dec.hip_latency = True, True
        # sub-batch lanes of one batch (two BATCHES in flight already fill each other's idle CUs: each then runs as one lane)
        def lane_arg(v):
            return v if v == "auto" else int(v)
        la = str(args.lanes).split(",")            # "auto" | N | E,D (encoder lanes, decoder lanes)
        self.lane_setting = (1, 1) if max(1, args.in_flight) > 1 else (lane_arg(la[0]), lane_arg(la[-1]))
        self.set_lanes(self.lane_setting)
        # what a maintainer's first forward does (boxdreamer_amd/model.py): the load-time self-check of the mode on the batch's first
        # sample, promoting the Linears that need it -- BEFORE anything is captured or timed; a no-op outside the f16c8 family
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.calibration = calibrate.calibrate(self.enc, self.dec, images, bbox, mask)
        self.B, self.T = images.shape[:2]
        self.kp_all = torch.empty((self.B, 8, 2), dtype=torch.float32, device=device)
        self.graphed = None
        self.cached = None
        self.lanes = []              # batches in flight: one captured graph + stream each (lane 0 = self.graphed on its own stream)
        self.k = 0
        if args.cache_refs:
            from boxdreamer_amd.cache import RefFeatureCache
            cache = RefFeatureCache(self.enc)
            qidx = torch.full((self.B,), self.T - 1, dtype=torch.long, device=device)
            self.cached = cache.place(cache.encode(images[:, : self.T - 1]), qidx, self.T)
        use_graph = args.graph if args.graph is not None else not args.cache_refs
        if use_graph:
            if args.cache_refs:
                raise SystemExit("--graph is wired for the plain step (not --cache-refs)")
            from boxdreamer_amd.graph import GraphedPath
            self.graphed = GraphedPath(self.enc, self.dec, self.B, self.T, 224, torch.bfloat16, device)
            self.graphed.set_inputs(images, bbox)
            # Two batches in flight (default): a second, independent copy of the path (own weights, workspace and captured graph)
            # replayed on a second stream, batch k on lane k % 2.  The kernels of one batch fill the idle CUs of the other's
            # tail rounds (DINOv2's N = 768 GEMMs run 3.06 rounds of 256 CUs, attention 13.5, ...); every batch is still
            # computed in full and in order on its lane.  `--in-flight 1` is the single-stream step.
            self.lanes.append({"g": self.graphed, "s": torch.cuda.Stream(device=device), "done": torch.cuda.Event(), "free": torch.cuda.Event()})
            for li in range(1, max(1, args.in_flight)):
                try:
                    enc2, dec2 = build_models(prec, device, weights)
                    enc2.model.lanes, dec2.hip_lanes = 1, 1
                    if self.calibration.get("state"):
                        calibrate.set_state(enc2, dec2, self.calibration["state"])
                    g2 = GraphedPath(enc2, dec2, self.B, self.T, 224, torch.bfloat16, device)
                    # the lane's own batch: B more distinct samples (another seed), so K steps really are K x B different-or-
                    # repeated-per-lane poses, not one batch fed to both lanes
                    from boxdreamer_amd import synth
                    other = synth.make_batch(seed=100 + rank + 1000 * li, B=self.B, T=self.T)
                    g2.set_inputs(other["images"].to(torch.bfloat16).to(device), other["bbox_feat"].to(torch.bfloat16).to(device))
                except (RuntimeError, MemoryError) as e:          # e.g. not enough memory for a second copy: one batch at a time
                    print(f"bench: second in-flight lane not available ({type(e).__name__}: {e}); timing one batch at a time", file=sys.stderr)
                    break
                self.lanes.append({"g": g2, "s": torch.cuda.Stream(device=device), "done": torch.cuda.Event(), "free": torch.cuda.Event()})
            if dist is not None:    # every rank must time the same number of lanes (the single-stream leg has its own barriers)
                n = torch.tensor([len(self.lanes)], dtype=torch.int32, device=device)
                dist.all_reduce(n, op=dist.ReduceOp.MIN)
                self.lanes = self.lanes[: int(n.item())]
            main = torch.cuda.current_stream(device)
            for ln in self.lanes:
                ln["free"].record(main)

    def set_lanes(self, setting):
        self.enc.model.lanes, self.dec.hip_lanes = setting if isinstance(setting, tuple) else (setting, setting)

    def effective_lanes(self) -> int:
        from boxdreamer_amd import _lib
        return max(_lib.resolve_lanes(self.enc.model.lanes, self.B * self.T, self.B * self.T, self.prec),
                   _lib.resolve_lanes(self.dec.hip_lanes, self.B * self.T, self.B, self.prec))

    def recapture(self, setting):
        """Re-capture the step's graph with another lane setting (same modules, same static inputs)."""
        from boxdreamer_amd.graph import GraphedPath
        assert self.graphed is not None and len(self.lanes) == 1
        imgs, bb = self.graphed.images, self.graphed.bbox_feat
        self.lanes[0]["g"] = None
        self.graphed = None              # lifts the freeze of the modules (graph.py)
        self.set_lanes(setting)
        self.graphed = GraphedPath(self.enc, self.dec, self.B, self.T, 224, torch.bfloat16, self.device)
        self.graphed.set_inputs(imgs, bb)
        self.lanes[0]["g"] = self.graphed

    def eager(self):
        if self.cached is not None:
            from boxdreamer_amd.cache import merge_cached_features
            feats = merge_cached_features(self.enc, self.images, self.cached[0], self.cached[1])
        else:
            feats = self.enc.predict(self.images)
        heat = self.dec(self.bbox, self.images, self.mask, feats, None)
        kp, _, _ = self.hip_ops.decode_topk(heat, want_idx=False)
        self.kp_all.copy_(kp)
        return self.kp_all

    def step_single(self):
        kp = self.graphed.replay()[1] if self.graphed is not None else self.eager()
        return self.gather(kp, self.world) if self.dist is not None else kp

    def step(self):
        if len(self.lanes) <= 1:
            return self.step_single()
        ln = self.lanes[self.k % len(self.lanes)]
        self.k += 1
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(ln["s"]):
            ln["s"].wait_event(ln["free"])           # the lane's previous corners have been gathered / consumed
            kp = ln["g"].replay()[1]
            ln["done"].record(ln["s"])
        if self.dist is not None:                    # the one collective of the sweep stays on the main stream, in batch order
            main.wait_event(ln["done"])
            out = self.gather(kp, self.world)
            ln["free"].record(main)
            return out
        ln["free"].record(ln["s"])
        return kp

    def last_outputs(self, out) -> dict:
        """What a caller received from the last step, as host fp32 arrays: the corners the step returned (`out`, all ranks' when they
        are gathered) and, when the step replays a captured graph, that graph's heat maps and normalised corners (this rank's batch)."""
        o = {"corners_px": out}
        g = self.lanes[(self.k - 1) % len(self.lanes)]["g"] if len(self.lanes) > 1 else self.graphed
        if g is not None:
            heat, _, kn, _ = g.out
            o.update(heat=heat, corners_norm=kn)
        torch.cuda.synchronize(self.device)
        return {k: v.detach().float().cpu().numpy() for k, v in o.items()}

    def close(self):
        self.graphed = None          # lifts the modules' freeze (graph.py) and releases the capture pool
        self.lanes = []


def trace_launches(lib, _lib, run_once, n_runs: int, cap: int = 8192):
    """HIP events on the launch stream around every GEMM / attention launch of `n_runs` un-graphed executions."""
    _lib.check(lib.bd_trace_begin(cap), "bd_trace_begin")
    t1 = time.perf_counter()
    for _ in range(n_runs):
        run_once()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t1) * 1e3
    buf = (_lib.TraceRecord * cap)()
    n = lib.bd_trace_end(buf, cap)
    return [(buf[i].kind, buf[i].M, buf[i].N, buf[i].K, buf[i].ms) for i in range(n)], wall_ms


def gather_latency_ms(kp, world, dist, gather, reps: int = 50, sync=None) -> float:
    """Mean latency of the corner all-gather alone (the only collective of the sweep), barrier-aligned."""
    sync = torch.cuda.synchronize if sync is None else sync
    for _ in range(5):
        gather(kp, world)
    barrier(dist, kp.device if kp.is_cuda else None)
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        gather(kp, world)
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def roofline_block(prec, recs, ms_per_step, trace_runs, value_per_gpu, fpp, counters, counters_why):
    peak = PEAK_MFMA_FP8 if prec in ("fp8", "fp8_mixed") else PEAK_MFMA_16BIT      # (mixed: priced against the e4m3 peak too: conservative)
    g = [(2.0 * m * n * k, ms) for kind, m, n, k, ms in recs if kind == 0]
    a = [(4.0 * m * n * n * k, ms) for kind, m, n, k, ms in recs if kind == 1]   # 4*S^2*d per (batch*head)
    gemm_tf = sum(f for f, _ in g) / max(sum(ms for _, ms in g), 1e-9) / 1e9 if g else 0.0
    attn_tf = sum(f for f, _ in a) / max(sum(ms for _, ms in a), 1e-9) / 1e9 if a else 0.0
    r = {"bound": "mfma", "kernel": "gemm_kernel_pc (persistent producer/consumer, 256x192 tiles, LDS-DMA operands, v_mfma_f32_32x32x16) + gemm_kernel_glds for the shapes it does not take",
         "achieved": round(gemm_tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(gemm_tf / peak, 4),
         "traffic": counters["gemm_hbm_bytes_per_call"] if counters else None,
         "traffic_source": counters["how"] if counters else counters_why,
         "algorithmic_bytes_per_launch": counters["gemm_algorithmic_bytes_per_call"] if counters else None,
         "traffic_over_algorithmic": counters["gemm_traffic_over_algorithmic"] if counters else None,
         "mfma_busy": ({"gemm": counters["per_kernel_class"].get("gemm", {}).get("mfma_busy"),
                        "attention": counters["per_kernel_class"].get("attention", {}).get("mfma_busy"),
                        "whole_step_one_batch_at_a_time": counters["mfma_busy_whole_step"],
                        "unit": "fraction of SIMD cycles with the MFMA pipe busy (counted, rocprofv3 PMC)"} if counters else None),
         "mfma_busy_gemm": counters["per_kernel_class"].get("gemm", {}).get("mfma_busy") if counters else None,
         "mfma_busy_whole_step": counters["mfma_busy_whole_step"] if counters else None,
         "counters_measured_in_this_run": bool(counters and counters.get("measured_in_this_run")),
         "algorithmic_flops_per_launch": round(sum(f for f, _ in g) / max(len(g), 1)), "launches": len(g),
         "events": f"HIP events (launch stream) around every GEMM / attention launch of {trace_runs} un-graphed ONE-LANE executions of "
                   "the step on the same buffers right after the timed region (events cannot be timed inside a captured graph; with "
                   "sub-batch lanes two launches overlap and a per-launch duration is not defined)",
         "avg_launch_ms": round(sum(ms for _, ms in g) / max(len(g), 1), 4),
         "mfma_passes_per_algorithmic_flop": MFMA_PASSES.get(prec, 1.0),
         "attention_achieved": round(attn_tf, 2),
         "attention_avg_launch_ms": round(sum(ms for _, ms in a) / max(len(a), 1), 4),
         # kernel time per step (event-timed, un-graphed, one lane) over the timed ONE-LANE step time (graph replay)
         "gemm_time_frac_of_step": round(sum(ms for _, ms in g) / trace_runs / ms_per_step, 4),
         "attention_time_frac_of_step": round(sum(ms for _, ms in a) / trace_runs / ms_per_step, 4),
         "peak_note": "peak = dense MFMA rate at 2.4 GHz (MI355X_MICROARCH.md).  Under its 1400 W cap the part does not hold that clock in a dense "
                      "GEMM: the same persistent kernels on HALF the CUs deliver 72-82 % of the full-chip rate (profiles/r4_cu_limit_probe.md), every "
                      "MFMA-heavy launch draws 1398-1400 W at a reported 1.73-1.93 GHz (profiles/r4_power_by_kernel.md; this run's board power: the "
                      "`power` block of the line); a pure MFMA loop without memory traffic sustains 1.9-2.0 PFLOP/s on CONSTANT operands (profiles/r2_mfma_util.md) "
                      "and 1.75-1.8 PFLOP/s at 1.53-1.68 GHz when its operands change every instruction (profiles/r5_mfma_toggle.md)",
         "whole_path_achieved": round(value_per_gpu * fpp / 1e12, 2),
         "whole_path_frac": round(value_per_gpu * fpp / 1e12 / peak, 4)}
    return r


def apply_counters(rf: dict, c: dict) -> None:
    """Overwrite a roofline block's counter-derived fields with figures measured in THIS run (inline_counters)."""
    pk = c["per_kernel_class"]
    rf.update(traffic=c["gemm_hbm_bytes_per_call"], traffic_source="measured in THIS run: " + c["how"],
              algorithmic_bytes_per_launch=c["gemm_algorithmic_bytes_per_call"], traffic_over_algorithmic=c["gemm_traffic_over_algorithmic"],
              mfma_busy={"gemm": pk.get("gemm", {}).get("mfma_busy"), "attention": pk.get("attention", {}).get("mfma_busy"),
                         "whole_step_one_batch_at_a_time": c["mfma_busy_whole_step"],
                         "unit": "fraction of SIMD cycles with the MFMA pipe busy (counted, rocprofv3 PMC)"},
              mfma_busy_gemm=pk.get("gemm", {}).get("mfma_busy"), mfma_busy_whole_step=c["mfma_busy_whole_step"],
              counters_measured_in_this_run=True, counter_pass_seconds=c.get("pass_seconds"),
              counters_run_configuration="a rocprofv3 child process of this run: the same step UN-GRAPHED as ONE lane (per-kernel counters need "
                                         "one launch at a time); `value` / `achieved` are the graphed step with sub-batch lanes -- the counter "
                                         "figures describe the kernels, not that schedule",
              gemm_ms_per_step_under_the_counters=pk.get("gemm", {}).get("ms_per_step"),
              delivered_clock_ghz_gemm=pk.get("gemm", {}).get("delivered_clock_ghz"))


def calibration_summary(rep: dict) -> dict:
    if not rep.get("applicable"):
        return {"applicable": False}
    return {"applicable": True, "self_check_unpromoted_max_abs_dlogits": rep["delta_unpromoted"], "self_check_final": rep["delta_final"],
            "budget": rep["budget"], "ok": rep["ok"], "promoted_units": len(rep["promoted"]), "units": rep["units"],
            "promoted_work_frac": rep["promoted_cost_frac"], "forwards": rep["forwards"], "seconds": rep.get("seconds"),
            "reference": rep["reference"]}


def measure_mode(prec, args, device, world, rank, dist, images, bbox, mask, weights: str = "plain", keep_outputs: bool = False):
    """Times K steps of one mode.  With --full also the one-lane / one-stream record of the same K steps and (rank 0) the roofline
    block from a launch trace; `keep_outputs`: the last timed step's outputs as host arrays (res["outputs"], rank 0)."""
    from boxdreamer_amd import _lib
    lib = _lib.load()
    run = ModeRun(prec, args, device, world, rank, dist, images, bbox, mask, weights)
    sync = torch.cuda.synchronize if dist is None else interruptible_sync(device)
    B, T = run.B, run.T
    sub_lanes = run.effective_lanes()
    one_lane = None
    if args.full and sub_lanes > 1 and run.graphed is not None and len(run.lanes) == 1:
        # for the record, first: the same K steps with the batch as ONE lane on one stream (the form of rounds 1-3), then the laned form
        run.recapture(1)
        dt1, _, out1 = timed_steps(run.step_single, args.steps, args.warmup, world, dist, sync, device)
        one_lane = {"value": round(B * world * args.steps / dt1, 2), "ms_per_step": round(dt1 / args.steps * 1e3, 3), "sub_batch_lanes": 1}
        run.recapture(run.lane_setting)
    dt, per_rank, out = timed_steps(run.step, args.steps, args.warmup, world, dist, sync, device)
    assert out.shape[0] == B * world and torch.isfinite(out).all()
    res = {"dt": dt, "per_rank": per_rank, "out": out, "run": run, "in_flight": max(1, len(run.lanes)), "sub_lanes": sub_lanes,
           "calibration": calibration_summary(run.calibration)}
    if keep_outputs and rank == 0:
        res["outputs"] = run.last_outputs(out)
    if one_lane is not None:
        assert torch.equal(out, out1), "sub-batch lanes changed the corners (they must be bit-identical to the one-lane form)"
        res["single_stream"] = one_lane
    if args.full and len(run.lanes) > 1:        # the same K steps one batch at a time on one stream, for the record
        dt1, _, out1 = timed_steps(run.step_single, args.steps, 1, world, dist, sync, device)
        assert out1.shape == out.shape and torch.isfinite(out1).all()     # (lanes hold different batches: values differ by design)
        res["single_stream"] = {"value": round(B * world * args.steps / dt1, 2), "ms_per_step": round(dt1 / args.steps * 1e3, 3)}
    if rank == 0:
        value = B * world * args.steps / dt
        fpp = flops_per_pose(T) if not args.cache_refs else DINO_FLOP_PER_IMAGE + betr_flops(T)
        res.update(value=value, fpp=fpp, ms_per_step=dt / args.steps * 1e3)
    if rank == 0 and args.full:
        TRACE = 3
        run.set_lanes(1)             # per-launch durations are only defined with one launch at a time: the trace runs the one-lane form
        recs, _ = trace_launches(lib, _lib, run.eager, TRACE)
        run.set_lanes(run.lane_setting)
        counters, why = (None, "reference features cached: other algorithmic traffic") if args.cache_refs else load_counters(prec, B, T)
        if weights != "plain" and run.calibration.get("promoted"):
            counters, why = None, "promoted Linears: the counter file describes the unpromoted mode"
        # (kernel-time fractions are of the ONE-LANE step the trace executes, where there is one)
        res["roofline"] = roofline_block(prec, recs, one_lane["ms_per_step"] if one_lane else dt / args.steps * 1e3, TRACE, value / world,
                                         fpp, counters, why)
    return res


# at most this many bytes in all under --dump-outputs (np.save's headers stay far inside the margin to 64 MB)
DUMP_LIMIT_BYTES = 64 * 10 ** 6 - 64 * 1024


def dump_outputs(path: str, arrays: dict) -> list:
    """`--dump-outputs DIR`: every array as DIR/<name>.npy in float32, smallest first.  An array that would take the set past
    DUMP_LIMIT_BYTES keeps a fixed, seeded sample of its leading-axis entries (in order), the same entries for the same arguments."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left, written = DUMP_LIMIT_BYTES, []
    for name, a in sorted(arrays.items(), key=lambda kv: (kv[1].nbytes, kv[0])):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.nbytes > left:
            keep = min(a.shape[0], left // max(1, a.nbytes // max(1, a.shape[0])))
            a = np.ascontiguousarray(a[np.sort(np.random.default_rng(0).choice(a.shape[0], size=keep, replace=False))])
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes
        written.append(name + ".npy")
    return written


def h2d_inclusive(run: "ModeRun", steps: int) -> dict:
    """MEASURED host-buffer rate: every step's inputs start in PINNED host memory; a copy stream uploads batch i+1 into the
    second of two device buffer sets while the compute stream runs batch i (events order copy -> compute -> reuse)."""
    dev = run.device
    orig = (run.images, run.bbox)
    host_img = run.images.cpu().pin_memory()
    host_bb = run.bbox.cpu().pin_memory()
    dimg = [torch.empty_like(run.images) for _ in range(2)]
    dbb = [torch.empty_like(run.bbox) for _ in range(2)]
    copy_s = torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    ready = [torch.cuda.Event() for _ in range(2)]
    free = [torch.cuda.Event() for _ in range(2)]

    def upload(i):
        b = i & 1
        with torch.cuda.stream(copy_s):
            copy_s.wait_event(free[b])
            dimg[b].copy_(host_img, non_blocking=True)
            dbb[b].copy_(host_bb, non_blocking=True)
            ready[b].record(copy_s)

    def compute(i):
        b = i & 1
        main.wait_event(ready[b])
        if run.graphed is not None:
            run.graphed.set_inputs(dimg[b], dbb[b])
            run.graphed.replay()
        else:
            run.images, run.bbox = dimg[b], dbb[b]
            run.eager()
        free[b].record(main)

    for b in range(2):
        free[b].record(main)
    torch.cuda.synchronize()
    # serialised: copy, then compute, no overlap
    t0 = time.perf_counter()
    for i in range(steps):
        upload(i); compute(i)
        torch.cuda.synchronize()
    ser = (time.perf_counter() - t0) / steps
    # double-buffered: upload of batch i+1 issued before the compute of batch i
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    upload(0)
    for i in range(steps):
        if i + 1 < steps:
            upload(i + 1)
        compute(i)
    torch.cuda.synchronize()
    ovl = (time.perf_counter() - t0) / steps
    nbytes = host_img.numel() * host_img.element_size() + host_bb.numel() * host_bb.element_size()
    t0 = time.perf_counter()
    for _ in range(3):
        dimg[0].copy_(host_img, non_blocking=True); dbb[0].copy_(host_bb, non_blocking=True)
    torch.cuda.synchronize()
    copy_ms = (time.perf_counter() - t0) / 3 * 1e3
    run.images, run.bbox = orig
    if run.graphed is not None:
        run.graphed.set_inputs(*orig)
    return {"input_mb_per_batch": round(nbytes / 1e6, 1), "h2d_ms_per_batch": round(copy_ms, 3),
            "h2d_gb_per_s": round(nbytes / copy_ms / 1e6, 1),
            "serialised_poses_per_s": round(run.B / ser, 1), "double_buffered_poses_per_s": round(run.B / ovl, 1),
            "how": "measured: pinned host buffers, copy stream + 2 device buffer sets, events between copy and compute"}


def facade_block(args, device, one: dict, prec: str, reference_value: float | None) -> dict:
    """the throughput of the surface the north_star says to keep -- `boxdreamer_amd.model.BoxDreamer(config).eval()(batch)`,
    what callers of `self.BoxDreamer(batch)` get (/root/reference/src/lightning/BoxDreamer_lightning_model.py:228, src/demo/demo.py:1501-1506)
    from INTEGRATION.md's 3-line patch: the configs[1] batch dict in, corners + host PnP out, default mode, bf16 inputs.  Eager (every launch
    from the host) and with `hip_graph: true` (the step replayed from one captured graph behind the facade); the constructor's `config` is the
    reference's own YAML as data (tests/golden/model_modules_config.json)."""
    import copy
    from boxdreamer_amd.model import BoxDreamer
    path = os.path.join(ROOT, "tests", "golden", "model_modules_config.json")
    if not os.path.exists(path):
        return {"skipped": "tests/golden/model_modules_config.json (the reference's YAML as data) is not in this tree"}
    bsd, dsd = state_dicts("plain")
    B, T = one["images"].shape[:2]
    batch = {k: ((v.to(torch.bfloat16) if v.is_floating_point() else v).to(device) if torch.is_tensor(v) else v) for k, v in one.items()}
    out, res = {}, {}
    for tag, graph, dev_pnp in (("eager", False, False), ("hip_graph", True, False), ("hip_graph_pnp_on_device", True, True)):
        mods = copy.deepcopy(json.load(open(path))["modules"])
        mods["decoder"].update(num_decoder_layers=12, hip_precision=prec)
        mods["encoder"]["dino"]["cfg"].update(state_dict=dsd, hip_precision=prec)
        mods["hip_graph"] = graph
        mods["pnp_on_device"] = dev_pnp
        model = BoxDreamer({"modules": mods})
        model.load_state_dict({"decoder." + k: v for k, v in bsd.items()}, strict=True)
        model = model.to(device).eval()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(max(2, args.warmup)):      # (the first forward runs the load-time calibration; with hip_graph also the capture)
                ret = model(dict(batch))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ret = model(dict(batch))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[tag] = ret
        res[tag] = {"poses_per_s": round(B * args.steps / dt, 2), "ms_per_forward": round(dt / args.steps * 1e3, 3)}
        if reference_value:
            res[tag]["vs_parity_mode_value"] = round(B * args.steps / dt / reference_value, 4)
        res[tag]["host_syncs_per_forward"] = list(model.host_syncs_per_forward or [])
        res[tag]["pose_solver"] = ret.get("pose_solver")
        if not dev_pnp:
            syncs, solver, lanes = list(model.host_syncs_per_forward or []), ret.get("pose_solver"), ret["hip_precision"].get("sub_batch_lanes")
        del model
        torch.cuda.empty_cache()
    same = all(torch.equal(out["eager"][k], out["hip_graph"][k]) for k in ("pred_bbox", "pred_poses", "regression_boxes", "pred_corners_px"))
    return {"what": "BoxDreamer(config).eval()(batch) on the configs[1] dict (1 query + 5 refs, batch %d, bf16 tensors on the device): encoder + decoder + "
                    "corner decode + ONE D2H + host PnP + the dict's outputs, per call; K = %d calls back to back" % (B, args.steps),
            "mode": prec, "eager": res["eager"], "hip_graph": res["hip_graph"], "poses_per_s": res["hip_graph"]["poses_per_s"],
            "hip_graph_pnp_on_device": dict(res["hip_graph_pnp_on_device"],
                                            what="config['modules']['pnp_on_device'] = True: the corners never leave the device (bd_solve_pnp), no host "
                                                 "synchronisation inside forward(); the heat maps / corners are bit-identical, the poses come from the HIP "
                                                 "solver instead of the host one (both un-pinned against OpenCV)"),
            "corners_identical_with_pnp_on_device": bool(torch.equal(out["hip_graph"]["pred_corners_px"], out["hip_graph_pnp_on_device"]["pred_corners_px"])),
            "outputs_bit_identical_eager_vs_graph": bool(same), "sub_batch_lanes": lanes, "pose_solver": solver,
            "host_syncs_per_forward": syncs,
            "not_overlapped": "the host PnP of batch i runs before the call returns (pred_poses is part of the returned dict); "
                              "`pnp_inclusive` shows what overlapping it with batch i + 1 buys a caller that defers it"}


def _hwmon_of(device) -> str | None:
    """hwmon directory (power1_input / power1_cap / freq1_input) of the amdgpu card behind a HIP device, matched by PCI address."""
    import glob
    try:
        pr = torch.cuda.get_device_properties(device)
        want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
    except Exception:  # noqa: BLE001
        return None
    for h in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"):
        pci = os.path.basename(os.path.realpath(os.path.join(h, "..", "..")))
        if pci.lower().startswith(want) and os.path.exists(os.path.join(h, "power1_input")):
            return h
    return None


def power_probe(run: "ModeRun", seconds: float = 1.5) -> dict:
    """Board power and shader clock WHILE the step runs back to back (sysfs hwmon of the card, sampled from a thread every ~5 ms):
    the evidence for `roofline.peak_note` in every bench line -- this path runs at the part's power cap, not at a pipe limit."""
    h = _hwmon_of(run.device)
    if h is None:
        return {"available": False, "why": "no amdgpu hwmon node for this device (power1_input) visible in this container"}

    def rd(name):
        try:
            return int(open(os.path.join(h, name)).read().strip())
        except (OSError, ValueError):
            return None
    cap = rd("power1_cap")
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            p, f = rd("power1_input"), rd("freq1_input")
            if p is not None:
                samples.append((time.perf_counter(), p / 1e6, (f or 0) / 1e6))
            time.sleep(0.005)
    idle_w = (rd("power1_input") or 0) / 1e6
    th = threading.Thread(target=sampler, daemon=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    th.start()
    n = 0
    while time.perf_counter() - t0 < seconds:
        run.step_single() if len(run.lanes) <= 1 else run.step()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    stop.set(); th.join()
    # the SMU's reading lags the load by ~100 ms: the second half of the window is the steady state
    late = [(w, f) for (t, w, f) in samples if t - t0 > 0.5 * (t1 - t0)]
    if not late:
        return {"available": False, "why": "no samples"}
    ws, fs = [w for w, _ in late], [f for _, f in late]
    return {"available": True, "avg_w": round(sum(ws) / len(ws), 1), "max_w": round(max(ws), 1), "cap_w": round(cap / 1e6, 1) if cap else None,
            "frac_of_cap": round(sum(ws) / len(ws) / (cap / 1e6), 3) if cap else None, "before_the_load_w": round(idle_w, 1),
            "sclk_reported_mhz_avg": round(sum(fs) / len(fs)), "samples": len(late), "steps": n, "seconds": round(t1 - t0, 2),
            "poses_per_s_during_probe": round(n * run.B / (t1 - t0), 1),
            "joule_per_pose": round(sum(ws) / len(ws) / (n * run.B / (t1 - t0)), 3),
            "how": "sysfs hwmon power1_input / freq1_input of the card (matched by PCI address), 5 ms sampling from a thread while the captured step "
                   "replays back to back; steady-state half of the window (the reported sclk is the PLL target, not the delivered rate: "
                   "profiles/r2_gemm_phase_probe.md section 3)"}


def sustained_block(run: "ModeRun", seconds: float, step_ms: float) -> dict:
    """the timed window of `value` is K = 20 steps (< 1 s) on a part that sits at its board power cap.  This leg replays
    the same captured step back to back for >= `seconds` and reports the rate of the first and of the last 5 s, with board power, the
    reported shader clock and (where the hwmon node exposes them) the temperatures over the same two windows -- which of the two numbers is
    the steady state is then a reading, not a guess."""
    h = _hwmon_of(run.device)

    def rd(name):
        try:
            return int(open(os.path.join(h, name)).read().strip())
        except (OSError, ValueError, TypeError):
            return None
    temps = {}
    if h is not None:
        import glob
        for f in sorted(glob.glob(os.path.join(h, "temp*_input"))):
            lab = f.replace("_input", "_label")
            name = open(lab).read().strip() if os.path.exists(lab) else os.path.basename(f)[:-6]
            temps[name] = os.path.basename(f)
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            if h is not None:
                samples.append((time.perf_counter(), (rd("power1_input") or 0) / 1e6, (rd("freq1_input") or 0) / 1e6,
                                {k: (rd(v) or 0) / 1e3 for k, v in temps.items()}))
            time.sleep(0.05)
    th = threading.Thread(target=sampler, daemon=True)
    marks = []                       # (host time, steps completed) at every synchronisation
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    th.start()
    n = 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            run.step_single() if len(run.lanes) <= 1 else run.step()
        n += 8
        torch.cuda.synchronize()     # (one drain per 8 steps: < 0.1 % of the window, and it bounds the host's run-ahead)
        marks.append((time.perf_counter(), n))
    t1 = time.perf_counter()
    stop.set(); th.join()

    def window(lo, hi):
        inside = [(t, k) for t, k in marks if lo <= t - t0 <= hi]
        if len(inside) < 2:
            return None
        (ta, ka), (tb, kb) = inside[0], inside[-1]
        ws = [w for (t, w, f, tt) in samples if lo <= t - t0 <= hi]
        fs = [f for (t, w, f, tt) in samples if lo <= t - t0 <= hi]
        tm = {k: round(max(tt[k] for (t, w, f, tt) in samples if lo <= t - t0 <= hi), 1) for k in temps} if ws else {}
        return {"poses_per_s": round((kb - ka) * run.B / (tb - ta), 2), "ms_per_step": round((tb - ta) / (kb - ka) * 1e3, 3),
                "avg_w": round(sum(ws) / len(ws), 1) if ws else None, "sclk_reported_mhz_avg": round(sum(fs) / len(fs)) if fs else None,
                "temps_c_max": tm or None}
    total = t1 - t0
    first, last = window(0.0, 5.0), window(total - 5.0, total)
    out = {"mode": run.prec, "seconds": round(total, 2), "steps": n, "poses_per_s_whole_window": round(n * run.B / total, 2),
           "first_5s": first, "last_5s": last, "timed_region_ms_per_step": round(step_ms, 3),
           "cap_w": round((rd("power1_cap") or 0) / 1e6, 1) if h is not None else None,
           "hwmon": "sysfs hwmon of the card (power1_input, freq1_input, temp*_input with their labels), 50 ms sampling" if h is not None
                    else "no amdgpu hwmon node visible in this container: rates only"}
    if first and last:
        drop = 1.0 - last["poses_per_s"] / (run.B / (step_ms / 1e3))
        out["last_5s_vs_timed_region"] = round(last["poses_per_s"] / (run.B / (step_ms / 1e3)), 4)
        out["steady_state"] = ("the last 5 s are within 2 % of the 20-step figure: `value` is the steady state" if drop <= 0.02 else
                               f"the last 5 s are {drop * 100:.1f} % below the 20-step figure: the sustained rate (last_5s.poses_per_s) is the steady state, "
                               "`value` is the short-window figure the bench contract times")
    return out


def pnp_inclusive(run: "ModeRun", one, steps: int, step_ms: float) -> dict:
    """MEASURED PnP-inclusive rates (never `value`): one D2H of the decoded corners per batch + ONE batched host
    solve (boxdreamer_amd/pnp.py).  serialised: step, D2H, solve, next step.  overlapped: a host thread solves batch i
    while the GPU runs batch i+1 (measured wall over `steps` batches, not a min() of two rates)."""
    from boxdreamer_amd.box_utils import solve_poses_host
    from boxdreamer_amd import pnp as pnp_mod
    B = run.B
    b3 = one["bbox_3d"].float().reshape(-1, 8, 3)[-1:].repeat(B, 1, 1).numpy()
    Kq = one["non_ndc_intrinsics"].float().reshape(-1, 3, 3)[-1:].repeat(B, 1, 1).numpy()

    def solve(kp_dev):
        return solve_poses_host(kp_dev.float().cpu().numpy(), b3, Kq)

    kp = run.step_single()[:B]
    tp = []
    for _ in range(3):
        t1 = time.perf_counter()
        solve(kp)
        tp.append(time.perf_counter() - t1)
    pnp_ms = sorted(tp)[1] * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        solve(run.step_single()[:B])
    ser = (time.perf_counter() - t0) / steps
    # overlapped: corners of batch i are copied to a pinned host buffer (async, event), the solver thread waits for the
    # event and solves while the main thread has already enqueued batch i+1
    host_kp = [torch.empty((B, 8, 2), dtype=torch.float32).pin_memory() for _ in range(2)]
    evs = [torch.cuda.Event() for _ in range(2)]
    worker = [None]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        b = i & 1
        out = run.step_single()[:B]
        host_kp[b].copy_(out, non_blocking=True)
        evs[b].record()
        if worker[0] is not None:
            worker[0].join()

        def job(b=b):
            evs[b].synchronize()
            solve_poses_host(host_kp[b].numpy(), b3, Kq)
        worker[0] = threading.Thread(target=job)
        worker[0].start()
    worker[0].join()
    torch.cuda.synchronize()
    ovl = (time.perf_counter() - t0) / steps
    return {"pnp_ms_per_batch": round(pnp_ms, 2),
            "host": ("cv2.solvePnP" if pnp_mod._HAVE_CV2 else "bd_solve_pnp_host: native DLT + LM on 8 host threads (csrc/pnp.hip), parity vs OpenCV un-pinned"),
            "serialised_poses_per_s": round(B / ser, 1), "overlapped_poses_per_s": round(B / ovl, 1),
            "how": f"measured over {steps} batches: serialised = step -> D2H -> solve -> next step; overlapped = solver thread "
                   "on batch i while the GPU runs batch i+1 (pinned D2H + event)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prec", default=os.environ.get("BOXDREAMER_HIP_PREC", STRICT_PREC), choices=sorted(_PRECS),
                    help="the mode `value` is measured in.  Default: the package default, the mode that MEETS north_star's parity bar (round 6; "
                         "rounds 1-5 put the bf16 single-pass mode here, which does not -- it is now the `bf16_opt_in` block of the same line)")
    ap.add_argument("--batch", type=int, default=32, help="samples per GPU")
    ap.add_argument("--views", type=int, default=6, help="T = refs + 1")
    ap.add_argument("--cache-refs", action="store_true",
                    help="'next' row f1: reference features encoded once outside the timed region; per step the encoder "
                         "sees only the query crops (different algorithmic FLOPs -> reported as its own metric)")
    ap.add_argument("--graph", dest="graph", action="store_true", default=None,
                    help="replay the step from a captured HIP graph (default)")
    ap.add_argument("--no-graph", dest="graph", action="store_false", help="launch every kernel from the host each step")
    ap.add_argument("--in-flight", type=int, default=1,
                    help="batches in flight in graph mode: 1 = one batch at a time (default since round 4: the batch itself runs as "
                         "sub-batch lanes, --lanes), 2 = two captured copies of the path replayed alternately on two streams (rounds 2-4; "
                         "each batch then runs as one lane)")
    ap.add_argument("--lanes", default="auto",
                    help="sub-batch lanes of ONE batch (bd_*_forward_lanes, ABI v6): 'auto' (2 from 96 images per call on), or 1..4; "
                         "bit-identical results for every value")
    ap.add_argument("--no-strict", action="store_true", help="skip the second (strict-mode) timing")
    ap.add_argument("--no-trained-like", action="store_true", help="skip the strict-mode leg on the trained-like outlier weights")
    ap.add_argument("--no-latency", action="store_true", help="skip the one-pose (B = 1) latency leg of the default single-GPU run")
    ap.add_argument("--latency-forms", action="store_true",
                    help="opt into the latency forms (`hip_latency: true`: split-K residual Linears for calls of one or two poses; deterministic, within "
                         "tolerance, not bit-identical to the same sample inside a larger batch) -- for --batch 1 / 2 runs")
    ap.add_argument("--no-fp8", action="store_true", help="skip the configs[4] leg (fp8 Linears, batch 64) of the default single-GPU run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--sustained", type=float, default=30.0,
                    help="seconds of back-to-back replays of the headline mode's step AFTER the timed region (the `sustained` block of the default "
                         "single-GPU line: first / last 5 s, power, clock, temperatures); 0 = skip")
    ap.add_argument("--no-facade", action="store_true", help="skip the `facade` block (BoxDreamer.forward on the batch dict, eager and hip_graph) of the default single-GPU run")
    ap.add_argument("--no-pnp", action="store_true", help="skip the PnP-inclusive side measurement (host PnP, SURVEY 8d / 8f3)")
    ap.add_argument("--no-h2d", action="store_true", help="skip the host-buffer (PCIe-inclusive) side measurement")
    ap.add_argument("--no-power", action="store_true", help="skip the board-power / clock probe (sysfs hwmon, 1.5 s of back-to-back steps per mode)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--cpu-plumbing", action="store_true",
                    help="run ONLY the launcher / barrier / corner-gather plumbing on CPU (tests); needs --backend gloo")
    ap.add_argument("--single-device-test", action="store_true",
                    help="TEST ONLY: every rank uses cuda:0 and the collectives go through gloo -- exercises the whole N > 1 bench flow "
                         "(sharded seeds, lane agreement, barriers, corner gather, failure report) with the real kernels on a 1-GPU box; "
                         "not a measurement (the ranks share one GPU) and not RCCL")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group and run every collective of the sweep (barriers, the corner all-gather, the per-rank "
                         "timing gather) even at world size 1: what a one-GPU box can execute of the RCCL path (tests/test_gpu_rccl.py, the "
                         "`rccl_world1` block of the default line)")
    ap.add_argument("--rccl-probe", action="store_true", help=argparse.SUPPRESS)        # child of rccl_world1_block
    ap.add_argument("--no-rccl-probe", action="store_true", help="skip the `rccl_world1` block of the default single-GPU line")
    ap.add_argument("--dry-run", action="store_true",
                    help="print the exact launch command + environment `--gpus N` turns into (JSON) and exit")
    ap.add_argument("--dist-timeout", type=int, default=600, help="collective timeout in seconds (a dead rank must not hang the others)")
    ap.add_argument("--plumbing-fail-rank", type=int, default=-1, help="(--cpu-plumbing) make this rank raise at --plumbing-fail-stage")
    ap.add_argument("--plumbing-fail-stage", default="before_timed", choices=["before_timed", "after_timed", "before_report"])
    ap.add_argument("--plumbing-short-rank", type=int, default=-1, help="(--cpu-plumbing) this rank offers only one in-flight lane")
    ap.add_argument("--plumbing-global-batch", type=int, default=0, help="(--cpu-plumbing) also gather a ragged global batch of this size")
    ap.add_argument("--counter-child", default="", help=argparse.SUPPRESS)        # what the rocprofv3 passes profile: comma-separated modes
    ap.add_argument("--no-inline-counters", action="store_true",
                    help="do not re-measure MFMA-busy / HBM traffic with rocprofv3 inside this run (single GPU; ~45 s); the stamped "
                         "profiles/counters_<mode>.json is then the source, if it matches the kernel sources")
    ap.add_argument("--counter-budget", type=float, default=75.0, help="seconds the in-run counter passes may take before they are abandoned")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, measure and check everything else the line reports (the other mode of record, rooflines, "
                         "parity, side measurements, the other configs, CPU baseline, in-run counters); the --no-* options trim it")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's outputs (corners; heat maps and normalised corners of a graphed step) as DIR/<name>.npy "
                         "in float32, at most 64 MB in all")
    ap.add_argument("--config3", action="store_true",
                    help="with --full: also time BASELINE configs[3]'s per-GPU shard (1 query + 16 refs, batch 32/GPU) in the same line "
                         "(default for --gpus > 1)")
    ap.add_argument("--measure-counters", action="store_true",
                    help="run the rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE, MFMA busy: one pass each) over this script for --prec and "
                         "write profiles/counters_<prec>.json, which later default runs report as roofline.traffic / mfma_busy")
    args = ap.parse_args()

    maybe_respawn(args)
    if args.rccl_probe:
        return rccl_probe(args)
    if args.counter_child:
        return counter_child(args)
    if args.measure_counters:
        return measure_counters(args)
    _, rank0, _ = dist_env()
    try:
        return run(args)
    except BaseException as e:                   # noqa: BLE001 -- report, then re-raise with a non-zero exit
        if isinstance(e, SystemExit) and e.code in (0, None):
            raise
        if rank0 == 0:
            emit_failure(f"{type(e).__name__}: {e}")
        raise


def workload_name(B: int, T: int, prec: str, world: int, cache_refs: bool) -> str:
    """Which BASELINE.json config this invocation IS (the T = 17 and B = 1 lines used to be labelled configs[1])."""
    shape = f"1 query + {T - 1} ref, 224x224, batch {B}/GPU ({B} distinct seeded samples per rank and in-flight lane)"
    tail = ", DINOv2 ViT-B/14-reg + BETR-12 + top-20 decode, random-init weights, inputs bf16 in HBM"
    if cache_refs:
        return "SURVEY 8f1 (reference features cached): " + shape + tail
    if prec in ("fp8", "fp8_mixed") and T == 6 and B == 64:
        return ("configs[4]: fp8 (e4m3) Linears, " if prec == "fp8" else "configs[4], mixed policy: e4m3 MLPs / DINOv2 QKV, bf16 elsewhere, ") + shape + tail
    if T == 6 and B == 32 and prec not in ("fp8", "fp8_mixed"):
        return "configs[1]: " + shape + tail
    if T == 17:
        full = B * world == 256 and world == 8
        return ("configs[3]: " if full else f"configs[3] shape (the config itself is batch 256 over 8 GPUs; this run: batch {B * world} over {world}): ") + shape + tail
    if T == 2 and B == 1:
        return "configs[0] shape on the GPU: " + shape + tail
    return "custom (not a BASELINE.json config): " + shape + tail


def run(args):
    if args.cpu_plumbing:
        if args.backend != "gloo":
            raise SystemExit("--cpu-plumbing needs --backend gloo")
        return cpu_plumbing(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (MI355X); there is no CPU fallback for the product path")
    if args.backend != "nccl" and not (args.single_device_test and args.backend == "gloo"):
        raise SystemExit("the GPU sweep runs on RCCL (--backend nccl)")
    _, _, local_rank = dist_env()
    if args.single_device_test:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    world, rank, local_rank, dist = init_dist(args)
    # host threads: torch defaults to one per LOGICAL CPU (256 on the GPU box, under a 16-CPU quota): the seeded-weight generation, the
    # weight packing and rank 0's CPU-oracle parity probes crawl when oversubscribed.  Rank 0 (which runs the oracle) takes the quota.
    torch.set_num_threads(usable_cpus() if rank == 0 else max(1, usable_cpus() // world))

    from boxdreamer_amd import synth
    B, T, prec = args.batch, args.views, args.prec
    # synthetic batch: every rank gets its own shard (different seed), B DISTINCT samples, values pre-rounded to bf16 as
    # the reference dataset does; tensors are bf16 on device (the dataset's `precision`), resident before timing.
    one = synth.make_batch(seed=100 + rank, B=B, T=T)
    images = one["images"].to(torch.bfloat16).to(device)
    bbox = one["bbox_feat"].to(torch.bfloat16).to(device)
    mask = torch.zeros(B, T, dtype=torch.bool, device=device); mask[:, T - 1] = True
    PROGRESS["line"].update(metric="poses/s/GPU (5-ref, 224×224, bf16); heatmap max-abs err vs CPU ref", unit="poses/s",
                            steps=args.steps, warmup=args.warmup)
    PROGRESS["stage"] = "timed steps"

    main_res = measure_mode(prec, args, device, world, rank, dist, images, bbox, mask, keep_outputs=bool(args.dump_outputs))
    if rank == 0 and args.dump_outputs:
        files = dump_outputs(args.dump_outputs, main_res.pop("outputs"))
        print(f"bench: wrote {', '.join(files)} to {args.dump_outputs}", file=sys.stderr, flush=True)
    line = None
    rank_devices = None
    if dist is not None:       # every rank reports the device it ran on (an object collective: all ranks take part)
        rank_devices = [None] * world
        dist.all_gather_object(rank_devices, f"rank {rank}: {torch.cuda.get_device_name(device)} (cuda:{device.index})")
    if rank == 0:
        value, fpp = main_res["value"], main_res["fpp"]
        metric = "poses/s/GPU (5-ref, 224×224, bf16); heatmap max-abs err vs CPU ref"     # BASELINE.json's metric string
        if prec not in ("bf16", STRICT_PREC) or T != 6:      # another mode / view count: say so in the metric itself
            metric = f"poses/s/GPU ({T - 1}-ref, 224×224, {DTYPE_LABEL[prec]}); heatmap max-abs err vs CPU ref"
        if args.cache_refs:
            metric = "poses/s with reference features cached across queries (SURVEY 8f1; encoder on the query crop only)"
        line = {"metric": metric,
                "value": round(value, 2), "unit": "poses/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(main_res["ms_per_step"], 3), "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": DTYPE_LABEL[prec], "data": "synthetic",
                "dtype_note": "the arithmetic type of the MFMA operands; inputs are bf16 in HBM (the dataset's `precision`), accumulation / residual "
                              "statistics / softmax / logits fp32 in every mode",
                "config": {"workload": workload_name(B, T, prec, world, args.cache_refs),
                           "global_batch": B * world, "views": T, "parallelism": f"dp{world}",
                           "hip_graph": main_res["run"].graphed is not None, "gflop_per_pose": round(fpp / 1e9, 2),
                           "batches_in_flight": main_res["in_flight"], "sub_batch_lanes": main_res["sub_lanes"],
                           "sub_batch_lanes_note": "ONE batch at a time; inside the captured step the batch runs as this many contiguous sub-batches "
                                                   "on as many streams (bd_*_forward_lanes, ABI v6; outputs bit-identical to the one-lane form, "
                                                   "asserted on the corners by --full runs); `single_stream` (--full) is the same K steps as one lane "
                                                   "on one stream"},
                "poses_per_s_per_gpu": round(value / world, 2),
                "value_is": "whole-job aggregate over n_gpus (bench contract); the per-GPU figure of the metric is poses_per_s_per_gpu",
                "per_rank_ms_per_step": [round(t / args.steps * 1e3, 3) for t in main_res["per_rank"]],
                "value_mode": prec, "package_default_mode": STRICT_PREC}
        if "roofline" in main_res:
            line["roofline"] = main_res["roofline"]
        if main_res["calibration"].get("applicable"):
            line["calibration"] = main_res["calibration"]
        if "single_stream" in main_res:
            line["single_stream"] = main_res["single_stream"]
            line["value_single_stream"] = main_res["single_stream"]["value"]       # the batch as ONE lane on one stream (rounds 1-3's step)
        if dist is not None:   # what the collective layer itself saw (not the CLI argument): the first SCALE record must prove N ranks
            names = rank_devices
            line["distributed"] = {"backend": dist.get_backend(), "world_size_seen_by_the_collective": dist.get_world_size(),
                                   "nccl_version": ".".join(str(v) for v in torch.cuda.nccl.version()) if args.backend == "nccl" else None,
                                   "devices": names}
        PROGRESS["line"] = dict(line)
    if not args.full:                # a plain run ends with its headline figure
        main_res["run"].close()
        return report(line, rank, dist)
    PROGRESS["stage"] = "corner all-gather latency"
    if dist is not None:
        lat = gather_latency_ms(main_res["run"].kp_all, world, dist, main_res["run"].gather, sync=interruptible_sync(device))
        if rank == 0:
            line["corner_allgather_ms"] = round(lat, 4)
            PROGRESS["line"] = dict(line)
            line["collective"] = f"all_gather_into_tensor of ({B}, 8, 2) fp32 per rank over RCCL (xGMI), once per step"
    PROGRESS["stage"] = "parity / side measurements"
    if rank == 0:
        run = main_res["run"]
        if world == 1 and dist is None and not args.no_rccl_probe and not args.cache_refs and B == 32 and T == 6:
            line["rccl_world1"] = rccl_world1_block()
        if not args.no_parity:
            line["parity"] = parity_probe(prec, T, device, (run.enc, run.dec) if B >= 2 else None)   # a captured B = 1 path is frozen
            line["parity_meets_tolerance"] = line["parity"]["meets_tolerance"]
            line["logits_max_abs_err"] = line["parity"]["logits_max_abs_err"]
        if world == 1 and not args.no_h2d and not args.cache_refs:
            line["h2d_inclusive"] = h2d_inclusive(run, max(4, args.steps))
        if world == 1 and not args.no_pnp:
            line["pnp_inclusive"] = pnp_inclusive(run, one, max(4, args.steps), main_res["ms_per_step"])
        if world == 1 and not args.no_power and run.graphed is not None:
            line["power"] = power_probe(run)
        if world == 1 and args.sustained > 0 and run.graphed is not None and B == 32 and T == 6 and not args.cache_refs:
            PROGRESS["stage"] = "sustained-load leg"
            line["sustained"] = sustained_block(run, args.sustained, main_res["ms_per_step"])
            if line["sustained"].get("last_5s"):
                line["config"].update(sustained_last_5s_poses_per_s=line["sustained"]["last_5s"]["poses_per_s"],
                                      sustained_seconds=line["sustained"]["seconds"])
    main_res["run"].close()
    del main_res

    # ---- the strict mode, same invocation, same inputs (every rank takes part: same barrier / gather structure)
    PROGRESS["stage"] = "strict mode"
    if rank == 0:
        PROGRESS["line"] = dict(line)
    # The OTHER of the two modes of record: `value` is the parity-meeting default mode (round 6), this leg then the bf16 single-pass mode --
    # BASELINE.json's headline dtype, an explicit throughput opt-in that does NOT meet the 1e-3 bar; with `--prec bf16` the roles swap.
    ALT = "bf16" if prec == STRICT_PREC else STRICT_PREC
    alt_key = "strict" if ALT == STRICT_PREC else "bf16_opt_in"
    WHAT = {STRICT_PREC: "the package's DEFAULT mode.  Linears: one f16 MFMA pass + one e4m3 correction pass over a doubled K "
                         "(BD_PREC_F16C8); BETR's QKV Linear split by column: q, k (RMS-normalised right away) as ONE f16 pass, v as "
                         "the full F16C8 product; f16 attention where q/k are RMS-normalised, split-bf16 attention in DINOv2; LayerNorms "
                         "folded into the neighbouring Linears and the residual stream in the 3-byte operand form between them (round 6)",
            "bf16": "one v_mfma_f32_32x32x16_bf16 pass per product: BASELINE.json's headline dtype and the reference's own `precision`; an explicit "
                    "throughput opt-in (hip_precision: bf16) whose logits are ~4e-2 off the fp32 forward -- it does NOT meet north_star's 1e-3 bar"}
    if rank == 0:
        line["value_what"] = WHAT.get(prec)
        if prec == STRICT_PREC:      # the figures of record where the driver's `parsed` shows them
            line["value_meeting_parity"], line["value_meeting_parity_mode"] = line["value"], prec
            if "single_stream" in line:
                line["value_meeting_parity_single_stream"] = line["single_stream"]["value"]
            if "parity" in line:
                line["value_meeting_parity_logits_max_abs_err"] = line["parity"]["logits_max_abs_err"]
                line["value_meeting_parity_meets_tolerance"] = line["parity"]["meets_tolerance"]
    if not args.no_strict and not args.cache_refs:
        torch.cuda.empty_cache()
        sres = measure_mode(ALT, args, device, world, rank, dist, images, bbox, mask)
        if rank == 0:
            srun = sres["run"]
            line[alt_key] = {"mode": ALT, "what": WHAT[ALT],
                             "value": round(sres["value"], 2), "unit": "poses/s",
                             "poses_per_s_per_gpu": round(sres["value"] / world, 2),
                             "ms_per_step": round(sres["ms_per_step"], 3), "dtype": DTYPE_LABEL[ALT],
                             "roofline": sres["roofline"], "batches_in_flight": sres["in_flight"], "sub_batch_lanes": sres["sub_lanes"]}
            line[alt_key]["calibration"] = sres["calibration"]
            if ALT == STRICT_PREC:
                line["value_meeting_parity"] = line["strict"]["value"]
                line["value_meeting_parity_mode"] = STRICT_PREC
            if "single_stream" in sres:
                line[alt_key]["single_stream"] = sres["single_stream"]
                if ALT == STRICT_PREC:
                    line["value_meeting_parity_single_stream"] = sres["single_stream"]["value"]
            if world == 1 and not args.no_power and srun.graphed is not None:
                line[alt_key]["power"] = power_probe(srun)
            if not args.no_parity:
                line[alt_key]["parity"] = parity_probe(ALT, T, device, (srun.enc, srun.dec) if B >= 2 else None)
                if ALT == STRICT_PREC:
                    line["value_meeting_parity_logits_max_abs_err"] = line["strict"]["parity"]["logits_max_abs_err"]
                    line["value_meeting_parity_meets_tolerance"] = line["strict"]["parity"]["meets_tolerance"]
        sres["run"].close()
        del sres
    # ---- the drop-in surface itself: BoxDreamer.forward on the batch dict, default mode
    strict_value = None
    if rank == 0:
        strict_value = line["value"] if prec == STRICT_PREC else line.get("strict", {}).get("value")
    if rank == 0 and world == 1 and strict_value and not args.no_facade and not args.cache_refs and B == 32 and T == 6:
        PROGRESS["stage"] = "facade (BoxDreamer.forward)"
        torch.cuda.empty_cache()
        try:
            line["facade"] = facade_block(args, device, one, STRICT_PREC, strict_value)
            line["config"].update(facade_poses_per_s=line["facade"].get("poses_per_s"))
        except Exception as e:               # noqa: BLE001 -- a side measurement must not take the line down
            line["facade"] = {"error": f"{type(e).__name__}: {e}"}
    # ---- what the default mode costs on a checkpoint with outlier channels: the same step on the trained-like weight set, after the
    # load-time calibration promoted what it had to (one batch at a time; single GPU, default workload only)
    PROGRESS["stage"] = "strict mode on trained-like outlier weights"
    if rank == 0:
        PROGRESS["line"] = dict(line)
    if world == 1 and (prec == STRICT_PREC or not args.no_strict) and not args.no_trained_like and not args.cache_refs and B == 32 and T == 6:
        torch.cuda.empty_cache()
        argsT = argparse.Namespace(**{**vars(args), "in_flight": 1})
        tres = measure_mode(STRICT_PREC, argsT, device, world, rank, dist, images, bbox, mask, weights=TRAINED_LIKE)
        base = (line["value"] if prec == STRICT_PREC and line["config"]["batches_in_flight"] == 1 else
                (line.get("strict", {}).get("value") if line.get("strict", {}).get("batches_in_flight") == 1 else None))
        line["strict_trained_like"] = {"weights": TRAINED_LIKE + " (synth.*_state_dict_outliers: massive-activation channels, LayerNorm gain outliers, "
                                                  "MLP hidden units in the hundreds)", "mode": STRICT_PREC,
                                       "value": round(tres["value"], 2), "unit": "poses/s", "ms_per_step": round(tres["ms_per_step"], 3),
                                       "batches_in_flight": 1, "calibration": tres["calibration"],
                                       "throughput_vs_unpromoted": round(tres["value"] / base, 4) if base else None,
                                       "roofline": {k: tres["roofline"][k] for k in ("achieved", "frac", "whole_path_achieved") if k in tres["roofline"]}}
        if not args.no_parity:
            line["strict_trained_like"]["parity"] = parity_probe(STRICT_PREC, T, device, (tres["run"].enc, tres["run"].dec), weights=TRAINED_LIKE)
        tres["run"].close()
        del tres
    # ---- BASELINE configs[4]: fp8 (e4m3) Linears + bf16 attention at batch 64, single GPU, default workload only (its tolerance is
    # RESTATED: 3 mantissa bits cannot meet 1e-3) -- reported in the same line so the driver's run covers it
    PROGRESS["stage"] = "fp8 leg (configs[4])"
    if rank == 0:
        PROGRESS["line"] = dict(line)
    if world == 1 and not args.no_fp8 and prec != "fp8" and not args.cache_refs and B == 32 and T == 6:
        torch.cuda.empty_cache()
        B8 = 64
        one8 = synth.make_batch(seed=300 + rank, B=B8, T=T)
        img8, bb8 = one8["images"].to(torch.bfloat16).to(device), one8["bbox_feat"].to(torch.bfloat16).to(device)
        mask8 = torch.zeros(B8, T, dtype=torch.bool, device=device); mask8[:, T - 1] = True
        args8 = argparse.Namespace(**{**vars(args), "batch": B8, "in_flight": 1})
        fres = measure_mode("fp8", args8, device, world, rank, dist, img8, bb8, mask8)
        par = parity_probe("fp8", T, device, (fres["run"].enc, fres["run"].dec)) if not args.no_parity else None
        line["fp8"] = {"workload": workload_name(B8, T, "fp8", world, False), "value": round(fres["value"], 2), "unit": "poses/s",
                       "ms_per_step": round(fres["ms_per_step"], 3), "dtype": DTYPE_LABEL["fp8"], "batches_in_flight": 1,
                       "roofline": fres["roofline"],
                       "parity": par,
                       "tolerance_restated": "e4m3 Linears: logits <= 1.0 max-abs and <= 0.2 rms of a unit-rms heatmap at full depth "
                                             "(tests/test_gpu_path.py::test_fp8_mode_restated_tolerance); not a mode that meets the 1e-3 bar"}
        fres["run"].close()
        del fres
    # ---- one pose at a time (B = 1: the reference demo's per-frame call, 1 query + 5 references), both modes, HIP graph; single GPU, default
    # workload only.  A latency figure next to the throughput ones; never `value`.
    PROGRESS["stage"] = "one-pose latency leg (B = 1)"
    if rank == 0:
        PROGRESS["line"] = dict(line)
    if world == 1 and not args.no_latency and not args.cache_refs and B == 32 and T == 6:
        lat = {}
        one1 = synth.make_batch(seed=700, B=1, T=T)
        img1, bb1 = one1["images"].to(torch.bfloat16).to(device), one1["bbox_feat"].to(torch.bfloat16).to(device)
        mask1 = torch.zeros(1, T, dtype=torch.bool, device=device); mask1[:, T - 1] = True
        args1 = argparse.Namespace(**{**vars(args), "batch": 1, "in_flight": 1, "steps": max(args.steps, 30), "warmup": max(args.warmup, 8)})
        for m in dict.fromkeys([prec] + ([] if args.no_strict else [ALT])):
            torch.cuda.empty_cache()
            lres = measure_mode(m, args1, device, world, rank, dist, img1, bb1, mask1)
            lat[m] = {"ms_per_pose": round(lres["ms_per_step"], 3), "poses_per_s": round(lres["value"], 1), "hip_graph": lres["run"].graphed is not None}
            lres["run"].close()
            del lres
            if m in ("f16c8_qk16", "f16c8"):
                # the same call with the OPT-IN latency forms (`hip_latency: true`, ABI 9: split-K residual Linears): the figure of record for
                # one pose at a time; the row above is the throughput forms (bit-identical to the same sample inside any batch)
                torch.cuda.empty_cache()
                argsL = argparse.Namespace(**{**vars(args1), "latency_forms": True})
                lres = measure_mode(m, argsL, device, world, rank, dist, img1, bb1, mask1)
                par = parity_probe(m, T, device, (lres["run"].enc, lres["run"].dec), B=1) if not args.no_parity else None
                lat[m] = {"ms_per_pose": round(lres["ms_per_step"], 3), "poses_per_s": round(lres["value"], 1), "hip_graph": lres["run"].graphed is not None,
                          "forms": "latency forms (hip_latency: true)", "throughput_forms_ms_per_pose": lat[m]["ms_per_pose"],
                          "parity": par}
                lres["run"].close()
                del lres
        line["one_pose_latency"] = {"workload": "B = 1: 1 query + 5 references, 224x224, one forward at a time (HIP graph), inputs resident in HBM",
                                    "modes": lat}
        line["config"].update(one_pose_ms=lat[prec]["ms_per_pose"])
        if STRICT_PREC in lat:
            line["config"].update(parity_mode_one_pose_ms=lat[STRICT_PREC]["ms_per_pose"])
        if "bf16" in lat:
            line["config"].update(bf16_one_pose_ms=lat["bf16"]["ms_per_pose"])
    # ---- BASELINE configs[3]'s per-GPU shard in the same line: 1 query + 16 refs, batch 32 per GPU, headline mode;
    # every rank takes part (same barriers, same corner gather); default for N > 1, `--config3` at N = 1
    PROGRESS["stage"] = "configs[3] leg (T = 17)"
    if rank == 0:
        PROGRESS["line"] = dict(line)
    if (world > 1 or args.config3) and T == 6 and not args.cache_refs:
        torch.cuda.empty_cache()
        T3 = 17
        one3 = synth.make_batch(seed=500 + rank, B=B, T=T3)
        img3, bb3 = one3["images"].to(torch.bfloat16).to(device), one3["bbox_feat"].to(torch.bfloat16).to(device)
        mask3 = torch.zeros(B, T3, dtype=torch.bool, device=device); mask3[:, T3 - 1] = True
        args3 = argparse.Namespace(**{**vars(args), "views": T3, "in_flight": 1})
        cres = measure_mode(prec, args3, device, world, rank, dist, img3, bb3, mask3)
        if rank == 0:
            line["config3"] = {"workload": workload_name(B, T3, prec, world, False), "mode": prec, "value": round(cres["value"], 2), "unit": "poses/s",
                               "poses_per_s_per_gpu": round(cres["value"] / world, 2), "ms_per_step": round(cres["ms_per_step"], 3),
                               "global_batch": B * world, "views": T3, "gflop_per_pose": round(cres["fpp"] / 1e9, 2),
                               "per_rank_ms_per_step": [round(t / args.steps * 1e3, 3) for t in cres["per_rank"]],
                               "sub_batch_lanes": cres["sub_lanes"],
                               "roofline": {k: cres["roofline"][k] for k in ("achieved", "frac", "whole_path_achieved", "whole_path_frac", "attention_achieved")}}
            line["config"].update(config3_value=line["config3"]["value"], config3_ms_per_step=line["config3"]["ms_per_step"],
                                  config3_global_batch=B * world, config3_views=T3)
        cres["run"].close()
        del cres
    if rank == 0:
        if not args.no_cpu_baseline and world == 1:
            line["cpu_baseline"] = cpu_baseline(T)
            line["gpu_over_cpu"] = round(line["value"] / line["cpu_baseline"]["value"], 1)
        # ---- MFMA-busy and HBM traffic of the headline and the default mode, counted IN THIS RUN
        if world == 1 and not args.no_inline_counters and not args.cache_refs:
            PROGRESS["stage"] = "in-run counters (rocprofv3)"
            torch.cuda.empty_cache()
            modes = [prec] + ([ALT] if alt_key in line else [])
            got, why = inline_counters(modes, B, T, args.counter_budget)
            if got:
                apply_counters(line["roofline"], got[prec])
                if alt_key in line:
                    apply_counters(line[alt_key]["roofline"], got[ALT])
            else:
                line["roofline"]["counters_in_this_run_skipped"] = why
            if got and "fp8" in line:                      # the configs[4] leg at ITS batch size (three more passes)
                got8, why8 = inline_counters(["fp8"], 64, T, args.counter_budget)
                if got8:
                    apply_counters(line["fp8"]["roofline"], got8["fp8"])
                else:
                    line["fp8"]["roofline"]["counters_in_this_run_skipped"] = why8
        # ---- the figures of record as flat scalars inside the dicts the driver's record keeps
        par = line.get("parity") or {}
        line["config"].update(value_mode=prec, value_meets_parity=par.get("meets_tolerance"),
                              value_logits_max_abs_err=par.get("logits_max_abs_err"), value_top20_sets_equal_frac=par.get("top20_sets_equal_frac"))
        st = line.get("strict")
        if prec == STRICT_PREC:      # `value` IS the parity mode: the same flat fields, from the headline's own blocks
            st = {"mode": prec, "value": line["value"], "ms_per_step": line["ms_per_step"], "parity": line.get("parity"), "roofline": line["roofline"]}
        bo = line.get("bf16_opt_in")
        if bo:
            bp = bo.get("parity") or {}
            line["config"].update(bf16_value=bo["value"], bf16_ms_per_step=bo["ms_per_step"], bf16_meets_parity=bp.get("meets_tolerance"),
                                  bf16_logits_max_abs_err=bp.get("logits_max_abs_err"), bf16_top20_sets_equal_frac=bp.get("top20_sets_equal_frac"),
                                  bf16_gemm_frac_of_peak=bo["roofline"]["frac"], bf16_mfma_busy_gemm=bo["roofline"].get("mfma_busy_gemm"))
        if st:
            sp, srf = st.get("parity") or {}, st["roofline"]
            line["config"].update(parity_mode=st["mode"], parity_mode_value=st["value"], parity_mode_ms_per_step=st["ms_per_step"],
                                  parity_mode_logits_max_abs_err=sp.get("logits_max_abs_err"), parity_mode_meets_parity=sp.get("meets_tolerance"),
                                  parity_mode_top20_sets_equal_frac=sp.get("top20_sets_equal_frac"))
            line["roofline"].update(parity_mode=st["mode"], parity_mode_value=st["value"], parity_mode_ms_per_step=st["ms_per_step"],
                                    parity_mode_logits_max_abs_err=sp.get("logits_max_abs_err"), parity_mode_achieved=srf["achieved"],
                                    parity_mode_frac=srf["frac"], parity_mode_whole_path_frac=srf["whole_path_frac"],
                                    parity_mode_mfma_busy_gemm=srf.get("mfma_busy_gemm"), parity_mode_mfma_busy_whole_step=srf.get("mfma_busy_whole_step"),
                                    parity_mode_passes_per_flop=srf["mfma_passes_per_algorithmic_flop"],
                                    parity_mode_traffic_over_algorithmic=srf.get("traffic_over_algorithmic"),
                                    parity_mode_counters_measured_in_this_run=srf.get("counters_measured_in_this_run"))
    report(line, rank, dist)


def report(line, rank, dist):
    """Rank 0 prints the line; every rank leaves the process group."""
    if rank == 0:
        PROGRESS["printed"] = True
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
