"""CPU: bench.py's multi-rank entry.  `python bench.py --gpus N` must start N ranks by itself (the round-1 bench parsed
--gpus and ignored it).  Only the launcher / barrier / corner-gather plumbing is exercised here (gloo, world size 2,
`--cpu-plumbing`): the data path has no CPU form and stays GPU-only.  Replaces the reference's pickle + gloo gather
(/root/reference/src/utils/comm.py:179-219)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_bench_spawns_its_own_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--cpu-plumbing",
                        "--steps", "3", "--warmup", "1", "--batch", "4"], capture_output=True, text=True, env=_env(),
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                       # rank 0 prints ONE json line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["gathered_rows"] == 8 and j["gather_ok"] and j["steps"] == 3
    assert len(j["per_rank_ms_per_step"]) == 2


def test_world_size_must_match_gpus():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--cpu-plumbing"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in (r.stderr + r.stdout)


def _plumb(n, *extra, timeout=900):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "gloo", "--cpu-plumbing",
                           "--steps", "3", "--warmup", "1", "--batch", "4", "--dist-timeout", "120", *extra],
                          capture_output=True, text=True, env=_env(), timeout=timeout)


def _one_line(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(lines[0])


def test_world4_and_world8_ragged_seeds_and_lane_agreement():
    """VERDICT r2 item 7 (no multi-GPU hardware this round: harden what a CPU can check).  World sizes 4 and 8 (the driver's
    N = 4 / 8 sweeps): every rank's seeded shard differs, the in-flight lane count is agreed with all_reduce(MIN) when ONE rank can
    only offer one lane (bench.py ModeRun), a global batch that does not divide by the world size gathers in order, and the
    corner all-gather latency is reported."""
    for n, short, G in ((4, 2, 10), (8, 5, 29)):
        r = _plumb(n, "--plumbing-short-rank", str(short), "--plumbing-global-batch", str(G))
        assert r.returncode == 0, r.stderr[-2000:]
        j = _one_line(r)
        assert j["n_gpus"] == n and j["gathered_rows"] == 4 * n and j["gather_ok"]
        assert j["per_rank_seeds_distinct"] and j["lanes_agreed"] == 1 and j["ragged_ok"] is True
        assert len(j["per_rank_ms_per_step"]) == n and j["corner_allgather_ms"] > 0


def test_rank_failure_still_yields_one_line_and_nonzero_rc():
    """A rank that dies must not hang the sweep, and rank 0 must still print ONE JSON line with n_gpus (+ what was measured so
    far) and `error`; the launch exits non-zero.  Rank 2 of 4 dies before the timed region / rank 0 itself dies after it."""
    r = _plumb(4, "--plumbing-fail-rank", "2", "--plumbing-fail-stage", "before_timed")
    assert r.returncode != 0
    j = _one_line(r)
    assert j["n_gpus"] == 4 and j["value"] is None and "error" in j and "injected failure on rank 2" in r.stderr
    r = _plumb(4, "--plumbing-fail-rank", "0", "--plumbing-fail-stage", "after_timed")
    assert r.returncode != 0
    j = _one_line(r)
    assert j["n_gpus"] == 4 and len(j["per_rank_ms_per_step"]) == 4 and "injected failure on rank 0" in j["error"]
    assert j["failed_stage"] == "after_timed"


def test_dry_run_prints_the_launch_plan_and_ports_do_not_collide():
    plans = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "5", "--dry-run"],
                           capture_output=True, text=True, env=_env(), timeout=300)
        assert r.returncode == 0, r.stderr[-1000:]
        plans.append(json.loads(r.stdout.strip().splitlines()[-1]))
    p = plans[0]
    assert p["ranks"] == 8 and p["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and p["env"]["MASTER_ADDR"] == "127.0.0.1"
    cmd = p["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and "--dry-run" not in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    port = int(cmd[cmd.index("--master-port") + 1])
    assert 1024 < port < 65536 and str(port) == p["env"]["MASTER_PORT"]
    # a MASTER_PORT given by the caller is honoured (the driver passes its own --master-port to torch.distributed.run)
    env = _env(); env["MASTER_PORT"] = "23456"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert json.loads(r.stdout.strip().splitlines()[-1])["env"]["MASTER_PORT"] == "23456"


def test_workload_label_names_the_config_actually_run():
    """config.workload said "configs[1]" for every --views / --batch."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert m.workload_name(32, 6, "bf16", 1, False).startswith("configs[1]:")
    assert m.workload_name(32, 6, "f16c8_qk16", 8, False).startswith("configs[1]:")
    assert m.workload_name(32, 17, "bf16", 8, False).startswith("configs[3]:")
    assert m.workload_name(32, 17, "bf16", 1, False).startswith("configs[3] shape")
    assert m.workload_name(64, 6, "fp8", 1, False).startswith("configs[4]:")
    assert m.workload_name(1, 6, "bf16", 1, False).startswith("custom")
    assert m.workload_name(32, 6, "bf16", 1, True).startswith("SURVEY 8f1")
    # algorithmic GEMM bytes: 101 bd_gemm calls per step at T = 6, ~0.4 GB per call in bf16, more in the strict classes
    b16, calls = m.algorithmic_gemm_bytes("bf16", 32, 6)
    bs, _ = m.algorithmic_gemm_bytes("f16c8", 32, 6)
    assert calls == 101 and m.algorithmic_gemm_bytes("f16c8_qk16", 32, 6)[1] == 113 and 3.5e8 < b16 / calls < 4.5e8 and b16 < bs < 2 * b16


import pytest


@pytest.mark.gpu
def test_two_rank_flow_with_the_real_kernels_on_one_gpu():
    """The N > 1 flow of bench.py -- per-rank seeded shards, in-flight lane agreement, barrier-bracketed timed steps, max over ranks,
    corner gather every step, gather-latency probe -- executed with the REAL kernels by two ranks that share cuda:0
    (`--single-device-test`: collectives through gloo, since RCCL refuses two ranks on one device).  Not a measurement and not RCCL;
    it is the only multi-rank GPU execution a 1-GPU box allows, and what the driver's multi-GPU sweep runs except for the backend."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--single-device-test",
                        "--steps", "2", "--warmup", "1", "--full", "--no-strict", "--no-fp8", "--no-cpu-baseline", "--no-h2d", "--no-pnp", "--no-parity",
                        "--dist-timeout", "300"], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _one_line(r)
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 64 and j["config"]["parallelism"] == "dp2"
    assert len(j["per_rank_ms_per_step"]) == 2 and j["corner_allgather_ms"] > 0 and j["value"] > 0
    assert j["config"]["workload"].startswith("configs[1]:")
    # the same command emits BASELINE configs[3]'s per-GPU shard next to the weak-scaled configs[1] value
    c3 = j["config3"]
    assert c3["views"] == 17 and c3["global_batch"] == 64 and c3["value"] > 0 and len(c3["per_rank_ms_per_step"]) == 2
    assert c3["workload"].startswith("configs[3] shape") and j["config"]["config3_value"] == c3["value"]
    assert j["distributed"]["world_size_seen_by_the_collective"] == 2


@pytest.mark.gpu
def test_single_gpu_line_carries_the_parity_mode_and_counters_of_this_run():
    """The driver's record keeps `config`, `roofline` and `cpu_baseline` of the line (scalars only).  Round 6: `value` IS the parity-meeting
    default mode (the bf16 headline failed the bar); its figures are flat scalars there, the bf16 single-pass mode is
    the `bf16_opt_in` block + flat `config.bf16_*` scalars, and MFMA-busy / traffic come from counters measured in THIS run when rocprofv3
    is on the box -- else from the stamped file, and the line says which.  The facade and the RCCL world-1 probe ride in the same line."""
    import shutil
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-fp8", "--no-trained-like",
                        "--no-cpu-baseline", "--no-h2d", "--no-pnp", "--no-power", "--sustained", "6"], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _one_line(r)
    cfg, rf = j["config"], j["roofline"]
    assert j["value_mode"] == "f16c8_qk16" and cfg["value_mode"] == "f16c8_qk16" and cfg["value_meets_parity"] is True
    assert j["metric"].startswith("poses/s/GPU (5-ref") and j["config"]["workload"].startswith("configs[1]:")
    assert cfg["parity_mode"] == "f16c8_qk16" and cfg["parity_mode_meets_parity"] is True and cfg["parity_mode_top20_sets_equal_frac"] == 1.0
    assert cfg["parity_mode_value"] == j["value"] == j["value_meeting_parity"] and cfg["value_logits_max_abs_err"] <= 5e-4
    assert cfg["bf16_value"] > j["value"] and cfg["bf16_meets_parity"] is False and cfg["bf16_logits_max_abs_err"] > 1e-3
    assert j["bf16_opt_in"]["mode"] == "bf16" and j["bf16_opt_in"]["value"] == cfg["bf16_value"]
    assert rf["parity_mode"] == "f16c8_qk16" and rf["parity_mode_value"] == j["value"] and 0 < rf["frac"] == rf["parity_mode_frac"] < cfg["bf16_gemm_frac_of_peak"] < 1
    assert rf["parity_mode_passes_per_flop"] == 1.93 and rf["bound"] == "mfma" and rf["peak"] == 2500.0
    # one pose at a time (B = 1) of both modes, as flat scalars too: a latency far below a batch's step, the parity mode the slower one
    lat = j["one_pose_latency"]["modes"]
    assert cfg["one_pose_ms"] == cfg["parity_mode_one_pose_ms"] == lat["f16c8_qk16"]["ms_per_pose"] and cfg["bf16_one_pose_ms"] == lat["bf16"]["ms_per_pose"]
    assert 0.5 < cfg["bf16_one_pose_ms"] < cfg["parity_mode_one_pose_ms"] < j["ms_per_step"]
    # the drop-in surface, the sustained leg and the RCCL world-1 probe
    fa = j["facade"]
    assert fa["outputs_bit_identical_eager_vs_graph"] is True and fa["corners_identical_with_pnp_on_device"] is True
    assert 0.85 < fa["hip_graph"]["vs_parity_mode_value"] <= 1.02 and len(fa["host_syncs_per_forward"]) == 1
    assert fa["hip_graph_pnp_on_device"]["host_syncs_per_forward"] == []
    su = j["sustained"]
    assert su["seconds"] >= 6 and su["first_5s"]["poses_per_s"] > 0 and isinstance(su["steady_state"], str)
    assert j["rccl_world1"]["executed"] and j["rccl_world1"]["world_size_seen_by_the_collective"] == 1
    if rf["counters_measured_in_this_run"]:
        assert shutil.which("rocprofv3") and rf["parity_mode_counters_measured_in_this_run"] is True
        assert rf["traffic_source"].startswith("measured in THIS run") and len(rf["counter_pass_seconds"]) == 3
        assert 0.3 < rf["mfma_busy_gemm"] < 0.9 and 0.3 < j["bf16_opt_in"]["roofline"]["mfma_busy_gemm"] < 0.9
        assert 1.0 <= rf["traffic_over_algorithmic"] < 3.0 and rf["traffic"] > rf["algorithmic_bytes_per_launch"]
    else:       # no rocprofv3 on this box, or its passes failed / ran out of their time budget: the line must say why (and falls back to the stamped file)
        print("in-run counters skipped:", rf.get("counters_in_this_run_skipped"))
        assert isinstance(rf.get("counters_in_this_run_skipped"), str) and rf["counters_in_this_run_skipped"]


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A run without --full times the K steps of the headline mode and nothing else; --dump-outputs writes the last timed step's
    corners and (graphed step) heat maps as float32 .npy files."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _one_line(r)
    assert j["steps"] == 3 and j["value"] > 0 and j["unit"] == "poses/s" and j["higher_is_better"] is True
    assert j["dtype"] and j["metric"].startswith("poses/s/GPU (5-ref") and 0 < j["ms_per_step"] == j["per_rank_ms_per_step"][0]
    assert abs(j["value"] - 32 * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
    for k in ("roofline", "parity", "bf16_opt_in", "strict", "facade", "one_pose_latency", "cpu_baseline", "sustained", "single_stream"):
        assert k not in j, k
    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(out) == ["corners_norm", "corners_px", "heat"]
    assert out["corners_px"].shape == out["corners_norm"].shape == (32, 8, 2) and out["heat"].shape == (32, 8, 224, 224)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert np.abs(out["heat"]).max() <= 1.0 and (out["corners_px"] >= 0).all() and (out["corners_px"] < 224).all()


def test_dump_outputs_float32_under_the_size_limit(tmp_path):
    """--dump-outputs: float32 files, at most 64 MB in all; an array that does not fit keeps the same seeded sample of its rows."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    rng = np.random.default_rng(5)
    arrays = {"heat": rng.standard_normal((48, 8, 224, 224), dtype=np.float32), "corners_px": rng.uniform(0, 224, (48, 8, 2))}
    for d in ("a", "b"):
        assert b.dump_outputs(str(tmp_path / d), arrays) == ["corners_px.npy", "heat.npy"]
    files = [tmp_path / d / f for d in ("a", "b") for f in ("corners_px.npy", "heat.npy")]
    assert sum(os.path.getsize(f) for f in files[:2]) <= 64e6
    a = [np.load(f) for f in files]
    assert all(x.dtype == np.float32 for x in a) and np.array_equal(a[0], arrays["corners_px"].astype(np.float32))
    assert 0 < a[1].shape[0] < 48 and a[1].shape[1:] == (8, 224, 224) and np.array_equal(a[1], a[3])
    rows = [i for i in range(48) if any(np.array_equal(arrays["heat"][i], h) for h in a[1][:3])]
    assert len(rows) == 3 and rows == sorted(rows)


@pytest.mark.gpu
def test_rank_failure_on_the_gpu_box_is_reported():
    """`--gpus 2` on a box with ONE GPU: rank 1 cannot take cuda:1 and dies while rank 0 blocks in the RCCL rendezvous (a C++ call).
    The launch must end at once with ONE JSON line carrying n_gpus and `error`, and a non-zero rc (the sigwait watcher of bench.py)."""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("needs a box with exactly one GPU")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dist-timeout", "120"],
                       capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode != 0
    j = _one_line(r)
    assert j["n_gpus"] == 2 and j["value"] is None and "error" in j


def test_counter_passes_attribute_only_the_marked_steps(tmp_path, monkeypatch):
    """bench.py's in-run counter measurement: one child process runs several modes, each mode's measured steps
    bracketed by a marker kernel; the parser must attribute exactly those dispatches (not packing / calibration / warm-up) to the
    mode, per kernel class, and apply the gfx950 FETCH_SIZE correction.  Fed with a synthetic rocprofv3 CSV (no GPU)."""
    import csv
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    steps = 2

    def fake_pass(group, child, timeout_s=600):
        assert "--counter-child" in child and child[child.index("--counter-child") + 1] in ("bf16,f16c8_qk16", "f16c8_qk16,bf16")
        path = tmp_path / ("_".join(group) + ".csv")
        rows, did = [], 0

        def disp(name, values, dur=1000):
            nonlocal did
            did += 1
            for c in group:
                rows.append({"Dispatch_Id": did, "Kernel_Name": name, "Counter_Name": c, "Counter_Value": values.get(c, 0.0),
                             "Start_Timestamp": did * 10000, "End_Timestamp": did * 10000 + dur})
        for mode_scale in (1.0, 2.0):                              # two modes: the second moves twice the bytes
            disp("void at::native::pack_kernel", {"FETCH_SIZE": 999, "WRITE_SIZE": 999})             # load-time packing: not counted
            disp("gemm_kernel_pc<warmup>", {"FETCH_SIZE": 777, "SQ_VALU_MFMA_BUSY_CYCLES": 5e5, "SQ_BUSY_CYCLES": 1e3})   # warm-up: not counted
            disp("void at::native::erfinv_kernel", {})
            for _ in range(steps):
                disp("gemm_kernel_pc<x>", {"FETCH_SIZE": 100 * mode_scale, "WRITE_SIZE": 50 * mode_scale,
                                           "SQ_VALU_MFMA_BUSY_CYCLES": 512.0 * 1024, "SQ_BUSY_CYCLES": 32.0 * 1024,
                                           "TCC_EA0_RDREQ_32B_sum": 16, "TCC_EA0_RDREQ_64B_sum": 8, "TCC_EA0_RDREQ_128B_sum": 1592 * mode_scale,
                                           "TCC_EA0_RDREQ_sum": 1616}, dur=2000)
                disp("attn_kernel<y>", {"FETCH_SIZE": 10, "WRITE_SIZE": 5, "SQ_VALU_MFMA_BUSY_CYCLES": 256.0 * 1024, "SQ_BUSY_CYCLES": 32.0 * 1024})
                disp("decode_kernel<true>", {})
            disp("void at::native::erfinv_kernel", {})
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader(); w.writerows(rows)
        return str(path)

    monkeypatch.setattr(b, "_rocprof_pass", fake_pass)
    res = b.collect_counters(["bf16", "f16c8_qk16"], 32, 6, b.BASIC_GROUPS, steps=steps)
    g1, g2 = res["bf16"]["per_kernel_class"]["gemm"], res["f16c8_qk16"]["per_kernel_class"]["gemm"]
    assert g1["launches_per_step"] == 1 and g1["fetch_bytes_per_step"] == 2 * 100 * 1024 and g1["write_bytes_per_step"] == 50 * 1024
    assert g2["fetch_bytes_per_step"] == 2 * g1["fetch_bytes_per_step"]
    assert g1["mfma_busy"] == 0.5 and res["bf16"]["per_kernel_class"]["attention"]["mfma_busy"] == 0.25
    assert g1["ms_per_step"] == 0.002 and "harness (one-off torch / runtime kernels: weight packing, uploads)" not in res["bf16"]["per_kernel_class"]
    calls = res["bf16"]["gemm_calls_per_step"]
    assert res["bf16"]["gemm_hbm_bytes_per_call"] == round((2 * 100 + 50) * 1024 / calls)
    # the optional request-size pass: bytes summed by size, next to (never instead of) the corrected FETCH_SIZE
    assert "fetch_by_request_size" not in g1
    res4 = b.collect_counters(["bf16", "f16c8_qk16"], 32, 6, list(b.BASIC_GROUPS) + [b.REQSIZE_COUNTERS], steps=steps)
    q = res4["bf16"]["per_kernel_class"]["gemm"]["fetch_by_request_size"]
    assert q["bytes_per_step"] == 32 * 16 + 64 * 8 + 128 * 1592 == 2 * 100 * 1024 and q["over_corrected_FETCH_SIZE"] == 1.0
    assert res4["bf16"]["per_kernel_class"]["gemm"]["fetch_bytes_per_step"] == g1["fetch_bytes_per_step"]
    # a roofline block takes the figures over and says where they came from
    rf = {"traffic": None, "mfma_busy": None}
    res["bf16"]["measured_in_this_run"] = True
    b.apply_counters(rf, res["bf16"])
    assert rf["counters_measured_in_this_run"] is True and rf["mfma_busy_gemm"] == 0.5 and rf["traffic_source"].startswith("measured in THIS run")
    # a child that dies between the markers must not yield half a measurement
    def broken(group, child, timeout_s=600):
        p = fake_pass(group, child)
        lines = open(p).read().splitlines()
        open(p, "w").write("\n".join(lines[: len(lines) // 2]) + "\n")
        return p
    monkeypatch.setattr(b, "_rocprof_pass", broken)
    with pytest.raises(RuntimeError):
        b.collect_counters(["bf16", "f16c8_qk16"], 32, 6, b.BASIC_GROUPS, steps=steps)


def test_power_probe_degrades_without_a_card():
    """bench.py's board-power block reads the amdgpu hwmon node of the HIP device; where there is none (this CPU container, a box that hides
    sysfs) it must say so instead of raising."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    assert b._hwmon_of(torch.device("cpu")) is None or isinstance(b._hwmon_of(torch.device("cpu")), str)

    class _Run:
        device = torch.device("cpu")
    if b._hwmon_of(_Run.device) is None:
        rep = b.power_probe(_Run())
        assert rep["available"] is False and "why" in rep
