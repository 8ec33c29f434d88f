"""The pose stream that chooses its references on the device, measured: one call per frame for an object that comes with a DATABASE
of posed views (N = 32), k = 5 of which the decoder reads.

    python tools/stream_select_bench.py [--prec f16c8_qk16] [--rounds 10] [--calls 20] [--out profiles/pose_stream_select.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers), default mode, one 480 x 640 uint8 frame per call from pinned host
memory.  Legs, alternated inside one run (every round runs `calls` calls of every leg, rounds x calls >= 200 calls per leg), every leg
warmed up, host wall time PER CALL, every call ending in its own wait:
  (a)  `PoseStream.step` over FIXED references, T = k + 1 (the first k views of the database): the floor -- the difference to it is
       what selection costs;
  (b)  `PoseStream(select_k=k, select="dino").step`: the references chosen by appearance every frame;
  (c)  `PoseStream(select_k=k, select="track").step` in steady state: chosen by distance to the last frame's pose;
  (d)  the eager banked dense facade forward (`dense_cfg.enable`, filter = 'dino', `filter_topk` = k, `pnp_on_device: "wave"`) from
       `frames` + `crop_boxes` over the same bank: what a caller had per frame before the selecting stream -- the pinned frame's H2D,
       square_bbox and crop_intrinsics (torch), `model(batch)`, the pose's read-back.
At B = 1 with and without the latency forms (`hip_latency: true`), and once at the larger batch (default forms).  The figures are the
median and the 10th to 90th percentile over a leg's calls.  bd_match_view_sums + bd_stream_select_rows are also timed back to back
with events, at N = 32 and N = 1024."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, hip_ops, synth                   # noqa: E402
from boxdreamer_amd import preprocess as pp                        # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from boxdreamer_amd.stream import PoseStream                      # noqa: E402
from stream_bench import build, pct, timed                         # noqa: E402

H, W, S = 480, 640, 224
THRESHOLD = 0.05


def view_poses(n, seed):
    """n seeded poses on a ring around the object, looking at it from 4 m: a database's views."""
    r = np.random.default_rng(seed)
    out = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a, e = 2 * np.pi * i / n, r.uniform(-0.4, 0.4)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(e), -np.sin(e)], [0, np.sin(e), np.cos(e)]])
        out[i, :3, :3] = Rx @ Ry
        out[i, :3, 3] = [r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05), 4.0]
        out[i, 3, 3] = 1.0
    return torch.from_numpy(out)


class Flavour:
    """One model (plain or with the latency forms), one bank that holds every object's database, and the legs on it.  Everything
    eager runs once at its largest shape BEFORE the first capture: a live graph freezes the modules' workspaces."""

    def __init__(self, a, latency, batches):
        N, k = a.refs, a.topk
        self.N, self.k, self.T = N, k, N + 1
        self.model = model = build(a.prec, a.dino_depth, a.betr_depth, latency)
        self.dense = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": k, "multi_round": False}
        big = max(batches)
        warm = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in synth.make_batch(seed=a.seed, B=big, T=k + 1).items()}
        model(warm)                                                      # (the first forward runs the load-time calibration, once)
        self.bank = bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder, match_threshold=THRESHOLD, keep_poses=True)
        self.db = []
        for b in range(big):
            views = synth.make_batch(seed=a.seed + 10 + b, B=1, T=N)
            self.db.append(bank.add(views["images"][0].cuda(), bbox_feat=views["bbox_feat"][0].cuda(), poses=view_poses(N, a.seed + b).cuda()).tolist())
        g = torch.Generator().manual_seed(a.seed)
        self.frame = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
        dets = [[180.0, 100.0, 420.0, 330.0], [20.5, 30.0, 250.0, 240.5], [380.0, 200.0, 630.0, 470.0], [250.0, 10.0, 500.0, 250.0]]
        self.det = {b: torch.tensor([dets[i % 4] for i in range(b)]).pin_memory() for b in batches}
        K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
        self.K = {b: K.repeat(b, 1, 1).pin_memory() for b in batches}
        self.banked, bbox_3d = {}, {}
        for b in batches:
            full = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in synth.make_batch(seed=a.seed + b, B=b, T=N + 1).items()}
            bbox_3d[b] = full["bbox_3d"][:, N].clone()
            base = {k_: v for k_, v in full.items() if k_ not in ("images", "bbox_feat")}
            base["crop_boxes"] = torch.tensor([0, 0, 16, 16], dtype=torch.int32, device="cuda").repeat(b, N + 1, 1)
            base["frame_idx"] = torch.zeros((b, N + 1), dtype=torch.int32, device="cuda")
            base["non_ndc_intrinsics"] = base["non_ndc_intrinsics"].clone()
            base.update(ref_bank=bank, ref_rows=[r + [-1] for r in self.db[:b]])
            self.banked[b] = base
        for b in sorted(batches, reverse=True):
            self.eager_dense(b)
        kw = dict(frame_shape=(H, W))
        self.fixed = {b: PoseStream(model, bank, [r[:k] for r in self.db[:b]], bbox_3d[b], **kw) for b in batches}
        self.dino = {b: PoseStream(model, bank, self.db[:b], bbox_3d[b], select_k=k, select="dino", **kw) for b in batches}
        self.track = {b: PoseStream(model, bank, self.db[:b], bbox_3d[b], select_k=k, select="track", **kw) for b in batches}

    def eager_dense(self, b):
        m, T = self.model, self.T
        m.dense_cfg = self.dense
        try:
            base = self.banked[b]
            win = pp.square_bbox(self.det[b].cuda(non_blocking=True), 0.1)
            base["crop_boxes"][:, T - 1] = win
            base["non_ndc_intrinsics"][:, T - 1] = pp.crop_intrinsics(self.K[b].cuda(non_blocking=True), win, S)
            out = m(dict(base, frames=self.frame.cuda(non_blocking=True)))
            return out["pred_poses"][:, -1].cpu(), out["dense_ref_slots"]
        finally:
            m.dense_cfg = {"enable": False}

    def step(self, sessions, b):
        return sessions[b].step(self.frame, self.det[b], self.K[b])[:, :16]


def select_us(N, k, n=100):
    """bd_match_view_sums (one query crop) + bd_stream_select_rows (one object, both value arrays, the pose rule) back to back: device
    microseconds per pair, from events around n pairs."""
    g = torch.Generator().manual_seed(N)
    L, D = 256, 768
    feats, crops = torch.randn((1, L, D), generator=g).cuda(), torch.rand((1, 3, S, S), generator=g).cuda()
    sums, counts = torch.randn((N, D), generator=g).cuda(), torch.randint(1, L, (N,), generator=g).float().cuda()
    poses = view_poses(N, N).cuda()
    prev = torch.zeros((1, _lib.STREAM_ROW_FLOATS), device="cuda")
    prev[0, :16], prev[0, 17] = poses[N // 2].reshape(16), 1.0
    rows = torch.arange(N, dtype=torch.int32, device="cuda")[None]
    n_refs, force = torch.tensor([N], dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    q = hip_ops.match_view_sums(feats, crops, THRESHOLD)
    out = hip_ops.stream_select_rows(sums, counts, poses, N, *q, prev, rows, n_refs, force, L, k, _lib.STREAM_SELECT_TRACK)

    def pair():
        hip_ops.match_view_sums(feats, crops, THRESHOLD, *q)
        hip_ops.stream_select_rows(sums, counts, poses, N, *q, prev, rows, n_refs, force, L, k, _lib.STREAM_SELECT_TRACK, float("inf"), *out)

    for _ in range(10):
        pair()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        pair()
    e1.record()
    e1.synchronize()
    assert int(out[2][0]) == 1
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4, help="the larger batch the legs are also measured at (default forms)")
    ap.add_argument("--refs", type=int, default=32, help="N: views in every object's database")
    ap.add_argument("--topk", type=int, default=5, help="k: views the decoder reads")
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--prec", default=_lib.DEFAULT_PREC)
    ap.add_argument("--dino-depth", type=int, default=12)
    ap.add_argument("--betr-depth", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit the measured tree sits on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    if a.rounds * a.calls < 200:
        ap.error("rounds x calls must be at least 200 calls per leg")
    _lib.require_gpu()
    B, N, k = a.batch, a.refs, a.topk
    plain, lat = Flavour(a, False, (1, B)), Flavour(a, True, (1,))
    # what the legs compute, looked at once outside the timed calls: the "dino" stream selects what the dense forward selects and gives
    # its pose bit for bit; the "track" stream's steady state is the pose rule
    same = []
    for f, bs in ((plain, (1, B)), (lat, (1,))):
        for b in bs:
            pose, slots = f.eager_dense(b)
            got = f.step(f.dino, b).reshape(b, 4, 4).clone()
            same.append(bool(torch.equal(got, pose)) and bool(torch.equal(f.dino[b].sel.long(), slots.long())))
    legs = {}
    for sfx, f, b in (("", plain, 1), ("_lat", lat, 1), (f"_B{B}", plain, B)):
        legs.update({"a" + sfx: (lambda f=f, b=b: f.step(f.fixed, b)), "b" + sfx: (lambda f=f, b=b: f.step(f.dino, b)),
                     "c" + sfx: (lambda f=f, b=b: f.step(f.track, b)), "d" + sfx: (lambda f=f, b=b: f.eager_dense(b)[0])})
    times = timed(legs, a.rounds, a.calls, a.warmup)

    def used_after_a_step(f, b):
        f.step(f.track, b)
        return f.track[b].used.tolist()

    by_pose = {sfx: [used_after_a_step(f, b) for _ in range(5)] for sfx, f, b in (("", plain, 1), ("_lat", lat, 1), (f"_B{B}", plain, B))}
    kernels = {n: select_us(n, k) for n in (32, 1024)}
    stat = {key: (statistics.median(v), pct(v, 10), pct(v, 90)) for key, v in times.items()}
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    props = torch.cuda.get_device_properties(0)
    what = {"a": f"(a) `PoseStream.step`, fixed references, T = {k + 1}", "b": '(b) `PoseStream.step`, `select="dino"`',
            "c": '(c) `PoseStream.step`, `select="track"`, steady state',
            "d": f"(d) eager banked dense facade forward, `frames` + `crop_boxes`, `filter_topk` = {k}, wave PnP"}

    def section(title, sfx):
        out = [f"## {title}", "", "| leg | median ms per call | p10 | p90 | calls |", "|---|---|---|---|---|"]
        for key in "abcd":
            m, lo, hi = stat[key + sfx]
            out.append(f"| {what[key]} | {m:.3f} | {lo:.3f} | {hi:.3f} | {len(times[key + sfx])} |")
        fl, d = stat["a" + sfx][0], stat["d" + sfx]
        for key in "bc":
            m, lo, hi = stat[key + sfx]
            out += ["", f"({key}) costs {m - fl:+.3f} ms over the floor (a) at the median.  ({key}) below (d) by more than the run's own spread "
                        f"(p90 of ({key}) under p10 of (d)): **{hi < d[1]}** -- median {m:.3f} against {d[0]:.3f} ms, ({key}) / (d) = {m / d[0]:.3f}."]
        out += ["", f"`used` of the \"track\" session in five further calls (1 = the pose rule chose): {by_pose[sfx]}.", ""]
        return out

    lines = [
        "# Pose stream: each frame's references chosen on the device",
        "",
        f"`tools/stream_select_bench.py --batch {B} --refs {N} --topk {k} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} "
        f"--betr-depth {a.betr_depth} --rounds {a.rounds} --calls {a.calls}` on {torch.cuda.get_device_name(0)} "
        f"({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; parent commit of the measured "
        f"tree: `{commit}`.  A database of N = {N} views per object, k = {k}, one {H} x {W} uint8 frame per call from pinned host memory, host "
        "wall time per call, every call ends in its own wait (the legs are described at the top of the tool).  The legs alternate inside "
        "every round.",
        "",
        f"The \"dino\" stream selects the slots the eager dense forward selects and gives its pose bit for bit, in every flavour and batch "
        f"measured here: **{all(same)}**.",
        "",
    ]
    lines += section("B = 1, default forms", "")
    lines += section("B = 1, latency forms (`hip_latency: true`)", "_lat")
    lines += section(f"B = {B}, default forms", f"_B{B}")
    lines += ["## The two selection launches alone", "",
              "bd_match_view_sums (one query crop, L = 256, D = 768) + bd_stream_select_rows (one object, both value arrays, the pose rule), "
              "back to back on one stream, device time from events around 100 pairs:", "",
              "| N | microseconds per pair |", "|---|---|"]
    lines += [f"| {n} | {us:.1f} |" for n, us in kernels.items()]
    lines += ["", "Not measured here: device time of whole steps (the legs are host wall times of whole calls), other frame sizes, other k, "
                  "a device-resident frame source, more than one session per process."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
