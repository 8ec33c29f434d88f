"""The pose stream that follows each object's box from its own last pose, measured: does taking the box from the last pose
(`track_boxes=True`: bd_stream_track_windows in place of bd_stream_windows, five more floats per object in the step's one D2H) cost
anything against the same step with the boxes given from outside?

    python tools/stream_track_bench.py [--prec f16c8_qk16] [--rounds 10] [--calls 20] [--out profiles/pose_stream_track.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers), default mode, one 480 x 640 uint8 frame per call from pinned host
memory.  Legs, alternated inside one run (every round runs `calls` calls of every leg, rounds x calls >= 200 calls per leg), every leg
warmed up, host wall time PER CALL, every call ending in its own wait:
  (a)  `PoseStream.step` over FIXED references (T = k + 1) with the boxes given: the parent's path;
  (b)  the same session built with `track_boxes=True`, stepped with `det_boxes=None`;
  (c)  `PoseStream(select_k=k, select="track").step` with the boxes given;
  (d)  the same session built with `track_boxes=True`, stepped with `det_boxes=None`.
At B = 1 and at the larger batch.  The figures are the median and the 10th to 90th percentile over a leg's calls.  The expectation --
the tracking step costs nothing measurable -- is checked against the parent leg OF THE SAME RUN: the tracking leg's median should lie
within the parent leg's own p10-p90 spread.  What is written down is what was measured, whichever way it falls.  The two first-node
kernels are also timed back to back with events.

Not measured: tracking ACCURACY on real sequences.  The synthetic model's poses say nothing about it; which source a box had in the
timed calls is reported only to say what the kernel was deciding while it was timed."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, hip_ops, synth                   # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from boxdreamer_amd.stream import PoseStream                      # noqa: E402
from stream_bench import build, pct, timed                         # noqa: E402
from stream_select_bench import THRESHOLD, view_poses              # noqa: E402

H, W, S = 480, 640, 224


class Legs:
    """One model, one bank that holds every object's database, and the four sessions per batch size."""

    def __init__(self, a, batches):
        N, k = a.refs, a.topk
        self.model = model = build(a.prec, a.dino_depth, a.betr_depth, False)
        big = max(batches)
        model({k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in synth.make_batch(seed=a.seed, B=big, T=k + 1).items()})
        self.bank = bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder, match_threshold=THRESHOLD, keep_poses=True)
        db = []
        for b in range(big):
            views = synth.make_batch(seed=a.seed + 10 + b, B=1, T=N)
            db.append(bank.add(views["images"][0].cuda(), bbox_feat=views["bbox_feat"][0].cuda(), poses=view_poses(N, a.seed + b).cuda()).tolist())
        g = torch.Generator().manual_seed(a.seed)
        self.frame = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
        dets = [[180.0, 100.0, 420.0, 330.0], [20.5, 30.0, 250.0, 240.5], [380.0, 200.0, 630.0, 470.0], [250.0, 10.0, 500.0, 250.0]]
        self.det = {b: torch.tensor([dets[i % 4] for i in range(b)]).pin_memory() for b in batches}
        K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
        self.K = {b: K.repeat(b, 1, 1).pin_memory() for b in batches}
        self.sessions = {}
        for b in sorted(batches, reverse=True):             # (the largest first: a live graph freezes the modules' workspaces)
            bbox_3d = synth.make_batch(seed=a.seed + b, B=b, T=2)["bbox_3d"][:, 1].cuda()
            fixed, kw = [r[:k] for r in db[:b]], dict(frame_shape=(H, W))
            sel = dict(select_k=k, select="track", **kw)
            self.sessions[b] = {"a": PoseStream(model, bank, fixed, bbox_3d, **kw), "b": PoseStream(model, bank, fixed, bbox_3d, track_boxes=True, **kw),
                                "c": PoseStream(model, bank, db[:b], bbox_3d, **sel), "d": PoseStream(model, bank, db[:b], bbox_3d, track_boxes=True, **sel)}
            for key in "bd":                                # the tracking sessions start from a detection, as a live caller would
                self.sessions[b][key].step(self.frame, self.det[b], self.K[b])

    def step(self, key, b):
        s = self.sessions[b][key]
        return s.step(self.frame, None if s.track_boxes else self.det[b], self.K[b])[:, :16]


def first_node_us(n, n_calls=200):
    """bd_stream_windows and bd_stream_track_windows (with the keep-box and tail outputs) for n objects, each back to back on one
    stream: device microseconds per launch, from events around n_calls launches."""
    g = torch.Generator().manual_seed(n)
    prev = torch.zeros((n, _lib.STREAM_ROW_FLOATS))
    prev[:, :16], prev[:, 17] = torch.eye(4).reshape(16), 1.0
    prev[:, 11] = 4.0
    prev = prev.cuda()
    box3 = (torch.rand((n, 8, 3), generator=g) - 0.5).cuda()
    K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]]).repeat(n, 1, 1).cuda()
    det = torch.tensor([180.0, 100.0, 420.0, 330.0]).repeat(n, 1).cuda()
    zeros = torch.zeros((n,), dtype=torch.int32, device="cuda")
    state, keep, tail = det.clone(), torch.zeros((n, 4), dtype=torch.int32, device="cuda"), torch.zeros((n, 5), device="cuda")
    w, kc = hip_ops.stream_windows(det, K, 0.1, S)
    src = torch.zeros((n,), dtype=torch.int32, device="cuda")

    def plain():
        hip_ops.stream_windows(det, K, 0.1, S, w, kc)

    def track():
        hip_ops.stream_track_windows(prev, box3, K, det, zeros, zeros, state, 0.1, S, (H, W), windows=w, K_crop=kc, box_src=src, keep_boxes=keep, track=tail)

    out = []
    for fn in (plain, track):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / n_calls * 1e3)
    return out + [int((src == _lib.STREAM_BOX_TRACKED).sum())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4, help="the larger batch the legs are also measured at")
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
    batches = (1, B)
    legs_on = Legs(a, batches)
    legs = {f"{key}_B{b}": (lambda key=key, b=b: legs_on.step(key, b)) for b in batches for key in "abcd"}
    times = timed(legs, a.rounds, a.calls, a.warmup)
    sources = {}
    for b in batches:
        for key in "bd":
            seen = []
            for _ in range(5):
                legs_on.step(key, b)
                seen.append([int(x) for x in legs_on.sessions[b][key].track_host[:, 4].tolist()])
            sources[(key, b)] = seen
    kernels = {n: first_node_us(n) for n in (1, B, 64)}
    stat = {key: (statistics.median(v), pct(v, 10), pct(v, 90)) for key, v in times.items()}
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    props = torch.cuda.get_device_properties(0)
    what = {"a": f"(a) `PoseStream.step`, fixed references, T = {k + 1}, boxes given (the parent's path)",
            "b": "(b) the same with `track_boxes=True`, `det_boxes=None`",
            "c": '(c) `PoseStream.step`, `select="track"`, boxes given', "d": '(d) the same with `track_boxes=True`, `det_boxes=None`'}

    def section(b):
        out = [f"## B = {b}", "", "| leg | median ms per call | p10 | p90 | calls |", "|---|---|---|---|---|"]
        for key in "abcd":
            m, lo, hi = stat[f"{key}_B{b}"]
            out.append(f"| {what[key]} | {m:.3f} | {lo:.3f} | {hi:.3f} | {len(times[f'{key}_B{b}'])} |")
        for parent, key in (("a", "b"), ("c", "d")):
            (pm, plo, phi), (m, _, _) = stat[f"{parent}_B{b}"], stat[f"{key}_B{b}"]
            out += ["", f"({key}) against ({parent}): {m - pm:+.3f} ms at the median ({m:.3f} against {pm:.3f}).  The tracking leg's median lies within "
                        f"the parent leg's own p10-p90 spread [{plo:.3f}, {phi:.3f}]: **{plo <= m <= phi}**."]
        out += ["", f"Box sources in five further calls (0 = detector, 1 = tracked, 2 = held): (b) {sources[('b', b)]}, (d) {sources[('d', b)]}.", ""]
        return out

    lines = [
        "# Pose stream: each object's box followed from its last pose on the device",
        "",
        f"`tools/stream_track_bench.py --batch {B} --refs {N} --topk {k} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} "
        f"--betr-depth {a.betr_depth} --rounds {a.rounds} --calls {a.calls}` on {torch.cuda.get_device_name(0)} "
        f"({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; parent commit of the measured "
        f"tree: `{commit}`.  A database of N = {N} views per object, k = {k}, one {H} x {W} uint8 frame per call from pinned host memory, host "
        "wall time per call, every call ends in its own wait (the legs are described at the top of the tool).  The legs alternate inside "
        "every round.",
        "",
    ]
    for b in batches:
        lines += section(b)
    lines += ["## The first node alone", "",
              "bd_stream_windows against bd_stream_track_windows (keep-box and tail outputs written, the last pose trusted), each back to back on "
              "one stream, device time from events around 200 launches:", "",
              "| objects | bd_stream_windows, microseconds per launch | bd_stream_track_windows | boxes tracked |", "|---|---|---|---|"]
    lines += [f"| {n} | {p:.1f} | {t:.1f} | {tracked} |" for n, (p, t, tracked) in kernels.items()]
    lines += ["", "Not measured here: tracking ACCURACY on real sequences -- the synthetic model's poses say nothing about it, and the sources "
                  "listed above only say what the kernel was deciding while it was timed.  Also not measured: device time of whole steps (the "
                  "legs are host wall times of whole calls), other frame sizes, the latency forms, a device-resident frame source."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
