"""The pose stream, measured at the reference demo's operating point (src/demo/demo.py:1451-1514: one call per frame at batch 1,
T = 6, the same five references for every frame, one 480 x 640 frame per call).

    python tools/stream_bench.py [--prec f16c8_qk16] [--rounds 10] [--calls 20] [--out profiles/pose_stream.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers).  Legs, alternated inside one run (every round runs `calls` calls of
every leg, rounds x calls >= 200 calls per leg), every leg warmed up, host wall time PER CALL, every call ending in its own wait:
  (a)  the facade with `hip_graph: true`, un-banked, host PnP: `model(batch)` on a device-resident batch dict of T crops and heat
       maps (all T views encoded every frame); the wait is the facade's own (the corners' D2H) plus the pose's read-back;
  (b)  the eager facade forward over the entry-token bank with `pnp_on_device: "wave"`, taking `frames` + `crop_boxes`: the pinned
       frame's H2D, square_bbox and crop_intrinsics (torch), `model(batch)`, the pose's read-back;
  (c)  `PoseStream.step` on the pinned frame: one captured graph, one D2H of the result rows, one wait for its event.
(a) to (c) are measured again on a model with the latency forms (`hip_latency: true`), and (b), (c) at B = 4 (four tracked objects
in the one frame).  The figures are the median and the 10th to 90th percentile over a leg's calls."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, synth                            # noqa: E402
from boxdreamer_amd import preprocess as pp                        # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from boxdreamer_amd.model import BoxDreamer                       # noqa: E402
from boxdreamer_amd.stream import PoseStream                      # noqa: E402

H, W, S = 480, 640, 224


def build(prec, dino_depth, betr_depth, latency):
    cfg = {"modules": {
        "use_keypoints": False, "use_matching": False, "use_tracking": False, "use_rgb": True, "use_pp": True,
        "regression_intri": True, "rotation_type": None, "coordinate": "object", "pose_representation": "bb8",
        "bbox_representation": "heatmap", "patchify_rays": True, "dense_cfg": {"enable": False}, "pnp_on_device": "wave",
        "decoder": {"d_model": 768, "nhead": 8, "num_decoder_layers": betr_depth, "decoder_only": True, "patch_size": 14, "img_size": 224,
                    "diff_emb": False, "nvs_supervision": False, "ray_supervision": True, "use_mask": False, "hip_precision": prec},
        "encoder": {"name": "dino", "dino": {"ckpt_path": None, "cfg": {"model_type": "dinov2_vitb14_reg", "synthetic_seed": 4321,
                                                                        "depth": dino_depth, "hip_precision": prec}}}}}
    if latency:
        cfg["modules"]["hip_latency"] = True
    model = BoxDreamer(cfg)
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(seed=1234, depth=betr_depth).items()}, strict=True)
    return model.cuda().eval()


def device_batch(B, T, seed):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(seed=seed, B=B, T=T).items()}


class Flavour:
    """One model (plain or with the latency forms) and the legs on it.  Everything eager runs once at its largest shape BEFORE the
    first capture: a live graph freezes the modules' workspaces."""

    def __init__(self, a, latency):
        T, self.T = a.views, a.views
        self.model = model = build(a.prec, a.dino_depth, a.betr_depth, latency)
        self.plain = {b: device_batch(b, T, a.seed + b) for b in (1, a.batch)}
        model(dict(self.plain[a.batch]))                                # (the first forward runs the load-time calibration, once)
        self.bank = bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
        refs = self.plain[a.batch]
        self.ref_rows = [bank.add(refs["images"][b, :T - 1], bbox_feat=refs["bbox_feat"][b, :T - 1]).tolist() for b in range(a.batch)]
        g = torch.Generator().manual_seed(a.seed)
        self.frame = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
        dets = [[180.0, 100.0, 420.0, 330.0], [20.5, 30.0, 250.0, 240.5], [380.0, 200.0, 630.0, 470.0], [250.0, 10.0, 500.0, 250.0]]
        self.det = {b: torch.tensor([dets[i % 4] for i in range(b)]).pin_memory() for b in (1, a.batch)}
        K = torch.tensor([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
        self.K = {b: K.repeat(b, 1, 1).pin_memory() for b in (1, a.batch)}
        self.banked = {}
        for b in (1, a.batch):
            base = {k: v for k, v in self.plain[b].items() if k not in ("images", "bbox_feat")}
            base["crop_boxes"] = torch.tensor([0, 0, 16, 16], dtype=torch.int32, device="cuda").repeat(b, T, 1)
            base["frame_idx"] = torch.zeros((b, T), dtype=torch.int32, device="cuda")
            base["non_ndc_intrinsics"] = base["non_ndc_intrinsics"].clone()
            base.update(ref_bank=bank, ref_rows=[r + [-1] for r in self.ref_rows[:b]])
            self.banked[b] = base
        for b in (a.batch, 1):
            self.eager_banked(b)
        self.graphed(1)                                                 # captures the un-banked graph at B = 1
        self.sessions = {b: PoseStream(model, bank, self.ref_rows[:b], self.plain[b]["bbox_3d"][:, T - 1], frame_shape=(H, W))
                         for b in (a.batch, 1)}

    def graphed(self, b):
        m = self.model
        m.hip_graph, m.pnp_on_device = True, False
        out = m(dict(self.plain[b]))
        return out["pred_poses"][:, self.T - 1].cpu()

    def eager_banked(self, b):
        m, T = self.model, self.T
        m.hip_graph, m.pnp_on_device = False, "wave"
        base = self.banked[b]
        win = pp.square_bbox(self.det[b].cuda(non_blocking=True), 0.1)
        base["crop_boxes"][:, T - 1] = win
        base["non_ndc_intrinsics"][:, T - 1] = pp.crop_intrinsics(self.K[b].cuda(non_blocking=True), win, S)
        out = m(dict(base, frames=self.frame.cuda(non_blocking=True)))
        return out["pred_poses"][:, T - 1].cpu()

    def stream(self, b):
        return self.sessions[b].step(self.frame, self.det[b], self.K[b])[:, :16]


def timed(legs, rounds, calls, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, round(p / 100 * (len(v) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4, help="the larger batch (b), (c) are also measured at")
    ap.add_argument("--views", type=int, default=6)
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
    B = a.batch
    plain, lat = Flavour(a, False), Flavour(a, True)
    # the stream's pose against the eager banked forward's, per flavour (tests/test_gpu_stream.py holds them to the same bits)
    same = all(bool(torch.equal(f.stream(b).reshape(b, 4, 4).clone(), f.eager_banked(b))) for f in (plain, lat) for b in (1, B))
    legs = {"a": lambda: plain.graphed(1), "b": lambda: plain.eager_banked(1), "c": lambda: plain.stream(1),
            "a_lat": lambda: lat.graphed(1), "b_lat": lambda: lat.eager_banked(1), "c_lat": lambda: lat.stream(1),
            f"b_B{B}": lambda: plain.eager_banked(B), f"c_B{B}": lambda: plain.stream(B),
            f"b_lat_B{B}": lambda: lat.eager_banked(B), f"c_lat_B{B}": lambda: lat.stream(B)}
    times = timed(legs, a.rounds, a.calls, a.warmup)
    stat = {k: (statistics.median(v), pct(v, 10), pct(v, 90)) for k, v in times.items()}
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    props = torch.cuda.get_device_properties(0)
    what = {"a": "(a) facade, `hip_graph: true`, un-banked, host PnP", "b": "(b) eager facade over the entry bank, `frames` + `crop_boxes`, wave PnP",
            "c": "(c) `PoseStream.step`"}

    def row(key, label):
        m, lo, hi = stat[key]
        return f"| {label} | {m:.3f} | {lo:.3f} | {hi:.3f} | {len(times[key])} |"

    def verdict(c, other):
        """(c) below `other` by more than the run's own spread: (c)'s 90th percentile under the other leg's 10th."""
        return stat[c][2] < stat[other][1]

    def section(title, keys, sfx):
        out = [f"## {title}", "", "| leg | median ms per call | p10 | p90 | calls |", "|---|---|---|---|---|"]
        out += [row(k + sfx, what[k]) for k in keys]
        c = "c" + sfx
        for k in keys:
            if k == "c":
                continue
            o = k + sfx
            out += ["", f"(c) below ({k}) by more than the run's own spread (p90 of (c) under p10 of ({k})): **{verdict(c, o)}** -- "
                        f"median {stat[c][0]:.3f} against {stat[o][0]:.3f} ms, (c) / ({k}) = {stat[c][0] / stat[o][0]:.3f}."]
        return out + [""]

    lines = [
        "# Pose stream: one captured graph per frame over banked references",
        "",
        f"`tools/stream_bench.py --batch {B} --views {a.views} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} --betr-depth "
        f"{a.betr_depth} --rounds {a.rounds} --calls {a.calls}` on {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, "
        f"{props.multi_processor_count} CUs), torch {torch.__version__}; parent commit of the measured tree: `{commit}`.  T = {a.views}, one "
        f"{H} x {W} uint8 frame per call from pinned host memory, host wall time per call, every call ends in its own wait (the legs are "
        "described at the top of the tool).  The legs alternate inside every round.",
        "",
        f"The stream's pose equals the eager banked forward's pose bit for bit, in every flavour and batch measured here: **{same}**.",
        "",
    ]
    lines += section("B = 1, default forms", ("a", "b", "c"), "")
    lines += section("B = 1, latency forms (`hip_latency: true`)", ("a", "b", "c"), "_lat")
    lines += section(f"B = {B}, default forms", ("b", "c"), f"_B{B}")
    lines += section(f"B = {B}, latency forms", ("b", "c"), f"_lat_B{B}")
    lines += ["Not measured here: device time alone (these are host wall times of whole calls), other frame sizes, other T, a device-"
              "resident frame source, more than one session per process."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
