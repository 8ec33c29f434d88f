"""The pose stream fed camera-native frames, measured: what does a step cost when the frame arrives as NV12 or BGRA and the crop
kernel converts the pixels under the crop as it stages them, against the RGB stream and against what an NV12 source had to do
before (convert the whole frame, then the RGB stream)?

    python tools/stream_format_bench.py [--prec f16c8_qk16] [--rounds 10] [--calls 20] [--out profiles/pose_stream_formats.md]
                                        [--parent "median,p10,p90"] [--same-tool "median,p10,p90"]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers), default mode, B = 1, T = 6 fixed references (tools/stream_bench.py's
operating point), one frame per call from pinned host memory, at 480 x 640 and at 1080 x 1920.  Legs, alternated inside one run
(every round runs `calls` calls of every leg, rounds x calls >= 200 calls per leg), every leg warmed up, host wall time PER CALL,
every call ending in its own wait:
  (a)  the "rgb" stream fed RGB: the parent's path;
  (b)  the "nv12" stream fed NV12;
  (c)  what an NV12 source had to do before: the NV12 frame uploaded, `frames_to_rgb` as torch ops on the device, the "rgb" stream;
  (d)  the "bgra" stream fed BGRA.
The figures are the median and the 10th to 90th percentile over a leg's calls.  `--parent` takes the figures of the parent commit's
fixed-reference stream at B = 1 (leg (c) of its tools/stream_bench.py, run in the same session on the same device): leg (a) at
480 x 640 is the same operating point and should lie within that spread; `--same-tool` takes the same leg of the same tool on
this tree, which leaves the tree as the only difference.  The crop kernel alone is timed per format with events:
back to back, and one launch at a time after a write that evicts the caches.  What is written down is what was measured."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, synth                            # noqa: E402
from boxdreamer_amd import preprocess as pp                        # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from boxdreamer_amd.stream import PoseStream                      # noqa: E402
from stream_bench import build, device_batch, pct, timed          # noqa: E402

S = 224
SIZES = ((480, 640), (1080, 1920))
FORMATS = ("rgb", "nv12", "bgra")


def source(fmt, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, pp.frame_shape_of(pp.resolve_format(fmt), 1, H, W), generator=g, dtype=torch.uint8)


class Legs:
    """One model, one bank of T - 1 references, and per frame size one session per format."""

    def __init__(self, a):
        T = a.views
        self.model = model = build(a.prec, a.dino_depth, a.betr_depth, False)
        batch = device_batch(1, T, a.seed + 1)
        model(dict(batch))                                              # (the first forward runs the load-time calibration, once)
        self.bank = bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
        rows = [bank.add(batch["images"][0, :T - 1], bbox_feat=batch["bbox_feat"][0, :T - 1]).tolist()]
        bbox_3d = batch["bbox_3d"][:, T - 1]
        self.sessions, self.frames, self.det, self.K = {}, {}, {}, {}
        for H, W in SIZES:
            sx, sy = W / 640.0, H / 480.0
            self.det[H] = torch.tensor([[180.0 * sx, 100.0 * sy, 420.0 * sx, 330.0 * sy]]).pin_memory()
            self.K[H] = torch.tensor([[600.0 * sx, 0.0, W / 2.0], [0.0, 600.0 * sy, H / 2.0], [0.0, 0.0, 1.0]])[None].pin_memory()
            for fmt in FORMATS:
                self.sessions[(H, fmt)] = PoseStream(model, bank, rows, bbox_3d, frame_shape=(H, W), frame_format=fmt)
                self.frames[(H, fmt)] = source(fmt, H, W, a.seed + H).pin_memory()
            self.frames[(H, "nv12_dev")] = torch.zeros_like(self.frames[(H, "nv12")], device="cuda")

    def step(self, H, fmt):
        return self.sessions[(H, fmt)].step(self.frames[(H, fmt)], self.det[H], self.K[H])[:, :16]

    def convert_then_rgb(self, H):
        dev = self.frames[(H, "nv12_dev")]
        dev.copy_(self.frames[(H, "nv12")], non_blocking=True)
        return self.sessions[(H, "rgb")].step(pp.frames_to_rgb(dev, "nv12"), self.det[H], self.K[H])[:, :16]


def kernel_us(H, W, n_calls=200, cold_calls=20):
    """bd_crop_resize_frames[_fmt] alone on one H x W frame per format, the window of the legs: device microseconds per launch, (back to
    back on one stream from events around n_calls launches, the median of cold_calls single launches each after 512 MiB were written)."""
    sx, sy = W / 640.0, H / 480.0
    boxes = pp.square_bbox(torch.tensor([[180.0 * sx, 100.0 * sy, 420.0 * sx, 330.0 * sy]], device="cuda"))
    out = torch.zeros((1, 3, S, S), device="cuda")
    evict = torch.zeros((512 << 20,), dtype=torch.uint8, device="cuda")
    res = {}
    for fmt in ("rgb", "bgr", "rgba", "bgra", "nv12"):
        f = source(fmt, H, W, 3).cuda()

        def fn():
            pp.crop_resize_frames(f, boxes, out=out, frame_format=fmt)
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            fn()
        e1.record()
        e1.synchronize()
        warm = e0.elapsed_time(e1) / n_calls * 1e3
        cold = []
        for i in range(cold_calls):
            evict.fill_(i & 1)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            cold.append(e0.elapsed_time(e1) * 1e3)
        res[fmt] = (warm, statistics.median(cold), int(boxes[0, 2] - boxes[0, 0]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--prec", default=_lib.DEFAULT_PREC)
    ap.add_argument("--dino-depth", type=int, default=12)
    ap.add_argument("--betr-depth", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help='"median,p10,p90" in ms: the parent commit\'s fixed-reference stream at B = 1, same session')
    ap.add_argument("--same-tool", default=None, help='"median,p10,p90" in ms: leg (c) of tools/stream_bench.py on THIS tree, same session')
    ap.add_argument("--commit", default=None, help="commit the measured tree sits on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    if a.rounds * a.calls < 200:
        ap.error("rounds x calls must be at least 200 calls per leg")
    _lib.require_gpu()
    on = Legs(a)
    # the contract, on the frames that are timed: the nv12 stream's crop is the rgb stream's crop of the converted frame
    same = {}
    for H, W in SIZES:
        on.step(H, "nv12")
        on.convert_then_rgb(H)
        same[H] = bool(torch.equal(on.sessions[(H, "nv12")].crops, on.sessions[(H, "rgb")].crops))
    legs = {}
    for H, _ in SIZES:
        legs.update({f"a_{H}": (lambda H=H: on.step(H, "rgb")), f"b_{H}": (lambda H=H: on.step(H, "nv12")),
                     f"c_{H}": (lambda H=H: on.convert_then_rgb(H)), f"d_{H}": (lambda H=H: on.step(H, "bgra"))})
    times = timed(legs, a.rounds, a.calls, a.warmup)
    stat = {key: (statistics.median(v), pct(v, 10), pct(v, 90)) for key, v in times.items()}
    kernels = {(H, W): kernel_us(H, W) for H, W in SIZES}
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    props = torch.cuda.get_device_properties(0)
    what = {"a": '(a) the `"rgb"` stream fed RGB (the parent\'s path)', "b": '(b) the `"nv12"` stream fed NV12',
            "c": "(c) NV12 uploaded, `frames_to_rgb` as torch ops on the device, then the `\"rgb\"` stream", "d": '(d) the `"bgra"` stream fed BGRA'}
    bytes_of = {"a": 3.0, "b": 1.5, "c": 1.5, "d": 4.0}
    extra = (f' --parent "{a.parent}"' if a.parent else "") + (f' --same-tool "{a.same_tool}"' if a.same_tool else "")
    lines = [
        "# Pose stream: camera-native frames (NV12, BGRA) converted under the crop",
        "",
        f"`tools/stream_format_bench.py --views {a.views} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} --betr-depth "
        f"{a.betr_depth} --rounds {a.rounds} --calls {a.calls}{extra}` on {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, "
        f"{props.multi_processor_count} CUs), torch {torch.__version__}; parent commit of the measured tree: `{commit}`.  B = 1, T = {a.views} "
        "fixed references, one frame per call from pinned host memory, host wall time per call, every call ends in its own wait (the legs "
        "are described at the top of the tool).  The legs alternate inside every round.",
        "",
    ]
    for H, W in SIZES:
        lines += [f"## {H} x {W}", "", f"The `\"nv12\"` stream's crops equal the `\"rgb\"` stream's crops of the converted frame bit for bit: **{same[H]}**.", "",
                  "| leg | frame bytes uploaded | median ms per call | p10 | p90 | calls |", "|---|---|---|---|---|---|"]
        for key in "abcd":
            m, lo, hi = stat[f"{key}_{H}"]
            lines.append(f"| {what[key]} | {int(bytes_of[key] * H * W)} | {m:.3f} | {lo:.3f} | {hi:.3f} | {len(times[f'{key}_{H}'])} |")
        (am, alo, ahi), (bm, _, bhi), (cm, clo, _), (dm, _, _) = (stat[f"{k}_{H}"] for k in "abcd")
        lines += ["", f"(b) against (c): {bm - cm:+.3f} ms at the median; (b)'s p90 under (c)'s p10: **{bhi < clo}**.  (b) against (a): {bm - am:+.3f} ms; "
                      f"(d) against (a): {dm - am:+.3f} ms; (a)'s own p10-p90 spread is [{alo:.3f}, {ahi:.3f}].", ""]
    if a.parent:
        pm, plo, phi = (float(x) for x in a.parent.split(","))
        am = stat[f"a_{SIZES[0][0]}"][0]
        lines += ["## Leg (a) against the parent commit", "",
                  f"The parent commit's fixed-reference stream (leg (c) of its `tools/stream_bench.py`, B = 1, T = {a.views}, 480 x 640, run in the same "
                  f"session on the same device): median {pm:.3f} ms, p10-p90 [{plo:.3f}, {phi:.3f}].  Leg (a) here at 480 x 640: median {am:.3f} ms.  "
                  f"That is {am - pm:+.3f} ms against the parent's median.  Within the parent's own spread: **{plo <= am <= phi}**; "
                  f"not above its p90: **{am <= phi}**.", ""]
        if a.same_tool:
            sm, slo, shi = (float(x) for x in a.same_tool.split(","))
            lines += [f"The same tool and leg on this tree (`tools/stream_bench.py`, leg (c), B = 1; the `\"rgb\"` session through another "
                      f"driver loop, in a process that holds that tool's other sessions): median {sm:.3f} ms, p10-p90 [{slo:.3f}, {shi:.3f}]; "
                      f"{sm - pm:+.3f} ms against the parent's median.  Within the parent's own spread: **{plo <= sm <= phi}**.", ""]
    lines += ["## The crop kernel alone", "",
              "One launch for the legs' window on one frame, `out_size` 224, fp32 out; device time from events: back to back (200 launches on one "
              "stream, the frame in cache) and cold (the median of 20 single launches, each after 512 MiB were written).", "",
              "| frame | format | crop side | back to back, microseconds per launch | cold |", "|---|---|---|---|---|"]
    for (H, W), res in kernels.items():
        lines += [f"| {H} x {W} | {fmt} | {side} | {warm:.1f} | {cold:.1f} |" for fmt, (warm, cold, side) in res.items()]
    lines += ["", "Not measured here: a device-resident frame source (a decoder surface handed over without the H2D: the step can now read one, "
                  "nobody has timed it); B > 1 and other T; the latency forms; device time of whole steps (the legs are host wall times of whole "
                  "calls); NV12 surfaces with a padded pitch or luma height; image quality against a full-precision colour conversion."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
