"""Time the device crop + resize (bd_crop_resize_frames) next to the host chain it replaces (profiles/preprocess.md).

    python tools/preprocess_probe.py [--out FILE] [--repeats 20]

Device: HIP events around `boxdreamer_amd.preprocess.crop_resize_frames`, median of `--repeats` calls after 3 warm-up calls, for
m = 1 and m = 192 crops (32 x 6 views, one frame per crop) of VGA and 1080p frames at scale ~0.5, 1.3, 4 and 8 (box side = scale x 224,
centred, so the large ones leave the frame as a padded crop does), plus the pinned host-to-device copy of the uint8 frames.
The achieved rate is the frame bytes the kernel must read once (3 x valid rectangle per crop) over the kernel time.
Host: the reference's sequence per crop -- PIL crop (black outside), / 255 in fp32, torch.nn.functional.interpolate(mode="bilinear",
antialias=True) to 224 -- on a pool of 16 threads (one torch thread each), plus the pinned H2D of the fp32 crops.
Facade: one B = 1, T = 2 eval forward with "frames" + "crop_boxes" against the same call with host-made "images" (host chain + H2D
included), hip_graph on, 2 layers of synthetic weights: the difference is the preprocessing, not the model.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxdreamer_amd import preprocess as pp  # noqa: E402
from boxdreamer_amd import synth  # noqa: E402

S = 224
SCALES = (0.5, 1.3, 4.0, 8.0)
SIZES = {"VGA": (480, 640), "1080p": (1080, 1920)}


def median_ms(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def host_chain(frame_img, box):
    from PIL import Image  # noqa: F401
    crop = frame_img.crop(tuple(box))
    t = torch.from_numpy(np.asarray(crop).copy()).permute(2, 0, 1).float().div(255)
    return torch.nn.functional.interpolate(t[None], (S, S), mode="bilinear", antialias=True, align_corners=False)[0].clamp(0.0, 1.0)


def host_ms(frames_np, boxes, repeats, pool):
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames_np]
    out = torch.empty((len(boxes), 3, S, S), pin_memory=True)

    def one(k):
        out[k] = host_chain(imgs[k % len(imgs)], boxes[k])
    ts = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        list(pool.map(one, range(len(boxes))))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is no fallback"
    torch.set_num_threads(1)                        # the host chain runs one crop per pool thread, as a 16-worker data loader would
    rng = np.random.default_rng(0)
    pool = ThreadPoolExecutor(max_workers=16)
    rows = []
    for name, (H, W) in SIZES.items():
        for m in (1, 192):
            n_host = min(m, 8)                      # distinct host frames; the device batch repeats them to m frames
            frames_np = rng.integers(0, 256, (n_host, H, W, 3), dtype=np.uint8)
            pinned = torch.from_numpy(frames_np[np.arange(m) % n_host]).pin_memory()
            dev = torch.empty_like(pinned, device="cuda")
            out = torch.empty((m, 3, S, S), device="cuda")
            for scale in SCALES:
                s = int(round(scale * S))
                x0, y0 = (W - s) // 2, (H - s) // 2
                boxes = [[x0 + (k % 7), y0 + (k % 5), x0 + (k % 7) + s, y0 + (k % 5) + s] for k in range(m)]
                b = torch.tensor(boxes, dtype=torch.int32, device="cuda")
                k_ms = median_ms(lambda: pp.crop_resize_frames(dev, b, out=out), args.repeats)
                h2d_u8 = median_ms(lambda: dev.copy_(pinned, non_blocking=True), args.repeats)
                both = median_ms(lambda: (dev.copy_(pinned, non_blocking=True), pp.crop_resize_frames(dev, b, out=out)), args.repeats)
                valid = sum((min(bx[2], W) - max(bx[0], 0)) * (min(bx[3], H) - max(bx[1], 0)) * 3 for bx in boxes)
                h_ms, crops = host_ms(frames_np, boxes, max(3, args.repeats // 4) if m > 1 else args.repeats, pool)
                h2d_f32 = median_ms(lambda: out.copy_(crops, non_blocking=True), args.repeats)
                rows.append({"frame": name, "m": m, "scale": scale, "side": s, "kernel_ms": k_ms, "h2d_uint8_frames_ms": h2d_u8,
                             "device_total_ms": both, "read_bytes": valid, "kernel_GBps": valid / k_ms / 1e6,
                             "host_chain_16thr_ms": h_ms, "h2d_fp32_crops_ms": h2d_f32, "host_total_ms": h_ms + h2d_f32})
                print(json.dumps(rows[-1]), flush=True)
    # facade, B = 1
    from boxdreamer_amd.model import BoxDreamer
    mods = copy.deepcopy(json.load(open(os.path.join(ROOT, "tests", "golden", "model_modules_config.json")))["modules"])
    mods["decoder"].update(num_decoder_layers=2)
    mods["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=2)
    mods["hip_graph"] = True
    model = BoxDreamer({"modules": mods})
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(1234, 2).items()}, strict=True)
    model = model.cuda().eval()
    H, W = SIZES["VGA"]
    frames_np = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    pinned = torch.from_numpy(frames_np).pin_memory()
    dev = torch.empty_like(pinned, device="cuda")
    bl = [[170, 90, 470, 390], [100, 40, 500, 440]]
    boxes = torch.tensor([bl], dtype=torch.int32, device="cuda")
    base = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(seed=11, B=1, T=2).items() if k != "images"}
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames_np]
    crops = torch.empty((1, 2, 3, S, S), pin_memory=True)

    def with_frames():
        dev.copy_(pinned, non_blocking=True)
        model({**base, "frames": dev, "crop_boxes": boxes})

    def with_images():
        list(pool.map(lambda k: crops[0].__setitem__(k, host_chain(imgs[k], bl[k])), range(2)))
        model({**base, "images": crops.cuda(non_blocking=True)})

    def wall(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))
    facade = {"facade_B1_T2_frames_ms": wall(with_frames), "facade_B1_T2_host_images_ms": wall(with_images)}
    print(json.dumps(facade), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "facade": facade}, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
