"""Write tests/golden/preprocess_vectors.npz: the reference's own crop + resize chain on seeded frames and boxes.

    python tools/make_golden_preprocess.py [--reference PATH]

Runs the REAL functions of the reference's src/datasets/utils/preprocess.py (`square_bbox`, `pad_and_resize_image`, `_crop_image`
with `bbox_obj`, `pad_image_based_on_bbox`, `adjust_intrinsic_matrix`), loaded from the file by path.  What this image lacks is
replaced by stand-ins, and three of them DO ARITHMETIC (torchvision is absent), so they are named here and in the fixture's `doc`:

  * `transforms.ToTensor`             = uint8 HWC / 255 -> fp32 CHW (`torch.from_numpy(np.asarray(img)).permute(2, 0, 1).float().div(255)`);
  * `transforms.Resize(size, antialias=True)` on a tensor
                                      = `torch.nn.functional.interpolate(x[None], size, mode="bilinear", antialias=True,
                                        align_corners=False)[0]`, which is what torchvision dispatches to (square crops only: `size`
                                        is applied to both sides);
  * `functional.crop(img, top, left, height, width)` on a PIL image
                                      = `img.crop((left, top, left + width, top + height))` (black outside the image).

`transforms.Compose` applies its list in order; the sibling modules the file star-imports (`camera_transform`, `data_io`, `data_utils`)
are empty.  Everything else runs as the reference wrote it.

Per case the file holds: the frame index (`c{i}_frame`; frames are shared, `frame_{k}`), the raw float box, the reference's square float
box, the integer window its `_crop_image` cut, the optional object box (`bbox_obj`, background masking), out_size, the reference's fp32
output, the intrinsics before / after `adjust_intrinsic_matrix`, an fp64 evaluation of the filter as this project defines it
(include/boxdreamer_hip.h: bd_crop_resize_frames) and the reference output's max-abs distance from it (`c{i}_err_ref`).  The fixture
must stay below 1 MiB, so the cases use small out_size values (28 ... 56, one constant-colour case at 224); the production size is
covered by the GPU tests' randomised sweep against the same fp64 restatement.  Test infrastructure only: nothing on the GPU path
imports this file.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "preprocess_vectors.npz")
DOC = ("reference: src/datasets/utils/preprocess.py run by tools/make_golden_preprocess.py with arithmetic stand-ins for torchvision: "
       "ToTensor = uint8 HWC / 255 -> fp32 CHW; Resize(size, antialias=True) = torch.nn.functional.interpolate(x[None], size, "
       "mode='bilinear', antialias=True, align_corners=False); functional.crop = PIL Image.crop((left, top, left + w, top + h)). "
       "c{i}_exact is an fp64 evaluation of the triangle filter defined in include/boxdreamer_hip.h; c{i}_err_ref = max |ref - exact|.")


def load_reference(ref):
    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)

    class Resize:
        def __init__(self, size, antialias=None):
            assert antialias is True
            self.size = int(size)

        def __call__(self, x):
            assert x.shape[-1] == x.shape[-2], "square crops only"
            return torch.nn.functional.interpolate(x[None], (self.size, self.size), mode="bilinear", antialias=True, align_corners=False)[0]

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Resize, tr.Compose = ToTensor, Resize, Compose
    fn = types.ModuleType("torchvision.transforms.functional")
    fn.crop = lambda img, top, left, height, width: img.crop((left, top, left + width, top + height))
    tv.transforms, tr.functional = tr, fn
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    for name in ("src", "src.utils", "src.utils.camera_transform", "src.datasets", "src.datasets.utils", "src.datasets.utils.data_io",
                 "src.datasets.utils.data_utils"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("src.datasets.utils.preprocess", os.path.join(ref, "src/datasets/utils/preprocess.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def aa_weights(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] fp64 weights of the antialiased triangle filter (ATen _upsample_bilinear2d_aa, align_corners = False)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    Wm = np.zeros((n_out, n_in))
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        j = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs(j - c + 0.5) / support)
        Wm[i, lo:hi] = w / w.sum()
    return Wm


def exact_fp64(frame: np.ndarray, box, out_size: int, keep=None) -> np.ndarray:
    """fp64 [3, S, S]: zero-padded integer crop (keep box: both edges inclusive) / 255, separable filter, clamp."""
    x0, y0, x1, y1 = (int(v) for v in box)
    s = x1 - x0
    H, Wd, _ = frame.shape
    ys, xs = np.arange(y0, y1), np.arange(x0, x1)
    vy, vx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < Wd)
    if keep is not None:
        vx &= (xs >= int(keep[0])) & (xs <= int(keep[2]))
        vy &= (ys >= int(keep[1])) & (ys <= int(keep[3]))
    crop = np.zeros((s, s, 3))
    crop[np.ix_(vy, vx)] = frame[np.ix_(ys[vy], xs[vx])].astype(np.float64)
    crop /= 255.0
    Wf = aa_weights(s, out_size)
    out = np.einsum("ih,hwc->iwc", Wf, crop)
    out = np.einsum("jw,iwc->ijc", Wf, out)
    return np.clip(out.transpose(2, 0, 1), 0.0, 1.0)


def make_frame(rng, H, W):
    """Left half noise, right half smooth gradients with a sharp diagonal edge."""
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.stack([255 * xx / max(W - 1, 1), 255 * yy / max(H - 1, 1), 127.5 + 127.5 * np.sin(xx / 17.0 + yy / 29.0)], -1)
    g[(xx - W * 0.75) + (yy - H / 2) * 0.4 > 0] *= 0.25
    half = W // 2
    f[:, half:] = np.clip(np.rint(g[:, half:]), 0, 255).astype(np.uint8)
    return f


def raw_box_for(int_box, rng, padding=0.1):
    """A non-square float box whose reference square_bbox truncates to `int_box` (x0 y0 x1 y1, square)."""
    x0, y0, x1, y1 = int_box
    s = x1 - x0
    fx, fy = rng.uniform(0.05, 0.4, 2)
    # the square float box: [x0 + fx, ... + side] with side in (s, s + 1) so that int(side) == s
    side = s + rng.uniform(0.1, 0.8)
    cx, cy = x0 + fx + side / 2, y0 + fy + side / 2
    if x0 < 0:          # int() truncates towards zero: a negative left edge needs a fraction BELOW the integer
        cx -= 2 * fx
    if y0 < 0:
        cy -= 2 * fy
    half = side / 2 / (1 + padding)
    aspect = rng.uniform(0.5, 0.95)
    if rng.random() < 0.5:
        return np.array([cx - half, cy - half * aspect, cx + half, cy + half * aspect])
    return np.array([cx - half * aspect, cy - half, cx + half * aspect, cy + half])


# (frame, integer window, out_size, keep box or None, label)
CASES = [
    (0, (40, 60, 62, 82), 32, None, "inside, scale 0.69"),
    (0, (130, 90, 163, 123), 32, None, "inside, scale 1.03, across the noise / gradient seam"),
    (0, (20, 30, 63, 73), 32, None, "inside, scale 1.34, noise"),
    (0, (100, 10, 175, 85), 56, None, "inside, scale 1.34"),
    (0, (96, 8, 320, 232), 56, None, "inside, scale 4"),
    (0, (10, 5, 234, 229), 28, None, "inside, scale 8"),
    (0, (-25, 100, 39, 164), 32, None, "leaves on the left"),
    (0, (280, 100, 350, 170), 32, None, "leaves on the right"),
    (0, (150, -31, 210, 29), 32, None, "leaves at the top"),
    (0, (60, 200, 130, 270), 32, None, "leaves at the bottom"),
    (1, (-20, -30, 180, 170), 40, None, "leaves on all sides (frame 161 x 97 inside the window)"),
    (0, (-70, -110, 380, 340), 56, None, "larger than the frame in both directions, scale 8.04"),
    (0, (50, 40, 106, 96), 56, None, "identity: side == out_size"),
    (0, (33, 44, 34, 45), 224, None, "side 1, out_size 224 (constant)"),
    (1, (90, 50, 91, 51), 32, None, "side 1"),
    (1, (17, 9, 64, 56), 33, None, "odd sizes: side 47 -> 33"),
    (1, (100, 30, 161, 91), 45, None, "odd sizes: side 61 -> 45, touches the right edge"),
    (0, (30, 20, 150, 140), 32, (55, 41, 118, 127), "keep box (bbox_obj): background masked"),
    (0, (180, 60, 300, 180), 32, (200, 20, 330, 150), "keep box leaving the window and the frame"),
    (1, (5, 5, 55, 55), 32, None, "two crops from one frame (a)"),
    (1, (70, 20, 140, 90), 32, None, "two crops from one frame (b)"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BOXDREAMER_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(1)
    rng = np.random.default_rng(20261017)
    frames = [make_frame(rng, 240, 320), make_frame(rng, 97, 161)]
    out = {"doc": np.array(DOC), "n_cases": np.array(len(CASES)), "labels": np.array([c[4] for c in CASES])}
    for k, f in enumerate(frames):
        out[f"frame_{k}"] = f
    for i, (fk, ibox, S, keep, label) in enumerate(CASES):
        frame = frames[fk]
        img = Image.fromarray(frame)
        while True:
            # pad_and_resize_image squares a box AGAIN, with integer truncation, when its two float extents differ (an ulp is enough);
            # the window is then not square in general, which is outside this project's scope: such a draw is replaced
            raw = raw_box_for(ibox, rng)
            sq = ref.square_bbox(raw)                                       # float64, padding 0.1
            if (sq[2] - sq[0]) == (sq[3] - sq[1]):
                break
        image_t, _, _, bbox = ref.pad_and_resize_image(img, True, S, bbox_anno=sq, bbox_obj=None if keep is None else np.array(keep, dtype=np.float64))
        assert bbox is not None and np.array_equal(np.asarray(bbox, dtype=np.float64), sq), "the reference re-squared the box"
        left, top, w, h = int(bbox[0]), int(bbox[1]), int(bbox[2] - bbox[0]), int(bbox[3] - bbox[1])
        got = np.array([left, top, left + w, top + h], dtype=np.int64)
        assert np.array_equal(got, np.array(ibox)), (label, got, ibox)
        # the dataset's other route to the same pixels: pad the image to hold the box, then crop at the shifted position
        padded, info = ref.pad_image_based_on_bbox(img, got.astype(np.float64))
        if info is not None and keep is None:
            shifted = got + np.array([info["left"], info["top"], info["left"], info["top"]], dtype=np.int64)
            a = np.asarray(ref._crop_image(padded, shifted.astype(np.float64)))
            b = np.asarray(ref._crop_image(img, got.astype(np.float64)))
            assert np.array_equal(a, b), label
        ref32 = image_t.numpy()
        assert ref32.shape == (3, S, S) and ref32.dtype == np.float32
        exact = exact_fp64(frame, got, S, keep)
        K = np.array([[rng.uniform(400, 700), 0, frame.shape[1] / 2 + rng.normal() * 5], [0, rng.uniform(400, 700), frame.shape[0] / 2 + rng.normal() * 5],
                      [0, 0, 1.0]])
        K_crop = ref.adjust_intrinsic_matrix(K, (S / w, S / h), (left, top))
        err = float(np.abs(ref32.astype(np.float64) - exact).max())
        out.update({f"c{i}_frame": np.array(fk), f"c{i}_raw_box": raw, f"c{i}_square_box": np.asarray(sq, dtype=np.float64), f"c{i}_int_box": got,
                    f"c{i}_keep": np.array(keep if keep is not None else [], dtype=np.int64), f"c{i}_out_size": np.array(S),
                    f"c{i}_ref": ref32, f"c{i}_exact": exact, f"c{i}_err_ref": np.array(err), f"c{i}_K": K, f"c{i}_K_crop": K_crop})
        print(f"case {i:2d} S {S:3d} side {w:4d} scale {w / S:5.2f} err_ref {err:.2e}  {label}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size} bytes)")
    assert size < (1 << 20), "fixture above 1 MiB"


if __name__ == "__main__":
    main()
