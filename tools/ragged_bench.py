"""Ragged batches, measured: one forward over samples with different view counts against what a uniform-T path can do for them.

    python tools/ragged_bench.py [--samples 32] [--seed 20261016] [--prec f16c8_qk16] [--repeats 7] [--out profiles/ragged_batches.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers), encoder -> decoder -> corner decode per forward, no host post-solve.
The view counts are drawn ONCE from {3, 4, 6, 9, 17} with the recorded seed.  Three legs, each warmed up on every shape it uses and
timed with device events around `inner` back-to-back forwards; the legs alternate inside every repeat so that drift hits all three
alike; the figure of a leg is the median over the repeats, its spread (max - min) / median:
  (a) ragged     ONE forward over all samples (`view_counts`): packed views, one attention launch per block;
  (b) grouped    what the uniform path can do for the same samples: one uniform forward per distinct T, summed;
  (c) uniform    a uniform batch of (about) the same total views at one T -- the cost of the rows without the mix's attention profile.
(a) and (b) compute the same results (checked here, bit for bit)."""
import argparse
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, hip_ops, synth                    # noqa: E402
from boxdreamer_amd.betr import BETR                               # noqa: E402
from boxdreamer_amd.encoder import DinoV2Wrapper                   # noqa: E402

CHOICES = (3, 4, 6, 9, 17)


def build(prec, dino_depth, betr_depth):
    enc = DinoV2Wrapper(None, {"model_type": "dinov2_vitb14_reg", "synthetic_seed": 4321, "depth": dino_depth, "hip_precision": prec})
    dec = BETR(d_model=768, nhead=8, num_decoder_layers=betr_depth, decoder_only=True, patch_size=14, img_size=224, diff_emb=False,
               nvs_supervision=False, ray_supervision=True, use_mask=False, use_pretrained=True, patchify_rays=True,
               pose_representation="bb8", bbox_representation="heatmap", hip_precision=prec)
    dec.load_state_dict(synth.betr_state_dict(seed=1234, depth=betr_depth), strict=True)
    dec = dec.cuda().eval()
    dec.validate_inputs = False
    return enc, dec


def uniform_forward(enc, dec, img, bf, mask):
    heat = dec(bf, img, mask, enc.predict(img), None)
    return hip_ops.decode_topk(heat)[0], dec.last_logits


def ragged_forward(enc, dec, img, bf, mask, counts, index):
    feats = enc.predict(img.flatten(0, 1).index_select(0, index))
    heat = dec(bf, img, mask, feats, None, view_counts=counts)
    return hip_ops.decode_topk(heat)[0], dec.last_logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--prec", default=_lib.DEFAULT_PREC)
    ap.add_argument("--dino-depth", type=int, default=12)
    ap.add_argument("--betr-depth", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit the measured tree sits on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    rng = random.Random(a.seed)
    counts = [rng.choice(CHOICES) for _ in range(a.samples)]
    B, t_max, n_views = len(counts), max(counts), sum(counts)
    enc, dec = build(a.prec, a.dino_depth, a.betr_depth)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(a.seed)
    img = torch.rand((B, t_max, 3, 224, 224), generator=g).to(torch.bfloat16).to(dev)
    bf = (torch.rand((B, t_max, 8, 224, 224), generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    query = [c - 1 for c in counts]
    mask = torch.zeros((B, t_max), dtype=torch.bool)
    mask[torch.arange(B), torch.tensor(query)] = True
    mask = mask.to(dev)
    index = torch.tensor(_lib.packing_index(counts, t_max)).to(dev)
    # (b): the samples grouped by T, each group a uniform batch of its own
    groups = []
    for t in sorted(set(counts)):
        ids = [i for i, c in enumerate(counts) if c == t]
        sel = torch.tensor(ids).to(dev)
        groups.append((ids, img[sel, :t].contiguous(), bf[sel, :t].contiguous(), mask[sel, :t].contiguous()))
    # (c): one T, about the same number of views
    t_c = 6
    b_c = max(1, round(n_views / t_c))
    img_c, bf_c = img[:1, :1].expand(b_c, t_c, -1, -1, -1).contiguous(), bf[:1, :1].expand(b_c, t_c, -1, -1, -1).contiguous()
    mask_c = torch.zeros((b_c, t_c), dtype=torch.bool, device=dev)
    mask_c[:, t_c - 1] = True

    legs = {
        "a_ragged": lambda: ragged_forward(enc, dec, img, bf, mask, counts, index),
        "b_grouped": lambda: [uniform_forward(enc, dec, gi, gb, gm) for _, gi, gb, gm in groups],
        "c_uniform": lambda: uniform_forward(enc, dec, img_c, bf_c, mask_c),
    }
    # same results: (a) against (b), bit for bit
    _, la = legs["a_ragged"]()
    la = la.clone()
    same = True
    for ids, gi, gb, gm in groups:
        _, lg = uniform_forward(enc, dec, gi, gb, gm)
        same = same and bool(torch.equal(lg, la[torch.tensor(ids).to(dev)]))
    torch.cuda.synchronize()
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    hist = {t: counts.count(t) for t in sorted(set(counts))}
    lines = [
        "# Ragged batches: one forward against one forward per distinct T",
        "",
        f"`tools/ragged_bench.py --samples {a.samples} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} --betr-depth {a.betr_depth} "
        f"--repeats {a.repeats} --inner {a.inner}` on {torch.cuda.get_device_name(0)}; parent commit of the measured tree: `{commit}`.",
        "",
        f"Mix: {a.samples} samples, view counts drawn once from {list(CHOICES)} with seed {a.seed}: {hist} (count per T), "
        f"{n_views} views in all, T_max = {t_max} (padding to T_max would run {B * t_max} views).",
        f"(a) and (b) give bit-identical logits: **{same}**.",
        "",
        "| leg | what runs | ms per forward (median) | min | max | spread |",
        "|---|---|---|---|---|---|",
        f"| (a) ragged | one forward, `view_counts`, {n_views} packed views, decoder on one lane | {med['a_ragged']:.2f} | {min(times['a_ragged']):.2f} | {max(times['a_ragged']):.2f} | {spread['a_ragged'] * 100:.1f} % |",
        f"| (b) grouped | {len(groups)} uniform forwards, one per distinct T, summed | {med['b_grouped']:.2f} | {min(times['b_grouped']):.2f} | {max(times['b_grouped']):.2f} | {spread['b_grouped'] * 100:.1f} % |",
        f"| (c) uniform | one uniform forward, B = {b_c}, T = {t_c} ({b_c * t_c} views) | {med['c_uniform']:.2f} | {min(times['c_uniform']):.2f} | {max(times['c_uniform']):.2f} | {spread['c_uniform'] * 100:.1f} % |",
        "",
        f"(a) / (b) = {med['a_ragged'] / med['b_grouped']:.3f}; (a) / (c) = {med['a_ragged'] / med['c_uniform']:.3f} "
        f"(per view: {med['a_ragged'] / n_views * 1e3:.1f} us against {med['c_uniform'] / (b_c * t_c) * 1e3:.1f} us).",
        "",
        "Device-event times around back-to-back forwards (encoder, decoder, corner decode; no host post-solve), every shape warmed up, the "
        "legs alternating inside each repeat.  Attention work grows with the square of a sample's views, so (a) carries the mix's long "
        "samples where (c) does not: the per-view difference between (a) and (c) is that, plus the missing sub-batch lanes of the ragged decoder call.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
