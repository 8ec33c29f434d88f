"""Dense-reference mode over the reference bank, measured: the banked dense forward (B query crops encoded, references scored, selected
and gathered from the bank) against the un-banked dense forward (every database view through the encoder, every forward), on a uniform
batch and on one ragged mix of database sizes.

    python tools/dense_bank_bench.py [--batch 8] [--refs 32] [--topk 5] [--prec f16c8_qk16] [--repeats 7] [--inner 3] [--out profiles/dense_bank.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers) behind the facade, `BoxDreamer(config)(data)` with `dense_cfg.enable`,
filter = 'dino': a forward is everything the facade does, the corners' D2H and the host pose solve included.  Every leg is warmed up
and timed with a host clock around `inner` back-to-back forwards that end in a device synchronise (repeats x inner >= 20 steps); the
legs alternate inside every repeat so that drift hits all alike; a leg's figure is the median over the repeats.  Uniform batch:
  (a)  un-banked  `dense_cfg.enable` alone: B (N + 1) views through the encoder, bd_dino_match_scores + bd_topk_mask, boolean-mask re-pack;
  (c)  banked     `ref_bank` with match summaries: B crops encoded, bd_match_view_sums + bd_match_select_rows + bd_gather_view_rows.
Ragged mix (database sizes drawn once from [--ragged-min, --ragged-max]): the un-banked dense mode takes no `view_counts`, so
  (a') is every sample run alone, un-banked, at its own size (B forwards of batch 1), and
  (c') is ONE banked forward with `view_counts`.
(a) and (c) -- and (a') and (c') -- give the same logits and the same selection (checked here, bit for bit).  The three new launches
are also timed alone."""
import argparse
import os
import random
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boxdreamer_amd import _lib, hip_ops, synth                   # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from boxdreamer_amd.model import BoxDreamer                       # noqa: E402

THRESHOLD = 0.05


def build(prec, dino_depth, betr_depth, topk):
    cfg = {"modules": {
        "use_keypoints": False, "use_matching": False, "use_tracking": False, "use_rgb": True, "use_pp": True,
        "regression_intri": True, "rotation_type": None, "coordinate": "object", "pose_representation": "bb8",
        "bbox_representation": "heatmap", "patchify_rays": True,
        "dense_cfg": {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": topk, "multi_round": False},
        "decoder": {"d_model": 768, "nhead": 8, "num_decoder_layers": betr_depth, "decoder_only": True, "patch_size": 14, "img_size": 224,
                    "diff_emb": False, "nvs_supervision": False, "ray_supervision": True, "use_mask": False, "hip_precision": prec},
        "encoder": {"name": "dino", "dino": {"ckpt_path": None, "cfg": {"model_type": "dinov2_vitb14_reg", "synthetic_seed": 4321,
                                                                        "depth": dino_depth, "hip_precision": prec}}}}}
    model = BoxDreamer(cfg)
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(seed=1234, depth=betr_depth).items()}, strict=True)
    return model.cuda().eval()


def make_batch(B, T, seed, dev):
    """A batch dict on the device, bf16: crops in [0, 1] with a black border of a different width per view (distinct foreground
    counts), the query in the last slot."""
    data = synth.make_batch(seed=seed, B=B, T=T, dtype=torch.bfloat16)
    img = (data["images"].float() * 0.25 + 0.5).clamp(0, 1)
    for b in range(B):
        for t in range(T):
            w = 14 * ((3 * b + 2 * t) % 5)
            img[b, t, :, :w] = 0
            img[b, t, :, 224 - w:] = 0
            img[b, t, :, :, :w] = 0
            img[b, t, :, :, 224 - w:] = 0
    data["images"] = img.to(torch.bfloat16)
    return {k: v.to(dev) if torch.is_tensor(v) and k != "query_idx" else v for k, v in data.items()}


def fill(bank, data, counts, query):
    """Each sample's references into the bank -> the (B, T_max) host table, -1 at the query."""
    t_max = data["images"].shape[1]
    table = []
    for b, (c, q) in enumerate(zip(counts, query)):
        slots = [t for t in range(c) if t != q]
        ids = bank.add(data["images"][b, slots]).tolist()
        row = [-1] * t_max
        for t, r in zip(slots, ids):
            row[t] = r
        table.append(row)
    return table


def timed(legs, repeats, inner, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return times


def launch_us(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--refs", type=int, default=32)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--ragged-min", type=int, default=8)
    ap.add_argument("--ragged-max", type=int, default=48)
    ap.add_argument("--seed", type=int, default=20261018)
    ap.add_argument("--prec", default=_lib.DEFAULT_PREC)
    ap.add_argument("--dino-depth", type=int, default=12)
    ap.add_argument("--betr-depth", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="commit the measured tree sits on (default: git rev-parse, where the tree is a checkout)")
    a = ap.parse_args()
    if a.repeats * a.inner < 20:
        ap.error("repeats x inner must be at least 20 steps")
    _lib.require_gpu()
    dev = torch.device("cuda")
    model = build(a.prec, a.dino_depth, a.betr_depth, a.topk)
    B, N, k = a.batch, a.refs, a.topk
    T = N + 1
    data = make_batch(B, T, a.seed, dev)
    query = [T - 1] * B
    out_a = model(dict(data))                                      # (the first forward also runs the load-time calibration, once)
    logits_a, bbox_a = model.decoder.last_logits.clone(), out_a["bbox_feat"].clone()
    bank = RefFeatureBank(model.rgb_encoder, keep_images=False, match_threshold=THRESHOLD)
    table = fill(bank, data, [T] * B, query)
    out_c = model(dict(data, ref_bank=bank, ref_rows=table))
    same_u = bool(torch.equal(model.decoder.last_logits, logits_a) and torch.equal(out_c["bbox_feat"], bbox_a)
                  and torch.equal(out_c["pred_corners_px"], out_a["pred_corners_px"]))
    syncs_c = list(model.host_syncs_per_forward)
    record = dict(out_c["hip_precision"]["ref_bank"])

    # ragged mix
    rng = random.Random(a.seed)
    sizes = [rng.randint(a.ragged_min, a.ragged_max) for _ in range(B)]
    counts = [n + 1 for n in sizes]
    t_max = max(counts)
    rdata = make_batch(B, t_max, a.seed + 1, dev)
    rquery = [c - 1 for c in counts]
    rdata["query_idx"] = torch.tensor(rquery)
    rbank = RefFeatureBank(model.rgb_encoder, keep_images=False, match_threshold=THRESHOLD)
    rtable = fill(rbank, rdata, counts, rquery)
    alone = [{key: (v[b:b + 1, :c].contiguous() if v.dim() > 1 else v[b:b + 1]) for key, v in rdata.items()} for b, c in enumerate(counts)]

    def leg_alone():
        return [model(dict(d)) for d in alone]

    def leg_ragged():
        return model(dict(rdata, ref_bank=rbank, ref_rows=rtable, view_counts=counts))

    l_alone = []
    for d in alone:
        model(dict(d))
        l_alone.append(model.decoder.last_logits.clone())
    leg_ragged()
    same_r = bool(torch.equal(model.decoder.last_logits, torch.cat(l_alone)))

    legs = {
        "a": lambda: model(dict(data)),
        "c": lambda: model(dict(data, ref_bank=bank, ref_rows=table)),
        "ar": leg_alone,
        "cr": leg_ragged,
    }
    times = timed(legs, a.repeats, a.inner, a.warmup)
    med = {key: statistics.median(v) for key, v in times.items()}

    # the three new launches alone, on the uniform batch's tables
    plan = _lib.dense_bank_tables(_lib.ref_rows_table(table, B, T), [T] * B, k, query)
    rows_d, n_refs_d, q_d, q_flat = bank.dense_tables(plan[0], plan[1], plan[2], plan[3], T, dev)
    crops = data["images"].reshape(B * T, *data["images"].shape[2:]).index_select(0, q_flat)
    fresh = model.rgb_encoder.predict(crops)
    q_sums, q_counts = hip_ops.match_view_sums(fresh, crops, THRESHOLD)
    scores, sel, src = bank.select(fresh, crops, rows_d, n_refs_d, k)
    alone_us = {
        "bd_match_view_sums": launch_us(lambda: hip_ops.match_view_sums(fresh, crops, THRESHOLD, q_sums, q_counts)),
        "bd_match_select_rows": launch_us(lambda: hip_ops.match_select_rows(bank._msums, bank._mcounts, len(bank), q_sums, q_counts, rows_d,
                                                                            n_refs_d, bank.tokens_per_view, k)),
        "bd_gather_view_rows": launch_us(lambda: bank.gather(src, fresh, (B, k + 1))),
    }
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"

    def row(label, what, key):
        v = times[key]
        return f"| {label} | {what} | {med[key]:.2f} | {min(v):.2f} | {max(v):.2f} | {(max(v) - min(v)) / med[key] * 100:.1f} % |"

    P, C = bank.tokens_per_view, bank.feature_dim
    props = torch.cuda.get_device_properties(0)
    faster = med["c"] < med["a"]
    lines = [
        "# Dense-reference mode over the reference bank: score, select, gather",
        "",
        f"`tools/dense_bank_bench.py --batch {B} --refs {N} --topk {k} --ragged-min {a.ragged_min} --ragged-max {a.ragged_max} --seed {a.seed} "
        f"--prec {a.prec} --dino-depth {a.dino_depth} --betr-depth {a.betr_depth} --repeats {a.repeats} --inner {a.inner}` on "
        f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
        f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}; parent commit of the measured tree: `{commit}`.  "
        f"{a.repeats * a.inner} timed forwards per leg.",
        "",
        f"## Uniform batch, B = {B}, N = {N} database views per sample, k = {k}",
        "",
        f"(a) and (c) give bit-identical logits, corners and re-packed `bbox_feat` (hence the same selection): **{same_u}**.",
        "",
        "| leg | what runs | ms per forward (median) | min | max | spread |",
        "|---|---|---|---|---|---|",
        row("(a) un-banked dense", f"all {B * T} views through the encoder, `bd_dino_match_scores` + `bd_topk_mask`, boolean-mask re-pack", "a"),
        row("(c) banked dense", f"{B} query crops through the encoder, `bd_match_view_sums` + `bd_match_select_rows` + "
            f"`bd_gather_view_rows`, integer-index re-pack; decoder on ({B}, {k + 1})", "c"),
        "",
        f"(c) / (a) = {med['c'] / med['a']:.3f} ({med['a'] / med['c']:.2f}x).  (c) faster than (a): **{faster}**.  The forward's record: "
        f"`{record}`; what waited for the device in (c): `{syncs_c}`.",
        "",
        f"The bank holds {len(bank)} views: {bank.bytes_per_view / 1e3:.0f} KB of operand row and {(C + 1) * 4 / 1e3:.1f} KB of match summary "
        f"per view (P = {P}, C = {C}).",
        "",
        f"## Ragged mix: {B} samples, database sizes drawn once from [{a.ragged_min}, {a.ragged_max}] with seed {a.seed}: {sizes} "
        f"({sum(sizes)} database views, T_max = {t_max})",
        "",
        f"(a') and (c') give bit-identical logits: **{same_r}**.",
        "",
        "| leg | what runs | ms per batch (median) | min | max | spread |",
        "|---|---|---|---|---|---|",
        row("(a') un-banked, sample by sample", f"{B} un-banked dense forwards of batch 1, each at its own size ({sum(counts)} views encoded)", "ar"),
        row("(c') banked, ragged", f"ONE banked dense forward with `view_counts`: {B} crops encoded, {sum(sizes)} references scored", "cr"),
        "",
        f"(c') / (a') = {med['cr'] / med['ar']:.3f} ({med['ar'] / med['cr']:.2f}x).",
        "",
        "## The three new launches alone (uniform batch's tables)",
        "",
        "| launch | work | us per launch |",
        "|---|---|---|",
        f"| `bd_match_view_sums` | {B} query views, {P} x {C} fp32 features each | {alone_us['bd_match_view_sums']:.1f} |",
        f"| `bd_match_select_rows` | {B} workgroups: {B * N} pair scores from {C}-float summaries, top-{k} of {N}, compaction | {alone_us['bd_match_select_rows']:.1f} |",
        f"| `bd_gather_view_rows` | {B * (k + 1)} views of {bank.bytes_per_view / 1e3:.0f} KB from the device `src` table | {alone_us['bd_gather_view_rows']:.1f} |",
        "",
        "Mean of 50 launches in a row after 5 warm-up launches, device events around the loop (the gather's output allocation included); "
        "back to back the inputs stay in cache, so these are launch-bound figures, not HBM-bound ones.  `bd_match_view_sums` is the "
        "per-view kernel of `bd_dino_match_scores` unchanged (one workgroup per view, so that a view's summary has the same bits "
        f"whichever entry made it): with {B} views it occupies {B} of the device's CUs and its time is the latency of one view's two "
        "passes over its features, not a throughput figure.",
        "",
        "Forward times are host-clock times around back-to-back facade forwards ending in a device synchronise (encoder, selection, decoder, "
        "corner decode, the corners' D2H and the host pose solve), every leg warmed up, the legs alternating inside each repeat.",
    ]
    if not faster:
        lines += ["", "**(c) is not faster than (a): a defect, to be explained here before this file is relied on.**"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
