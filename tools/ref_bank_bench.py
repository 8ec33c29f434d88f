"""Cached reference features, measured: the reference bank (one bd_gather_view_rows launch) against the mask-indexing cache path and
against no cache at all, on a uniform batch and on one ragged mix.

    python tools/ref_bank_bench.py [--batch 32] [--views 6] [--prec f16c8_qk16] [--repeats 7] [--inner 3] [--out profiles/ref_bank.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers), encoder -> decoder -> corner decode per forward, no host post-solve.
Every leg is warmed up and timed with device events around `inner` back-to-back forwards (repeats x inner >= 20 steps); the legs
alternate inside every repeat so that drift hits all alike; a leg's figure is the median over the repeats.  Uniform batch (B, T):
  (a)  uncached   every view through the encoder;
  (b)  cache      RefFeatureCache.place + merge_cached_features (boolean-mask writes, fp32 + operand clones), measured TWICE
                  ((b1), (b2)): their difference is the run-to-run spread (c) is judged against;
  (b') merge      the same with `place` hoisted out of the forward (what a caller with a fixed batch layout can do);
  (c)  bank       RefFeatureBank: the B query crops through the encoder, one gather launch, operand-only features.
Ragged mix (tools/ragged_bench.py's draw): (a') `view_counts` uncached against (c') `view_counts` + bank.
(a), (b), (c) -- and (a'), (c') -- compute the same logits (checked here, bit for bit).  The gather launch is also timed alone."""
import argparse
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from boxdreamer_amd import _lib, hip_ops                          # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank, RefFeatureCache, merge_cached_features      # noqa: E402
from ragged_bench import CHOICES, build                            # noqa: E402


def banked_forward(enc, dec, bank, img, bf, mask, rows, counts, t_max):
    B = img.shape[0]
    cts = counts if counts is not None else [t_max] * B
    src, encode, _ = bank.tables(rows, cts, t_max, img.device)
    fresh = enc.predict(img.flatten(0, 1).index_select(0, encode))
    feats = bank.gather(src, fresh, (B, t_max) if counts is None else (sum(cts),))
    heat = dec(bf, img, mask, feats, None, view_counts=counts)
    return hip_ops.decode_topk(heat)[0], dec.last_logits


def plain_forward(enc, dec, img, bf, mask, feats=None, counts=None, index=None):
    if feats is None:
        feats = enc.predict(img if index is None else img.flatten(0, 1).index_select(0, index))
    heat = dec(bf, img, mask, feats, None, view_counts=counts)
    return hip_ops.decode_topk(heat)[0], dec.last_logits


def make_inputs(B, t_max, query, seed, dev):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, t_max, 3, 224, 224), generator=g).to(torch.bfloat16).to(dev)
    bf = (torch.rand((B, t_max, 8, 224, 224), generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
    mask = torch.zeros((B, t_max), dtype=torch.bool)
    mask[torch.arange(B), torch.tensor(query)] = True
    return img, bf, mask.to(dev)


def fill(bank, img, counts, query):
    """Each sample's references into the bank -> the (B, T_max) host table."""
    t_max = img.shape[1]
    table = []
    for b, (c, q) in enumerate(zip(counts, query)):
        slots = [t for t in range(c) if t != q]
        ids = bank.add(img[b, slots]).tolist()
        row = [-1] * t_max
        for t, r in zip(slots, ids):
            row[t] = r
        table.append(row)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--ragged-samples", type=int, default=32)
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
    if a.repeats * a.inner < 20:
        ap.error("repeats x inner must be at least 20 steps")
    dev = torch.device("cuda")
    enc, dec = build(a.prec, a.dino_depth, a.betr_depth)
    B, T = a.batch, a.views
    query = [T - 1] * B
    img, bf, mask = make_inputs(B, T, query, a.seed, dev)
    qidx = torch.tensor(query).to(dev)
    # (b): today's cache
    cache = RefFeatureCache(enc)
    ref_feats = cache.encode(img[:, :T - 1].contiguous())
    placed = cache.place(ref_feats, qidx, T)
    # (c): the bank
    bank = RefFeatureBank(enc, keep_images=False)
    rows = _lib.ref_rows_table(fill(bank, img, [T] * B, query), B, T)
    # ragged mix
    rng = random.Random(a.seed)
    counts = [rng.choice(CHOICES) for _ in range(a.ragged_samples)]
    Br, t_max, n_views = len(counts), max(counts), sum(counts)
    rquery = [c - 1 for c in counts]
    rimg, rbf, rmask = make_inputs(Br, t_max, rquery, a.seed + 1, dev)
    index = torch.tensor(_lib.packing_index(counts, t_max)).to(dev)
    rbank = RefFeatureBank(enc, keep_images=False)
    rrows = _lib.ref_rows_table(fill(rbank, rimg, counts, rquery), Br, t_max)

    def leg_b():
        cached, valid = cache.place(ref_feats, qidx, T)
        return plain_forward(enc, dec, img, bf, mask, merge_cached_features(enc, img, cached, valid))

    legs = {
        "a": lambda: plain_forward(enc, dec, img, bf, mask),
        "b1": leg_b,
        "bm": lambda: plain_forward(enc, dec, img, bf, mask, merge_cached_features(enc, img, *placed)),
        "c": lambda: banked_forward(enc, dec, bank, img, bf, mask, rows, None, T),
        "b2": leg_b,
        "ar": lambda: plain_forward(enc, dec, rimg, rbf, rmask, counts=counts, index=index),
        "cr": lambda: banked_forward(enc, dec, rbank, rimg, rbf, rmask, rrows, counts, t_max),
    }
    logits = {k: fn()[1].clone() for k, fn in legs.items()}
    same_u = all(bool(torch.equal(logits["a"], logits[k])) for k in ("b1", "bm", "c"))
    same_r = bool(torch.equal(logits["ar"], logits["cr"]))
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
    # the gather launch alone
    gather = {}
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    for name, bk, rw, cts, tm, im in (("uniform", bank, rows, [T] * B, T, img), ("ragged", rbank, rrows, counts, t_max, rimg)):
        src, encode, n_fresh = bk.tables(rw, cts, tm, dev)
        fresh = enc.predict(im.flatten(0, 1).index_select(0, encode))
        nv = sum(cts)
        for _ in range(3):
            bk.gather(src, fresh, (nv,))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            bk.gather(src, fresh, (nv,))
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        # the same launch with the caches flushed before it: a 1 GiB fill (four times the 256 MB last-level cache) evicts the bank rows,
        # as a forward's encoder and decoder traffic does between two gathers
        cold = []
        for _ in range(10):
            flush.fill_(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bk.gather(src, fresh, (nv,))
            e1.record()
            e1.synchronize()
            cold.append(e0.elapsed_time(e1) * 1e3)
        cold_us = statistics.median(cold)
        moved = 2 * nv * bk.bytes_per_view                     # every byte of the operand is read once and written once
        gather[name] = (nv, us, moved, moved / (us * 1e-6) / 1e12, cold_us, moved / (cold_us * 1e-6) / 1e12)
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    spread = abs(med["b1"] - med["b2"])
    b_worst = max(med["b1"], med["b2"])
    ok = med["c"] <= b_worst + spread
    P, C = bank.tokens_per_view, bank.feature_dim
    old_bytes = B * T * P * C * 4 + B * T * bank.bytes_per_view

    def row(label, what, k):
        v = times[k]
        return f"| {label} | {what} | {med[k]:.2f} | {min(v):.2f} | {max(v):.2f} | {(max(v) - min(v)) / med[k] * 100:.1f} % |"

    hist = {t: counts.count(t) for t in sorted(set(counts))}
    lines = [
        "# Reference bank: cached reference features through one gather launch",
        "",
        f"`tools/ref_bank_bench.py --batch {B} --views {T} --ragged-samples {a.ragged_samples} --seed {a.seed} --prec {a.prec} "
        f"--dino-depth {a.dino_depth} --betr-depth {a.betr_depth} --repeats {a.repeats} --inner {a.inner}` on "
        f"{torch.cuda.get_device_name(0)}; parent commit of the measured tree: `{commit}`.  {a.repeats * a.inner} timed steps per leg.",
        "",
        f"## Uniform batch, B = {B}, T = {T} ({B * T} views, {B} of them queries)",
        "",
        f"(a), (b), (b'), (c) give bit-identical logits: **{same_u}**.",
        "",
        "| leg | what runs | ms per forward (median) | min | max | spread |",
        "|---|---|---|---|---|---|",
        row("(a) uncached", f"all {B * T} views through the encoder", "a"),
        row("(b1) cache", "`RefFeatureCache.place` + `merge_cached_features`, first measurement", "b1"),
        row("(b2) cache", "the same leg measured again in the same run", "b2"),
        row("(b') merge only", "`merge_cached_features` with `place` hoisted out of the forward", "bm"),
        row("(c) bank", f"`RefFeatureBank`: {B} crops encoded, one `bd_gather_view_rows` launch, operand-only features", "c"),
        "",
        f"Run-to-run spread of (b): |(b1) - (b2)| = {spread:.3f} ms.  (c) - max(b1, b2) = {med['c'] - b_worst:+.3f} ms "
        f"((c) / (b) = {med['c'] / b_worst:.3f}; (c) / (a) = {med['c'] / med['a']:.3f}).  "
        f"(c) not slower than (b) beyond that spread: **{ok}**.",
        "",
        f"Bytes per forward for the feature hand-off: (b) clones {old_bytes / 1e6:.0f} MB (fp32 + operand copy of all {B * T} views, read and "
        f"written) before its masked writes; (c) writes the {B * T * bank.bytes_per_view / 1e6:.0f} MB operand once.",
        "",
        f"## Ragged mix: {Br} samples, view counts drawn once from {list(CHOICES)} with seed {a.seed}: {hist} (count per T), {n_views} views, T_max = {t_max}",
        "",
        f"(a') and (c') give bit-identical logits: **{same_r}**.",
        "",
        "| leg | what runs | ms per forward (median) | min | max | spread |",
        "|---|---|---|---|---|---|",
        row("(a') ragged uncached", f"`view_counts`, all {n_views} packed views through the encoder", "ar"),
        row("(c') ragged bank", f"`view_counts` + bank: {Br} crops encoded, one gather launch over {n_views} views", "cr"),
        "",
        f"(c') / (a') = {med['cr'] / med['ar']:.3f}.",
        "",
        "## The gather launch alone",
        "",
        "| batch | views | bytes moved (read + written) | back to back: us per launch | TB/s | caches flushed: us per launch | TB/s |",
        "|---|---|---|---|---|---|---|",
    ] + [f"| {k} | {nv} | {moved / 1e6:.1f} MB | {us:.1f} | {tbs:.2f} | {cus:.1f} | {ctbs:.2f} |"
         for k, (nv, us, moved, tbs, cus, ctbs) in gather.items()] + [
        "",
        "\"Back to back\" is the mean of 20 launches in a row over the same source rows (output allocation included): the rows stay in the "
        "L2 / last-level cache between launches, so that rate is a cache figure, NOT an HBM-bound one.  \"Caches flushed\" is the median of "
        "10 single launches, each after a 1 GiB fill that evicts the rows -- the state a forward leaves behind; its time includes the "
        "launch's own start-up, which a single timed launch cannot hide.  The (c) against (b) comparison above depends on neither.",
        "",
        "Device-event times around back-to-back forwards (encoder, decoder, corner decode; no host post-solve), every leg warmed up, the "
        "legs alternating inside each repeat.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
