"""Dense MULTI-ROUND decode over a reference bank that keeps poses, measured: the multi-round facade forward (decode the filter_topk
kept references in rounds of sub_batch_size, one RANSAC pose over all rounds' corners, a fine decode on the fine_topk references
nearest to it) in three forms, in one run:

  (u)  un-banked      every one of the B (N + 1) views through the encoder on every forward (dense.process_multi_round, unchanged code:
                      the parent commit's figure)
  (f)  feature bank   RefFeatureBank(match_threshold, keep_poses=True): B query crops encoded; bd_match_select_rows, bd_round_sources,
                      bd_gather_view_rows, bd_pose_select_rows
  (e)  entry bank     the same bank with decoder=: the decoder assembles its token stream from the bank's entry rows, no heat map read

    python tools/dense_rounds_bench.py [--batch 8] [--refs 32] [--topk 20] [--sub 5] [--fine 5] [--out profiles/dense_rounds_bank.md]

each with pnp_on_device "wave" (bd_solve_pnp_ransac_wave) and with the host RANSAC, on a uniform batch and on one ragged mix of
database sizes (the un-banked mode takes no view_counts: there it is every sample run alone).  Full-depth synthetic models behind
the facade; legs warmed up, alternating inside every repeat, timed with a host clock around `inner` back-to-back forwards that end
in a device synchronise; a leg's figure is the median over the repeats.  With synthetic weights the decoded corners are noise, so the
RANSAC never stops early: its share here is the worst case.  No ratio is fixed in advance; a banked form that is not faster is
reported as such."""
import argparse
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from boxdreamer_amd import _lib, hip_ops                          # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from dense_bank_bench import THRESHOLD, build, launch_us, make_batch, timed   # noqa: E402


def posed(data):
    """The synthetic batch's poses are all the identity: give every view a translation of its own, ~0.1 apart in length, so that the
    fine level has an order to find (and no tie that two implementations may break differently)."""
    T = data["poses"].shape[1]
    t = torch.arange(T, device=data["poses"].device, dtype=torch.float32)
    data["poses"][:, :, :3, 3] = torch.stack([0.05 * t, -0.03 * t, 1 + 0.125 * t], dim=-1).to(data["poses"].dtype)
    return data


def fill(bank, data, counts, query, entry):
    t_max = data["images"].shape[1]
    table = []
    for b, (c, q) in enumerate(zip(counts, query)):
        slots = [t for t in range(c) if t != q]
        kw = {"bbox_feat": data["bbox_feat"][b, slots]} if entry else {}
        ids = bank.add(data["images"][b, slots], poses=data["poses"][b, slots], **kw).tolist()
        row = [-1] * t_max
        for t, r in zip(slots, ids):
            row[t] = r
        table.append(row)
    return table


def banks_for(model, data, counts, query):
    out = {}
    for name, entry in (("f", False), ("e", True)):
        bank = RefFeatureBank(model.rgb_encoder, keep_images=False, match_threshold=THRESHOLD, keep_poses=True,
                              decoder=model.decoder if entry else None)
        out[name] = (bank, fill(bank, data, counts, query, entry))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--refs", type=int, default=32)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--sub", type=int, default=5)
    ap.add_argument("--fine", type=int, default=5)
    ap.add_argument("--ragged-min", type=int, default=20)
    ap.add_argument("--ragged-max", type=int, default=48)
    ap.add_argument("--seed", type=int, default=20261019)
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
    if a.ragged_min < a.topk:
        ap.error("every database needs at least --topk views")
    _lib.require_gpu()
    dev = torch.device("cuda")
    model = build(a.prec, a.dino_depth, a.betr_depth, a.topk)
    model.dense_cfg = dict(model.dense_cfg, multi_round=True, sub_batch_size=a.sub, fine_level=True, fine_topk=a.fine, dense_mem_friendly=False)
    B, N, k, sub, fk = a.batch, a.refs, a.topk, a.sub, a.fine
    T, R = N + 1, -(-k // sub)
    data = posed(make_batch(B, T, a.seed, dev))
    query = [T - 1] * B
    model.pnp_on_device = "wave"
    model(dict(data))                                              # (the first forward also runs the load-time calibration, once)
    banks = banks_for(model, data, [T] * B, query)

    rng = random.Random(a.seed)
    sizes = [rng.randint(a.ragged_min, a.ragged_max) for _ in range(B)]
    counts = [n + 1 for n in sizes]
    t_max = max(counts)
    rdata = posed(make_batch(B, t_max, a.seed + 1, dev))
    rquery = [c - 1 for c in counts]
    rdata["query_idx"] = torch.tensor(rquery)
    rbanks = banks_for(model, rdata, counts, rquery)
    alone = [{key: (v[b:b + 1, :c].contiguous() if v.dim() > 1 else v[b:b + 1]) for key, v in rdata.items()} for b, c in enumerate(counts)]

    def uniform(name):
        if name == "u":
            return model(dict(data))
        bank, table = banks[name]
        return model(dict(data, ref_bank=bank, ref_rows=table))

    def ragged(name):
        if name == "u":
            return [model(dict(d)) for d in alone]
        bank, table = rbanks[name]
        return model(dict(rdata, ref_bank=bank, ref_rows=table, view_counts=counts))

    # the same outputs, and what waited for the device
    same, syncs, record = {}, {}, {}
    for solver in ("wave", False):
        model.pnp_on_device = solver
        uniform("u")
        want = (model.decoder.last_logits.clone(),)
        l_alone = []
        for d in alone:
            model(dict(d))
            l_alone.append(model.decoder.last_logits.clone())
        for name in ("f", "e"):
            out = uniform(name)
            same[(solver, name)] = bool(torch.equal(model.decoder.last_logits, want[0]))
            syncs[(solver, name)] = list(model.host_syncs_per_forward)
            record[name] = dict(out["hip_precision"]["ref_bank"])
            ragged(name)
            same[(solver, name, "ragged")] = bool(torch.equal(model.decoder.last_logits, torch.cat(l_alone)))

    def leg(solver, fn, name):
        def run():
            model.pnp_on_device = solver
            return fn(name)
        return run

    legs = {(s, shape, n): leg(s, fn, n) for s in ("wave", False) for shape, fn in (("uniform", uniform), ("ragged", ragged))
            for n in ("u", "f", "e")}
    times = timed(legs, a.repeats, a.inner, a.warmup)
    med = {key: statistics.median(v) for key, v in times.items()}

    # the two new launches alone, on the uniform batch's tables
    bank, table = banks["f"]
    plan = _lib.dense_bank_tables(_lib.ref_rows_table(table, B, T), [T] * B, k, query)
    rows_d, n_refs_d, q_d, q_flat = bank.dense_tables(plan[0], plan[1], plan[2], plan[3], T, dev)
    crops = data["images"].reshape(B * T, *data["images"].shape[2:]).index_select(0, q_flat)
    fresh = model.rgb_encoder.predict(crops)
    sel = bank.select(fresh, crops, rows_d, n_refs_d, k)[1]
    zero = bank.zero_row
    pred = torch.eye(4, device=dev).expand(B, 4, 4).contiguous()
    alone_us = {
        "bd_round_sources": launch_us(lambda: hip_ops.round_sources(rows_d, sel, len(bank), sub, zero, 0)),
        "bd_pose_select_rows": launch_us(lambda: hip_ops.pose_select_rows(bank.poses, len(bank), pred, rows_d, sel, fk)),
    }
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"

    solver_name = {"wave": '`"wave"`', False: "host"}
    what = {"u": "(u) un-banked", "f": "(f) feature bank", "e": "(e) entry bank"}

    def table_for(shape, unit):
        out = [f"| RANSAC | leg | ms per {unit} (median) | min | max | spread | vs (u) |", "|---|---|---|---|---|---|---|"]
        for s in ("wave", False):
            for n in ("u", "f", "e"):
                v, m = times[(s, shape, n)], med[(s, shape, n)]
                out.append(f"| {solver_name[s]} | {what[n]} | {m:.2f} | {min(v):.2f} | {max(v):.2f} | {(max(v) - min(v)) / m * 100:.1f} % | "
                           f"{m / med[(s, shape, 'u')]:.3f} ({med[(s, shape, 'u')] / m:.2f}x) |")
        return out

    slower = [f"{what[n]}, {shape}, {'wave' if s else 'host'} RANSAC" for (s, shape, n), m in med.items() if n != "u" and m >= med[(s, shape, "u")]]
    props = torch.cuda.get_device_properties(0)
    lines = [
        "# Dense multi-round decode over a reference bank that keeps poses",
        "",
        f"`tools/dense_rounds_bench.py --batch {B} --refs {N} --topk {k} --sub {sub} --fine {fk} --ragged-min {a.ragged_min} --ragged-max "
        f"{a.ragged_max} --seed {a.seed} --prec {a.prec} --dino-depth {a.dino_depth} --betr-depth {a.betr_depth} --repeats {a.repeats} "
        f"--inner {a.inner}` on {torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
        f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}; parent commit of the measured tree: `{commit}`.  "
        f"{a.repeats * a.inner} timed forwards per leg, all legs in this one run.",
        "",
        f"`dense_cfg`: multi_round, filter_topk {k}, sub_batch_size {sub} (R = {R} rounds, {R * sub - k} zero views pad the last one), "
        f"fine_level with fine_topk {fk}, ransac_trials default (1000).  (u) is `dense.process_multi_round`, which this change does not touch.",
        "",
        f"## Uniform batch, B = {B}, N = {N} database views per sample",
        "",
        *table_for("uniform", "forward"),
        "",
        f"Final logits bit-identical to (u)'s: " + ", ".join(f"{what[n]} / {'wave' if s else 'host'}: **{same[(s, n)]}**" for s in ("wave", False) for n in ("f", "e")) + ".",
        f"The forward's record: (f) `{record['f']}`, (e) `{record['e']}`.  What waited for the device: "
        + "; ".join(f"{what[n]} / {'wave' if s else 'host'}: `{syncs[(s, n)]}`" for s in ("wave", False) for n in ("f", "e")) + ".",
        "",
        f"## Ragged mix: {B} samples, database sizes drawn once from [{a.ragged_min}, {a.ragged_max}] with seed {a.seed}: {sizes} "
        f"({sum(sizes)} database views, T_max = {t_max})",
        "",
        f"(u) is {B} un-banked forwards of batch 1, each at its own size ({sum(counts)} views encoded); (f) and (e) are ONE banked forward with "
        "`view_counts`.",
        "",
        *table_for("ragged", "batch"),
        "",
        "Final logits bit-identical to the samples run alone: "
        + ", ".join(f"{what[n]} / {'wave' if s else 'host'}: **{same[(s, n, 'ragged')]}**" for s in ("wave", False) for n in ("f", "e")) + ".",
        "",
        "## The two new launches alone (uniform batch's tables)",
        "",
        "| launch | work | us per launch |",
        "|---|---|---|",
        f"| `bd_round_sources` | {B} workgroups: {B * R * (sub + 1)} entries of `src` and of `view` | {alone_us['bd_round_sources']:.1f} |",
        f"| `bd_pose_select_rows` | {B} workgroups: {B * k} fp64 pose distances, {fk} of {k} by rank, compaction | {alone_us['bd_pose_select_rows']:.1f} |",
        "",
        "Mean of 50 launches in a row after 5 warm-up launches, device events around the loop, the wrappers' output allocations included: "
        "launch-bound figures.",
        "",
        "Forward times are host-clock times around back-to-back facade forwards ending in a device synchronise, every leg warmed up, the "
        "legs alternating inside each repeat.  The models carry synthetic weights: the decoded corners are noise, every RANSAC runs all "
        "its trials and fails, and the fine level ranks the references against an all-zero coarse pose -- the arithmetic and the launches "
        "are those of a real forward, the RANSAC's share is its worst case.",
    ]
    if slower:
        lines += ["", "**Not faster than (u): " + "; ".join(slower) + ".**"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
