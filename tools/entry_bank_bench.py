"""Decoder-entry tokens kept in the reference bank, measured: a forward over an entry-token bank (RefFeatureBank(decoder=...): the
decoder assembles its token stream from banked rows, no heat map is patchified or embedded) against the forward over the feature bank
(whose code is unchanged), in one run, on
  case 1   a uniform batch, B = 32, T = 6 (plain banked forward), and
  case 2   the banked dense mode, B = 8, N = 32 database views per sample, filter_topk = 5.

    python tools/entry_bank_bench.py [--prec f16c8_qk16] [--repeats 7] [--inner 3] [--out profiles/entry_bank.md]

Full-depth synthetic models (DINOv2 ViT-B/14 + 12 BETR layers) behind the facade, `BoxDreamer(config)(data)`, on tools/dense_bank_bench.py's
harness: a forward is everything the facade does, the corners' D2H and the host pose solve included; every leg is warmed up and timed
with a host clock around `inner` back-to-back forwards that end in a device synchronise (repeats x inner >= 20 steps); the legs
alternate inside every repeat so that drift hits all alike; a leg's figure is the median over the repeats.  Legs per case:
  (f1), (f2)  the feature bank, measured twice: their difference is the run-to-run spread the others are judged against;
  (e)         the entry bank with `bbox_feat` in the dict (never read by the decoder; cloned into `pred_bbox` as ever);
  (n)         the entry bank without `bbox_feat` (no clone; `pred_query_bbox` instead).
All legs of a case compute the same logits (checked here, bit for bit).  The bd_assemble_entry_tokens launch is also timed alone,
back to back and after a cache flush."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from boxdreamer_amd import _lib, hip_ops                          # noqa: E402
from boxdreamer_amd.cache import RefFeatureBank                   # noqa: E402
from dense_bank_bench import THRESHOLD, build, make_batch, timed  # noqa: E402

MARGIN = 0.02      # profiles/ref_bank.md: two measurements of one configuration in one run lay 26.52 / 26.09 ms apart


def fill(bank, data, query, entry):
    """Each sample's references into the bank (an entry bank: with their heat maps) -> the (B, T) host table, -1 at the query."""
    T = data["images"].shape[1]
    table = []
    for b, q in enumerate(query):
        slots = [t for t in range(T) if t != q]
        kw = {"bbox_feat": data["bbox_feat"][b, slots]} if entry else {}
        ids = bank.add(data["images"][b, slots], **kw).tolist()
        table.append([-1 if t == q else ids.pop(0) for t in range(T)])
    return table


def run_case(model, data, match, a):
    """-> (median ms per leg, all times, logits identical, the entry bank, its table)."""
    B, T = data["images"].shape[:2]
    query = [T - 1] * B
    kw = {"match_threshold": THRESHOLD} if match else {}
    fbank = RefFeatureBank(model.rgb_encoder, keep_images=False, **kw)
    ebank = RefFeatureBank(model.rgb_encoder, keep_images=False, decoder=model.decoder, **kw)
    ftable, etable = fill(fbank, data, query, False), fill(ebank, data, query, True)
    lean = {k: v for k, v in data.items() if k != "bbox_feat"}
    legs = {
        "f1": lambda: model(dict(data, ref_bank=fbank, ref_rows=ftable)),
        "e": lambda: model(dict(data, ref_bank=ebank, ref_rows=etable)),
        "n": lambda: model(dict(lean, ref_bank=ebank, ref_rows=etable)),
        "f2": lambda: model(dict(data, ref_bank=fbank, ref_rows=ftable)),
    }
    logits = {}
    for k, fn in legs.items():
        fn()
        logits[k] = model.decoder.last_logits.clone()
    same = all(bool(torch.equal(logits["f1"], v)) for v in logits.values())
    times = timed(legs, a.repeats, a.inner, a.warmup)
    return {k: statistics.median(v) for k, v in times.items()}, times, same, ebank, etable


def assemble_alone(model, bank, src, n_fresh, dev):
    """The bd_assemble_entry_tokens launch of one forward, alone: (views, bytes read + written, us back to back, us after a cache flush)."""
    w = model.decoder._weights(dev, model.decoder.hip_precision)
    pos = w.named["pos_table"]
    qtok = model.decoder.bbox_learnable_query.detach().float().reshape(-1).contiguous()
    P, D = bank.entry_tokens.shape[1:]
    nv = int(src.numel())
    rgb = torch.randn((n_fresh, P, D), device=dev)
    out = torch.empty((nv, P, D), device=dev)
    fn = lambda: hip_ops.assemble_entry_tokens(bank.entry_tokens, len(bank), rgb, n_fresh, pos, qtok, src, out, nv, P, D)
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    e1.synchronize()
    warm = e0.elapsed_time(e1) / 20 * 1e3
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)       # four times the 256 MB last-level cache
    cold = []
    for _ in range(10):
        flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        cold.append(e0.elapsed_time(e1) * 1e3)
    moved = 2 * nv * P * D * 4 + n_fresh * P * D * 4                  # every view read once and written once; the query views also read pos
    return nv, moved, warm, statistics.median(cold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--dense-batch", type=int, default=8)
    ap.add_argument("--dense-refs", type=int, default=32)
    ap.add_argument("--topk", type=int, default=5)
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
    _lib.require_gpu()
    dev = torch.device("cuda")
    dense_model = build(a.prec, a.dino_depth, a.betr_depth, a.topk)
    plain_model = build(a.prec, a.dino_depth, a.betr_depth, a.topk)
    plain_model.dense_cfg = None                                       # case 1: the plain banked forward
    B, T, Bd, N, k = a.batch, a.views, a.dense_batch, a.dense_refs, a.topk
    cases = []
    for name, model, data, match in ((f"uniform batch, B = {B}, T = {T}", plain_model, make_batch(B, T, a.seed, dev), False),
                                     (f"banked dense mode, B = {Bd}, N = {N}, k = {k}", dense_model, make_batch(Bd, N + 1, a.seed + 1, dev), True)):
        model(dict({kk: v[:2] for kk, v in data.items()}))              # (the first forward runs the load-time calibration, once)
        med, times, same, ebank, etable = run_case(model, data, match, a)
        nb = data["images"].shape[0]
        tv = data["images"].shape[1]
        if match:                                                       # the table bd_match_select_rows writes for this batch
            plan = _lib.dense_bank_tables(_lib.ref_rows_table(etable, nb, tv), [tv] * nb, k, [tv - 1] * nb)
            rows_d, n_refs_d, _, q_flat = ebank.dense_tables(plan[0], plan[1], plan[2], plan[3], tv, dev)
            crops = data["images"].reshape(nb * tv, *data["images"].shape[2:]).index_select(0, q_flat)
            src = ebank.select(model.rgb_encoder.predict(crops), crops, rows_d, n_refs_d, k)[2]
        else:
            src = ebank.tables(_lib.ref_rows_table(etable, nb, tv), [tv] * nb, tv, dev)[0]
        cases.append((name, med, times, same, assemble_alone(model, ebank, src, nb, dev), ebank, data))
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    props = torch.cuda.get_device_properties(0)
    lines = [
        "# Reference bank with decoder-entry tokens: a banked forward without bbox_feat",
        "",
        f"`tools/entry_bank_bench.py --batch {B} --views {T} --dense-batch {Bd} --dense-refs {N} --topk {k} --seed {a.seed} --prec {a.prec} "
        f"--dino-depth {a.dino_depth} --betr-depth {a.betr_depth} --repeats {a.repeats} --inner {a.inner}` on "
        f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; "
        f"parent commit of the measured tree: `{commit}`.  {a.repeats * a.inner} timed forwards per leg; a forward is the whole facade call "
        "(encoder on the query crops, decoder, corner decode, the corners' D2H, host pose solve).",
        "",
    ]
    verdicts = []
    for name, med, times, same, alone, ebank, data in cases:
        feat = statistics.median(times["f1"] + times["f2"])
        spread = abs(med["f1"] - med["f2"])
        bbox_mb = data["bbox_feat"].numel() * data["bbox_feat"].element_size() / 1e6

        def row(label, what, key):
            v = times[key]
            return f"| {label} | {what} | {med[key]:.2f} | {min(v):.2f} | {max(v):.2f} | {med[key] / feat:.3f} |"

        ok = med["e"] <= feat * (1 + MARGIN) and med["n"] <= feat * (1 + MARGIN)
        verdicts.append(ok)
        nv, moved, warm, cold = alone
        lines += [
            f"## {name}",
            "",
            f"All four legs give bit-identical logits: **{same}**.  The feature bank's figure is the median over both of its legs' repeats: "
            f"{feat:.2f} ms; |(f1) - (f2)| = {spread:.3f} ms ({spread / feat * 100:.1f} %).",
            "",
            "| leg | what runs | ms per forward (median) | min | max | ratio to the feature bank |",
            "|---|---|---|---|---|---|",
            row("(f1) feature bank", "`bd_gather_view_rows` + the whole decoder chain on every view's heat maps", "f1"),
            row("(e) entry bank, `bbox_feat` in the dict", f"`bd_decoder_forward_entry`; the batch's {bbox_mb:.0f} MB `bbox_feat` goes into `pred_bbox` as ever (re-packed first in the dense mode), never read by the decoder", "e"),
            row("(n) entry bank, no `bbox_feat`", "`bd_decoder_forward_entry`; `pred_query_bbox` instead of the clone", "n"),
            row("(f2) feature bank", "the same leg as (f1), measured again in the same run", "f2"),
            "",
            f"Entry bank no slower than the feature bank beyond the {MARGIN * 100:.0f} % margin: **{ok}** "
            f"((e) / feature = {med['e'] / feat:.3f}, (n) / feature = {med['n'] / feat:.3f}).",
            "",
            f"`bd_assemble_entry_tokens` alone on this batch's source table: {nv} views of {ebank.entry_bytes_per_view / 1e3:.0f} KB, "
            f"{moved / 1e6:.1f} MB read + written.  Back to back: {warm:.1f} us per launch ({moved / (warm * 1e-6) / 1e12:.2f} TB/s, a cache "
            f"figure: the rows stay in the L2 / last-level cache between launches); after a 1 GiB fill that evicts them (median of 10 single "
            f"launches, the launch's own start-up included): {cold:.1f} us ({moved / (cold * 1e-6) / 1e12:.2f} TB/s).",
            "",
            f"Per banked view the entry store holds {ebank.entry_bytes_per_view} bytes next to the feature row's {ebank.bytes_per_view}.",
            "",
        ]
    lines += [
        "Host-clock times around back-to-back forwards that end in a device synchronise, every leg warmed up, the legs alternating "
        "inside each repeat.  From FLOP counts the references' adapter and `bbox_emb` work is about 2 % of the decoder: a few percent on "
        "the step, and the removal of the `bbox_feat` clone in (n), is all this mode is expected to give.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if not all(verdicts):
        sys.exit(f"the entry-bank forward is slower than the feature-bank forward beyond {MARGIN * 100:.0f} %")


if __name__ == "__main__":
    main()
