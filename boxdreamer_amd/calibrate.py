"""Load-time self-check and per-Linear promotion of the default precision mode.

The default mode (`f16c8_qk16`: F16C8 Linears, ~15 significant bits per product) meets the path's 1e-3 bar on the heatmap logits with a
4.5x margin on plain weights, but trained checkpoints carry massive-activation channels, LayerNorm gain outliers and MLP hidden units in
the hundreds (reference modules: /root/reference/src/models/sources/DINOv2/layers/block.py:89-114, src/models/modules/backbone/utils/
blocks.py:35-56, 808-886); there a handful of Linears -- not necessarily the ones whose operands are large: the ones UPSTREAM of an
amplifying channel -- decide the error.  They are found by MEASUREMENT on the device, on one calibration sample:

  reference   every Linear split-f16 (fp32-faithful products) + split-bf16 attention: bit-identical to `f16x3_attn_x3`, the most
              precise GPU mode (include/boxdreamer_hip.h: BD_PREC_F16X3)
  e[u]        max |logits - reference| with ONLY unit u left in the default class  (u = a block's QKV / proj / MLP / attention form,
              or one of the Linears outside the blocks)
  choice      units sorted by e[u] per unit of saved work; the longest prefix that may stay in the default class with
              max |logits - reference| <= budget (4e-4 on two calibration samples: the reference itself is within 0.5e-4 - 4e-4 of
              the fp32 forward on the weight sets tried, and other samples of a batch land up to ~1.5x the calibration samples' value)

Everything that is not in that prefix is PROMOTED (bd_block_weights.promote, include/boxdreamer_hip.h).  ~100 batch-1 forwards, about
a second at load time; nothing here runs in the per-batch path.  Host logic only: the forwards are the HIP path itself.
"""
from __future__ import annotations

import warnings

import torch

from . import _lib

BUDGET = 4e-4
_BLOCK_UNITS = (("qkv", _lib.PROMOTE_QKV), ("proj", _lib.PROMOTE_PROJ), ("mlp", _lib.PROMOTE_FC1 | _lib.PROMOTE_FC2),
                ("attn", _lib.PROMOTE_ATTN))


def applicable(encoder, decoder) -> bool:
    """Promotion exists for the F16C8 family only (the other modes are either the reference itself or opt-in throughput modes)."""
    return (_lib.operand_prec(decoder.hip_precision) == _lib.PREC_F16C8 and _lib.operand_prec(encoder.prec) == _lib.PREC_F16C8)


def units_of(encoder, decoder):
    """[(name, where, block index | None, bits, relative cost of promoting it)]; where: 'enc' / 'dec' / 'enc_misc' / 'dec_misc'."""
    u = [("dino.patch_embed", "enc_misc", None, _lib.PROMOTE_PATCH_EMBED, 0.8)]
    for i in range(len(encoder.model.promote)):
        u += [(f"dino.{i}.qkv", "enc", i, _lib.PROMOTE_QKV, 3.0), (f"dino.{i}.proj", "enc", i, _lib.PROMOTE_PROJ, 1.0),
              (f"dino.{i}.mlp", "enc", i, _lib.PROMOTE_FC1 | _lib.PROMOTE_FC2, 8.0)]
    u += [("betr.adapter", "dec_misc", None, _lib.PROMOTE_ADAPTER_FC1 | _lib.PROMOTE_ADAPTER_FC2, 2.0),
          ("betr.bbox_emb", "dec_misc", None, _lib.PROMOTE_BBOX_EMB, 2.0), ("betr.bbox_proj", "dec_misc", None, _lib.PROMOTE_BBOX_PROJ, 0.4)]
    qk16 = _lib.prec_id(decoder.hip_precision) == _lib.PREC_F16C8_QK16
    for i in range(len(decoder.hip_promote)):
        u += [(f"betr.{i}.qkv", "dec", i, _lib.PROMOTE_QKV, 5.0 if qk16 else 3.0), (f"betr.{i}.proj", "dec", i, _lib.PROMOTE_PROJ, 1.0),
              (f"betr.{i}.mlp", "dec", i, _lib.PROMOTE_FC1 | _lib.PROMOTE_FC2, 8.0), (f"betr.{i}.attn", "dec", i, _lib.PROMOTE_ATTN, 8.0)]
    return u


def get_state(encoder, decoder) -> dict:
    return {"enc": list(encoder.model.promote), "enc_misc": int(encoder.model.promote_misc), "dec": list(decoder.hip_promote),
            "dec_misc": int(decoder.hip_promote_misc)}


def set_state(encoder, decoder, state: dict) -> None:
    """Apply a promotion state (from `get_state` / a calibration report) to an encoder / decoder pair of the same architecture."""
    encoder.model.promote = list(state["enc"])
    encoder.model.promote_misc = int(state["enc_misc"])
    decoder.hip_promote = list(state["dec"])
    decoder.hip_promote_misc = int(state["dec_misc"])
    # the encoder hands its features over in the class the decoder's first Linear reads
    encoder.model.feats_prec = _lib.PREC_F16X3 if decoder.hip_promote_misc & _lib.PROMOTE_ADAPTER_FC1 else 0


def has_state(encoder, decoder) -> bool:
    """True when some Linear is promoted already (a state applied through `set_state` / `load_state`, or an earlier calibration)."""
    st = get_state(encoder, decoder)
    return bool(any(st["enc"]) or st["enc_misc"] or any(st["dec"]) or st["dec_misc"])


def sync_state_across_ranks(encoder, decoder, src: int = 0) -> bool:
    """Multi-rank runs (one process per GPU, weights replicated): every rank calibrates on its own first batch, so the promotion sets
    could differ from rank to rank -- and with them the bits of the result for the same sample.  Rank `src`'s state is broadcast and
    applied everywhere (a few hundred bytes, once per checkpoint load).  No-op without an initialised process group.  Returns whether
    this rank's state changed."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return False
    mine = get_state(encoder, decoder)
    box = [mine if dist.get_rank() == src else None]
    dist.broadcast_object_list(box, src=src)
    if isinstance(box[0], dict) and "error" in box[0]:
        raise RuntimeError(f"rank {src} could not calibrate: {box[0]['error']}")
    if box[0] == mine:
        return False
    set_state(encoder, decoder, box[0])
    return True


def broadcast_failure(reason: str, src: int = 0) -> None:
    """What rank `src` sends INSTEAD of its state when its calibration raised: the other ranks, which all reach the same broadcast (model.py
    calls it from ONE place in forward()), raise too instead of waiting for a state that never comes."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and dist.get_rank() == src:
        dist.broadcast_object_list([{"error": str(reason)}], src=src)


def _state_of(units, promoted, n_enc, n_dec) -> dict:
    st = {"enc": [0] * n_enc, "enc_misc": 0, "dec": [0] * n_dec, "dec_misc": 0}
    for (name, where, idx, bits, _), on in zip(units, promoted):
        if not on:
            continue
        if idx is None:
            st[where] |= bits
        else:
            st[where][idx] |= bits
    return st


@torch.no_grad()
def _logits(encoder, decoder, images, bbox_feat, masks) -> torch.Tensor:
    heat = decoder(bbox_feat, images, masks, encoder.predict(images), None)
    del heat
    return decoder.last_logits.clone()


@torch.no_grad()
def self_check(encoder, decoder, images, bbox_feat, masks) -> float:
    """max |logits(current promotion state) - logits(every unit promoted)| on the given samples: what the active mode costs against
    the most precise GPU mode.  Leaves the promotion state as it found it."""
    keep = get_state(encoder, decoder)
    units = units_of(encoder, decoder)
    cur = _logits(encoder, decoder, images, bbox_feat, masks)
    try:
        set_state(encoder, decoder, _state_of(units, [True] * len(units), len(keep["enc"]), len(keep["dec"])))
        ref = _logits(encoder, decoder, images, bbox_feat, masks)
    finally:
        set_state(encoder, decoder, keep)
    return float((cur - ref).abs().max())


MAX_SAMPLES = 2      # samples of a batch the self-check measures on (model.py prepares exactly these for a banked batch)


@torch.no_grad()
def calibrate(encoder, decoder, images, bbox_feat, masks, *, budget: float = BUDGET, promote: bool = True, max_samples: int = MAX_SAMPLES,
              verbose: bool = False) -> dict:
    """Measure the default mode against the all-promoted reference on `max_samples` samples of the given batch and, if it exceeds
    `budget`, promote the cheapest sufficient set of units.  Returns (and stores in `decoder.hip_calibration`) the report; warns when
    promotion was needed or -- with promote=False -- when the self-check fails.

    promote=True REPLACES whatever promotion state the pair was entered with by the measured one.  promote=False changes nothing: it
    measures the all-unpromoted mode AND the state the pair was entered with (`delta_entry_state`), and leaves that state in place.

    images (B, T, 3, H, W), bbox_feat (B, T, 8, H, W), masks (B, T) bool: as `BETR.forward` / `DinoV2Wrapper.predict` take them."""
    rep = {"mode": str(decoder.hip_precision), "budget": budget, "applicable": applicable(encoder, decoder)}
    if not rep["applicable"]:
        rep["note"] = "per-Linear promotion exists for the f16c8 family only; nothing measured"
        decoder.hip_calibration = rep
        return rep
    n = max(1, min(int(max_samples), images.shape[0]))
    images, bbox_feat, masks = images[:n].contiguous(), bbox_feat[:n].contiguous(), masks[:n].contiguous()
    validate, decoder.validate_inputs = decoder.validate_inputs, False
    units = units_of(encoder, decoder)
    n_enc, n_dec, nu = len(encoder.model.promote), len(decoder.hip_promote), len(units)
    forwards = 0
    import time
    torch.cuda.synchronize()
    t_start = time.perf_counter()

    def run(promoted):
        nonlocal forwards
        forwards += 1
        set_state(encoder, decoder, _state_of(units, promoted, n_enc, n_dec))
        return _logits(encoder, decoder, images, bbox_feat, masks)

    entry_state = get_state(encoder, decoder)
    try:
        ref = run([True] * nu)
        d0 = float((run([False] * nu) - ref).abs().max())
        rep.update(delta_unpromoted=d0, samples=n, views=int(images.shape[1]),
                   reference="every Linear split-f16 + split-bf16 attention (bit-identical to f16x3_attn_x3)")
        chosen = [False] * nu
        if not promote:
            entry_promoted = any(entry_state["enc"]) or entry_state["enc_misc"] or any(entry_state["dec"]) or entry_state["dec_misc"]
            if entry_promoted:
                forwards += 1
                set_state(encoder, decoder, entry_state)
                rep["delta_entry_state"] = float((_logits(encoder, decoder, images, bbox_feat, masks) - ref).abs().max())
        if d0 > budget and promote:
            # e[u]: only unit u in the default class
            e = []
            for k in range(nu):
                on = [True] * nu
                on[k] = False
                e.append(float((run(on) - ref).abs().max()))
            # Which units may stay in the default class?  A knapsack: keep as much WORK as possible while the errors -- which add
            # roughly in quadrature -- stay inside the budget.  Two greedy orders (e^2 per unit of work: the knapsack ratio; e per
            # unit of work), each with a MEASURED binary search for the longest admissible prefix; the cheaper result wins.
            best = None
            for key in (lambda k: e[k] * e[k] / units[k][4], lambda k: e[k] / units[k][4]):
                order = sorted(range(nu), key=key)
                lo, hi = 0, nu                 # invariant: keeping order[:lo] is fine, keeping order[:hi] is not (hi = nu: d0 > budget)
                deltas = {0: 0.0, nu: d0}
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    on = [True] * nu
                    for k in order[:mid]:
                        on[k] = False
                    deltas[mid] = float((run(on) - ref).abs().max())
                    if deltas[mid] <= budget:
                        lo = mid
                    else:
                        hi = mid
                cost = sum(units[k][4] for k in order[lo:])
                if best is None or cost < best[0]:
                    best = (cost, order, lo, deltas[lo])
            _, order, lo, dfin = best
            chosen = [True] * nu
            for k in order[:lo]:
                chosen[k] = False
            rep.update(delta_final=dfin, unit_errors={units[k][0]: round(e[k], 7) for k in sorted(range(nu), key=lambda k: -e[k])[:12]})
        else:
            rep.update(delta_final=d0)
        if promote:
            set_state(encoder, decoder, _state_of(units, chosen, n_enc, n_dec))
        else:                                                   # measurement only: the pair leaves as it came
            set_state(encoder, decoder, entry_state)
            rep["delta_final"] = rep.get("delta_entry_state", d0)
            cur = get_state(encoder, decoder)
            chosen = [bool((cur[w] if i is None else cur[w][i]) & bits) for (_, w, i, bits, _) in units]
        rep.update(promoted=[units[k][0] for k in range(nu) if chosen[k]], units=nu, forwards=forwards,
                   promoted_cost_frac=round(sum(units[k][4] for k in range(nu) if chosen[k]) / sum(u[4] for u in units), 4),
                   state=get_state(encoder, decoder), ok=bool(rep["delta_final"] <= budget))
        torch.cuda.synchronize()
        rep["seconds"] = round(time.perf_counter() - t_start, 3)
    except BaseException:
        set_state(encoder, decoder, entry_state)          # a failed measurement leaves the pair as it found it
        raise
    finally:
        decoder.validate_inputs = validate
    if d0 > budget and (promote or rep["delta_final"] > budget):
        msg = (f"BoxDreamer HIP path: the default precision mode '{decoder.hip_precision}' is {d0:.2e} off the split-f16 reference on the "
               f"heatmap logits of the calibration sample (budget {budget:.1e}); ")
        msg += (f"{len(rep['promoted'])} of {nu} units promoted to split-f16 -> {rep['delta_final']:.2e}" if promote else
                "promotion is disabled (hip_calibrate=False): expect to miss the 1e-3 parity bar; use hip_precision='f16x3'")
        warnings.warn(msg, stacklevel=2)
    if verbose:
        print("[calibrate] " + ", ".join(f"{k}={v}" for k, v in rep.items() if k not in ("state", "unit_errors")), flush=True)
    decoder.hip_calibration = rep
    return rep


# ---------------------------------------------------------------------------------------------- persistence (optional)
# The promotion state depends on the weights only (and mildly on the calibration sample): a deployment can measure once and reuse.

def weights_fingerprint(encoder, decoder) -> str:
    """A cheap content stamp of both weight sets (shapes + a few float64 sums): a stored promotion state is applied only to the weights
    it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for name, sd in (("dec", decoder.state_dict()), ("enc", encoder.model.sd)):
        for k in sorted(sd):
            t = sd[k].detach()
            h.update(f"{name}.{k}:{tuple(t.shape)}:{float(t.double().sum()):.10e}:{float(t.double().abs().sum()):.10e}".encode())
    return h.hexdigest()[:24]


def save_state(path: str, encoder, decoder, report: dict | None = None) -> None:
    import json
    rec = {"fingerprint": weights_fingerprint(encoder, decoder), "mode": str(decoder.hip_precision), "state": get_state(encoder, decoder)}
    if report:
        rec["report"] = {k: v for k, v in report.items() if k not in ("state",)}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def load_state(path: str, encoder, decoder) -> bool:
    """Apply a stored promotion state if it was measured on THESE weights in THIS mode; False (and nothing applied) otherwise."""
    import json, os
    if not os.path.isfile(path):
        return False
    rec = json.load(open(path))
    if rec.get("mode") != str(decoder.hip_precision) or rec.get("fingerprint") != weights_fingerprint(encoder, decoder):
        return False
    st = rec["state"]
    if len(st["enc"]) != len(encoder.model.promote) or len(st["dec"]) != len(decoder.hip_promote):
        return False
    set_state(encoder, decoder, st)
    decoder.hip_calibration = dict(rec.get("report") or {}, applicable=True, loaded_from=path, state=st,
                                   promoted=(rec.get("report") or {}).get("promoted", []))
    return True
