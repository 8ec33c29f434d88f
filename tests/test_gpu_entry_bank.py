"""GPU: decoder-entry tokens kept in the reference bank -- bd_assemble_entry_tokens, bd_decoder_entry_tokens,
bd_decoder_forward_entry[_ragged], cache.RefFeatureBank(decoder=...), BETR.entry_tokens / forward_entry and a BoxDreamer forward over
such a bank, with and without `bbox_feat` in the batch dict.

The kernel moves banked views as bits and computes the query views with bd_query_substitute's association order, so it is compared as
bytes, whole buffers at a time.  Everything above it is held to the project's standing invariant: a forward over the entry bank is
BIT-identical to the un-banked forward of the same data (and, in the dense mode, to the feature bank's)."""
import warnings

import pytest
import torch

from boxdreamer_amd import _lib, cache as cache_mod, calibrate, hip_ops, synth
from boxdreamer_amd.cache import RefFeatureBank
from test_gpu_facade import _dense_model_and_batch
from test_gpu_path import _build
from test_gpu_ragged import DEPTH, OUT_KEYS, _facade, _ragged_batch, _to_dev

pytestmark = pytest.mark.gpu

BANK_VIEWS, N_FRESH, SRC = 4, 3, [0, -1, 3, 3, -3, 1, -2]
FILL = 0x5a


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _assemble_case(P, dim, seed=0):
    """A bank of every bit pattern (NaNs included), finite fresh rows / table / token."""
    e = P * dim
    g = torch.Generator().manual_seed(seed)
    bank = torch.randint(0, 256, (BANK_VIEWS, e * 4), dtype=torch.uint8, generator=g).cuda().view(torch.float32).reshape(BANK_VIEWS, P, dim)
    rgb = torch.randn((N_FRESH, P, dim), generator=g).cuda()
    pos = torch.randn((P, dim), generator=g).cuda()
    q = (torch.randn((dim,), generator=g) * 3).cuda()
    return bank, rgb, pos, q


def _assemble(case, src, P, dim, bank_views=BANK_VIEWS, n_fresh=N_FRESH):
    """One launch into a buffer with two guard views -> (the whole buffer, what it must hold)."""
    bank, rgb, pos, q = case
    n = len(src)
    out = torch.full((n + 2, P, dim), 0.0, device="cuda")
    _bits(out).fill_(FILL)
    want = out.clone()
    hip_ops.assemble_entry_tokens(bank if bank_views else None, bank_views, rgb if n_fresh else None, n_fresh, pos, q,
                                  torch.tensor(src, dtype=torch.int32).cuda(), out, n, P, dim)
    torch.cuda.synchronize()
    for v, s in enumerate(src):
        if 0 <= s < bank_views:
            _bits(want)[v].copy_(_bits(bank)[s])                  # as bytes: NaN payloads included
        elif s < 0 and -(s + 1) < n_fresh:
            want[v] = (q[None, :] + rgb[-(s + 1)]) + pos          # query_sub_kernel's order, in fp32 torch
    return out, want


@pytest.mark.parametrize("shape", [(256, 768), (5, 48)])
def test_assemble_entry_tokens_whole_buffers_bit_for_bit(hip, shape):
    """(256, 768): the path's shape.  (5, 48): 240 floats = 60 chunks per view -- the one workgroup of a view is partial."""
    P, dim = shape
    case = _assemble_case(P, dim)
    assert torch.isnan(case[0]).any()                                    # the bank does hold NaN payloads
    for src in (SRC, [2], [-2]):
        out, want = _assemble(case, src, P, dim)
        assert torch.equal(_bits(out), _bits(want)), (shape, src)
    out, want = _assemble(case, [-1, -3, -2], P, dim, bank_views=0)      # an empty bank: every view fresh
    assert torch.equal(_bits(out), _bits(want)), shape
    # one entry == bank_views, one == -(n_fresh + 1): exactly those two views keep the fill
    out, want = _assemble(case, [0, BANK_VIEWS, -1, -(N_FRESH + 1), 2], P, dim)
    assert torch.equal(_bits(out), _bits(want)), shape
    kept = [bool((_bits(out[v]) == FILL).all()) for v in range(7)]
    assert kept == [False, True, False, True, False, True, True]        # (views 5, 6: the guards)


def test_assemble_entry_tokens_argument_checks(hip):
    lib = _lib.load()
    P, dim = 5, 48
    bank, rgb, pos, q = _assemble_case(P, dim)
    src = torch.tensor(SRC, dtype=torch.int32).cuda()
    big = torch.full((len(SRC) * P * dim + 8,), 7.0, device="cuda")
    out = big[:len(SRC) * P * dim]

    def call(bank=bank, bv=BANK_VIEWS, rgb=rgb, nf=N_FRESH, pos=pos, q=q, src=src, out=out, n=len(SRC), P=P, dim=dim):
        rc = lib.bd_assemble_entry_tokens(_lib.ptr(bank), bv, _lib.ptr(rgb), nf, _lib.ptr(pos), _lib.ptr(q), _lib.ptr(src), _lib.ptr(out), n, P,
                                          dim, _lib.stream())
        _lib.check(0, "reset")
        return rc

    for kw in ({"bank": None}, {"rgb": None}, {"pos": None}, {"q": None}, {"src": None}, {"out": None}):
        assert call(**kw) == -5, kw
    assert call(bv=-1) == -1 and call(nf=-1) == -1 and call(n=-1) == -1 and call(P=0) == -1 and call(dim=-3) == -1
    assert call(P=5, dim=47) == -3                                        # P * dim % 4 != 0
    assert call(out=big[1:]) == -3 and call(rgb=rgb.flatten()[1:]) == -3 and call(pos=pos.flatten()[2:]) == -3       # not 16-byte aligned
    assert call(out=bank.flatten()[P * dim:]) == -1 and call(out=rgb.flatten()) == -1                                 # x_out inside an input
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (big == 7.0).all()                                             # nothing was launched


# ---- bd_decoder_entry_tokens / bd_decoder_forward_entry through the plugin surface
def _decode_plain(enc, dec, data):
    B, T = data["images"].shape[:2]
    img, bf = data["images"].cuda(), data["bbox_feat"].cuda()
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[torch.arange(B), data["query_idx"]] = True
    heat = dec(bf, img, mask.cuda(), enc.predict(img), None)
    torch.cuda.synchronize()
    return dec.last_logits.clone(), heat.clone()


def _decode_entry(enc, dec, data):
    """The same batch with every reference's entry rows made by bd_decoder_entry_tokens, view by view (row = b * T + t)."""
    B, T = data["images"].shape[:2]
    img, bf = data["images"].cuda(), data["bbox_feat"].cuda()
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[torch.arange(B), data["query_idx"]] = True
    refs = (~mask).flatten().nonzero().flatten().cuda()
    rows = dec.entry_tokens(bf.flatten(0, 1)[refs], enc.predict(img.flatten(0, 1)[refs]))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (B * (T - 1), 256, 768)
    src, k = [], 0
    for b in range(B):
        for t in range(T):
            if t == int(data["query_idx"][b]):
                src.append(-(b + 1))
            else:
                src.append(k)
                k += 1
    fresh = enc.predict(torch.stack([img[b, int(q)] for b, q in enumerate(data["query_idx"])]))
    heat = dec.forward_entry(rows, len(rows), torch.tensor(src, dtype=torch.int32).cuda(), fresh, mask.cuda())
    torch.cuda.synchronize()
    return dec.last_logits.clone(), heat.clone()


@pytest.mark.parametrize("state", ["default", "adapter fc1 + bbox_emb promoted"])
def test_entry_rows_equal_the_rows_of_the_plain_forward(hip, state):
    """A 3-view uniform forward against the entry decoder on the same images and heat maps: the decoder's blocks see the same stream
    only if bd_decoder_entry_tokens' rows are the rows bd_decoder_forward builds, so equal logits pin them bit for bit -- in the
    default classes and with the adapter's first Linear and bbox_emb promoted to split-f16 (the features then arrive as split-f16)."""
    enc, dec = _build(_lib.DEFAULT_PREC, DEPTH, DEPTH)
    if state != "default":
        st = calibrate.get_state(enc, dec)
        st["dec_misc"] = _lib.PROMOTE_ADAPTER_FC1 | _lib.PROMOTE_ADAPTER_FC2 | _lib.PROMOTE_BBOX_EMB
        calibrate.set_state(enc, dec, st)
        assert dec.feats_class() == _lib.PREC_F16X3
    data = synth.make_batch(seed=31, B=1, T=3)
    data["query_idx"] = torch.tensor([1])
    want = _decode_plain(enc, dec, data)
    got = _decode_entry(enc, dec, data)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), state
    assert dec.recast_count == 0
    # two samples, their queries at different slots, as two sub-batch lanes
    two = synth.make_batch(seed=32, B=2, T=3)
    two["query_idx"] = torch.tensor([2, 0])
    want = _decode_plain(enc, dec, two)
    for lanes in (1, 2):
        dec.hip_lanes = lanes
        got = _decode_entry(enc, dec, two)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (state, lanes)


# ---- facade
def _fill(bank, parts):
    """Each sample's references through bank.add with their heat maps, sample by sample -> per-sample list of (slot, row)."""
    placed = []
    for p in parts:
        q = int(p["query_idx"][0])
        slots = [t for t in range(p["images"].shape[1]) if t != q]
        rows = bank.add(p["images"][0, slots].cuda(), bbox_feat=p["bbox_feat"][0, slots].cuda())
        assert rows.dtype == torch.int64 and not rows.is_cuda and tuple(rows.shape) == (len(slots),)
        placed.append(list(zip(slots, rows.tolist())))
    return placed


def _table(placed, t_max, pad=10 ** 6):
    rows = []
    for slots in placed:
        n = len(slots) + 1
        row = [-1] * n + [pad] * (t_max - n)             # junk in the padded slots
        for t, r in slots:
            row[t] = r
        rows.append(row)
    return rows


def _parts_of(data):
    return [{k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in data.items()} for b in range(data["images"].shape[0])]


def _poison(data, table, drop_bbox_feat=False):
    """NaN into the images of every banked slot and into EVERY slot's heat maps, the query's included (or no heat maps at all)."""
    data = dict(data, images=data["images"].clone())
    for b, row in enumerate(table):
        for t, r in enumerate(row):
            if r >= 0:
                data["images"][b, t] = float("nan")
    if drop_bbox_feat:
        del data["bbox_feat"]
    else:
        data["bbox_feat"] = torch.full_like(data["bbox_feat"], float("nan"))
    return data


def _keep(model, out):
    return dict({k: out[k].clone() for k in OUT_KEYS}, logits=model.decoder.last_logits.clone())


def _assert_entry_forward(model, out, want, data, counts, where, bbox_feat):
    """bbox_feat: "real" (every output key equal), "nan" (present, NaN: pred_bbox is the NaN clone with the prediction at the query),
    "absent" (no pred_bbox; pred_query_bbox holds the prediction)."""
    B = len(counts)
    q = data["query_idx"]
    assert torch.equal(model.decoder.last_logits, want["logits"]), where
    assert torch.equal(out["pred_corners_px"], want["pred_corners_px"]), where
    for b, c in enumerate(counts):
        for k in ("pred_poses", "regression_boxes"):
            assert torch.equal(out[k][b, :c], want[k][b, :c]), (where, b, k)
    ar = torch.arange(B)
    if bbox_feat == "absent":
        assert "pred_bbox" not in out and "bbox_feat" not in out
        assert out["pred_query_bbox"].shape == (B, 8, 224, 224)
        assert torch.equal(out["pred_query_bbox"].to(want["pred_bbox"].dtype), want["pred_bbox"][ar, q]), where
    else:
        assert "pred_query_bbox" not in out
        assert torch.equal(out["pred_bbox"][ar, q], want["pred_bbox"][ar, q]), where
        if bbox_feat == "real":
            for b, c in enumerate(counts):
                assert torch.equal(out["pred_bbox"][b, :c], want["pred_bbox"][b, :c]), (where, b)
        else:
            for b, c in enumerate(counts):
                assert all(torch.isnan(out["pred_bbox"][b, t]).all() for t in range(c) if t != int(q[b])), (where, b)


_SHARED = {}


def _shared():
    """One model (default mode; its first forward runs the load-time calibration) and the ragged batch of tests/test_gpu_ragged.py
    with its un-banked forward."""
    if not _SHARED:
        model = _facade(_lib.DEFAULT_PREC)
        data, parts = _ragged_batch()
        want = _keep(model, model(_to_dev(data)))
        _SHARED.update(model=model, data=data, parts=parts, want=want, syncs=len(model.host_syncs_per_forward))
    return _SHARED


def test_facade_uniform_entry_bank_bit_identical(hip):
    sh = _shared()
    model = sh["model"]
    B, T = 3, 4
    data = synth.make_batch(seed=41, B=B, T=T)
    data["query_idx"] = torch.tensor([3, 0, 2])
    want = _keep(model, model(_to_dev(data)))
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    assert bank.has_entry_tokens
    table = _table(_fill(bank, _parts_of(data)), T)
    assert len(bank) == B * (T - 1) and bank.entry_bytes_per_view == 256 * 768 * 4 and bank.entry_tokens.shape[1:] == (256, 768)
    recasts = model.decoder.recast_count
    try:
        for lanes in (1, "auto", 2, 3):
            model.decoder.hip_lanes = lanes
            out = model(dict(_to_dev(data), ref_bank=bank, ref_rows=table))
            for k in OUT_KEYS:
                assert torch.equal(out[k], want[k]), (lanes, k)
            _assert_entry_forward(model, out, want, data, [T] * B, f"lanes {lanes}", "real")
            rec = out["hip_precision"]
            assert rec["ref_bank"] == {"banked_views": B * (T - 1), "encoded_views": B, "refreshed": False, "entry_tokens": True}
            assert rec["sub_batch_lanes"] == _lib.resolve_lanes(lanes, B * T, B, _lib.DEFAULT_PREC) and "ragged_views" not in rec
            assert len(model.host_syncs_per_forward) == sh["syncs"]
            out = model(dict(_to_dev(_poison(data, table)), ref_bank=bank, ref_rows=torch.tensor(table)))
            _assert_entry_forward(model, out, want, data, [T] * B, f"lanes {lanes}, NaN heat maps", "nan")
            out = model(dict(_to_dev(_poison(data, table, drop_bbox_feat=True)), ref_bank=bank, ref_rows=table))
            _assert_entry_forward(model, out, want, data, [T] * B, f"lanes {lanes}, no bbox_feat", "absent")
    finally:
        model.decoder.hip_lanes = "auto"
    assert model.decoder.recast_count == recasts
    # a device-side query_idx that is not the table's -1 slot: reported with the corners' D2H; a host one before any launch
    with pytest.raises(ValueError, match="exactly one query view"):
        model(dict(_to_dev(data), ref_bank=bank, ref_rows=table, query_idx=torch.tensor([3, 1, 2]).cuda()))
    with pytest.raises(ValueError, match="must be the query view"):
        model(dict(_to_dev(data), ref_bank=bank, ref_rows=table, query_idx=torch.tensor([3, 1, 2])))
    out = model(dict(_to_dev(data), ref_bank=bank, ref_rows=table, query_idx=data["query_idx"].cuda()))
    _assert_entry_forward(model, out, want, data, [T] * B, "device query_idx", "real")
    # hip_graph: a banked batch takes the eager branch
    model.hip_graph = True
    try:
        out = model(dict(_to_dev(_poison(data, table, drop_bbox_feat=True)), ref_bank=bank, ref_rows=table))
        _assert_entry_forward(model, out, want, data, [T] * B, "hip_graph", "absent")
        assert model._graph is None
    finally:
        model.hip_graph = False
    # a forward without bbox_feat needs the entry bank: the feature bank's decoder reads the heat maps
    plain, ptable = RefFeatureBank(model.rgb_encoder), []
    for b, q in enumerate(data["query_idx"].tolist()):
        ids = plain.add(data["images"][b, [t for t in range(T) if t != q]].cuda()).tolist()
        ptable.append([-1 if t == q else ids.pop(0) for t in range(T)])
    with pytest.raises(KeyError, match="bbox_feat"):
        model(dict(_to_dev(_poison(data, ptable, drop_bbox_feat=True)), ref_bank=plain, ref_rows=ptable))


def test_facade_ragged_entry_bank_bit_identical_and_each_sample_alone(hip):
    """view_counts = [3, 2, 5]: equal to the un-banked ragged forward, and every sample to that sample run alone."""
    sh = _shared()
    model, data, parts, want = sh["model"], sh["data"], sh["parts"], sh["want"]
    counts, t_max = data["view_counts"], data["images"].shape[1]
    assert counts == [3, 2, 5]
    B = len(counts)
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    table = _table(_fill(bank, parts), t_max)
    for variant, drop in (("real", None), ("nan", False), ("absent", True)):
        nan_fill, _ = _ragged_batch(fill=float("nan"))                   # NaN in the padded slots too
        batch = data if drop is None else _poison(nan_fill, table, drop_bbox_feat=drop)
        out = model(dict(_to_dev(batch), ref_bank=bank, ref_rows=table))
        _assert_entry_forward(model, out, want, data, counts, variant, variant)
        rec = out["hip_precision"]
        assert rec["ref_bank"] == {"banked_views": sum(counts) - B, "encoded_views": B, "refreshed": False, "entry_tokens": True}
        assert rec["sub_batch_lanes"] == 1 and rec["ragged_views"] == sum(counts)
        assert len(model.host_syncs_per_forward) == sh["syncs"]
    got = dict(logits=model.decoder.last_logits.clone(), pred_corners_px=out["pred_corners_px"].clone(),
               pred_query_bbox=out["pred_query_bbox"].clone())
    for b, p in enumerate(parts):
        one = model(_to_dev(p))
        q = int(p["query_idx"][0])
        assert torch.equal(got["logits"][b:b + 1], model.decoder.last_logits), b
        assert torch.equal(got["pred_corners_px"][b:b + 1], one["pred_corners_px"]), b
        assert torch.equal(got["pred_query_bbox"][b].to(one["pred_bbox"].dtype), one["pred_bbox"][0, q]), b
    # a device-side query_idx outside the table's slot
    with pytest.raises(ValueError, match="exactly one query view"):
        model(dict(_to_dev(data), ref_bank=bank, ref_rows=table, query_idx=torch.tensor([1, 0, 4]).cuda()))
    # row ids stay stable across a store growth: 5 rows, then 20 more
    assert len(bank) == 7
    cap0, first = bank._cap, bank.entry_tokens[:7].clone()
    extra = synth.make_batch(seed=43, B=4, T=5)
    more = bank.add(extra["images"].cuda(), bbox_feat=extra["bbox_feat"].cuda())
    assert more.tolist() == torch.arange(7, 27).reshape(4, 5).tolist() and bank._cap > cap0 and torch.equal(bank.entry_tokens[:7], first)
    out = model(dict(_to_dev(_poison(data, table, drop_bbox_feat=True)), ref_bank=bank, ref_rows=table))
    _assert_entry_forward(model, out, want, data, counts, "after growth", "absent")


def test_entry_bank_filled_before_the_first_forward_is_refreshed_once(hip):
    """The bank is filled BEFORE the model's first forward, under a promotion state of the decoder's adapter / bbox_emb that is not the
    one the load-time calibration arrives at (these plain weights need no promotion): the first forward -- an entry-bank batch
    whose own images of banked slots and heat maps are NaN or absent -- calibrates on the crops AND heat maps the bank kept, finds the
    entry rows stale by the decoder's stamp, re-encodes and re-embeds them once, and gives the un-banked model's bits."""
    sh = _shared()
    data, parts, want = sh["data"], sh["parts"], sh["want"]
    counts, t_max = data["view_counts"], data["images"].shape[1]
    model = _facade(_lib.DEFAULT_PREC)
    enc, dec = model.rgb_encoder, model.decoder
    zero = calibrate.get_state(enc, dec)
    assert not calibrate.has_state(enc, dec)
    calibrate.set_state(enc, dec, dict(zero, dec_misc=_lib.PROMOTE_BBOX_EMB))
    bank = RefFeatureBank(enc, decoder=dec)
    table = _table(_fill(bank, parts), t_max)
    old_rows, old_stamp = bank.entry_tokens[:len(bank)].clone(), bank.entry_stamp
    calibrate.set_state(enc, dec, zero)                                  # a fresh model's state again: the first forward measures
    cache_mod._WARNED_STALE_BANK = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = model(dict(_to_dev(_poison(data, table, drop_bbox_feat=True)), ref_bank=bank, ref_rows=table))
        out2 = model(dict(_to_dev(_poison(data, table)), ref_bank=bank, ref_rows=table))
    assert sum("re-encoding its rows" in str(x.message) for x in w) == 1
    rep = dec.hip_calibration
    assert rep["applicable"] and rep["delta_final"] == rep["delta_final"]          # the calibration ran, measured, and not on NaN
    ref = sh["model"].decoder.hip_calibration                            # (measured on the same first sample, with its real inputs)
    assert rep["state"] == ref["state"] and rep["delta_final"] == ref["delta_final"]
    assert out["hip_precision"]["ref_bank"]["refreshed"] is True and out2["hip_precision"]["ref_bank"]["refreshed"] is False
    assert bank.refresh_count == 1 and bank.entry_stamp != old_stamp and bank.entry_stamp[2] == dec.hip_promote_misc
    assert not torch.equal(bank.entry_tokens[:len(bank)], old_rows)      # bbox_emb ran in another operand class
    _assert_entry_forward(model, out, want, data, counts, "first forward", "absent")
    _assert_entry_forward(model, out2, want, data, counts, "second forward", "nan")
    # keep_images=False: a stale entry bank is refused before anything is launched, and so is its calibration batch
    lean = RefFeatureBank(enc, keep_images=False, decoder=dec)
    ltable = _table(_fill(lean, parts), t_max)
    out = model(dict(_to_dev(_poison(data, ltable, drop_bbox_feat=True)), ref_bank=lean, ref_rows=ltable))
    _assert_entry_forward(model, out, want, data, counts, "keep_images=False, fresh", "absent")
    dec.hip_promote_misc |= _lib.PROMOTE_BBOX_EMB
    lib = _lib.load()
    buf = (_lib.TraceRecord * 64)()
    _lib.check(lib.bd_trace_begin(64), "bd_trace_begin")
    try:
        with pytest.raises(RuntimeError, match="keep_images=False"):
            model(dict(_to_dev(data), ref_bank=lean, ref_rows=ltable))
    finally:
        launched = lib.bd_trace_end(buf, 64)
    assert launched == 0
    fresh_model = _facade(_lib.DEFAULT_PREC)
    lean2 = RefFeatureBank(fresh_model.rgb_encoder, keep_images=False, decoder=fresh_model.decoder)
    ltable2 = _table(_fill(lean2, parts), t_max)
    with pytest.raises(RuntimeError, match="keep_images=False"):          # its load-time calibration has no crops to measure on
        fresh_model(dict(_to_dev(data), ref_bank=lean2, ref_rows=ltable2))


# ---- dense mode over the entry bank: B = 2, N = 6, k = 2
K = 2
CFG = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": K, "multi_round": False}
SAME = ("regression_boxes", "pred_corners_px", "pred_poses", "query_idx", "camera_mask", "poses", "intrinsics", "non_ndc_intrinsics",
        "bbox_3d", "bbox_proj_crop", "pred_intrinsics")


def _dense_fill(bank, data, counts, entry):
    table = []
    for b, q in enumerate(data["query_idx"].tolist()):
        slots = [t for t in range(counts[b]) if t != q]
        kw = {"bbox_feat": data["bbox_feat"][b, slots].cuda()} if entry else {}
        ids = bank.add(data["images"][b, slots].cuda(), **kw).tolist()
        row = [10 ** 6] * data["images"].shape[1]
        row[q] = -1
        for t, r in zip(slots, ids):
            row[t] = r
        table.append(row)
    return table


@pytest.mark.parametrize("counts", [[7, 7], [7, 5]])
def test_facade_dense_entry_bank_equals_the_feature_bank(hip, counts):
    """Databases of 6 and 6, then 6 and 4, references: the same selection, scores and outputs as the feature bank's dense forward
    (which tests/test_gpu_dense_bank.py pins to the un-banked one), with bbox_feat real, NaN in every slot, and absent."""
    model, data = _dense_model_and_batch(CFG, B=2, T=7)
    data["query_idx"] = torch.tensor([6, 1])
    dev = lambda d, **more: dict({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}, **more)
    vc = {} if counts == [7, 7] else {"view_counts": counts}
    model(dev(data, **vc) if not vc else dev({k: v[:1] for k, v in data.items()}))      # (the load-time calibration, once)
    fbank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05)
    ftable = _dense_fill(fbank, data, counts, entry=False)
    out_f = model(dev(data, ref_bank=fbank, ref_rows=ftable, **vc))
    want = dict({k: out_f[k].clone() for k in SAME + ("pred_bbox", "dense_ref_slots", "dense_ref_scores")}, logits=model.decoder.last_logits.clone())
    assert "entry_tokens" not in out_f["hip_precision"]["ref_bank"]
    ebank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, decoder=model.decoder)
    etable = _dense_fill(ebank, data, counts, entry=True)
    assert etable == ftable
    B = 2
    ar, qk = torch.arange(B), torch.full((B,), K)
    for variant in ("real", "nan", "absent"):
        batch = data if variant == "real" else _poison(data, etable, variant == "absent")
        out = model(dev(batch, ref_bank=ebank, ref_rows=etable, **vc))
        assert torch.equal(model.decoder.last_logits, want["logits"]), (counts, variant)
        for k in SAME + ("dense_ref_slots", "dense_ref_scores"):
            assert out[k].dtype == want[k].dtype and torch.equal(out[k], want[k]), (counts, variant, k)
        assert out["hip_precision"]["ref_bank"] == {"banked_views": B * K, "encoded_views": B, "scored_views": sum(counts) - B,
                                                    "refreshed": False, "entry_tokens": True}
        assert out["images"].shape[1] == K + 1 and len(model.host_syncs_per_forward) == 1
        if variant == "absent":
            assert "pred_bbox" not in out and torch.equal(out["pred_query_bbox"].to(want["pred_bbox"].dtype), want["pred_bbox"][ar, qk])
        else:
            assert out["pred_bbox"].shape[:2] == (B, K + 1) and torch.equal(out["pred_bbox"][ar, qk], want["pred_bbox"][ar, qk])
            assert torch.equal(out["pred_bbox"], want["pred_bbox"]) == (variant == "real")
    with pytest.raises(ValueError, match="exactly one query view"):
        model(dev(data, ref_bank=ebank, ref_rows=etable, query_idx=torch.tensor([6, 2]).cuda(), **vc))
