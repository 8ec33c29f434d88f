"""GPU: the reference bank -- cached reference features for uniform AND ragged batches (bd_gather_view_rows, cache.RefFeatureBank,
features.OperandOnly, `ref_bank` / `ref_rows` in BoxDreamer's batch dict).

The kernel moves bytes, so it is compared as bytes (NaN payloads and e4m3 bytes must survive, and every byte it does not own must keep
its fill).  Everything above it is held to the project's standing invariant: a banked forward is BIT-identical to the uncached one."""
import warnings

import pytest
import torch

from boxdreamer_amd import _lib, cache as cache_mod, hip_ops, operand
from boxdreamer_amd.cache import RefFeatureBank
from test_gpu_path import LOGIT_TOL, _build
from test_gpu_ragged import DEPTH, OUT_KEYS, _decode, _facade, _oracle, _ragged_batch, _to_dev

pytestmark = pytest.mark.gpu

# class -> (bytes per element of plane 0, of plane 1)
CLASSES = {"bf16": (2, 0), "fp16": (2, 0), "fp8": (1, 0), "bf16x3": (2, 2), "f16x3": (2, 2), "f16c8": (2, 1)}
BANK_VIEWS, N_FRESH, SRC = 4, 3, [0, -1, 3, 3, -3, 1, -2]
FILL = 0x5a


class _Raw:
    """An operand tensor of `cap` views as raw bytes: plane 0, then (two-plane classes) plane 1 at `cap` views of 16-bit elements."""

    def __init__(self, name, cap, e, fill=None, seed=0):
        self.esz, self.p1 = CLASSES[name]
        self.cap, self.e = cap, e
        nbytes = cap * e * self.esz + (cap * e * 2 if self.p1 else 0)
        if fill is None:
            g = torch.Generator().manual_seed(seed)
            self.t = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).cuda()       # every bit pattern: NaNs included
        else:
            self.t = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        self.plane = cap * e if self.p1 else 0              # in 16-bit elements

    def view(self, v):
        """The byte runs view v owns."""
        e, out = self.e, [self.t[v * self.e * self.esz:(v + 1) * self.e * self.esz]]
        if self.p1:
            base = self.cap * e * 2
            out.append(self.t[base + v * e * self.p1:base + (v + 1) * e * self.p1])
        return out


def _expected(out, bank, fresh, src, out32=None, bank32=None, fresh32=None):
    exp = _Raw.__new__(_Raw)
    exp.__dict__.update(out.__dict__)
    exp.t = torch.full_like(out.t, FILL)
    exp32 = torch.full_like(out32, FILL) if out32 is not None else None
    for v, s in enumerate(src):
        ok = 0 <= s < BANK_VIEWS or 0 <= -(s + 1) < N_FRESH
        if not ok:
            continue
        from_, sv = (bank, s) if s >= 0 else (fresh, -(s + 1))
        for d, x in zip(exp.view(v), from_.view(sv)):
            d.copy_(x)
        if exp32 is not None:
            exp32[v] = (bank32 if s >= 0 else fresh32)[sv]
    return exp.t, exp32


@pytest.mark.parametrize("shape", [(256, 768), (5, 48)])
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_gather_view_rows_moves_whole_views_byte_for_byte(hip, name, shape):
    """(256, 768): the path's shape.  (5, 48): 240 elements -- the byte plane is one 16-byte chunk short of a full 256-thread sweep,
    the last workgroup of every view is partial."""
    P, dim = shape
    e, pid = P * dim, _lib.prec_id(name)
    bank, fresh = _Raw(name, BANK_VIEWS + 2, e, seed=1), _Raw(name, N_FRESH + 2, e, seed=2)       # three different plane strides
    g = torch.Generator().manual_seed(3)
    bank32 = torch.randint(0, 256, (BANK_VIEWS, e * 4), dtype=torch.uint8, generator=g).cuda()
    fresh32 = torch.randint(0, 256, (N_FRESH, e * 4), dtype=torch.uint8, generator=g).cuda()

    def run(src, with32):
        out = _Raw(name, len(src) + 2, e, fill=FILL)
        out32 = torch.full((len(src) + 2, e * 4), FILL, dtype=torch.uint8, device="cuda") if with32 else None
        s = torch.tensor(src, dtype=torch.int32).cuda()
        hip_ops.gather_view_rows(bank.t, BANK_VIEWS, fresh.t, N_FRESH, s, out.t, len(src), P, dim, prec=pid, bank_plane=bank.plane,
                                 fresh_plane=fresh.plane, out_plane=out.plane, bank32=bank32 if with32 else None,
                                 fresh32=fresh32 if with32 else None, out32=out32)
        torch.cuda.synchronize()
        want, want32 = _expected(out, bank, fresh, src, out32, bank32, fresh32)
        # one comparison of the WHOLE buffer: every owned byte equals its source, every other byte (the extra views, and for F16C8
        # the plane-1 storage past n_views * P * dim bytes) still holds the fill
        assert torch.equal(out.t, want), (name, shape, src)
        if with32:
            assert torch.equal(out32, want32), (name, shape, src)
        return out

    out = run(SRC, False)
    run(SRC, True)
    run([2], False)                                                     # n_views = 1
    run([-2], True)
    # one entry == bank_views, one == -(n_fresh + 1): exactly those two views keep the fill
    bad = [0, BANK_VIEWS, -1, -(N_FRESH + 1), 2]
    got = run(bad, True)
    assert all((x == FILL).all() for v in (1, 3) for x in got.view(v))
    if name == "f16c8":       # the layout is operand.row_planes': f16 plane 0, one-byte lo8 rows packed at the head of plane-1 storage
        def planes(r):
            return [p.reshape(r.cap, P, dim) for p in operand.row_planes(r.t.view(torch.float16).reshape(2, r.cap * P, dim), pid, r.cap * P)]
        for v, s in enumerate(SRC):
            from_, sv = (bank, s) if s >= 0 else (fresh, -(s + 1))
            for o, x in zip(planes(out), planes(from_)):
                assert torch.equal(o[v].contiguous().view(torch.uint8), x[sv].contiguous().view(torch.uint8)), (v, s)


def _fill_bank(bank, parts):
    """Each sample's references through bank.add, sample by sample -> per-sample list of (slot, row)."""
    placed = []
    for p in parts:
        q = int(p["query_idx"][0])
        slots = [t for t in range(p["images"].shape[1]) if t != q]
        rows = bank.add(p["images"][0, slots].cuda())
        assert rows.dtype == torch.int64 and not rows.is_cuda and tuple(rows.shape) == (len(slots),)
        placed.append(list(zip(slots, rows.tolist())))
    return placed


def _table(placed, t_max, pad=-1):
    rows = []
    for slots in placed:
        n = len(slots) + 1
        row = [-1] * n + [pad] * (t_max - n)
        for t, r in slots:
            row[t] = r
        rows.append(row)
    return rows


def _poison_banked(data, table):
    """NaN into the images of every banked slot: they are never read."""
    data = dict(data, images=data["images"].clone())
    for b, row in enumerate(table):
        for t, r in enumerate(row):
            if r >= 0:
                data["images"][b, t] = float("nan")
    return data


def _decode_banked(enc, dec, bank, data, table, counts=None):
    B, T = data["images"].shape[:2]
    img, bf = data["images"].cuda(), data["bbox_feat"].cuda()
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[torch.arange(B), data["query_idx"]] = True
    cts = counts if counts is not None else [T] * B
    rows = _lib.ref_rows_table(table, B, T)
    _lib.check_ref_rows(rows, cts, len(bank))
    src, encode, n_fresh = bank.tables(rows, cts, T, img.device)
    assert n_fresh == B and src.dtype == torch.int32 and src.numel() == sum(cts)
    fresh = enc.predict(img.flatten(0, 1).index_select(0, encode))
    feats = bank.gather(src, fresh, (B, T) if counts is None else (sum(cts),))
    assert feats.shape[-2:] == (bank.tokens_per_view, bank.feature_dim) == tuple(fresh.shape[1:])
    heat = dec(bf, img, mask.cuda(), feats, None, view_counts=counts)
    kp, kn, idx = hip_ops.decode_topk(heat)
    torch.cuda.synchronize()
    return dec.last_logits.clone(), heat.clone(), idx.clone(), kp.clone()


@pytest.mark.parametrize("prec", [_lib.DEFAULT_PREC, "bf16x3"])
def test_decoder_on_bank_rows_bit_identical_and_within_the_bar(hip, prec):
    enc, dec = _build(prec, DEPTH, DEPTH)
    data, parts = _ragged_batch()
    counts, t_max = data["view_counts"], data["images"].shape[1]
    bank = RefFeatureBank(enc)
    placed = _fill_bank(bank, parts)
    assert len(bank) == sum(counts) - len(counts) and bank.stamp == (enc.model.state_stamp(prec), enc.model.feats_class(prec))
    table = _table(placed, t_max, pad=10 ** 6)                  # junk in the padded slots
    want = _decode(enc, dec, data, counts)
    got = _decode_banked(enc, dec, bank, _poison_banked(data, table), table, counts)
    names = ("logits", "heat", "top-20 indices", "corners")
    for name, g, w in zip(names, got, want):
        assert torch.equal(g, w), (prec, name)
    for b, p in enumerate(parts):
        alone = _decode(enc, dec, p)
        for name, g, a in zip(names, got, alone):
            assert torch.equal(g[b:b + 1], a), (prec, b, name)
    assert dec.recast_count == 0
    for b in range(len(parts)):
        o = _oracle(b)
        err = (got[0][b:b + 1].cpu() - o["logits"]).abs().max().item()
        print(f"[ref bank {prec}] sample {b} (T = {counts[b]}): logits max-abs err {err:.3e}")
        assert err <= LOGIT_TOL[prec], (prec, b, err)
        assert torch.equal(got[2][b:b + 1].cpu().long().sort(-1)[0], o["topk_idx"].sort(-1)[0]), (prec, b)
    # a uniform batch through the bank == the plain uniform forward
    uni, uparts = _ragged_batch(samples=(0, 0))
    uni["bbox_feat"][1] = uni["bbox_feat"][1].flip(0)
    utable = _table([placed[0], placed[0]], 3)                  # both samples name the same rows
    a = _decode(enc, dec, uni, None)
    b_ = _decode_banked(enc, dec, bank, _poison_banked(uni, utable), utable, None)
    assert all(torch.equal(x, y) for x, y in zip(a, b_)) and dec.recast_count == 0


def _keep(model, out):
    return model.decoder.last_logits.clone(), {k: out[k].clone() for k in OUT_KEYS}


def _assert_same(model, out, want, counts, where):
    logits, keys = want
    assert torch.equal(model.decoder.last_logits, logits), where
    assert torch.equal(out["pred_corners_px"], keys["pred_corners_px"]), where
    for b, c in enumerate(counts):
        for k in ("pred_poses", "regression_boxes", "pred_bbox"):
            assert torch.equal(out[k][b, :c], keys[k][b, :c]), (where, b, k)


@pytest.mark.parametrize("prec", [_lib.DEFAULT_PREC, "bf16x3"])
def test_facade_banked_forward_bit_identical(hip, prec):
    model = _facade(prec)
    data, parts = _ragged_batch()
    counts, t_max = data["view_counts"], data["images"].shape[1]
    B = len(counts)
    want = _keep(model, model(_to_dev(data)))                    # (also runs the load-time calibration, once)
    n_syncs = len(model.host_syncs_per_forward)
    bank = RefFeatureBank(model.rgb_encoder, keep_images=True)
    placed = _fill_bank(bank, parts)
    table = _table(placed, t_max)
    out = model(dict(_to_dev(data), ref_bank=bank, ref_rows=table))
    for k in OUT_KEYS:
        assert torch.equal(out[k], want[1][k]), (prec, k)
    assert torch.equal(model.decoder.last_logits, want[0])
    assert len(model.host_syncs_per_forward) == n_syncs
    assert out["hip_precision"]["ref_bank"] == {"banked_views": sum(counts) - B, "encoded_views": B, "refreshed": False}
    assert out["hip_precision"]["ragged_views"] == sum(counts) and model.decoder.recast_count == 0
    # NaN in every banked slot's images and in the padded slots changes no bit; the table may be a CPU tensor
    nan_data, _ = _ragged_batch(fill=float("nan"))
    nan_data = _poison_banked(nan_data, table)
    out_n = model(dict(_to_dev(nan_data), ref_bank=bank, ref_rows=torch.tensor(table)))
    _assert_same(model, out_n, want, counts, "NaN in banked and padded slots")
    if prec != _lib.DEFAULT_PREC:
        return
    # an add() after the first forward (the store grows and is laid out again): earlier row ids stay valid, same bits
    cap0 = bank._cap
    more = bank.add(parts[2]["images"][:, :4].cuda())
    assert tuple(more.shape) == (1, 4) and more.flatten().tolist() == list(range(sum(counts) - B, sum(counts) - B + 4)) and bank._cap > cap0
    out_g = model(dict(_to_dev(nan_data), ref_bank=bank, ref_rows=table))
    _assert_same(model, out_g, want, counts, "after growth")
    # a bank row shared by two samples; a uniform banked batch keeps its sub-batch lanes
    sh, _ = _ragged_batch(samples=(0, 0, 2))
    sh_want = _keep(model, model(_to_dev(sh)))
    sh_table = _table([placed[0], placed[0], placed[2]], t_max)
    out_s = model(dict(_to_dev(_poison_banked(sh, sh_table)), ref_bank=bank, ref_rows=sh_table))
    _assert_same(model, out_s, sh_want, sh["view_counts"], "shared rows")
    uni, _ = _ragged_batch(samples=(0, 0))
    del uni["view_counts"]
    u_want = _keep(model, model(_to_dev(uni)))
    u_table = _table([placed[0], placed[0]], 3)
    out_u = model(dict(_to_dev(_poison_banked(uni, u_table)), ref_bank=bank, ref_rows=u_table))
    _assert_same(model, out_u, u_want, [3, 3], "uniform")
    assert out_u["hip_precision"]["ref_bank"]["banked_views"] == 4 and "ragged_views" not in out_u["hip_precision"]
    # hip_graph: a banked batch takes the eager branch; the bank is filled BEFORE the model's first forward (its calibration)
    graphed = _facade(prec, hip_graph=True)
    gbank = RefFeatureBank(graphed.rgb_encoder)
    gtable = _table(_fill_bank(gbank, parts), t_max)
    out_h = graphed(dict(_to_dev(nan_data), ref_bank=gbank, ref_rows=gtable))
    assert graphed._graph is None
    assert torch.equal(graphed.decoder.last_logits, want[0]) and torch.equal(out_h["pred_corners_px"], want[1]["pred_corners_px"])


def test_uniform_banked_batch_as_the_first_forward_of_a_fresh_model(hip):
    """The load-time calibration runs inside the first forward and measures on the first TWO samples of a uniform batch
    (calibrate.MAX_SAMPLES): with a bank, every banked slot it reads comes from the kept crops -- NaN in the batch's own images there
    (sample 1's included) reaches neither the promotion state nor a result."""
    from boxdreamer_amd import calibrate
    assert calibrate.MAX_SAMPLES == 2
    uni, parts = _ragged_batch(samples=(0, 2, 1))                  # three different samples, cut to their first two views below
    del uni["view_counts"]
    for k in uni:
        if torch.is_tensor(uni[k]) and uni[k].dim() >= 2:
            uni[k] = uni[k][:, :2].contiguous()
    uni["query_idx"] = torch.tensor([1, 0, 1])
    plain = _facade(_lib.DEFAULT_PREC)
    want = _keep(plain, plain(_to_dev(uni)))
    rep = plain.decoder.hip_calibration
    assert rep["applicable"] and rep["delta_final"] == rep["delta_final"]          # measured, and not NaN
    model = _facade(_lib.DEFAULT_PREC)
    bank = RefFeatureBank(model.rgb_encoder)
    rows = bank.add(torch.stack([uni["images"][b, 1 - int(q)] for b, q in enumerate(uni["query_idx"])]).cuda()).tolist()
    table = [[-1, -1] for _ in rows]
    for b, q in enumerate(uni["query_idx"].tolist()):
        table[b][1 - q] = rows[b]
    out = model(dict(_to_dev(_poison_banked(uni, table)), ref_bank=bank, ref_rows=table))
    got = model.decoder.hip_calibration
    assert got["delta_final"] == rep["delta_final"] and got.get("promoted") == rep.get("promoted")
    assert calibrate.get_state(model.rgb_encoder, model.decoder) == calibrate.get_state(plain.rgb_encoder, plain.decoder)
    for k in OUT_KEYS:
        assert torch.equal(out[k], want[1][k]), k
    assert torch.equal(model.decoder.last_logits, want[0])
    assert out["hip_precision"]["ref_bank"]["banked_views"] == 3 and out["hip_precision"]["ref_bank"]["encoded_views"] == 3


def test_stale_bank_refreshes_once_or_refuses(hip):
    model = _facade(_lib.DEFAULT_PREC)
    data, parts = _ragged_batch()
    counts, t_max = data["view_counts"], data["images"].shape[1]
    model(_to_dev(data))
    enc = model.rgb_encoder
    bank = RefFeatureBank(enc, keep_images=True)
    table = _table(_fill_bank(bank, parts), t_max)
    old = bank.stamp
    enc.model.promote[0] |= _lib.PROMOTE_QKV                      # the encoder's promotion state moves on after the bank was filled
    want = _keep(model, model(_to_dev(data)))
    banked = dict(_to_dev(_poison_banked(data, table)), ref_bank=bank, ref_rows=table)
    cache_mod._WARNED_STALE_BANK = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = model(dict(banked))
        out2 = model(dict(banked))
    assert sum("re-encoding its rows" in str(x.message) for x in w) == 1
    assert out["hip_precision"]["ref_bank"]["refreshed"] is True and out2["hip_precision"]["ref_bank"]["refreshed"] is False
    assert bank.stamp != old and bank.stamp[0] == enc.model.state_stamp(enc.prec) and bank.refresh_count == 1
    _assert_same(model, out, want, counts, "refreshed")
    _assert_same(model, out2, want, counts, "after the refresh")
    # keep_images=False: a stale bank is refused before anything is launched
    lean = RefFeatureBank(enc, keep_images=False)
    lean_table = _table(_fill_bank(lean, parts), t_max)
    _assert_same(model, model(dict(_to_dev(data), ref_bank=lean, ref_rows=lean_table)), want, counts, "keep_images=False, fresh")
    enc.model.promote[1] |= _lib.PROMOTE_QKV
    lib = _lib.load()
    stale_batch = dict(_to_dev(data), ref_bank=lean, ref_rows=lean_table)
    buf = (_lib.TraceRecord * 64)()
    _lib.check(lib.bd_trace_begin(64), "bd_trace_begin")
    try:
        with pytest.raises(RuntimeError, match="keep_images=False"):
            model(stale_batch)
    finally:
        launched = lib.bd_trace_end(buf, 64)
    assert launched == 0
    with pytest.raises(RuntimeError):
        lean.add(parts[0]["images"][0, :1].cuda())                 # never rows of two states in one bank
    # decoder side: its adapter's first Linear changes class after the bank was filled -- nothing to re-cast from
    fresh_bank = RefFeatureBank(enc)
    ftable = _table(_fill_bank(fresh_bank, parts), t_max)
    model.decoder.hip_promote_misc |= _lib.PROMOTE_ADAPTER_FC1
    with pytest.raises(ValueError, match="operand class"):
        model(dict(_to_dev(data), ref_bank=fresh_bank, ref_rows=ftable))


def test_facade_errors(hip):
    model = _facade(_lib.DEFAULT_PREC)
    data, parts = _ragged_batch()
    t_max = data["images"].shape[1]
    bank = RefFeatureBank(model.rgb_encoder)
    table = _table(_fill_bank(bank, parts), t_max)
    dev = _to_dev(data)
    with pytest.raises(TypeError):
        model(dict(dev, ref_bank=bank, ref_rows=torch.tensor(table).cuda()))
    for b, t, v in ((0, 0, len(bank)), (2, 3, -2)):
        bad = [list(r) for r in table]
        bad[b][t] = v
        with pytest.raises(ValueError):
            model(dict(dev, ref_bank=bank, ref_rows=bad))
    for bad in (table[:2], [r[:-1] for r in table], torch.tensor(table).flatten()):
        with pytest.raises(ValueError):
            model(dict(dev, ref_bank=bank, ref_rows=bad))
    with pytest.raises(NotImplementedError, match="cached_rgb_feat"):
        model(dict(dev, ref_bank=bank, ref_rows=table, cached_rgb_feat=torch.zeros(1), cached_rgb_mask=torch.zeros(1)))
    with pytest.raises(KeyError):
        model(dict(dev, ref_bank=bank))
    bad = [list(r) for r in table]
    bad[0][0] = len(bank)
    with pytest.raises(ValueError):                                  # the explicit self-check validates the table like forward()
        model.calibrate(dict(dev, ref_bank=bank, ref_rows=bad))
    dense = _facade(_lib.DEFAULT_PREC, dense_cfg={"enable": True})
    with pytest.raises(NotImplementedError, match="dense_cfg"):
        dense(dict(dev, ref_bank=bank, ref_rows=table))
    assert len(bank) == 7
    bank.clear()
    assert len(bank) == 0 and bank.stamp is None
