"""CPU: the host side of the decoder-entry-token bank -- cache.RefFeatureBank(decoder=...)'s contract (add with heat maps, the second
store, its stamp and staleness rules, exercised with stand-in encoder / decoder objects so that nothing is launched), the `ref_rows`
rules of a forward over such a bank (all checked before any launch, so on a box without a GPU), and the argument validation of
bd_assemble_entry_tokens / bd_decoder_entry_tokens / bd_decoder_forward_entry."""
import os
import re
import types
import warnings

import pytest
import torch

from boxdreamer_amd import _lib, cache as cache_mod, features
from boxdreamer_amd.cache import RefFeatureBank
from test_dense_bank_host import DENSE, _batch, _model

P, C, S = 4, 32, 8                       # 3 * S * S = 192 image elements >= P * C = 128 "features"


class _EncModel:
    def __init__(self):
        self.state = 0

    def state_stamp(self, prec=None):
        return ("enc", self.state)

    def feats_class(self, prec=None):
        return _lib.PREC_BF16


class _Encoder:
    """Stands in for DinoV2Wrapper: `predict` returns tagged features made of the crop's own values and the encoder's state."""
    prec = "bf16"

    def __init__(self):
        self.model, self.calls = _EncModel(), 0

    def get_device(self):
        return torch.device("cpu")

    def to_device(self, dev):
        pass

    def predict(self, images):
        self.calls += 1
        n = images.shape[0]
        f32 = (images.float().reshape(n, -1)[:, :P * C] + self.model.state).reshape(n, P, C).contiguous()
        return features.attach(f32, f32.reshape(n * P, C).to(torch.bfloat16), _lib.PREC_BF16, self.model.state_stamp())


class _Decoder:
    """Stands in for BETR: what a bank reads of it -- d_model, the three parts of the entry stamp, entry_tokens."""
    d_model, hip_precision = C, "bf16"

    def __init__(self):
        self.weights, self.hip_promote_misc, self.calls = 0, 0, 0

    def _signature(self):
        return (("w", self.weights),)

    def entry_tokens(self, bbox_feat, feats, out=None):
        self.calls += 1
        assert features.tag_of(feats) is not None and feats.shape[0] == bbox_feat.shape[0]
        out.copy_(feats + bbox_feat.float().mean(dim=(1, 2, 3))[:, None, None] + 100 * self.weights)
        return out


def _views(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, S, S), generator=g), torch.rand((n, 8, S, S), generator=g).to(torch.bfloat16) * 2 - 1


def _want(enc, dec, img, heat):
    return img.reshape(len(img), -1)[:, :P * C].reshape(-1, P, C) + enc.model.state + heat.float().mean(dim=(1, 2, 3))[:, None, None] + 100 * dec.weights


def test_bank_without_a_decoder_is_todays_bank():
    enc = _Encoder()
    bank = RefFeatureBank(enc)
    assert bank.has_entry_tokens is False and bank.decoder is None and bank.entry_tokens is None and bank.entry_bytes_per_view == 0
    img, heat = _views(3, 1)
    assert bank.add(img).tolist() == [0, 1, 2] and bank.add(img[None]).tolist() == [[3, 4, 5]]
    assert len(bank) == 6 and bank.entry_tokens is None and bank.entry_stamp is None and not bank.is_stale()
    with pytest.raises(ValueError, match="keeps no decoder-entry tokens"):
        bank.add(img, bbox_feat=heat)
    assert len(bank) == 6 and enc.calls == 2


def test_add_validates_before_anything_is_encoded():
    enc, dec = _Encoder(), _Decoder()
    bank = RefFeatureBank(enc, decoder=dec)
    img, heat = _views(3, 2)
    assert bank.has_entry_tokens is True
    with pytest.raises(ValueError, match="needs the references' heat maps"):
        bank.add(img)
    for bad in (heat[:2], heat[None], heat[:, :7], heat[..., :4], torch.zeros(3, 8, S, S + 1)):
        with pytest.raises(ValueError, match="bbox_feat must be"):
            bank.add(img, bbox_feat=bad)
    with pytest.raises(ValueError, match="bbox_feat must be"):
        bank.add(img[None], bbox_feat=heat)
    assert len(bank) == 0 and enc.calls == 0 and dec.calls == 0


def test_entry_store_grows_with_the_feature_store_and_keeps_row_ids():
    enc, dec = _Encoder(), _Decoder()
    bank = RefFeatureBank(enc, decoder=dec)
    bank.ENTRY_CHUNK = 8                                                 # the second add is embedded in three calls
    a, ha = _views(5, 3)
    b, hb = _views(20, 4)
    assert bank.add(a, bbox_feat=ha).tolist() == list(range(5))
    cap0 = bank._cap
    first = bank.entry_tokens[:5].clone()
    assert bank.add(b.reshape(4, 5, 3, S, S), bbox_feat=hb.reshape(4, 5, 8, S, S)).tolist() == torch.arange(5, 25).reshape(4, 5).tolist()
    assert bank._cap > cap0 and tuple(bank.entry_tokens.shape) == (bank._cap, P, C) and bank.entry_tokens.dtype == torch.float32
    assert bank.entry_bytes_per_view == P * C * 4 and dec.calls == 1 + 3
    assert torch.equal(bank.entry_tokens[:5], first) and torch.equal(first, _want(enc, dec, a, ha))
    assert torch.equal(bank.entry_tokens[5:25], _want(enc, dec, b, hb))
    assert bank.entry_stamp == ((("w", 0),), "bf16", 0) and bank.stamp == (("enc", 0), _lib.PREC_BF16)
    assert torch.equal(bank.heatmaps_of(7), hb[2]) and bank.heatmaps_of(7).dtype == torch.bfloat16 and torch.equal(bank.image_of(7), b[2])
    rows = [[0, -1, 7], [24, 3, -1]]
    like = torch.zeros(2, 3, 3, S, S)
    got = bank.real_heatmaps(rows, 2, like)
    assert got.dtype == torch.bfloat16 and torch.equal(got[0, 0], ha[0]) and torch.equal(got[0, 2], hb[2]) and torch.equal(got[1, 0], hb[19])
    assert (got[0, 1] == 0).all() and (got[1, 2] == 0).all()
    bank.clear()
    assert len(bank) == 0 and bank.entry_tokens is None and bank.entry_stamp is None


@pytest.mark.parametrize("what", ["decoder weights", "decoder promotion", "decoder precision", "encoder state"])
def test_stale_by_either_stamp_refreshes_once_with_one_warning(what):
    enc, dec = _Encoder(), _Decoder()
    bank = RefFeatureBank(enc, keep_images=True, decoder=dec)
    a, ha = _views(3, 5)
    b, hb = _views(2, 6)
    bank.add(a, bbox_feat=ha)
    bank.add(b, bbox_feat=hb)
    assert not bank.is_stale() and bank.ensure_fresh() is False
    old = bank.entry_tokens[:5].clone()
    if what == "decoder weights":
        dec.weights = 1
    elif what == "decoder promotion":
        dec.hip_promote_misc = _lib.PROMOTE_BBOX_EMB
    elif what == "decoder precision":
        dec.hip_precision = "f16c8_qk16"
    else:
        enc.model.state = 2
    assert bank.is_stale()
    cache_mod._WARNED_STALE_BANK = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert bank.ensure_fresh() is True and bank.ensure_fresh() is False
        assert bank.add(a[:1], bbox_feat=ha[:1]).tolist() == [5]
    assert sum("re-encoding its rows" in str(x.message) for x in w) == 1
    assert bank.refresh_count == 1 and len(bank) == 6 and not bank.is_stale()
    assert bank.entry_stamp == (dec._signature(), dec.hip_precision, dec.hip_promote_misc) and bank.stamp[0] == enc.model.state_stamp()
    want = _want(enc, dec, torch.cat([a, b]), torch.cat([ha, hb]))
    assert torch.equal(bank.entry_tokens[:5], want)
    assert torch.equal(bank.entry_tokens[:5], old) == (what in ("decoder promotion", "decoder precision"))   # (the stand-ins' values ignore those two)
    assert torch.equal(bank.heatmaps_of(4), hb[1])
    # the adapter's fc1 promotion implies fc2's: the stamp does not tell the two spellings apart
    dec.hip_promote_misc = _lib.PROMOTE_ADAPTER_FC1
    assert bank.is_stale() and bank.ensure_fresh() is True
    dec.hip_promote_misc = _lib.PROMOTE_ADAPTER_FC1 | _lib.PROMOTE_ADAPTER_FC2
    assert not bank.is_stale()


def test_stale_without_kept_images_raises():
    enc, dec = _Encoder(), _Decoder()
    bank = RefFeatureBank(enc, keep_images=False, decoder=dec)
    a, ha = _views(3, 7)
    bank.add(a, bbox_feat=ha)
    assert bank._images == [] and bank._heat == []
    dec.weights = 3
    for call in (bank.ensure_fresh, lambda: bank.add(a, bbox_feat=ha)):
        with pytest.raises(RuntimeError, match="keep_images=False"):
            call()
    with pytest.raises(RuntimeError, match="keep_images=False"):
        bank.real_heatmaps([[0, -1]], 1, torch.zeros(1, 2, 3, S, S))
    assert len(bank) == 3 and bank.refresh_count == 0


# ---- the facade's checks, which all run before any launch
def _entry_bank(model, rows=40, **kw):
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder, **kw)
    bank._n = rows
    return bank


def test_facade_table_rules_of_an_entry_bank():
    model = _model(None)
    data, table = _batch()
    del data["bbox_feat"]                                                # an entry bank's batch needs none
    bank = _entry_bank(model)
    stray = [list(r) for r in table]
    stray[1][4] = -1
    with pytest.raises(ValueError, match=r"ref_rows\[1\]\[4\] = -1 at a reference slot: an entry bank takes no freshly encoded references"):
        model(dict(data, ref_bank=bank, ref_rows=stray))
    moved = [list(r) for r in table]
    moved[0][5], moved[0][2] = 7, -1
    with pytest.raises(ValueError, match="must be the query view"):
        model(dict(data, ref_bank=bank, ref_rows=moved))
    none = [list(r) for r in table]
    none[0][5] = 3
    with pytest.raises(ValueError, match="names no slot to encode"):
        model(dict(data, ref_bank=bank, ref_rows=none))
    with pytest.raises(ValueError, match="nor a row of the bank"):
        model(dict(data, ref_bank=_entry_bank(model, rows=3), ref_rows=table))
    with pytest.raises(ValueError, match="is not among the sample's"):
        model(dict(data, ref_bank=bank, ref_rows=table, view_counts=[5, 6]))
    other = _model(None)
    foreign = RefFeatureBank(model.rgb_encoder, decoder=other.decoder)
    foreign._n = 40
    with pytest.raises(ValueError, match="another decoder"):
        model(dict(data, ref_bank=foreign, ref_rows=table))
    # a feature bank's batch still needs bbox_feat
    plain = RefFeatureBank(model.rgb_encoder)
    plain._n = 40
    with pytest.raises(KeyError, match="bbox_feat"):
        model(dict(data, ref_bank=plain, ref_rows=table))
    # the dense mode over an entry bank applies the same rule first, and keeps its own limits
    dense = _model(DENSE)
    dbank = _entry_bank(dense, match_threshold=0.05)
    with pytest.raises(ValueError, match="an entry bank takes no freshly encoded references"):
        dense(dict(data, ref_bank=dbank, ref_rows=stray))
    with pytest.raises(ValueError, match="match summaries"):
        dense(dict(data, ref_bank=_entry_bank(dense), ref_rows=table))
    multi = _model(dict(DENSE, multi_round=True, sub_batch_size=2))
    with pytest.raises(NotImplementedError, match="multi_round"):
        multi(dict(data, ref_bank=_entry_bank(multi, match_threshold=0.05), ref_rows=table))


def test_entry_bank_queries():
    rows = [[4, 5, -1, 6, 99], [-1, 0, 1, 2, 3]]
    assert _lib.entry_bank_queries(rows, [4, 5], [2, 0]) == [2, 0] and _lib.entry_bank_queries(rows, [4, 5]) == [2, 0]
    with pytest.raises(ValueError, match=r"ref_rows\[0\]\[1\] = -1 at a reference slot"):
        _lib.entry_bank_queries([[4, -1, -1, 6, 99], rows[1]], [4, 5], [2, 0])
    with pytest.raises(ValueError, match=r"ref_rows\[0\]\[2\] = -1 at a reference slot"):
        _lib.entry_bank_queries([[4, -1, -1, 6, 99], rows[1]], [4, 5])
    assert _lib.entry_bank_queries([[4, -1, 7, 6, -1], rows[1]], [4, 5]) == [1, 0]         # a padded slot may hold anything


def test_abi_declares_the_entries_and_they_validate_before_any_launch():
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "boxdreamer_hip.h")).read()
    for name, ret in (("bd_assemble_entry_tokens", "int"), ("bd_decoder_entry_tokens", "int"), ("bd_decoder_forward_entry", "int"),
                      ("bd_decoder_forward_entry_ragged", "int"), ("bd_decoder_entry_tokens_workspace_bytes", "size_t"),
                      ("bd_decoder_entry_workspace_bytes", "size_t"), ("bd_decoder_entry_workspace_bytes_ragged", "size_t")):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"^" + ret + " " + name + r"\(", header, re.M), name
    assert lib.bd_abi_version() == 9
    p = [0x10000000 * (i + 1) for i in range(6)]        # made-up addresses: every call below returns before anything is dereferenced

    def asm(ptrs=p, bank_views=4, n_fresh=3, n_views=7, P=256, dim=768):
        return lib.bd_assemble_entry_tokens(ptrs[0], bank_views, ptrs[1], n_fresh, ptrs[2], ptrs[3], ptrs[4], ptrs[5], n_views, P, dim, None)

    assert asm(n_views=0) == 0                                           # BD_OK without a launch
    for i in range(6):
        assert asm(ptrs=[None if j == i else x for j, x in enumerate(p)], n_views=0) == -5, i
    assert asm(ptrs=[None] + p[1:], bank_views=0, n_views=0) == 0 and asm(ptrs=p[:1] + [None] + p[2:], n_fresh=0, n_views=0) == 0
    assert asm(bank_views=-1) == -1 and asm(n_fresh=-1) == -1 and asm(n_views=-1) == -1 and asm(P=0) == -1 and asm(dim=0) == -1
    assert asm(P=3, dim=5, n_views=0) == -3                              # P * dim % 4 != 0
    for i in range(6):
        off = 2 if i == 4 else 4                                         # (src: 4-byte aligned; the float tensors: 16)
        assert asm(ptrs=[x + off if j == i else x for j, x in enumerate(p)], n_views=0) == -3, i
    for i in range(5):                                                   # x_out inside an input
        assert asm(ptrs=p[:5] + [p[i]]) == -1, i
    w = _lib.BetrWeights()
    assert lib.bd_decoder_entry_tokens_workspace_bytes(None, 3, 0) == 0 and lib.bd_decoder_entry_workspace_bytes(None, 2, 3, 0, 1) == 0
    assert lib.bd_decoder_entry_workspace_bytes_ragged(None, 5, 2, 0) == 0
    assert lib.bd_decoder_entry_tokens(None, p[0], 0, p[1], 0, 3, 224, p[2], p[3], 0, 0, None) == -5
    assert lib.bd_decoder_entry_tokens(w, p[0], 0, p[1], 0, 3, 224, None, p[3], 0, 0, None) == -5
    assert lib.bd_decoder_entry_tokens(w, p[0], 7, p[1], 0, 3, 224, p[2], p[3], 0, 0, None) == -2
    assert lib.bd_decoder_forward_entry(None, p[0], 4, p[1], p[2], 0, p[3], 2, 3, 224, p[4], p[4], p[5], 0, 0, 1, None) == -5
    assert lib.bd_decoder_forward_entry(w, p[0], 4, None, p[2], 0, p[3], 2, 3, 224, p[4], p[4], p[5], 0, 0, 2, None) == -5
    assert lib.bd_decoder_forward_entry_ragged(w, p[0], 4, p[1], p[2], 0, None, p[3], 2, 5, 3, 224, p[4], p[4], p[5], 0, 0, None) == -5


# ---- one table of bad arguments through every validating decoder entry point.  Made-up addresses: every call returns before anything
# is dereferenced or launched (a call that went on would fault here).
_ADDR = {k: 0x10000000 * (i + 1) for i, k in enumerate(("bbox", "f16", "qidx", "vs", "src", "bank", "out", "ws"))}
_GOOD = dict(_ADDR, in_dtype=2, prec=0, B=2, T=3, n_views=5, max_views=3, bank_views=4, size=224, ws_bytes=1 << 40)
# entry point -> (the call, the pointers it takes, reads a heat map, kind of batch)
_ENTRY_POINTS = {
    "forward": (lambda lib, w, a: lib.bd_decoder_forward(w, a.bbox, a.in_dtype, a.f16, 0, a.qidx, a.B, a.T, a.size, a.out, a.out, a.ws,
                                                         a.ws_bytes, a.prec, None),
                ("bbox", "f16", "qidx", "out", "ws"), True, "uniform"),
    "forward_lanes(2)": (lambda lib, w, a: lib.bd_decoder_forward_lanes(w, a.bbox, a.in_dtype, a.f16, 0, a.qidx, a.B, a.T, a.size, a.out, a.out,
                                                                        a.ws, a.ws_bytes, a.prec, 2, None),
                         ("bbox", "f16", "qidx", "out", "ws"), True, "uniform"),
    "forward_ragged": (lambda lib, w, a: lib.bd_decoder_forward_ragged(w, a.bbox, a.in_dtype, a.f16, 0, a.vs, a.qidx, a.B, a.n_views, a.max_views,
                                                                       a.size, a.out, a.out, a.ws, a.ws_bytes, a.prec, None),
                       ("bbox", "f16", "vs", "qidx", "out", "ws"), True, "ragged"),
    "forward_entry(1)": (lambda lib, w, a: lib.bd_decoder_forward_entry(w, a.bank, a.bank_views, a.src, a.f16, 0, a.qidx, a.B, a.T, a.size, a.out,
                                                                        a.out, a.ws, a.ws_bytes, a.prec, 1, None),
                         ("bank", "src", "f16", "qidx", "out", "ws"), False, "uniform"),
    "forward_entry(2)": (lambda lib, w, a: lib.bd_decoder_forward_entry(w, a.bank, a.bank_views, a.src, a.f16, 0, a.qidx, a.B, a.T, a.size, a.out,
                                                                        a.out, a.ws, a.ws_bytes, a.prec, 2, None),
                         ("bank", "src", "f16", "qidx", "out", "ws"), False, "uniform"),
    "forward_entry_ragged": (lambda lib, w, a: lib.bd_decoder_forward_entry_ragged(w, a.bank, a.bank_views, a.src, a.f16, 0, a.vs, a.qidx, a.B,
                                                                                   a.n_views, a.max_views, a.size, a.out, a.out, a.ws,
                                                                                   a.ws_bytes, a.prec, None),
                             ("bank", "src", "f16", "vs", "qidx", "out", "ws"), False, "ragged"),
    "entry_tokens": (lambda lib, w, a: lib.bd_decoder_entry_tokens(w, a.bbox, a.in_dtype, a.f16, 0, a.n_views, a.size, a.out, a.ws, a.ws_bytes,
                                                                   a.prec, None),
                     ("bbox", "f16", "out", "ws"), True, "tokens"),
}
# case -> (expected code, what it changes: for every kind of batch, or per kind)
_BAD = {
    **{f"NULL {p}": (-5, {p: None}) for p in ("w", *_ADDR)},
    "bad prec": (-2, {"prec": 99}),
    "in_dtype 3": (-2, {"in_dtype": 3}),                 # bd_decoder_forward too, before anything is enqueued
    "B 0": (-1, {"uniform": {"B": 0}, "ragged": {"B": 0}, "tokens": {"n_views": 0}}),
    "size 200": (-1, {"size": 200}),
    "misaligned workspace": (-3, {"ws": _ADDR["ws"] + 16}),
    "ws_bytes 1024": (-4, {"ws_bytes": 1024}),
    # P = 256 token rows per view: 2^23 views are 2^31 rows -- the uniform entry points too
    "2^31 token rows": (-1, {"uniform": {"B": 1 << 12, "T": 1 << 11}, "ragged": {"n_views": 1 << 23, "max_views": 1 << 22},
                             "tokens": {"n_views": 1 << 23}}),
}


@pytest.fixture(scope="module")
def betr_struct():
    from boxdreamer_amd import pack, synth
    pk = pack.pack_betr(synth.betr_state_dict(1234, 1), "bf16", "cpu", 8)
    yield pk.struct
    del pk


def _applies(entry, case):
    _, pointers, reads_heat_map, _ = _ENTRY_POINTS[entry]
    return (case[5:] in ("w", *pointers)) if case.startswith("NULL ") else (reads_heat_map or case != "in_dtype 3")


@pytest.mark.parametrize("entry,case", [(e, c) for e in _ENTRY_POINTS for c in _BAD if _applies(e, c)])
def test_every_decoder_entry_point_rejects_the_same_bad_arguments_with_the_same_codes(betr_struct, entry, case):
    lib = _lib.load()
    call, _, _, kind = _ENTRY_POINTS[entry]
    code, change = _BAD[case]
    change = change[kind] if set(change) <= {"uniform", "ragged", "tokens"} else change
    args = types.SimpleNamespace(**dict(_GOOD, **change))
    assert call(lib, None if case == "NULL w" else betr_struct, args) == code, (entry, case)
