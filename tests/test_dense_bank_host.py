"""CPU: the host side of the dense-reference mode over the reference bank -- the `ref_rows` contract of a banked dense batch
(_lib.dense_bank_tables, BoxDreamer's checks, all of which run before any launch and so on a box without a GPU), the integer-index
re-pack of the batch dict against dense.filter_by_neighbor_mask, and the argument validation of bd_match_view_sums /
bd_match_select_rows."""
import os
import re

import pytest
import torch

from boxdreamer_amd import _lib, dense
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.model import BoxDreamer

K = 3
DENSE = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": K, "multi_round": False}


def _model(dense_cfg):
    cfg = {"modules": {
        "use_keypoints": False, "use_matching": False, "use_tracking": False, "use_rgb": True, "use_pp": True,
        "regression_intri": True, "rotation_type": None, "coordinate": "object", "pose_representation": "bb8",
        "bbox_representation": "heatmap", "patchify_rays": True, "dense_cfg": dense_cfg,
        "decoder": {"d_model": 768, "nhead": 8, "num_decoder_layers": 1, "decoder_only": True, "patch_size": 14,
                    "img_size": 224, "diff_emb": False, "nvs_supervision": False, "ray_supervision": True, "use_mask": False},
        "encoder": {"name": "dino", "dino": {"ckpt_path": None, "cfg": {"model_type": "dinov2_vitb14_reg",
                                                                        "synthetic_seed": 1, "depth": 1}}}}}
    return BoxDreamer(cfg).eval()


def _bank(model, rows=40, **kw):
    """A bank that claims `rows` rows (nothing is encoded on this box: every case below is refused before the bank is read)."""
    bank = RefFeatureBank(model.rgb_encoder, **kw)
    bank._n = rows
    return bank


def _batch(B=2, T=6, query=(5, 1)):
    data = {"images": torch.zeros(B, T, 3, 8, 8), "bbox_feat": torch.zeros(B, T, 8, 8, 8), "query_idx": torch.tensor(query)}
    table = [[b * T + t for t in range(T)] for b in range(B)]
    for b, q in enumerate(query):
        table[b][q] = -1
    return data, table


def test_table_validation_each_with_its_own_message():
    model = _model(DENSE)
    bank = _bank(model, match_threshold=0.05)
    data, table = _batch()
    stray = [list(r) for r in table]
    stray[1][4] = -1
    with pytest.raises(ValueError, match="exactly one slot is -1"):
        model(dict(data, ref_bank=bank, ref_rows=stray))
    moved = [list(r) for r in table]
    moved[0][5], moved[0][2] = 7, -1
    with pytest.raises(ValueError, match="must be the query view"):
        model(dict(data, ref_bank=bank, ref_rows=moved))
    with pytest.raises(ValueError, match="fewer than dense_cfg.filter_topk"):      # sample 1 keeps 2 references
        model(dict(data, ref_bank=bank, ref_rows=table, view_counts=[6, 3]))
    with pytest.raises(ValueError, match="match summaries"):
        model(dict(data, ref_bank=_bank(model), ref_rows=table))
    with pytest.raises(ValueError, match="is not among the sample's"):             # the ragged mode's host query_idx rule
        model(dict(data, ref_bank=bank, ref_rows=table, view_counts=[5, 6]))
    with pytest.raises(ValueError, match="nor a row of the bank"):
        model(dict(data, ref_bank=_bank(model, rows=3, match_threshold=0.05), ref_rows=table))


def test_combinations_that_stay_unimplemented_say_so():
    data, table = _batch()
    multi = _model(dict(DENSE, multi_round=True, sub_batch_size=2))
    with pytest.raises(NotImplementedError, match="multi_round"):
        multi(dict(data, ref_bank=_bank(multi, match_threshold=0.05), ref_rows=table))
    model = _model(DENSE)
    with pytest.raises(NotImplementedError, match="needs a ref_bank"):
        model(dict(data, view_counts=[6, 4]))
    with pytest.raises(NotImplementedError, match="cached_rgb_feat"):
        model(dict(data, view_counts=[6, 4], cached_rgb_feat=torch.zeros(1), cached_rgb_mask=torch.zeros(1)))
    plain = _model({"enable": True})                                   # no DINO filter: nothing to select by
    with pytest.raises(NotImplementedError, match="dense_cfg"):
        plain(dict(data, ref_bank=_bank(plain, match_threshold=0.05), ref_rows=table))


def test_bank_summaries_flag_and_constructor_default():
    model = _model(DENSE)
    assert RefFeatureBank(model.rgb_encoder).has_match_summaries is False
    assert RefFeatureBank(model.rgb_encoder).match_threshold is None
    bank = RefFeatureBank(model.rgb_encoder, keep_images=False, match_threshold=0.05)
    assert bank.has_match_summaries is True and bank.match_threshold == 0.05 and len(bank) == 0
    with pytest.raises(ValueError, match="match summaries"):
        RefFeatureBank(model.rgb_encoder).select(None, None, None, None, K)


def test_dense_bank_tables():
    rows = [[4, 5, -1, 6, 7, 99, 99], [-1, 0, 1, 2, 3, 8, 9], [1, 1, 2, -1, 50, 50, 50]]
    counts = [5, 7, 4]
    out, n_refs, n_max, query = _lib.dense_bank_tables(rows, counts, 3, [2, 0, 3])
    assert (n_refs, n_max, query) == ([4, 6, 3], 6, [2, 0, 3])
    assert out == [[4, 5, 6, 7, -1, -1], [0, 1, 2, 3, 8, 9], [1, 1, 2, -1, -1, -1]]     # a row may serve two slots of one sample
    assert _lib.dense_bank_tables(rows, counts, 3) == (out, n_refs, n_max, query)       # a device-side query_idx: the table names the query
    with pytest.raises(ValueError, match="fewer than"):
        _lib.dense_bank_tables(rows, counts, 4)
    with pytest.raises(ValueError, match="more than the 1024"):
        _lib.dense_bank_tables([[-1] + [0] * 1025], [1026], 3)


def test_integer_repack_equals_filter_by_neighbor_mask():
    """dense.filter_by_view_index on the view indices of a selection == dense.filter_by_neighbor_mask on its mask, key for key."""
    B, T, k = 3, 6, 3
    g = torch.Generator().manual_seed(5)
    keys = {"bbox_feat": (8, 4, 4), "images": (3, 4, 4), "poses": (4, 4), "original_poses": (4, 4), "intrinsics": (3, 3),
            "non_ndc_intrinsics": (3, 3), "original_intrinsics": (3, 3), "scale": (3,), "bbox_3d": (8, 3), "bbox_proj_crop": (8, 2)}
    data = {key: torch.randn((B, T) + shape, generator=g) for key, shape in keys.items()}
    data["other"] = torch.randn(B, T, 2, generator=g)
    query = torch.tensor([5, 0, 2])
    sel = torch.tensor([[0, 2, 4], [1, 2, 3], [0, 1, 4]])              # reference slots, ascending
    cm = torch.zeros(B, T, dtype=torch.bool)
    cm[torch.arange(B), query] = True
    nm = torch.zeros(B, T - 1, dtype=torch.bool)
    nm[torch.arange(B)[:, None], sel] = True
    want = dense.filter_by_neighbor_mask(dict(data), nm, data["bbox_feat"], data["images"], cm, None, None)[0]
    idx = torch.cat([sel + (sel >= query[:, None]).long(), query[:, None]], dim=1)
    got = dict(data)
    qi = dense.filter_by_view_index(got, idx, torch.arange(B))
    assert set(got) == set(want) and qi.tolist() == [k] * B
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert torch.equal(got["other"], data["other"])                    # a key the reference does not re-pack stays as it is


def test_original_images_repacked_on_the_host():
    model = _model(DENSE)
    org = [[f"v{t}b{b}" for b in range(2)] for t in range(6)]          # [T][B]
    data = {"original_images": org}
    slots_host = [[0, 2, 4], [0, 1, 3]]                                # as they come back with the corners' D2H
    syncs = []
    model._repack_original_images(data, [5, 1], None, slots_host, syncs)
    assert data["original_images"] == [["v0b0", "v0b1"], ["v2b0", "v2b1"], ["v4b0", "v4b1"], ["v5b0", "v1b1"]] and syncs == []


def test_abi_declares_both_entries_and_they_validate_before_any_launch():
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "boxdreamer_hip.h")).read()
    for name in ("bd_match_view_sums", "bd_match_select_rows"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    p = [0x10000000 * (i + 1) for i in range(9)]        # made-up addresses: every call below returns before anything is dereferenced

    def select(ptrs=p, R=20, B=3, N_max=9, L=16, D=96, k=3):
        return lib.bd_match_select_rows(ptrs[0], ptrs[1], R, ptrs[2], ptrs[3], ptrs[4], ptrs[5], B, N_max, L, D, k, ptrs[6], ptrs[7],
                                        ptrs[8], None)

    assert select(N_max=1025) == -1 and select(N_max=1025, k=1025) == -1
    assert select(k=10) == -1 and select(k=0) == -1 and select(k=-2) == -1
    assert select(B=0) == -1 and select(N_max=0) == -1 and select(L=0) == -1 and select(D=0) == -1 and select(R=-1) == -1
    for i in range(9):
        assert select(ptrs=[None if j == i else x for j, x in enumerate(p)]) == -5, i
    assert select(ptrs=[None] * 9, N_max=1025) == -5                  # NULL is reported first

    def sums(feats=p[0], images=p[1], dt=_lib.DTYPE_F32, V=0, L=16, D=96, H=16, W=16, s=p[2], c=p[3]):
        return lib.bd_match_view_sums(feats, images, dt, V, L, D, H, W, 0.05, s, c, None)

    assert sums() == 0                                                  # V == 0: BD_OK without a launch
    assert sums(V=-1) == -1 and sums(L=1025) == -1 and sums(L=0) == -1 and sums(D=0) == -1 and sums(H=0) == -1 and sums(W=0) == -1
    assert sums(dt=7) == -2
    assert sums(feats=None) == -5 and sums(images=None) == -5 and sums(s=None) == -5 and sums(c=None) == -5
