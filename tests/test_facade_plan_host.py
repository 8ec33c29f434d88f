"""CPU: BoxDreamer._plan, the host record one forward is run from -- the mode and the fields of one batch of each kind, and which rule
speaks first for a batch that breaks two (the refusals go through forward(): they come before anything is launched)."""
import pytest
import torch

from boxdreamer_amd.cache import RefFeatureBank
from test_dense_rounds_host import _model

DENSE = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": 2, "multi_round": False}
ROUNDS = dict(DENSE, multi_round=True, sub_batch_size=2, fine_level=False)
QUERY = (2, 0)
NO_DENSE_PLAN = dict(ref_rows=None, n_refs=None, n_max=None, query=None, k=None)


def _batch(T, query=QUERY):
    B = len(query)
    data = {"images": torch.zeros(B, T, 3, 8, 8), "bbox_feat": torch.zeros(B, T, 8, 8, 8), "query_idx": torch.tensor(query)}
    table = [[-1 if t == q else b * T + t for t in range(T)] for b, q in enumerate(query)]
    return data, table


def _bank(model, n=40, **kw):
    bank = RefFeatureBank(model.rgb_encoder, **kw)
    bank._n = n                     # (rows that are never read: the plan looks at the bank's length and at what it keeps)
    return bank


def _assert_plan(plan, **want):
    for name, value in want.items():
        got = getattr(plan, name)
        assert (got is value) if name == "bank" else (got == value), (name, got, value)


def test_plan_of_one_batch_of_each_kind():
    model = _model(None)
    data, table = _batch(3)
    base = dict(B=2, T=3, counts=None, views_per_sample=[3, 3], query_idx=[2, 0], dense=False, multi_round=False, bank=None, rows=None,
                entry=False, entry_query=None, **NO_DENSE_PLAN)
    _assert_plan(model._plan(data, 2, 3), mode="eager", **base)
    _assert_plan(model._plan(dict(data, view_counts=[3, 3]), 2, 3), mode="eager", **base)             # every count == T: the uniform batch
    # ragged [3, 2] of T_max = 3
    ragged = dict(data, view_counts=torch.tensor([3, 2]), query_idx=torch.tensor([2, 1]))
    _assert_plan(model._plan(ragged, 2, 3), mode="eager", **dict(base, counts=[3, 2], views_per_sample=[3, 2], query_idx=[2, 1]))
    # cached features: eager, and under hip_graph too (on the CPU nothing is captured either way)
    cached = dict(data, cached_rgb_feat=torch.zeros(1), cached_rgb_mask=torch.zeros(1))
    for graph in (False, True):
        model.hip_graph = graph
        _assert_plan(model._plan(cached, 2, 3), mode="eager", **base)
    model.hip_graph = False
    # feature bank: the references of sample 0 banked, sample 1 encodes all its views
    bank = _bank(model)
    rows = [table[0], [-1, -1, -1]]
    _assert_plan(model._plan(dict(data, ref_bank=bank, ref_rows=torch.tensor(rows)), 2, 3), mode="eager", **dict(base, bank=bank, rows=rows))
    # entry-token bank, uniform and ragged; bbox_feat may be absent
    ebank = _bank(model, decoder=model.decoder)
    no_heat = {k: v for k, v in data.items() if k != "bbox_feat"}
    for d in (data, no_heat):
        _assert_plan(model._plan(dict(d, ref_bank=ebank, ref_rows=table), 2, 3), mode="entry_bank",
                     **dict(base, bank=ebank, rows=table, entry=True, entry_query=[2, 0]))
    rtable = [table[0], [3, -1, 99]]
    _assert_plan(model._plan(dict(ragged, ref_bank=ebank, ref_rows=rtable), 2, 3), mode="entry_bank",
                 **dict(base, counts=[3, 2], views_per_sample=[3, 2], query_idx=[2, 1], bank=ebank, rows=rtable, entry=True, entry_query=[2, 1]))


@pytest.mark.parametrize("cfg", [DENSE, ROUNDS], ids=["single", "multi_round"])
def test_plan_of_a_banked_dense_batch(cfg):
    """k = 2 over 4 references per sample."""
    model = _model(cfg)
    data, table = _batch(5)
    multi = bool(cfg["multi_round"])
    want = dict(B=2, T=5, counts=None, views_per_sample=[5, 5], query_idx=[2, 0], dense=True, multi_round=multi, rows=table,
                ref_rows=[[0, 1, 3, 4], [6, 7, 8, 9]], n_refs=[4, 4], n_max=4, query=[2, 0], k=2)
    bank = _bank(model, match_threshold=0.05, keep_poses=multi)
    _assert_plan(model._plan(dict(data, ref_bank=bank, ref_rows=table), 2, 5), mode="banked_dense", bank=bank, entry=False,
                 entry_query=None, **want)
    ebank = _bank(model, match_threshold=0.05, keep_poses=multi, decoder=model.decoder)
    _assert_plan(model._plan(dict(data, ref_bank=ebank, ref_rows=table), 2, 5), mode="banked_dense", bank=ebank, entry=True,
                 entry_query=[2, 0], **want)
    # the un-banked dense mode is an eager step
    _assert_plan(model._plan(data, 2, 5), mode="eager", dense=True, multi_round=multi, bank=None, **NO_DENSE_PLAN)


def test_the_earlier_rule_speaks_for_a_batch_that_breaks_two():
    """view_counts, then the mode, then bbox_feat, then the entry bank's table, then the dense bank's."""
    model = _model(DENSE)
    data, table = _batch(5)
    cached = dict(cached_rgb_feat=torch.zeros(1), cached_rgb_mask=torch.zeros(1))
    no_heat = {k: v for k, v in data.items() if k != "bbox_feat"}
    # a view count outside [2, T] + view_counts with cached_rgb_feat: the count
    with pytest.raises(ValueError, match=r"view_counts\[1\] = 7 is outside \[2, 5\]"):
        model(dict(data, view_counts=[5, 7], **cached))
    # view_counts with cached_rgb_feat + no bbox_feat: the mode
    with pytest.raises(NotImplementedError, match="view_counts together with cached_rgb_feat"):
        model(dict(no_heat, view_counts=[5, 4], **cached))
    # a ref_bank without ref_rows + no bbox_feat: the mode
    with pytest.raises(KeyError, match="needs both 'ref_bank'"):
        model(dict(no_heat, ref_bank=_bank(model, match_threshold=0.05)))
    # no bbox_feat over a feature bank + that bank keeps no match summaries: bbox_feat
    with pytest.raises(KeyError, match="^'bbox_feat'$"):
        model(dict(no_heat, ref_bank=_bank(model), ref_rows=table))
    # the entry tokens of another decoder + no match summaries: the entry bank's rule
    other = _bank(model, decoder=_model(None).decoder)
    with pytest.raises(ValueError, match="entry tokens of another decoder"):
        model(dict(no_heat, ref_bank=other, ref_rows=table))
    # a sample with two slots to encode, over an entry bank in the dense mode: the entry bank's wording, not the dense bank's
    ebank = _bank(model, match_threshold=0.05, decoder=model.decoder)
    two = [[-1, 1, -1, 3, 4], table[1]]
    with pytest.raises(ValueError, match=r"ref_rows\[0\]\[0\] = -1 at a reference slot"):
        model(dict(data, ref_bank=ebank, ref_rows=two))
