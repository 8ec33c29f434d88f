"""Ragged batches (a different number of views per sample), the parts that need no GPU: the new C entry points are exported and
reject bad arguments before any launch, the ragged workspace equals the uniform one at equal views, and the host-side bookkeeping
(packing index, offsets, the attention work list the kernels derive from the offsets, the facade's validation)."""
import ctypes
import json
import os

import pytest
import torch

from boxdreamer_amd import _lib, pack, synth
from boxdreamer_amd.betr import BETR
from boxdreamer_amd.model import BoxDreamer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bd_attention_varlen", "bd_query_substitute_varlen", "bd_gather_query_rows_f32_varlen", "bd_gather_query_tokens_varlen",
       "bd_decoder_workspace_bytes_ragged", "bd_decoder_forward_ragged"]
P1 = ctypes.c_void_p(0x10000)          # a non-NULL, 256-byte aligned address that no rejected call may touch
BETR_KW = dict(d_model=768, nhead=8, num_decoder_layers=1, decoder_only=True, patch_size=14, img_size=224, diff_emb=False,
               nvs_supervision=False, ray_supervision=True, use_mask=False, use_pretrained=True, patchify_rays=True,
               pose_representation="bb8", bbox_representation="heatmap")


def test_new_symbols_are_additive():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "boxdreamer_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"{name}(" in hdr
    assert lib.bd_abi_version() == 9                     # purely additive: the ABI version does not move


def test_attention_varlen_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()

    def call(qkv=P1, out=P1, vs=P1, batch=3, n_views=9, max_views=4, tpv=256, heads=8, hd=96, prec=_lib.PREC_F16):
        return lib.bd_attention_varlen(qkv, 0, out, 0, vs, batch, n_views, max_views, tpv, heads, hd, 0.1, None, prec, None)

    assert call(qkv=None) == -5 and call(out=None) == -5 and call(vs=None) == -5
    assert call(hd=64) == -1 and call(hd=128) == -1       # head_dim 96 only
    assert call(tpv=100) == -1 and call(tpv=64) == -1 and call(tpv=0) == -1      # whole q-blocks and key tiles per view
    assert call(batch=0) == -1 and call(heads=0) == -1
    assert call(n_views=2) == -1                          # fewer views than samples
    assert call(max_views=0) == -1 and call(max_views=8) == -1      # 3 samples in 9 views: no sample can have 8
    assert call(n_views=1 << 20, max_views=1 << 19, tpv=256) == -1  # one sample's rows beyond the 2 GiB buffer descriptor
    assert call(qkv=ctypes.c_void_p(0x10008)) == -3
    assert call(prec=_lib.PREC_F16C8) == -2 and call(prec=99) == -2


def test_ragged_layout_operators_reject_bad_arguments():
    lib = _lib.load()
    assert lib.bd_query_substitute_varlen(P1, P1, P1, P1, None, P1, 2, 256, 768, None) == -5
    assert lib.bd_query_substitute_varlen(P1, P1, P1, P1, P1, None, 2, 256, 768, None) == -5
    assert lib.bd_query_substitute_varlen(P1, P1, P1, P1, P1, P1, 0, 256, 768, None) == -1
    assert lib.bd_gather_query_rows_f32_varlen(P1, None, P1, P1, 2, 256, 768, None) == -5
    assert lib.bd_gather_query_rows_f32_varlen(P1, P1, P1, P1, 2, 256, 770, None) == -1
    assert lib.bd_gather_query_tokens_varlen(P1, P1, None, P1, 0, 2, 256, 768, 0, None) == -5
    assert lib.bd_gather_query_tokens_varlen(P1, P1, P1, P1, 0, 2, 256, 772, 0, None) == -1
    assert lib.bd_gather_query_tokens_varlen(P1, P1, P1, P1, 0, 2, 0, 768, 0, None) == -1


@pytest.fixture(scope="module")
def betr_weights():
    return pack.pack_betr(synth.betr_state_dict(1234, 1), "bf16", "cpu", 8)


def test_decoder_ragged_rejects_bad_arguments_and_sizes_its_workspace(betr_weights):
    lib = _lib.load()
    w = betr_weights.struct

    def call(bf=P1, f16=P1, vs=P1, qv=P1, B=3, n_views=9, max_views=4, size=224, ws=P1, ws_bytes=1 << 40, prec=0, in_dtype=2):
        return lib.bd_decoder_forward_ragged(w, bf, in_dtype, f16, 0, vs, qv, B, n_views, max_views, size, P1, P1, ws, ws_bytes, prec, None)

    assert call(bf=None) == -5 and call(f16=None) == -5 and call(vs=None) == -5 and call(qv=None) == -5 and call(ws=None) == -5
    assert call(prec=99) == -2 and call(in_dtype=3) == -2
    assert call(B=0) == -1 and call(n_views=2) == -1 and call(max_views=0) == -1 and call(max_views=8) == -1
    assert call(max_views=2) == -1                        # 3 samples of at most 2 views cannot hold 9
    assert call(size=200) == -1
    assert call(ws=ctypes.c_void_p(0x10010)) == -3
    assert call(ws_bytes=1024) == -4                      # checked before the first launch
    assert lib.bd_decoder_workspace_bytes_ragged(None, 9, 3, 0) == 0 and lib.bd_decoder_workspace_bytes_ragged(w, 2, 3, 0) == 0
    for prec in ("bf16", "fp16", "bf16x3", "fp8", "f16c8", "f16c8_qk16", "f16x3", "f16x3_attn_x3"):
        pid = _lib.prec_id(prec)
        for B, T in ((1, 2), (3, 6), (32, 6), (2, 17)):
            assert lib.bd_decoder_workspace_bytes_ragged(w, B * T, B, pid) == lib.bd_decoder_workspace_bytes(w, B, T, pid) > 0
    # sized by views, not by B x the longest sample
    assert lib.bd_decoder_workspace_bytes_ragged(w, 30, 5, 13) < lib.bd_decoder_workspace_bytes(w, 5, 17, 13)


PRECS = ("bf16", "fp16", "bf16x3", "fp8", "f16c8", "f16c8_qk16", "f16x3", "f16x3_attn_x3")


def _workspace_row(lib, wd, we, B, T, pid):
    """Every *_workspace_bytes* entry point of the whole-path calls at one batch, in the fixture's column order."""
    n = B * T
    return ([lib.bd_decoder_workspace_bytes(wd, B, T, pid), lib.bd_decoder_workspace_bytes_ragged(wd, n, B, pid)] +
            [lib.bd_decoder_workspace_bytes_lanes(wd, B, T, pid, l) for l in (1, 2, 4)] +
            [lib.bd_decoder_entry_tokens_workspace_bytes(wd, n, pid), lib.bd_decoder_entry_workspace_bytes_ragged(wd, n, B, pid)] +
            [lib.bd_decoder_entry_workspace_bytes(wd, B, T, pid, l) for l in (1, 2, 4)] +
            [lib.bd_encoder_workspace_bytes(we, n, pid)] + [lib.bd_encoder_workspace_bytes_lanes(we, n, pid, l) for l in (1, 2, 4)])


def test_workspace_bytes_are_pinned_and_share_one_layout(betr_weights):
    """The workspace sizes are part of the contract with callers that size their blobs once (graph capture, the facade's cache): every
    entry point returns the bytes recorded in tests/golden/workspace_bytes.json (computed once, before the decoder's carvers became
    one), and the sizes relate as the one take() order -- a_heat, t1, t2, rgb, qtok, proj, blk -- implies."""
    lib = _lib.load()
    wd = betr_weights.struct
    enc = pack.pack_dino(synth.dino_state_dict(4321, 1), "bf16", "cpu", 12)
    we = enc.struct
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")))
    try:
        for prec in PRECS:
            for B, T, lat in ((1, 2, 0), (1, 2, 1), (3, 6, 0), (32, 6, 0), (2, 17, 0)):
                wd.latency_mode = we.latency_mode = lat
                row = _workspace_row(lib, wd, we, B, T, _lib.prec_id(prec))
                assert row == want[f"{prec} B={B} T={T} latency={lat}"], (prec, B, T, lat)
    finally:
        wd.latency_mode = we.latency_mode = 0

    def takes(off, sizes):                                   # csrc/forward.hip Carver.take, then the 256 spare bytes of every total
        for s in sizes:
            off = (off + 255) // 256 * 256 + s
        return off + 256

    P, D, F = wd.grid * wd.grid, wd.dim, wd.patch * wd.patch * wd.box_dim
    for prec in PRECS:
        pid = _lib.prec_id(prec)
        e = 2 * (2 if prec not in ("bf16", "fp16", "fp8") else 1)          # bytes per element of a 16-bit operand buffer (both planes)
        for B, T in ((1, 2), (3, 6), (32, 6), (2, 17)):
            n = B * T
            Mb, Mq = n * P, B * P
            stack = [Mq * D * e, Mq * F * 4,                               # the head: qtok, proj
                     Mb * D * 4, Mb * D * e, Mb * 3 * D * e, Mb * D * e, Mb * 4 * D * e, Mb * ((D + 95) // 96) * 8]      # the blocks' buffers
            tokens = lib.bd_decoder_entry_tokens_workspace_bytes(wd, n, pid)
            assert tokens == takes(0, [Mb * wd.kpad * e, Mb * D * e, Mb * D * 4, Mb * D * 4])
            assert lib.bd_decoder_workspace_bytes_ragged(wd, n, B, pid) == takes(tokens - 256, stack)
            ragged = lib.bd_decoder_entry_workspace_bytes_ragged(wd, n, B, pid)
            assert ragged == takes(0, [Mq * D * e, Mq * D * 4, Mq * D * 4] + stack)                # no a_heat, the adapter on the query rows
            assert 0 <= lib.bd_decoder_entry_workspace_bytes(wd, B, T, pid, 1) - ragged < 256
            assert 0 <= lib.bd_decoder_workspace_bytes_lanes(wd, B, T, pid, 1) - lib.bd_decoder_workspace_bytes(wd, B, T, pid) < 256


def test_packing_index_and_offsets():
    counts, t_max = [2, 6, 3, 17, 2], 17
    idx = _lib.packing_index(counts, t_max)
    assert len(idx) == sum(counts) == 30 and idx == sorted(idx)
    padded = torch.arange(len(counts) * t_max).reshape(len(counts), t_max)
    assert torch.equal(padded.flatten()[torch.tensor(idx)], torch.cat([padded[b, :c] for b, c in enumerate(counts)]))
    vs = _lib.view_starts(counts)
    assert vs == [0, 2, 8, 11, 28, 30]
    assert _lib.packing_index([3, 3], 3) == list(range(6))              # all counts == T_max: the identity


def _device_decomposition(wg, view_start, heads, bpv, query_only):
    """What a workgroup of the VL kernels does with its work-item number (csrc/attention.hip), restated on the host."""
    B = len(view_start) - 1
    if query_only:
        qb, bh = wg % bpv, wg // bpv
        return bh // heads, bh % heads, qb
    ipv = bpv * heads
    b = sum(1 for i in range(B) if view_start[i + 1] * ipv <= wg)        # the ballot count
    nqb = (view_start[b + 1] - view_start[b]) * bpv
    local = wg - view_start[b] * ipv
    return b, local // nqb, local % nqb


@pytest.mark.parametrize("counts", [[2, 6, 3, 17, 2], [4, 4, 4], [2], [3, 1, 5]])
@pytest.mark.parametrize("q_block", [256, 128])
def test_attention_work_list_matches_the_kernels_decomposition(counts, q_block):
    heads, tpv = 8, 256
    vs = _lib.view_starts(counts)
    for query_only in (False, True):
        work = _lib.attention_work_list(counts, heads, tpv, q_block, query_only)
        units = len(counts) if query_only else sum(counts)
        assert len(work) == units * (tpv // q_block) * heads              # the grid: exactly the batch's q-blocks, no idle workgroups
        assert len(set(work)) == len(work)
        for wg, item in enumerate(work):
            assert _device_decomposition(wg, vs, heads, tpv // q_block, query_only) == item
    # the q-blocks of one (sample, head) are consecutive items: the XCD remap keeps them on one L2
    work = _lib.attention_work_list(counts, heads, tpv, q_block)
    for a, b in zip(work, work[1:]):
        assert a[:2] == b[:2] and b[2] == a[2] + 1 or b[2] == 0


def test_view_counts_validation_on_the_host():
    assert _lib.view_counts_list([3, 2]) == [3, 2] and _lib.view_counts_list(torch.tensor([3, 2], dtype=torch.int32)) == [3, 2]
    with pytest.raises(TypeError):
        _lib.view_counts_list(torch.tensor([3.0, 2.0]))
    with pytest.raises(TypeError):
        _lib.view_counts_list([3, 2.5])
    with pytest.raises(ValueError):
        _lib.view_counts_list([3, 2], B=3)
    for bad in ([1, 3], [3, 6], [0, 2], [-1, 2]):
        with pytest.raises(ValueError):
            _lib.check_view_counts(bad, 5)
    _lib.check_view_counts([2, 5], 5, [1, 4])
    with pytest.raises(ValueError):
        _lib.check_view_counts([2, 5], 5, [2, 4])          # the query view of sample 0 is a padded slot
    # the facade's reading of the batch-dict key
    data = {"view_counts": [3, 5], "query_idx": torch.tensor([2, 4])}
    assert BoxDreamer._view_counts(data, 2, 5) == [3, 5]
    assert BoxDreamer._view_counts({"query_idx": torch.tensor([2, 4])}, 2, 5) is None
    assert BoxDreamer._view_counts({"view_counts": torch.tensor([5, 5]), "query_idx": torch.tensor([2, 4])}, 2, 5) is None    # == uniform
    with pytest.raises(ValueError):
        BoxDreamer._view_counts({"view_counts": [3, 5], "query_idx": torch.tensor([3, 4])}, 2, 5)
    with pytest.raises(ValueError):
        BoxDreamer._view_counts({"view_counts": [1, 5], "query_idx": torch.tensor([0, 4])}, 2, 5)
    with pytest.raises(ValueError):
        BoxDreamer._view_counts({"view_counts": [3, 6], "query_idx": torch.tensor([0, 4])}, 2, 5)


def test_betr_validates_view_counts_before_it_needs_a_gpu():
    m = BETR(**BETR_KW).eval()
    x, img, feat = torch.zeros(2, 3, 8, 224, 224), torch.zeros(2, 3, 3, 224, 224), torch.zeros(2, 3, 256, 768)
    mask = torch.tensor([[False, True, False], [False, False, True]])
    with pytest.raises(ValueError):
        m(x, img, mask, feat, None, view_counts=[1, 3])
    with pytest.raises(ValueError):
        m(x, img, mask, feat, None, view_counts=[2, 4])
    with pytest.raises(ValueError):
        m(x, img, mask, feat, None, view_counts=[2, 3, 3])
    with pytest.raises(TypeError):
        m(x, img, mask, feat, None, view_counts=torch.tensor([2.0, 3.0]))
    if not torch.cuda.is_available():                       # valid counts: the product path then fails loudly for want of a device
        with pytest.raises(_lib.HipLibraryError):
            m(x, img, mask, feat, None, view_counts=[2, 3])
