"""Host: a pose stream that chooses its references on the device (stream.PoseStream(select_k=...), csrc/stream.hip:
bd_stream_select_rows) -- the constructor's refusals that need no device, the host mirror of the kernel's decision and rankings
(stream.select_rows_host) against hand-written expectations and against dense.pose_select_rows_host, and the entry point's argument
checks, which run before any launch."""
import math
import os
import re

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, dense, stream
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.stream import PoseStream, select_rows_host
from test_dense_rounds_host import spread_poses
from test_stream_host import _host_model

INF, NAN = math.inf, math.nan


def test_constructor_refusals_that_need_no_device():
    model = _host_model()
    enc, dec = model.rgb_encoder, model.decoder
    box, kw = torch.zeros((1, 8, 3)), dict(frame_shape=(96, 128))
    full = RefFeatureBank(enc, decoder=dec, match_threshold=0.05, keep_poses=True)
    full._n = 2000                                             # (nothing is encoded without a device: the length alone is looked at)
    with pytest.raises(ValueError, match=r"match_threshold=0\.05"):                                  # a bank without summaries
        PoseStream(model, RefFeatureBank(enc, decoder=dec), [[0, 1, 2]], box, select_k=2, **kw)
    with pytest.raises(ValueError, match=r"match_threshold=0\.05"):
        PoseStream(model, RefFeatureBank(enc, decoder=dec, keep_poses=True), [[0, 1, 2]], box, select_k=2, select="track", **kw)
    no_poses = RefFeatureBank(enc, decoder=dec, match_threshold=0.05)
    no_poses._n = 8
    with pytest.raises(ValueError, match="keep_poses=True"):                                         # "track" over a bank without poses
        PoseStream(model, no_poses, [[0, 1, 2]], box, select_k=2, select="track", **kw)
    with pytest.raises(ValueError, match=r"RefFeatureBank\(encoder, decoder=model\.decoder\)"):      # no entry tokens: as before
        PoseStream(model, RefFeatureBank(enc, match_threshold=0.05, keep_poses=True), [[0, 1, 2]], box, select_k=2, **kw)
    with pytest.raises(ValueError, match="select_k = 3 exceeds the smallest database"):              # k > min(n_refs)
        PoseStream(model, full, [[0, 1, 2, 3], [4, 5]], torch.zeros((2, 8, 3)), select_k=3, select="track", **kw)
    with pytest.raises(ValueError, match="select_k must be a positive integer"):
        PoseStream(model, full, [[0, 1, 2, 3]], box, select_k=0, **kw)
    with pytest.raises(ValueError, match="at most 1024"):                                            # N_max > 1024
        PoseStream(model, full, [list(range(1025))], box, select_k=5, **kw)
    with pytest.raises(ValueError, match="unknown select"):
        PoseStream(model, full, [[0, 1, 2]], box, select_k=2, select="pose", **kw)
    with pytest.raises(ValueError, match="unknown select"):                                          # ... whether or not it selects
        PoseStream(model, full, [[0, 1, 2]], box, select="nearest", **kw)
    with pytest.raises(ValueError, match="not a row of the bank"):
        PoseStream(model, full, [[0, 2000]], box, select_k=1, **kw)
    with pytest.raises(ValueError, match="not a row of the bank"):                                   # -1 is no database entry
        PoseStream(model, full, [[0, -1]], box, select_k=1, **kw)
    with pytest.raises(ValueError, match="max_rms_px is NaN"):
        PoseStream(model, full, [[0, 1]], box, select_k=1, select="track", max_rms_px=NAN, **kw)
    with pytest.raises(ValueError, match=r"bbox_3d must be a tensor of shape \(2, 8, 3\)"):          # ragged databases are taken: B = 2
        PoseStream(model, full, [[0, 1, 2, 3], [4, 5]], box, select_k=2, **kw)
    with pytest.raises(ValueError, match=r"\(B, T_max\)"):                     # without select_k ragged lengths are refused, unchanged
        PoseStream(model, full, [[0, 1], [2]], torch.zeros((2, 8, 3)), **kw)
    # relocalise: one integer or bool flag per tracked object
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.bool), [1], 1):
        with pytest.raises(ValueError, match=r"relocalise must be \(2,\)"):
            stream._relocalise(bad, 2)
    with pytest.raises(ValueError, match="integers or bools"):
        stream._relocalise(torch.zeros(2), 2)
    assert stream._relocalise([1, 0], 2).tolist() == [1, 0] and stream._relocalise(torch.tensor([True, False]), 2).dtype == torch.bool
    assert stream._ref_database([[3, 1, 1], [2, 0]], 4, 2) == ([[3, 1, 1], [2, 0]], [3, 2], 3)


def _prev(B, ok=1.0, rms=0.5):
    prev = np.zeros((B, _lib.STREAM_ROW_FLOATS), np.float32)
    prev[:, 16], prev[:, 17] = rms, ok
    return prev


def test_select_rows_host_appearance_ranking():
    scores = np.array([[0.5, 0.9, 0.9, -INF, 0.1, 0.9],            # equal scores: the lower slots
                       [-INF, 0.3, -INF, -INF, 0.2, 0.7],          # n_refs = 4: -inf slots are picked last, in slot order
                       [0.1, 0.2, 0.3, 0.4, 0.5, 0.6],             # n_refs = k: everything is chosen
                       [NAN, 0.2, NAN, 0.1, -INF, NAN]], np.float32)                # a NaN is never picked
    n_refs = [6, 4, 3, 6]
    used, sel = select_rows_host(scores, None, _prev(4), [0] * 4, n_refs, 3, "dino")
    assert used.tolist() == [0] * 4 and used.dtype == np.int32 and sel.dtype == np.int32
    assert sel.tolist() == [[1, 2, 5], [0, 1, 2], [0, 1, 2], [1, 3, 4]]
    assert select_rows_host(scores, None, _prev(4), [0] * 4, n_refs, 2, "dino")[1].tolist() == [[1, 2], [0, 1], [1, 2], [1, 3]]
    assert select_rows_host(scores, None, _prev(4), [0] * 4, n_refs, 1, _lib.STREAM_SELECT_DINO)[1].tolist() == [[1], [1], [2], [1]]
    # fewer candidates than k: -1 at the end; n_refs is clamped into [0, N_max]
    used, sel = select_rows_host(scores, None, _prev(4), [0] * 4, [2, 0, 9, -3], 4, "dino")
    assert sel.tolist() == [[0, 1, -1, -1], [-1] * 4, [2, 3, 4, 5], [-1] * 4]
    with pytest.raises(ValueError, match="unknown rule"):
        select_rows_host(scores, None, _prev(4), [0] * 4, n_refs, 2, "nearest")


def test_select_rows_host_pose_ranking_and_the_rule():
    # object 0: an exact tie (slots 1, 4), a NaN (slot 2: after every number), +inf an ordinary value (slot 5), and slot 3 no view
    # (its row is outside the store: score -inf, distance +inf) -- never chosen, not even when a NaN is
    dist = np.array([[0.30, 0.10, NAN, INF, 0.10, INF, 0.20]], np.float32)
    scores = np.array([[0.1, 0.2, 0.9, -INF, 0.3, 0.8, 0.7]], np.float32)
    for k, want in ((1, [1]), (2, [1, 4]), (3, [1, 4, 6]), (4, [0, 1, 4, 6]), (5, [0, 1, 4, 5, 6]), (6, [0, 1, 2, 4, 5, 6]),
                    (7, [0, 1, 2, 4, 5, 6, -1])):
        used, sel = select_rows_host(scores, dist, _prev(1), [0], [7], k, "track", 2.0)
        assert used.tolist() == [1] and sel.tolist() == [want], k
    # among NaNs: by position
    d2 = np.array([[NAN, 0.5, NAN, NAN]], np.float32)
    s2 = np.zeros((1, 4), np.float32)
    assert select_rows_host(s2, d2, _prev(1), [0], [4], 3, "track")[1].tolist() == [[0, 1, 2]]
    assert select_rows_host(s2, d2, _prev(1), [0], [4], 2, "track")[1].tolist() == [[0, 1]]
    assert select_rows_host(s2, d2, _prev(1), [0], [3], 3, "track")[1].tolist() == [[0, 1, 2]]          # n_refs == k
    # every way the rule falls back to appearance, against the same arrays: ok = 0, rms > max, rms = NaN, force, rule = DINO
    by_pose, by_look = [1, 4, 6], [2, 5, 6]
    cases = [(_prev(1), [0], "track", 1, by_pose), (_prev(1, rms=2.0), [0], "track", 1, by_pose),   # (rms == max: trusted)
             (_prev(1, ok=0.0), [0], "track", 0, by_look), (_prev(1, rms=2.5), [0], "track", 0, by_look),
             (_prev(1, rms=NAN), [0], "track", 0, by_look), (_prev(1), [1], "track", 0, by_look), (_prev(1), [-7], "track", 0, by_look),
             (_prev(1), [0], "dino", 0, by_look), (_prev(1, ok=0.5), [0], "track", 0, by_look)]
    for prev, force, rule, want_used, want in cases:
        used, sel = select_rows_host(scores, dist, prev, force, [7], 3, rule, 2.0)
        assert used.tolist() == [want_used] and sel.tolist() == [want], (prev[0, 16:18], force, rule)
    # max_rms_px = inf (the default) trusts every solved pose, a NaN rms still none; the rule is per object
    prev = np.concatenate([_prev(1, rms=1e30), _prev(1, rms=NAN), _prev(1, rms=INF)])
    used, sel = select_rows_host(np.tile(scores, (3, 1)), np.tile(dist, (3, 1)), prev, [0, 0, 0], [7, 7, 7], 3, "track")
    assert used.tolist() == [1, 0, 1] and sel.tolist() == [by_pose, by_look, by_pose]
    with pytest.raises(ValueError, match="no distances"):
        select_rows_host(scores, None, _prev(1), [0], [7], 3, "track")


def test_pose_branch_picks_what_pose_select_rows_host_picks():
    B, N, k = 3, 9, 4
    poses, pred = zip(*(spread_poses(N, 60 + b) for b in range(B)))
    bank, pred = torch.cat(poses), torch.stack(pred)
    bank[N + 5] = bank[N + 2]                                      # a tie in object 1
    bank[2 * N + 1, 0, 0] = NAN
    n_refs = [9, 9, 6]
    rows = [[b * N + n for n in range(N)] for b in range(B)]
    rows[0][3] = B * N + 5                                         # a row outside the bank
    cand = [[i if i < n_refs[b] else -1 for i in range(N)] for b in range(B)]
    d64, _, _ = dense.pose_select_rows_host(bank, B * N, pred, rows, cand, N)
    dist = np.asarray(d64, dtype=np.float64).astype(np.float32)
    scores = np.zeros((B, N), np.float32)
    scores[0, 3] = -INF
    for b in range(B):
        scores[b, n_refs[b]:] = -INF
    prev = _prev(B)
    prev[:, :16] = pred.reshape(B, 16).numpy()
    for fk in (1, 2, k, 6):
        _, fine_pos, _ = dense.pose_select_rows_host(bank, B * N, pred, rows, cand, fk)
        used, sel = select_rows_host(scores, dist, prev, [0] * B, n_refs, fk, "track", 1.0)
        assert used.tolist() == [1] * B and sel.tolist() == fine_pos, fk
    assert 3 not in select_rows_host(scores, dist, prev, [0] * B, n_refs, 8, "track")[1][0].tolist()


def test_abi_declares_the_entry_and_it_validates_before_any_launch():
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "boxdreamer_hip.h")).read()
    assert "bd_stream_select_rows" in _lib.EXPORTS and hasattr(lib, "bd_stream_select_rows")
    assert re.search(r"^int bd_stream_select_rows\(", header, re.M)
    assert re.search(r"^#define BD_STREAM_SELECT_DINO 0$", header, re.M) and re.search(r"^#define BD_STREAM_SELECT_TRACK 1$", header, re.M)
    assert (_lib.STREAM_SELECT_DINO, _lib.STREAM_SELECT_TRACK) == (0, 1) and stream.SELECT_RULES == {"dino": 0, "track": 1}
    assert lib.bd_abi_version() == 9                                # the entry is an addition
    p = [0x10000000 * (i + 1) for i in range(15)]                   # made-up addresses: every call below returns before anything is dereferenced
    NULL, SHAPE = -5, -1

    def call(ptrs=p, R=9, B=5, N_max=7, L=16, D=100, k=3, rule=1, max_rms=2.0):
        return lib.bd_stream_select_rows(ptrs[0], ptrs[1], ptrs[2], R, ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], ptrs[8], B, N_max, L, D,
                                         k, rule, max_rms, ptrs[9], ptrs[10], ptrs[11], ptrs[12], ptrs[13], None)

    for kw in (dict(B=0), dict(B=-2), dict(R=-1), dict(N_max=0), dict(N_max=1025, k=5), dict(k=0), dict(k=-1), dict(k=8), dict(L=0),
               dict(D=0), dict(rule=2), dict(rule=-1)):
        assert call(**kw) == SHAPE, kw
    for i in range(14):                                             # poses (2) and dist (10) among them: the rule is TRACK
        assert call(ptrs=[None if j == i else x for j, x in enumerate(p)]) == NULL, i
    assert call(ptrs=[None] * 15, k=0) == NULL                      # NULL is reported first
    no_poses = [None if j in (2, 10) else x for j, x in enumerate(p)]
    assert call(ptrs=no_poses, rule=1) == NULL                      # poses may be NULL only with rule == DINO ...
    assert call(ptrs=no_poses, rule=0, k=8) == SHAPE                # ... where the call goes on to the shape checks
    assert call(ptrs=[None if j == 10 else x for j, x in enumerate(p)], rule=0) == NULL        # poses given: dist is written
