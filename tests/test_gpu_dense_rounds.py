"""GPU: the dense multi-round decode over a reference bank that keeps poses -- bd_round_sources and bd_pose_select_rows
(csrc/rounds.hip) against their CPU restatements (dense.round_sources_host / dense.pose_select_rows_host), the fine level's choice
through the facade on poses whose nearest two are known, and the banked multi-round forward BIT-identical to the un-banked one
(dense.process_multi_round) on the same crops: feature bank, entry-token bank with and without bbox_feat, round by round or at once,
coarse and fine, uniform and ragged.  Seeds: the batch is synth.make_batch(seed=13) (tests/test_gpu_facade.py's dense recipe), the model's are 4321 / 1234, the poses come
from _posed() below (seed 31)."""
import math

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, cache as cache_mod, dense, hip_ops, operand, synth
from boxdreamer_amd.betr import BETR
from boxdreamer_amd.cache import RefFeatureBank
from boxdreamer_amd.model import BoxDreamer
from test_dense_rounds_host import spread_poses
from test_gpu_facade import STRICT_DEFAULT, _config_with
from test_gpu_pnp_ransac import R_ROUNDS, SUB, _multi_round_batch
from test_gpu_pnp_wave import _config

pytestmark = pytest.mark.gpu

NO_VIEW = 0x7FFFFFFF
B, N_MAX = 3, 9
BANK = 40                                    # bank views in use; rows 30 .. 39 belong to nobody


def _i32(x):
    return torch.tensor(x, dtype=torch.int32).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- bd_round_sources

ROWS = [[3, 7, 0, 19, 11, 5, 8, 2, 14], [6, 1, 5, 17, 29, 28, 27, 26, 25], [9, 4, 13, 10, 16, 12, 99, -1, 21]]


def _cand(k):
    cand = [list(range(1, 1 + k)), list(range(9 - k, 9)), [0, 2, 4, 5, 8][:k] if k <= 5 else list(range(k))]
    cand[1][0] = -1                          # no candidate
    cand[0][k - 1] = N_MAX                   # a candidate past N_max
    if k >= 3:
        cand[2][1], cand[2][2] = 6, 7        # rows outside the bank: 99 and -1
    return cand


@pytest.mark.parametrize("per_round", [0, 1])
@pytest.mark.parametrize("k,sub", [(5, 2), (4, 2), (3, 5)])
def test_round_sources_against_the_cpu_form(hip, k, sub, per_round):
    lib = _lib.load()
    cand, zero = _cand(k), 33
    want_src, want_view = dense.round_sources_host(ROWS, cand, BANK, sub, zero, per_round)
    n = B * (-(-k // sub)) * (sub + 1)
    assert len(want_src) == n and NO_VIEW in want_src and (zero in want_src) == (k % sub != 0)
    src = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    view = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rows, cd = _i32(ROWS), _i32(cand)
    _lib.check(lib.bd_round_sources(_lib.ptr(rows), _lib.ptr(cd), BANK, B, N_MAX, k, sub, zero, per_round, _lib.ptr(src[8:n + 8]),
                                    _lib.ptr(view[8:n + 8]), _lib.stream()), "bd_round_sources")
    torch.cuda.synchronize()
    assert src[8:n + 8].tolist() == want_src and view[8:n + 8].tolist() == want_view
    for t in (src, view):                    # guard bands
        assert (t[:8] == 0x5A5A5A5A).all() and (t[n + 8:] == 0x5A5A5A5A).all()
    got = hip_ops.round_sources(rows, cd, BANK, sub, zero, per_round)
    assert got[0].tolist() == want_src and got[1].tolist() == want_view


# ------------------------------------------------------------------------------------------------------------- bd_pose_select_rows

K_POSE = 6
_POSES = {}


def _pose_case():
    """Bank poses [BANK, 4, 4], coarse poses [B, 4, 4], rows, cand (B, 6) -- built on the CPU.  Sample 0: positions 1 and 3 hold the
    SAME pose (an exact tie).  Sample 1: an all-zero coarse pose (a failed RANSAC).  Sample 2: one NaN pose and one invalid candidate."""
    if not _POSES:
        bank = torch.zeros(BANK, 4, 4)
        pred = torch.zeros(B, 4, 4)
        rows = [[b * N_MAX + n for n in range(N_MAX)] for b in range(B)]
        for b in range(B):
            p, base = spread_poses(N_MAX, 60 + b)
            bank[b * N_MAX:(b + 1) * N_MAX] = p
            pred[b] = base
        pred[1] = 0.0
        cand = [[0, 1, 3, 4, 6, 8], [1, 2, 3, 5, 7, 8], [0, 2, 3, 5, 6, 7]]
        bank[rows[0][4]] = bank[rows[0][1]]                   # sample 0: cand positions 1 and 3
        bank[rows[2][3], 1, 1] = float("nan")                 # sample 2: position 2
        rows[2][6] = BANK + 5                                 # sample 2: position 4 names a row outside the bank
        _POSES.update(bank=bank, pred=pred, rows=rows, cand=cand)
    return _POSES


@pytest.mark.parametrize("fk", [1, 2, 6])
def test_pose_select_rows_against_the_fp64_form(hip, fk):
    lib = _lib.load()
    c = _pose_case()
    bank, pred, rows, cand = c["bank"], c["pred"], c["rows"], c["cand"]
    ref, want_pos, want_src = dense.pose_select_rows_host(bank, BANK, pred, rows, cand, fk)
    # before any launch: apart from the deliberate tie, NaN and invalid entries the sorted distances are >= 1e-3 apart
    for b in range(B):
        d = sorted(x for x in ref[b] if math.isfinite(x))
        gaps = [y - x for x, y in zip(d, d[1:]) if not (b == 0 and y == x)]
        assert min(gaps) >= 1e-3, (b, d)
    assert ref[0][1] == ref[0][3] and math.isnan(ref[2][2]) and ref[2][4] == math.inf and sum(math.isfinite(x) for x in ref[2]) == 4
    n = B * K_POSE
    dist = torch.full((n + 16,), float("nan"), device="cuda")
    dist.view(torch.int32)[:] = 0x7FC01234
    pos = torch.full((B * fk + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    src = torch.full((B * (fk + 1) + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bank_d, pred_d, rows_d, cand_d = bank.cuda(), pred.cuda(), _i32(rows), _i32(cand)

    def launch(nb, first, d, p, s):
        _lib.check(lib.bd_pose_select_rows(_lib.ptr(bank_d), BANK, _lib.ptr(pred_d[first:first + nb]), _lib.ptr(rows_d[first:first + nb]),
                                           _lib.ptr(cand_d[first:first + nb]), nb, N_MAX, K_POSE, fk, _lib.ptr(d), _lib.ptr(p), _lib.ptr(s),
                                           _lib.stream()), "bd_pose_select_rows")
        torch.cuda.synchronize()

    launch(B, 0, dist[8:n + 8], pos[8:B * fk + 8], src[8:B * (fk + 1) + 8])
    assert (dist.view(torch.int32)[:8] == 0x7FC01234).all() and (dist.view(torch.int32)[n + 8:] == 0x7FC01234).all()
    assert (pos[:8] == 0x5A5A5A5A).all() and (pos[B * fk + 8:] == 0x5A5A5A5A).all()
    assert (src[:8] == 0x5A5A5A5A).all() and (src[B * (fk + 1) + 8:] == 0x5A5A5A5A).all()
    got = dist[8:n + 8].reshape(B, K_POSE).double().cpu()
    want = torch.tensor(ref, dtype=torch.float64)
    finite = torch.isfinite(want)
    err = (got - want).abs()[finite]
    bound = 1e-7 + 2.0 ** -22 * want[finite].abs()
    print(f"[dense_rounds] fk={fk}: max |dist - fp64| {err.max().item():.3g} (bound {bound.min().item():.3g} ..)")
    assert (err <= bound).all()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got == math.inf, want == math.inf)
    assert pos[8:B * fk + 8].reshape(B, fk).tolist() == want_pos and src[8:B * (fk + 1) + 8].tolist() == want_src
    if fk == 2:
        assert 3 not in want_pos[0] or 1 in want_pos[0]      # the tie: position 3 never without position 1
    if fk == 6:
        assert want_pos[2] == [0, 1, 2, 3, 5, -1] and want_src[2 * 7 + 5] == NO_VIEW
    # a sample alone: the same bits as inside the batch (its query entry names fresh view 0 then)
    for b in range(B):
        d1 = torch.empty(K_POSE, device="cuda")
        p1 = torch.empty(fk, dtype=torch.int32, device="cuda")
        s1 = torch.empty(fk + 1, dtype=torch.int32, device="cuda")
        launch(1, b, d1, p1, s1)
        assert torch.equal(_bits(d1), _bits(dist[8 + b * K_POSE:8 + (b + 1) * K_POSE])), b
        assert torch.equal(p1, pos[8 + b * fk:8 + (b + 1) * fk]) and s1[fk].item() == -1
        assert torch.equal(s1[:fk], src[8 + b * (fk + 1):8 + b * (fk + 1) + fk])
    out = hip_ops.pose_select_rows(bank_d, BANK, pred_d, rows_d, cand_d, fk)
    assert torch.equal(_bits(out[0].reshape(-1)), _bits(dist[8:n + 8])) and out[1].tolist() == want_pos and out[2].tolist() == want_src


# ------------------------------------------------------------------------------------------------- the facade: a known selection

def _dev(data, **more):
    return dict({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}, **more)


def _fill(bank, data, counts=None, entry=False):
    """Every sample's references into the bank, with their poses -> the ref_rows table (junk in the padded slots)."""
    table = []
    for b, q in enumerate(data["query_idx"].tolist()):
        c = counts[b] if counts is not None else data["images"].shape[1]
        slots = [t for t in range(c) if t != q]
        kw = {"bbox_feat": data["bbox_feat"][b, slots].cuda()} if entry else {}
        ids = bank.add(data["images"][b, slots].cuda(), poses=data["poses"][b, slots].double(), **kw).tolist()
        row = [10 ** 6] * data["images"].shape[1]
        row[q] = -1
        for t, r in zip(slots, ids):
            row[t] = r
        table.append(row)
    return table


def test_facade_fine_level_picks_the_known_nearest_references(hip):
    """tests/test_gpu_pnp_ransac.py's posed batch (references = the true pose turned by 0.2 rad x a per-sample permutation) over a
    bank: a BETR whose forward / forward_entry emit heat maps peaked at the true projections (rounds 0 and 1; random pixels in round
    2) -- dense_fine_slots are the two nearest references, with the device RANSAC and with the host's, feature bank and entry bank."""
    from boxdreamer_amd.bbox_features import make_bbox_features
    nb = 3
    data, proj, gt, nearest = _multi_round_batch(nb)
    T = data["images"].shape[1]
    data["images"] = (data["images"].float() * 0.25 + 0.5).clamp(0, 1)
    rng = np.random.default_rng(23)
    rounds = proj[:, None].repeat(1, R_ROUNDS, 1, 1).clone()
    rounds[:, 2] = torch.from_numpy(rng.uniform(30, 194, (nb, 8, 2))).float()
    heat_true = make_bbox_features(proj.cuda(), "heatmap", (224, 224), group=1).float()
    heat_rounds = make_bbox_features(rounds.reshape(nb * R_ROUNDS, 8, 2).cuda(), "heatmap", (224, 224), group=1).float()

    class Peaked(BETR):
        def forward(self, pose_feat, *a, **k):
            self.mask_error = None
            return heat_rounds if pose_feat.shape[0] == nb * R_ROUNDS else heat_true

        def forward_entry(self, entry_rows, n_rows, src, query_feat, masks, *a, **k):
            self.mask_error = None
            return heat_rounds if masks.shape[0] == nb * R_ROUNDS else heat_true

    cfg = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": T - 1, "multi_round": True, "sub_batch_size": SUB,
           "dense_mem_friendly": False, "fine_level": True, "fine_topk": 2}
    model = BoxDreamer(_config(depth=1, pnp_on_device="wave", dense_cfg=cfg)).cuda().eval()
    model(_dev({k: v[:1] for k, v in data.items()}))                  # (the load-time calibration, once, with the real decoder)
    banks = {}
    for entry in (False, True):
        bank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True, decoder=model.decoder if entry else None)
        banks[entry] = (bank, _fill(bank, data, entry=entry))
    real = model.decoder.__class__
    model.decoder.__class__ = Peaked
    try:
        for solver in ("wave", False):
            model.pnp_on_device = solver
            for entry, (bank, table) in banks.items():
                out = model(_dev(data, ref_bank=bank, ref_rows=table))
                assert ("bd_solve_pnp_ransac_wave" in out["dense_pose_solver"]) == (solver == "wave")
                assert out["dense_fine_slots"].tolist() == nearest.tolist(), (solver, entry)
                assert out["dense_fine_dist"].shape == (nb, T - 1) and out["images"].shape[1] == 3
                d = out["dense_fine_dist"].cpu()
                for b in range(nb):                                   # 0.2 rad apart by construction (the coarse pose is within 0.03)
                    s = d[b].sort().values
                    assert abs(s[0] - 0.2) < 0.1 and abs(s[1] - 0.4) < 0.1 and s[2] > 0.5, (b, s)
                    assert torch.equal(out["poses"][b, :2].cpu(), data["poses"][b, nearest[b]])
                assert out["hip_precision"]["ref_bank"]["rounds"] == R_ROUNDS and out["hip_precision"]["ref_bank"]["padded_views"] == 0
    finally:
        model.decoder.__class__ = real


# ---------------------------------------------------------------------------- the facade: bit-identity with the real decoder

K, SUB_B, FK = 5, 2, 2
CFG = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": K, "multi_round": True, "sub_batch_size": SUB_B,
       "dense_mem_friendly": False, "fine_level": False, "fine_topk": FK, "ransac_trials": 200}
COARSE = ("pred_poses", "regression_boxes", "dense_pose_inliers")
FINE = ("pred_poses", "regression_boxes", "pred_corners_px", "poses", "intrinsics", "bbox_3d", "query_idx", "camera_mask")


def _posed(data):
    """Per-view poses that tell the views apart: a rotation by 0.15 (t + 1) + 0.05 b about an axis of its own, translations whose
    lengths differ by ~0.1 between views (so that even a failed, all-zero coarse pose ranks them with a wide margin)."""
    rng = np.random.default_rng(31)
    nb, T = data["images"].shape[:2]
    for b in range(nb):
        for t in range(T):
            a = rng.normal(size=3)
            data["poses"][b, t] = torch.eye(4)
            data["poses"][b, t, :3, 3] = torch.tensor([0.1 * t, -0.07 * t + 0.03 * b, 1 + 0.11 * t])
            data["poses"][b, t, :3, :3] = torch.from_numpy(_rotation(a, 0.15 * (t + 1) + 0.05 * b)).float()
    return data


def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def _assert_fine_margin(coarse_out, fk, where):
    """In fp64 on the CPU: the fk-th and (fk + 1)-th nearest kept references to the coarse pose are >= 1e-3 apart -- the un-banked
    fine level ranks fp32 torch distances, the banked one fp64 distances rounded once, and only a near tie could tell them apart."""
    k = coarse_out["poses"].shape[1] - 1
    for b in range(coarse_out["poses"].shape[0]):
        pred = coarse_out["pred_poses"][b, k].float().cpu()
        d = sorted(dense.pose_distance_host(pred, coarse_out["poses"][b, t].float().cpu()) for t in range(k))
        assert d[fk] - d[fk - 1] >= 1e-3, f"{where}: sample {b}: near tie {d} between the fine level's candidates -- change the poses' seed in _posed()"


def _query_slot(out):
    if "pred_bbox" not in out:
        return out["pred_query_bbox"].float()
    k = out["pred_bbox"].shape[1] - 1
    return out["pred_bbox"][:, k].float()


def _model_and_batch(nb, T, seed=13):
    """Reduced depth (1 DINO block, 1 BETR block, synthetic seeds), default precision mode; tests/test_gpu_facade.py's dense batch:
    crops in [0, 1] with a black border of a different width per view, so that the views' foreground counts differ."""
    cfg = _config_with(STRICT_DEFAULT, depth=1)
    cfg["modules"]["dense_cfg"] = dict(CFG)
    model = BoxDreamer(cfg)
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(1234, 1).items()}, strict=True)
    model = model.cuda().eval()
    data = synth.make_batch(seed=seed, B=nb, T=T)
    img = (data["images"].float() * 0.25 + 0.5).clamp(0, 1)
    for b in range(nb):
        for t in range(T):
            w = 14 * ((3 * b + 2 * t) % 5)
            m = torch.zeros(224, 224)
            m[w:224 - w, w:224 - w] = 1
            img[b, t] *= m
    data["images"] = img
    return model, data


_SHARED = {}


def _shared():
    if not _SHARED:
        model, data = _model_and_batch(2, 7)
        data["query_idx"] = torch.tensor([6, 1])
        data = _posed(data)
        model.pnp_on_device = "wave"
        model(_dev({k: v[:1] for k, v in data.items()}))              # (the load-time calibration, once)
        fbank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True)
        ebank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True, decoder=model.decoder)
        _SHARED.update(model=model, data=data, fbank=fbank, ftable=_fill(fbank, data), ebank=ebank, etable=_fill(ebank, data, entry=True))
    return _SHARED


def _no_bbox(data):
    return {k: v for k, v in data.items() if k != "bbox_feat"}


def _banked_variants(sh, data, **more):
    yield "feature bank", _dev(data, ref_bank=sh["fbank"], ref_rows=sh["ftable"], **more)
    yield "entry bank", _dev(data, ref_bank=sh["ebank"], ref_rows=sh["etable"], **more)
    yield "entry bank, no bbox_feat", _dev(_no_bbox(data), ref_bank=sh["ebank"], ref_rows=sh["etable"], **more)


@pytest.mark.parametrize("friendly", [False, True])
def test_banked_multi_round_coarse_bit_identical(hip, friendly):
    """B = 2, N = 6, filter_topk 5, sub_batch_size 2: R = 3 rounds, the last padded with the bank's zero view."""
    sh = _shared()
    model, data = sh["model"], sh["data"]
    model.dense_cfg = dict(CFG, dense_mem_friendly=friendly)
    want = model(_dev(data))
    assert "dense_ref_slots" not in want and want["pred_bbox"].shape[1] == K + 1
    feats = model.rgb_encoder.predict(data["images"].cuda())
    slots = dense.match_views(feats, data["images"].cuda(), data["query_idx"], K)[1].nonzero()[:, 1].reshape(2, K)
    recasts = model.decoder.recast_count
    for where, batch in _banked_variants(sh, data):
        out = model(batch)
        assert out is batch
        for key in COARSE:
            assert out[key].dtype == want[key].dtype and torch.equal(out[key], want[key]), (where, key)
        assert torch.equal(_query_slot(out), _query_slot(want)), where
        assert ("pred_bbox" in out) == ("bbox_feat" in batch)
        if "pred_bbox" in out:
            assert torch.equal(out["pred_bbox"], want["pred_bbox"]), where
        assert torch.equal(out["dense_ref_slots"].long(), slots), where
        assert torch.equal(out["pred_intrinsics"], want["pred_intrinsics"]) and torch.equal(out["poses"], want["poses"])
        rec = out["hip_precision"]["ref_bank"]
        assert (rec["rounds"], rec["padded_views"], rec["banked_views"], rec["encoded_views"]) == (3, 2, 2 * K, 2), rec
        assert model.host_syncs_per_forward == [], (where, model.host_syncs_per_forward)     # "wave": nothing waits for the device
    assert model.decoder.recast_count == recasts
    for bank in (sh["fbank"], sh["ebank"]):
        z = bank.zero_row
        assert len(bank) == 2 * 6 + 1 and z == 12 and not bank.poses_of(z).any() and bank.poses_of(3).any()
        assert not bank._msums[z].any() and bank._mcounts[z].item() == 0
        assert all(not p[z * bank.tokens_per_view:(z + 1) * bank.tokens_per_view].any()
                   for p in operand.row_planes(bank._t16, bank.operand_class, (z + 1) * bank.tokens_per_view))
        assert torch.equal(bank.poses_of(4).cpu(), data["poses"][0, 4])
    # the host RANSAC runs over the same corners
    model.pnp_on_device = False
    try:
        want_h = model(_dev(data))
        out_h = model(_dev(data, ref_bank=sh["fbank"], ref_rows=sh["ftable"]))
        for key in COARSE:
            assert torch.equal(out_h[key], want_h[key]), ("host RANSAC", key)
    finally:
        model.pnp_on_device = "wave"


@pytest.mark.parametrize("friendly", [False, True])
def test_banked_multi_round_fine_bit_identical(hip, friendly):
    sh = _shared()
    model, data = sh["model"], sh["data"]
    model.dense_cfg = dict(CFG, dense_mem_friendly=friendly)
    _assert_fine_margin(model(_dev(data)), FK, "fine level")
    model.dense_cfg = dict(CFG, dense_mem_friendly=friendly, fine_level=True)
    org = [[(t, b) for b in range(2)] for t in range(7)]
    want = model(_dev(data))
    logits = model.decoder.last_logits.clone()
    assert want["images"].shape[1] == FK + 1
    for where, batch in _banked_variants(sh, data, original_images=org):
        out = model(batch)
        assert torch.equal(model.decoder.last_logits, logits), where
        for key in FINE:
            assert out[key].dtype == want[key].dtype and torch.equal(out[key], want[key]), (where, key)
        assert torch.equal(_query_slot(out), _query_slot(want)), where
        fine = out["dense_fine_slots"].tolist()                        # both selections composed, the query last
        assert out["original_images"] == [[(s[j] + (s[j] >= q), b) for b, (s, q) in enumerate(zip(fine, data["query_idx"].tolist()))]
                                          for j in range(FK)] + [[(q, b) for b, q in enumerate(data["query_idx"].tolist())]], where
        assert out["dense_fine_slots"].shape == (2, FK) and out["dense_fine_dist"].shape == (2, K)
        for b, q in enumerate(data["query_idx"].tolist()):           # original reference slots, ascending: the views the dict now holds
            views = [s + (s >= q) for s in out["dense_fine_slots"][b].tolist()]
            assert views == sorted(views) and torch.equal(out["poses"][b, :FK].cpu(), data["poses"][b, views])
        syncs = model.host_syncs_per_forward
        # "wave": the mask verdict's 4 bytes and the slots original_images is re-packed from, as in the single-round banked mode
        assert len(syncs) <= 2 and all("mask verdict" in s or "original_images" in s for s in syncs), syncs


def test_ragged_banked_multi_round_equals_each_sample_alone(hip):
    """Databases of 4 and 6 views through view_counts (filter_topk 3, sub_batch_size 2: one padded view), fine level on: every
    sample equals that sample run alone, un-banked, at its own T."""
    sh = _shared()
    model = sh["model"]
    data = {k: v.clone() for k, v in sh["data"].items()}
    data["query_idx"] = torch.tensor([2, 1])
    counts = [5, 7]
    cfg = dict(CFG, filter_topk=3, fine_level=True)
    ragged = {k: v.clone() for k, v in data.items()}
    for key in ("images", "bbox_feat", "poses"):
        ragged[key][0, counts[0]:] = float("nan")                     # padded slots are never read
    for entry in (False, True):
        bank = RefFeatureBank(model.rgb_encoder, keep_images=False, match_threshold=0.05, keep_poses=True,
                              decoder=model.decoder if entry else None)
        table = _fill(bank, data, counts, entry=entry)
        model.dense_cfg = cfg
        out = model(_dev(ragged, ref_bank=bank, ref_rows=table, view_counts=counts))
        got = {k: out[k].clone() for k in FINE}
        got_logits, got_box = model.decoder.last_logits.clone(), _query_slot(out).clone()
        assert out["hip_precision"]["ref_bank"]["padded_views"] == 2 and out["images"].shape[1] == FK + 1
        for b, c in enumerate(counts):
            alone = {k: v[b:b + 1, :c].contiguous() if v.dim() > 1 else v[b:b + 1] for k, v in data.items()}
            model.dense_cfg = dict(cfg, fine_level=False)
            _assert_fine_margin(model(_dev(alone)), FK, "ragged")
            model.dense_cfg = cfg
            one = model(_dev(alone))
            assert torch.equal(model.decoder.last_logits, got_logits[b:b + 1]), (entry, b)
            assert torch.equal(_query_slot(one), got_box[b:b + 1]), (entry, b)
            for key in FINE:
                assert torch.equal(got[key][b:b + 1], one[key]), (entry, b, key)


def test_zero_row_survives_a_refresh_in_place(hip):
    """A refresh re-encodes the crops and leaves the zero view zero (a zero IMAGE would not encode to zero features), at its row, and
    the poses alone; clear() drops both."""
    sh = _shared()
    model, data = sh["model"], sh["data"]
    bank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True, decoder=model.decoder)
    _fill(bank, {k: v[:1] for k, v in data.items()}, entry=True)
    z = bank.zero_row
    assert z == 6 and bank.zero_row == z and len(bank) == 7           # made once
    bank.add(data["images"][1, :2].cuda(), bbox_feat=data["bbox_feat"][1, :2].cuda(), poses=data["poses"][1, :2])
    before_x, before_p = bank.entry_tokens[:len(bank)].clone(), bank.poses[:len(bank)].clone()
    bank._stamp = ("stale",) + tuple(bank._stamp[1:])
    cache_mod._WARNED_STALE_BANK = True
    assert bank.ensure_fresh() is True and bank.zero_row == z and len(bank) == 9
    assert torch.equal(_bits(bank.entry_tokens[:9]), _bits(before_x)) and torch.equal(bank.poses[:9], before_p)
    P = bank.tokens_per_view
    assert all(not p[z * P:(z + 1) * P].any() for p in operand.row_planes(bank._t16, bank.operand_class, 9 * P))
    assert not bank._msums[z].any() and bank._msums[z + 1].any()
    bank.clear()
    assert bank.poses is None and len(bank) == 0
    with pytest.raises(ValueError, match="empty reference bank"):
        bank.zero_row
