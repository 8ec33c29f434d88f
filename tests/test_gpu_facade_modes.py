"""GPU: what a forward through each of the facade's modes leaves behind -- the exact key set of the returned dict and of
data["hip_precision"], the length of host_syncs_per_forward and pose_solver -- for the captured graph, the eager step, the entry bank
and the banked dense mode's three forms (gathered features, entry tokens, multi-round with and without its fine level), under both
pose solvers.  The values are pinned mode against mode, bit for bit, by the suites of the modes themselves; this one pins the contract
around them.  One small model (2 DINO blocks, 2 BETR blocks), B = 2, T_max = 3, k = 2, calibrated once."""
import pytest
import torch

from boxdreamer_amd import pnp
from boxdreamer_amd.cache import RefFeatureBank
from test_gpu_dense_rounds import _dev, _fill, _posed
from test_gpu_facade import _dense_model_and_batch

pytestmark = pytest.mark.gpu

B, T, K = 2, 3, 2
SINGLE = {"enable": True, "filter": "dino", "filter_enable": True, "filter_topk": K, "multi_round": False}
ROUNDS = dict(SINGLE, multi_round=True, sub_batch_size=1, dense_mem_friendly=False, fine_level=False, fine_topk=1, ransac_trials=50)
PRECISION = {"decoder", "encoder", "source", "calibrated", "promoted_units", "self_check_max_abs_dlogits", "self_check_unpromoted",
             "self_check_budget", "self_check_ok", "sub_batch_lanes"}
OUTPUTS = {"camera_mask", "hip_precision", "pred_bbox", "regression_boxes", "pred_corners_px", "pose_solver", "pred_poses", "pred_intrinsics"}
SELECTION = {"dense_ref_slots", "dense_ref_scores"}
ROUND_POSE = {"dense_pose_solver", "dense_pose_inliers", "dense_pose_rms_px"}
SOLVER = {False: "host:cv2.solvePnP" if pnp._HAVE_CV2 else "host:bd_solve_pnp_host (native threads, DLT + LM; parity vs OpenCV un-pinned)",
          "wave": "hip:bd_solve_pnp_wave (one wavefront per pose, DLT + LM; parity vs OpenCV un-pinned)"}
# mode: (hip_graph, dense_cfg, bank, keys the forward adds to the batch's, what data["hip_precision"] gains, the whole tail runs)
CASES = {
    "graph": (True, None, None, OUTPUTS, set(), True),
    "eager": (False, None, None, OUTPUTS, set(), True),
    "entry_bank": (False, None, "ebank", OUTPUTS, {"ref_bank"}, True),
    "banked_dense": (False, SINGLE, "fbank", OUTPUTS | SELECTION, {"ref_bank"}, True),
    "banked_dense_entry": (False, SINGLE, "ebank", OUTPUTS | SELECTION, {"ref_bank"}, True),
    "banked_dense_rounds_fine": (False, dict(ROUNDS, fine_level=True), "fbank",
                                 OUTPUTS | SELECTION | ROUND_POSE | {"dense_fine_dist", "dense_fine_slots"}, {"ref_bank"}, True),
    "banked_dense_rounds_coarse": (False, ROUNDS, "fbank", (OUTPUTS - {"pred_corners_px", "pose_solver"}) | SELECTION | ROUND_POSE,
                                   {"ref_bank"}, False),
}
_SHARED = {}


def _shared():
    if not _SHARED:
        model, data = _dense_model_and_batch(None, B=B, T=T)
        data = _posed(data)
        model(_dev(data))                                               # (the load-time calibration, once)
        fbank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True)
        ebank = RefFeatureBank(model.rgb_encoder, match_threshold=0.05, keep_poses=True, decoder=model.decoder)
        _SHARED.update(model=model, data=data, fbank=(fbank, _fill(fbank, data)), ebank=(ebank, _fill(ebank, data, entry=True)))
    return _SHARED


@pytest.mark.parametrize("solver", [False, "wave"], ids=["host_pnp", "wave_pnp"])
@pytest.mark.parametrize("mode", list(CASES))
def test_what_a_forward_of_each_mode_leaves_behind(hip, mode, solver):
    sh = _shared()
    model = sh["model"]
    graph, dense_cfg, bank, added, record, tail = CASES[mode]
    batch = _dev(sh["data"]) if bank is None else _dev(sh["data"], ref_bank=sh[bank][0], ref_rows=sh[bank][1])
    given = set(batch)
    model.hip_graph, model.dense_cfg, model.pnp_on_device = graph, dense_cfg, solver
    try:
        out = model(batch)
        assert (model._graph is not None) == graph
        assert out is batch and set(out) == given | added | ({"pred_pose_rms_px"} if tail and solver == "wave" else set())
        assert set(out["hip_precision"]) == PRECISION | record
        assert out.get("pose_solver") == (SOLVER[solver] if tail else None)
        # host PnP: the ONE D2H of corners, box, K and verdict.  "wave": the 4 bytes of the decoder's deferred mask verdict, which the
        # captured graph does not have (query_idx indexes one view per sample by construction).  The coarse return reads nothing back.
        want_syncs = 0 if not tail or (graph and solver == "wave") else 1
        assert len(model.host_syncs_per_forward) == want_syncs, model.host_syncs_per_forward
        if want_syncs:
            assert ("ONE D2H" if solver is False else "mask verdict") in model.host_syncs_per_forward[0]
    finally:
        model.hip_graph, model.dense_cfg, model.pnp_on_device = False, None, False
        model._graph = None
