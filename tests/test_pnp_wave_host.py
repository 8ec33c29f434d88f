"""Host side of the wave form of the device PnP (bd_solve_pnp_wave, one wavefront per pose): the export, its argument checks (which
return before any launch) and the Python keywords that select it.  Nothing here needs a GPU."""
import copy
import ctypes as C
import json
import os

import pytest

from boxdreamer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BD_ERR_SHAPE, BD_ERR_NULL = -1, -5


def test_export_header_and_abi():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "boxdreamer_hip.h")).read()
    assert "bd_solve_pnp_wave" in _lib.EXPORTS and hasattr(lib, "bd_solve_pnp_wave") and "int bd_solve_pnp_wave(" in hdr
    assert "box_utils.py:139-199" in hdr[hdr.index("ONE WAVEFRONT per pose"):hdr.index("int bd_solve_pnp_wave(")]
    assert lib.bd_abi_version() == 9


def test_argument_checks_return_before_a_launch():
    """Same contract as bd_solve_pnp: a null pointer -> BD_ERR_NULL, a bad count -> BD_ERR_SHAPE, both before anything touches a device
    (the non-null pointers below are host buffers that no kernel may ever see)."""
    lib = _lib.load()
    kp, p3, K = (C.c_float * 128)(), (C.c_float * 192)(), (C.c_float * 9)()
    poses, rms = (C.c_float * 16)(), (C.c_float * 1)()
    a = lambda x: C.cast(x, C.c_void_p)
    good = [a(kp), a(p3), a(K), 1, 8, 30, a(poses), a(rms), None]
    for i in (0, 1, 2, 6):
        args = list(good)
        args[i] = None
        assert lib.bd_solve_pnp_wave(*args) == BD_ERR_NULL, i
    for field, value in ((4, 5), (4, 65), (3, 0), (5, -1)):
        args = list(good)
        args[field] = value
        assert lib.bd_solve_pnp_wave(*args) == BD_ERR_SHAPE, (field, value)
        args[7] = None                                            # rms_px may be NULL: still the shape error, not a null error
        assert lib.bd_solve_pnp_wave(*args) == BD_ERR_SHAPE, (field, value)


def test_solve_poses_device_keywords_raise_before_the_gpu():
    import torch
    from boxdreamer_amd.box_utils import solve_poses_device
    kp, p3, K = torch.zeros(1, 8, 2), torch.zeros(1, 8, 3), torch.eye(3)[None]
    with pytest.raises(ValueError, match="form"):
        solve_poses_device(kp, p3, K, form="warp")
    with pytest.raises(ValueError, match="want_rms"):
        solve_poses_device(kp, p3, K, form="thread", want_rms=True)
    with pytest.raises(ValueError, match="want_rms"):
        solve_poses_device(kp, p3, K, want_rms=True)            # "thread" stays the default form


def test_model_rejects_an_unknown_device_solver():
    from boxdreamer_amd.model import BoxDreamer
    mods = copy.deepcopy(json.load(open(os.path.join(ROOT, "tests", "golden", "model_modules_config.json")))["modules"])
    mods["decoder"].update(num_decoder_layers=1, hip_precision="bf16")
    mods["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=1, hip_precision="bf16")
    mods["pnp_on_device"] = "warp"
    with pytest.raises(ValueError, match="pnp_on_device"):
        BoxDreamer({"modules": mods})
    mods["pnp_on_device"] = "wave"
    assert BoxDreamer({"modules": mods}).pnp_on_device == "wave"
