"""CPU: camera-native frame formats (bgr, rgba / bgra, nv12) of boxdreamer_amd.preprocess -- the definition of the conversion and
everything about it that needs no device.

`preprocess.frames_to_rgb` is the definition: byte permutations for the packed formats, and for NV12 the int32 rule of
include/boxdreamer_hip.h (bd_crop_resize_frames_fmt) with nearest chroma.  The C entry `bd_frames_to_rgb_host` runs the per-pixel text
the kernel's stage runs (csrc/pixel_format.h) and must equal the mirror bit for bit; tests/test_gpu_frame_formats.py holds the kernel to
the same mirror.

Round-trip bound (RGB -> fp64 forward matrix -> rounded bytes -> the integer decode): each of Y, U, V is off by at most 0.5 after
rounding, so channel c is off by at most 0.5 (cy + sum |chroma gains of c|) before the decode's own rounding to nearest, which adds
at most 0.5 more; errors are integers: floor(0.5 (cy + sum |gains|) + 0.5), the gains as real numbers.  That is (1, 1, 2) for limited
range and (1, 1, 1) for full range.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib
from boxdreamer_amd import preprocess as pp
from test_preprocess import _host_facade
from test_stream_host import _host_model

TABLES = {("bt601", "limited"): (76309, 104597, 25675, 53279, 132201, 16), ("bt601", "full"): (65536, 91881, 22553, 46802, 116130, 0),
          ("bt709", "limited"): (76309, 117489, 13975, 34925, 138438, 16), ("bt709", "full"): (65536, 103206, 12276, 30679, 121609, 0)}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
NV12_TABLES = sorted(TABLES)


def _real_gains(colorspace, rng):
    kr, kb = KR_KB[colorspace]
    kg = 1.0 - kr - kb
    s = 255.0 / 224.0 if rng == "limited" else 1.0
    return (255.0 / 219.0 if rng == "limited" else 1.0, 2 * (1 - kr) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s, 2 * (1 - kb) * s)


def _nv12(Y, U, V):
    """One NV12 frame from a luma plane (H, W) and chroma planes (H / 2, W / 2)."""
    H, W = Y.shape
    uv = np.stack([U, V], -1).reshape(H // 2, W)
    return np.concatenate([Y, uv], 0).astype(np.uint8)[None]


def test_coefficient_tables_are_the_constants_and_the_formula():
    for (cs, rg), want in TABLES.items():
        assert pp.yuv_coefficients(cs, rg) == want
        assert tuple(int(math.floor(g * 65536 + 0.5)) for g in _real_gains(cs, rg)) == want[:5]
        assert want[5] == (16 if rg == "limited" else 0)
        assert pp.resolve_format("nv12", cs, rg).coef == want
        # the largest intermediate stays far inside int32
        assert 255 * want[0] + 128 * (want[2] + want[3]) + 32768 < 2 ** 26 and 255 * want[0] + 128 * want[4] + 32768 < 2 ** 26
    assert pp.resolve_format("nv12").coef == TABLES[("bt601", "limited")]
    with pytest.raises(ValueError, match="colorspace"):
        pp.yuv_coefficients("bt2020", "limited")
    with pytest.raises(ValueError, match="range"):
        pp.yuv_coefficients("bt601", "video")


def test_known_answers():
    def one(y, u, v, cs="bt601", rg="limited"):
        return pp.yuv_to_rgb(np.array([y]), np.array([u]), np.array([v]), pp.yuv_coefficients(cs, rg))[0].tolist()
    for y, grey in ((16, 0), (126, 128), (235, 255), (0, 0), (255, 255)):
        assert one(y, 128, 128) == [grey] * 3, y
    every = np.arange(256)
    mid = np.full(256, 128)
    for cs in ("bt601", "bt709"):
        assert np.array_equal(pp.yuv_to_rgb(every, mid, mid, pp.yuv_coefficients(cs, "full")), np.stack([every] * 3, -1))
    assert one(81, 90, 240) == [254, 0, 0]
    assert one(81, 90, 240, cs="bt709") == [255, 24, 0]
    # the same through a frame, numpy and torch
    f = _nv12(np.full((2, 2), 81), np.array([[90]]), np.array([[240]]))
    assert pp.frames_to_rgb(f, "nv12").tolist() == [[[[254, 0, 0]] * 2] * 2]
    assert pp.frames_to_rgb(torch.from_numpy(f), "nv12", colorspace="bt709").tolist() == [[[[255, 24, 0]] * 2] * 2]


@pytest.fixture(scope="module")
def cube():
    """The whole 256^3 (Y, U, V) cube as ONE 4096 x 4096 NV12 frame: chroma pair (cx, cy) holds U = cx % 256, V = cy % 256, and the
    64 blocks that share a (U, V) -- group g = 8 (cx // 256) + cy // 256 -- hold the luma values 4 g + 2 dy + dx."""
    cy, cx = np.mgrid[0:2048, 0:2048]
    g = 8 * (cx // 256) + cy // 256
    Y = np.empty((4096, 4096), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            Y[dy::2, dx::2] = 4 * g + 2 * dy + dx
    frame = _nv12(Y, cx % 256, cy % 256)
    seen = np.zeros((256, 256, 256), bool)
    seen[Y, np.repeat(np.repeat(cx % 256, 2, 0), 2, 1), np.repeat(np.repeat(cy % 256, 2, 0), 2, 1)] = True
    assert seen.all()
    return frame


@pytest.mark.parametrize("cs,rg", NV12_TABLES)
def test_host_entry_equals_the_mirror_on_the_whole_cube(cube, cs, rg):
    want = pp.frames_to_rgb(cube, "nv12", colorspace=cs, range=rg)
    got = pp.frames_to_rgb_host(cube, "nv12", colorspace=cs, range=rg)
    assert want.shape == got.shape == (1, 4096, 4096, 3) and want.dtype == got.dtype == np.uint8
    assert np.array_equal(got, want)
    # the torch form of the mirror is the numpy form (a slab of the cube: every U, every V, 32 luma values)
    slab = np.concatenate([cube[:, :512], cube[:, 4096:4096 + 256]], 1)
    assert np.array_equal(pp.frames_to_rgb(torch.from_numpy(slab), "nv12", colorspace=cs, range=rg).numpy(), want[:, :512])


@pytest.mark.parametrize("fmt", ["bgr", "rgba", "bgra", "rgb"])
def test_packed_formats_are_exact_permutations_on_strided_frames(fmt):
    rng = np.random.default_rng(3)
    n, H, W, ch = 2, 9, 13, 4 if fmt in ("rgba", "bgra") else 3
    rs = W * ch + 7
    fs = rs * H + 5
    flat = rng.integers(1, 256, n * fs + 3, dtype=np.uint8)          # (guard bytes between rows and frames: non-zero)
    view = np.lib.stride_tricks.as_strided(flat[3:], (n, H, W, ch), (fs, rs, ch, 1))
    order = [2, 1, 0] if fmt in ("bgr", "bgra") else [0, 1, 2]
    want = view[..., order]
    before = flat.copy()
    for got in (pp.frames_to_rgb(view, fmt), pp.frames_to_rgb_host(view, fmt), pp.frames_to_rgb(torch.from_numpy(flat)[3:].as_strided(
            (n, H, W, ch), (fs, rs, ch, 1)), fmt).numpy()):
        assert got.shape == (n, H, W, 3) and np.array_equal(got, want)
    assert np.array_equal(flat, before)


@pytest.mark.parametrize("cs,rg", NV12_TABLES)
def test_round_trip_through_the_forward_matrix(cs, rg):
    kr, kb = KR_KB[cs]
    kg = 1.0 - kr - kb
    rgb = np.random.default_rng(20261021).integers(0, 256, (2_000_000, 3)).astype(np.float64)
    yl = kr * rgb[:, 0] + kg * rgb[:, 1] + kb * rgb[:, 2]
    pb, pr = (rgb[:, 2] - yl) / (2 * (1 - kb)), (rgb[:, 0] - yl) / (2 * (1 - kr))
    if rg == "limited":
        yuv = np.stack([16 + yl * 219 / 255, 128 + pb * 224 / 255, 128 + pr * 224 / 255], -1)
    else:
        yuv = np.stack([yl, 128 + pb, 128 + pr], -1)
    q = np.clip(np.rint(yuv), 0, 255).astype(np.int32)
    back = pp.yuv_to_rgb(q[:, 0], q[:, 1], q[:, 2], pp.yuv_coefficients(cs, rg)).astype(np.int64)
    err = np.abs(back - rgb.astype(np.int64)).max(0)
    cy, crv, cgu, cgv, cbu = _real_gains(cs, rg)
    bound = [int(math.floor(0.5 * (cy + sum(g)) + 0.5)) for g in ((crv,), (cgu, cgv), (cbu,))]
    print(f"[formats] round trip {cs} {rg}: max |error| per channel {err.tolist()}, bound {bound}")
    assert bound == ([1, 1, 2] if rg == "limited" else [1, 1, 1])
    assert (err <= bound).all(), (err, bound)


def test_nv12_geometry_is_nearest_chroma_per_2x2_block():
    rng = np.random.default_rng(5)
    H, W = 6, 10
    U, V = rng.permutation(15).reshape(3, 5) * 16 + 8, rng.permutation(15).reshape(3, 5) * 15 + 20
    f = _nv12(np.full((H, W), 120), U, V)
    for conv in (lambda a: pp.frames_to_rgb(a, "nv12"), lambda a: pp.frames_to_rgb_host(a, "nv12"),
                 lambda a: pp.frames_to_rgb(torch.from_numpy(a), "nv12").numpy()):
        rgb = conv(f)[0]
        colours = set()
        for by in range(H // 2):
            for bx in range(W // 2):
                block = rgb[2 * by:2 * by + 2, 2 * bx:2 * bx + 2].reshape(4, 3)
                assert (block == block[0]).all(), (by, bx)                   # the last row and column included
                want = pp.yuv_to_rgb(np.array([120]), U[by, bx:bx + 1], V[by, bx:bx + 1], pp.yuv_coefficients())[0]
                assert np.array_equal(block[0], want)
                colours.add(tuple(block[0]))
        assert len(colours) == 15
    # a padded luma plane read in place: the chroma plane named by its byte offset
    rs = W + 6
    buf = rng.integers(1, 256, (H + 2 + H // 2) * rs, dtype=np.uint8).reshape(-1, rs)
    buf[:H, :W] = f[0, :H]
    buf[H + 2:, :W] = f[0, H:]
    padded = np.lib.stride_tricks.as_strided(buf, (1, H + H // 2, W), (0, rs, 1))
    assert np.array_equal(pp.frames_to_rgb_host(padded, "nv12", chroma_offset=(H + 2) * rs), pp.frames_to_rgb(f, "nv12"))


def test_c_abi_argument_checks_without_a_gpu():
    lib = _lib.load()
    assert lib.bd_abi_version() == 9
    for name in ("bd_crop_resize_frames_fmt", "bd_frames_to_rgb_host", "bd_crop_resize_frames"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert (_lib.PIXEL_RGB, _lib.PIXEL_BGR, _lib.PIXEL_RGBA, _lib.PIXEL_BGRA, _lib.PIXEL_NV12) == (0, 1, 2, 3, 4)
    p = ctypes.c_void_p(64)                  # never dereferenced: every check below fails before a launch
    coef = TABLES[("bt601", "limited")]
    ok = dict(frames=p, n=2, H=48, W=64, rs=64, fs=64 * 72, boxes=p, fi=None, kb=None, m=2, S=224, out=p, dt=_lib.DTYPE_F32,
              fmt=_lib.PIXEL_NV12, off=48 * 64, coef=coef)

    def call(**kw):
        a = {**ok, **kw}
        return lib.bd_crop_resize_frames_fmt(a["frames"], a["n"], a["H"], a["W"], a["rs"], a["fs"], a["boxes"], a["fi"], a["kb"], a["m"],
                                             a["S"], a["out"], a["dt"], a["fmt"], a["off"], *a["coef"], None)
    assert call(frames=None) == -5 and call(boxes=None) == -5 and call(out=None) == -5            # BD_ERR_NULL
    assert call(fmt=5) == -2 and call(fmt=-1) == -2 and call(dt=7) == -2                            # BD_ERR_DTYPE: no such format
    assert call(H=47) == -1 and call(W=63) == -1                                                    # NV12 with an odd side
    assert call(rs=63) == -1                                                                        # shorter than one luma row
    assert call(off=48 * 64 - 1) == -1 and call(off=0) == -1 and call(rs=80) == -1                  # chroma inside the luma plane
    assert call(coef=(1 << 21,) + coef[1:]) == -1 and call(coef=coef[:5] + (256,)) == -1
    assert call(m=0) == -1 and call(S=513) == -1 and call(m=3) == -1 and call(n=0) == -1
    for fmt, bpp in ((_lib.PIXEL_RGB, 3), (_lib.PIXEL_BGR, 3), (_lib.PIXEL_RGBA, 4), (_lib.PIXEL_BGRA, 4)):
        assert call(fmt=fmt, rs=64 * bpp - 1) == -1, fmt                                            # a row of the format does not fit
    # the host converter: the same layout checks
    out = (ctypes.c_uint8 * 16)()
    src = (ctypes.c_uint8 * 16)()
    f = lib.bd_frames_to_rgb_host
    assert f(None, 1, 2, 2, 2, 6, 4, 4, *coef, out) == -5 and f(src, 1, 2, 2, 2, 6, 4, 4, *coef, None) == -5
    assert f(src, 1, 2, 2, 2, 6, 9, 4, *coef, out) == -2
    assert f(src, 1, 3, 2, 2, 6, 4, 6, *coef, out) == -1 and f(src, 1, 2, 2, 1, 6, 4, 4, *coef, out) == -1
    assert f(src, 1, 2, 2, 2, 6, 4, 3, *coef, out) == -1
    assert f(src, 1, 2, 2, 2, 6, 4, 4, *coef, out) == 0


def test_binding_refusals_per_format():
    boxes = torch.tensor([[0, 0, 8, 8]], dtype=torch.int32)
    good = {"bgr": torch.zeros((1, 8, 8, 3), dtype=torch.uint8), "rgba": torch.zeros((1, 8, 8, 4), dtype=torch.uint8),
            "bgra": torch.zeros((1, 8, 8, 4), dtype=torch.uint8), "nv12": torch.zeros((1, 12, 8), dtype=torch.uint8)}
    for fmt, frames in good.items():
        with pytest.raises(_lib.HipLibraryError):                    # host tensors: the HIP path refuses, there is no CPU resize
            pp.crop_resize_frames(frames, boxes, out_size=8, frame_format=fmt)
        with pytest.raises(TypeError, match=fmt):                    # dtype
            pp.crop_resize_frames(frames.float(), boxes, frame_format=fmt)
        with pytest.raises(TypeError, match=r"\[n, H"):              # shape: the message names the layout expected
            pp.crop_resize_frames(frames[0], boxes, frame_format=fmt)
    with pytest.raises(TypeError, match=r"\[n, H, W, 4\]"):
        pp.crop_resize_frames(good["bgr"], boxes, frame_format="bgra")
    with pytest.raises(TypeError, match=r"\[n, H, W, 3\]"):
        pp.crop_resize_frames(good["rgba"], boxes, frame_format="bgr")
    with pytest.raises(TypeError, match=r"\[n, H, W, 3\]"):
        pp.crop_resize_frames(good["rgba"], boxes)                   # the default is still packed RGB
    for bad in ((1, 13, 8), (1, 10, 8), (1, 12, 7)):                 # rows that are no H + H / 2 of an even H, odd W
        with pytest.raises(ValueError, match="luma rows"):
            pp.crop_resize_frames(torch.zeros(bad, dtype=torch.uint8), boxes, frame_format="nv12")
    with pytest.raises(ValueError, match="contiguous pixels"):       # pixel bytes strided
        pp.crop_resize_frames(torch.zeros((1, 8, 8, 8), dtype=torch.uint8)[..., ::2], boxes, frame_format="rgba")
    with pytest.raises(ValueError, match="contiguous pixels"):
        pp.crop_resize_frames(torch.zeros((1, 12, 16), dtype=torch.uint8)[..., ::2], boxes, frame_format="nv12")
    with pytest.raises(ValueError, match="unknown frame_format"):
        pp.crop_resize_frames(good["bgr"], boxes, frame_format="yuyv")
    with pytest.raises(ValueError, match="colorspace"):
        pp.crop_resize_frames(good["nv12"], boxes, frame_format="nv12", colorspace="bt2020")
    with pytest.raises(ValueError, match="range"):
        pp.crop_resize_frames(good["nv12"], boxes, frame_format="nv12", range="tv")
    assert pp.frame_shape_of(pp.resolve_format("nv12"), 2, 480, 640) == (2, 720, 640)
    assert pp.frame_shape_of(pp.resolve_format("bgra"), 1, 480, 640) == (1, 480, 640, 4)
    with pytest.raises(ValueError, match="even"):
        pp.frame_shape_of(pp.resolve_format("nv12"), 1, 481, 640)
    assert pp.resolve_format({"frame_format": "nv12", "colorspace": "bt709", "range": "full"}).coef == TABLES[("bt709", "full")]
    with pytest.raises(ValueError, match="fields"):
        pp.resolve_format({"format": "nv12"})


def test_pose_stream_plan_refusals():
    from boxdreamer_amd.cache import RefFeatureBank
    from boxdreamer_amd.stream import PoseStream
    model = _host_model()
    bank = RefFeatureBank(model.rgb_encoder, decoder=model.decoder)
    box, kw = torch.zeros((1, 8, 3)), dict(frame_shape=(96, 128))
    with pytest.raises(ValueError, match="unknown frame_format"):
        PoseStream(model, bank, [[0]], box, frame_format="i420", **kw)
    with pytest.raises(ValueError, match="describe NV12"):
        PoseStream(model, bank, [[0]], box, frame_format="bgr", colorspace="bt709", **kw)
    with pytest.raises(ValueError, match="describe NV12"):
        PoseStream(model, bank, [[0]], box, range="full", **kw)
    with pytest.raises(ValueError, match="unknown colorspace"):
        PoseStream(model, bank, [[0]], box, frame_format="nv12", colorspace="srgb", **kw)
    for fmt in ("rgb", "bgra", "nv12"):          # a format that is fine: the next refusal is the (empty) bank's
        with pytest.raises(ValueError, match="nor a row of the bank"):
            PoseStream(model, bank, [[0]], box, frame_format=fmt, **kw)


def test_facade_frame_format_on_the_host():
    from boxdreamer_amd import synth
    m, seen = _host_facade()
    data = synth.make_batch(seed=3, B=1, T=2)
    images = data["images"]
    rest = {k: v for k, v in data.items() if k != "images"}
    boxes = torch.tensor([[[0, 0, 8, 8], [0, 0, 8, 8]]], dtype=torch.int32)
    nv12 = torch.zeros((2, 12, 8), dtype=torch.uint8)
    # "images" present: "frame_format" is not even looked at
    out = m({**data, "frame_format": "no such format"})
    assert seen["images"] is images and out["images"] is images
    with pytest.raises(ValueError, match="unknown frame_format"):
        m({**rest, "frames": nv12, "crop_boxes": boxes, "frame_format": "p010"})
    with pytest.raises(ValueError, match="describe NV12"):
        m({**rest, "frames": nv12, "crop_boxes": boxes, "frame_format": {"frame_format": "bgr", "range": "full"}})
    with pytest.raises(TypeError, match=r"\[n, H, W, 3\]"):           # absent (or None): packed RGB, today's path and its refusal
        m({**rest, "frames": nv12, "crop_boxes": boxes, "frame_format": None})
    with pytest.raises(TypeError, match=r"\[n, H, W, 4\]"):           # the layout of the format that was named
        m({**rest, "frames": nv12, "crop_boxes": boxes, "frame_format": "bgra"})
    for fmt in ("nv12", {"frame_format": "nv12", "colorspace": "bt709", "range": "full"}):
        with pytest.raises(_lib.HipLibraryError):                     # well-formed and on the host: the HIP path refuses
            m({**rest, "frames": nv12, "crop_boxes": boxes, "frame_format": fmt})
