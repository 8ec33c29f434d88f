"""GPU: bd_crop_resize_frames_fmt (csrc/preprocess.hip) -- camera-native frames (bgr, rgba / bgra, nv12) behind
preprocess.crop_resize_frames, PoseStream and BoxDreamer.forward's "frame_format" key.

One contract, checked with torch.equal everywhere: the crop of a frame in format F is the existing kernel's crop of
`preprocess.frames_to_rgb(frame, F)` (the mirror tests/test_frame_formats_host.py pins), bit for bit, because only the stage that
turns source bytes into pixels differs.  The frames are small (26 x 38: W even and no multiple of 4, more than one chroma row and
dword per row) and sit in a larger byte tensor at byte offsets 0..3 with an odd row stride, so that every alignment of the luma and
chroma dwords and of the 4-byte pixels occurs.
"""
import gc

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, synth
from boxdreamer_amd import preprocess as pp
from boxdreamer_amd.stream import PoseStream
from test_frame_formats_host import NV12_TABLES
from test_gpu_preprocess import _config
from test_gpu_ragged import _to_dev
from test_gpu_stream import CASES, H, S, W, _eq, _shared
from test_gpu_stream_select import DATABASES, K_SEL, MAX_RMS, _bank, _bbox_3d
from test_stream_host import bits

pytestmark = pytest.mark.gpu

FH, FW = 26, 38
FORMATS = [("bgr", {}), ("rgba", {}), ("bgra", {})] + [("nv12", dict(colorspace=cs, range=rg)) for cs, rg in NV12_TABLES]
IDS = ["-".join([f] + list(kw.values())) for f, kw in FORMATS]
ONE_PER_FORMAT = [("rgb", {}), ("bgr", {}), ("rgba", {}), ("bgra", {}), ("nv12", {}), ("nv12", dict(colorspace="bt709", range="full"))]

# x0 y0 x1 y1 on a 26 x 38 (H x W) frame
BOXES = [[3, 5, 23, 25],            # odd x0 and y0, inside
         [-7, 2, 25, 34],           # over the left and the bottom edge, negative x0
         [20, -9, 52, 23],          # over the right and the top edge
         [-5, -7, 45, 43],          # over all four
         [10, 10, 26, 26],          # holds the last luma rows: the last chroma row
         [37, 3, 57, 23],           # a valid rectangle 1 pixel wide: the last column
         [-19, 4, 1, 24],           # ... the first column
         [9, 1, 10, 2],             # one pixel
         [50, 50, 70, 70],          # entirely outside: zeros
         [11, 7, 14, 10],           # upscale by 10
         [1, 0, 27, 26],            # scale just under 1, odd x0
         [-100, -120, 200, 180]]    # downscale by 10
OUTSIDE = 8


def _frames(fmt, n=3, Hf=FH, Wf=FW, offset=1, seed=0, pad=5):
    """n seeded frames of the format as a strided view (odd row stride > the row, frames apart) into a flat device byte tensor, `offset`
    bytes past its start -> (flat, view).  Every byte of `flat` is random and non-zero: guard bytes show if they are read as pixels."""
    shape = pp.frame_shape_of(pp.resolve_format(fmt), n, Hf, Wf)
    row = shape[2] * (shape[3] if len(shape) == 4 else 1)
    rs = row + pad
    fs = rs * shape[1] + 7
    g = torch.Generator().manual_seed(1000 + seed)
    flat = torch.randint(1, 256, (n * fs + 8,), generator=g, dtype=torch.uint8).cuda()
    strides = (fs, rs, shape[3], 1) if len(shape) == 4 else (fs, rs, 1)
    return flat, flat.as_strided(shape, strides, offset)


def _boxes(b):
    return torch.tensor(b, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt,kw", FORMATS, ids=IDS)
def test_crop_of_a_format_is_the_crop_of_the_converted_frame(hip, fmt, kw, offset):
    flat, f = _frames(fmt, offset=offset, seed=offset, pad=5 + offset)
    before = flat.clone()
    rgb = pp.frames_to_rgb(f, fmt, **kw)
    assert rgb.shape == (3, FH, FW, 3) and rgb.is_contiguous()
    fi = _boxes([i % 3 for i in range(len(BOXES))]).reshape(-1)
    for out_size in (32, 30):                                        # (30: no multiple of 4, the scalar store path)
        got = pp.crop_resize_frames(f, _boxes(BOXES), frame_idx=fi, out_size=out_size, frame_format=fmt, **kw)
        want = pp.crop_resize_frames(rgb, _boxes(BOXES), frame_idx=fi, out_size=out_size)
        assert got.shape == (len(BOXES), 3, out_size, out_size)
        for k in range(len(BOXES)):
            assert torch.equal(got[k], want[k]), (fmt, kw, offset, out_size, BOXES[k], (got[k] - want[k]).abs().max().item())
        assert not got[OUTSIDE].any() and all(bool(got[k].any()) for k in range(len(BOXES)) if k != OUTSIDE)
    assert torch.equal(flat, before)                                 # the frame buffer, guard bytes included, is only read


@pytest.mark.parametrize("fmt,kw", ONE_PER_FORMAT[1:], ids=lambda v: v if isinstance(v, str) else "-".join(v.values()))
def test_keep_boxes_frame_idx_and_output_dtypes(hip, fmt, kw):
    _, f = _frames(fmt, offset=3, seed=11)
    rgb = pp.frames_to_rgb(f, fmt, **kw)
    boxes = _boxes(BOXES[:6])
    keep = _boxes([[5, 7, 19, 21], [1, 3, 37, 25], [21, 1, 35, 9], [0, 0, 37, 25], [13, 11, 13, 25], [3, 3, 40, 30]])    # odd edges
    fi = _boxes([2, 0, 2, 1, 1, 0]).reshape(-1)                      # reordered and repeated
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        got = pp.crop_resize_frames(f, boxes, frame_idx=fi, keep_boxes=keep, out_size=32, dtype=dtype, frame_format=fmt, **kw)
        want = pp.crop_resize_frames(rgb, boxes, frame_idx=fi, keep_boxes=keep, out_size=32, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, want), (fmt, dtype)
    plain = pp.crop_resize_frames(f, boxes, frame_idx=fi, out_size=32, frame_format=fmt, **kw)
    assert not torch.equal(plain, pp.crop_resize_frames(f, boxes, frame_idx=fi, keep_boxes=keep, out_size=32, frame_format=fmt, **kw))
    # no frame_idx: crop i reads frame i; and FramePreprocessor passes the format on
    assert torch.equal(pp.crop_resize_frames(f, boxes[:3], out_size=30, frame_format=fmt, **kw), pp.crop_resize_frames(rgb, boxes[:3], out_size=30))
    det = torch.tensor([[3.2, 5.9, 23.1, 25.0], [-7.5, 2.0, 25.0, 30.0], [20.0, -9.0, 36.5, 23.25]], device="cuda")
    img, _, bi = pp.FramePreprocessor(3, 32, frame_format=fmt, **kw)(f, det)
    assert torch.equal(img, pp.crop_resize_frames(rgb, bi, out_size=32))


@pytest.mark.parametrize("fmt,kw", ONE_PER_FORMAT[1:], ids=lambda v: v if isinstance(v, str) else "-".join(v.values()))
def test_the_two_rare_forms_of_the_kernel(hip, fmt, kw):
    """Weights on the fly (out_size x taps beyond the LDS table: support > 40 at out_size 64) and source bytes straight from global
    memory (a clipped row beyond the LDS stage: a frame wider than 4096 px, which at any out_size is also beyond the table)."""
    _, f = _frames(fmt, offset=1, seed=21)
    boxes = _boxes([[-1500, -1480, 1500, 1520], [-1399, -1401, 1402, 1400], [3, 5, 23, 25]])          # support 46.9, 43.8; the table
    fi = _boxes([1, 0, 2]).reshape(-1)
    got = pp.crop_resize_frames(f, boxes, frame_idx=fi, out_size=64, frame_format=fmt, **kw)
    assert torch.equal(got, pp.crop_resize_frames(pp.frames_to_rgb(f, fmt, **kw), boxes, frame_idx=fi, out_size=64)) and bool(got[:2].any())
    _, f = _frames(fmt, n=2, Hf=6, Wf=4500, offset=3, seed=22)
    boxes = _boxes([[50, -2200, 4450, 2200], [-3, -1, 4497, 4499], [4001, -100, 4301, 200]])            # direct, direct, staged
    fi = _boxes([0, 1, 1]).reshape(-1)
    got = pp.crop_resize_frames(f, boxes, frame_idx=fi, out_size=64, frame_format=fmt, **kw)
    want = pp.crop_resize_frames(pp.frames_to_rgb(f, fmt, **kw), boxes, frame_idx=fi, out_size=64)
    for k in range(3):
        assert torch.equal(got[k], want[k]) and bool(got[k].any()), (fmt, k)


def _call_fmt(lib, f, boxes, out, fmt_id, fi=None):
    rc = lib.bd_crop_resize_frames_fmt(_lib.ptr(f), f.shape[0], f.shape[1], f.shape[2], f.stride(1), f.stride(0), _lib.ptr(boxes),
                                       _lib.ptr(fi), None, boxes.shape[0], out.shape[-1], _lib.ptr(out), _lib.dtype_id(out), fmt_id, 0,
                                       0, 0, 0, 0, 0, 0, _lib.stream())
    _lib.check(rc, "bd_crop_resize_frames_fmt")
    return out


def test_rgb_through_the_new_entry_is_the_old_entry(hip):
    lib = _lib.load()
    fi = _boxes([i % 3 for i in range(len(BOXES))]).reshape(-1)
    for offset in range(4):
        _, f = _frames("rgb", offset=offset, seed=30 + offset)
        for out_size, dtype in ((32, torch.float32), (30, torch.float32), (32, torch.bfloat16)):
            old = pp.crop_resize_frames(f, _boxes(BOXES), frame_idx=fi, out_size=out_size, dtype=dtype)
            new = _call_fmt(lib, f, _boxes(BOXES), torch.full_like(old, -3.0), _lib.PIXEL_RGB, fi)
            assert torch.equal(old, new), (offset, out_size, dtype)
    _, f = _frames("rgb", n=2, Hf=6, Wf=4500, offset=1, seed=35)                               # the direct form
    boxes = _boxes([[50, -2200, 4450, 2200], [-3, -1, 4497, 4499]])
    old = pp.crop_resize_frames(f, boxes, out_size=64)
    assert torch.equal(old, _call_fmt(lib, f, boxes, torch.full_like(old, -3.0), _lib.PIXEL_RGB)) and bool(old.any())


def test_out_slice_is_the_only_memory_written(hip):
    for fmt, kw in ONE_PER_FORMAT[1:5]:
        flat, f = _frames(fmt, n=4, offset=2, seed=40)
        before = flat.clone()
        boxes = _boxes([[[0, 0, 20, 20], [13, 1, 37, 25]], [[-10, -10, 30, 30], [5, 3, 25, 23]]])
        for dtype in (torch.float32, torch.bfloat16):
            big = torch.full((4, 2, 3, 30, 30), -7.0, dtype=dtype, device="cuda")
            ret = pp.crop_resize_frames(f, boxes, out=big[1:3], out_size=30, frame_format=fmt, **kw)
            assert ret.data_ptr() == big[1:3].data_ptr() and ret.shape == (2, 2, 3, 30, 30)
            assert bool((big[0] == -7).all()) and bool((big[3] == -7).all())
            assert torch.equal(big[1:3], pp.crop_resize_frames(pp.frames_to_rgb(f, fmt, **kw), boxes, out_size=30, dtype=dtype))
            assert float(big[1:3].min()) >= 0.0
        assert torch.equal(flat, before), fmt


def test_capture_once_replay_with_new_boxes_and_new_bytes(hip):
    flat, f = _frames("nv12", n=2, offset=1, seed=50)
    boxes = _boxes([[3, 5, 23, 25], [-7, 2, 25, 34]])
    out = torch.zeros((2, 3, 32, 32), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pp.crop_resize_frames(f, boxes, out=out, out_size=32, frame_format="nv12")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pp.crop_resize_frames(f, boxes, out=out, out_size=32, frame_format="nv12")
    first = pp.crop_resize_frames(pp.frames_to_rgb(f, "nv12"), boxes, out_size=32)
    g.replay()
    assert torch.equal(out, first)
    new = _boxes([[11, 7, 14, 10], [-5, -7, 45, 43]])
    boxes.copy_(new)                                                 # on the device, no re-capture
    flat.copy_(_frames("nv12", n=2, offset=1, seed=51)[0])           # ... and new NV12 bytes in the same buffer
    g.replay()
    assert torch.equal(out, pp.crop_resize_frames(pp.frames_to_rgb(f, "nv12"), new, out_size=32)) and not torch.equal(out, first)


# ---- PoseStream: a session built for a format, fed that format, against a default session fed the converted frames
def _source(fmt, n_frames, step):
    g = torch.Generator().manual_seed(70 + step)
    return torch.randint(0, 256, pp.frame_shape_of(pp.resolve_format(fmt), n_frames, H, W), generator=g, dtype=torch.uint8)


def _same_step(a, b, where):
    assert np.array_equal(bits(a.rows_host.numpy()), bits(b.rows_host.numpy())), where
    for name in ("heat", "corners_px", "poses", "rms_px", "windows", "K_crop", "crops"):
        assert _eq(getattr(a, name), getattr(b, name)), (where, name)


def _K(B, step):
    K = torch.tensor([[150.0, 0.0, 64.0], [0.0, 140.0, 48.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    K[:, 0, 2] += torch.arange(B) * 1.5 + step
    return K


@pytest.mark.parametrize("fmt,kw", [("nv12", {}), ("bgra", {}), ("nv12", dict(colorspace="bt709", range="full"))], ids=["nv12", "bgra", "nv12-bt709-full"])
def test_stream_of_a_format_equals_the_default_stream_on_converted_frames(hip, fmt, kw):
    sh = _shared()
    B, T = 2, 3
    rows, fidx, dets = CASES[(B, T)]
    bbox_3d = _to_dev(synth.make_batch(seed=51, B=B, T=T))["bbox_3d"][:, T - 1]
    s = PoseStream(sh["model"], sh["bank"], rows, bbox_3d, frame_shape=(H, W), n_frames=2, frame_format=fmt, **kw)
    plain = PoseStream(sh["model"], sh["bank"], rows, bbox_3d, frame_shape=(H, W), n_frames=2)
    assert tuple(s.frames.shape) == pp.frame_shape_of(pp.resolve_format(fmt), 2, H, W) and s.frame_format.name == fmt
    # the default session: the buffers and the counters it always had
    assert tuple(plain.frames.shape) == (2, H, W, 3) and plain.frame_format.name == "rgb" and plain.frames.dtype == torch.uint8
    assert tuple(plain.crops.shape) == (B, 3, S, S) and plain.replays == 0 and len(plain.host_syncs_per_step) == 1
    assert tuple(plain.rows_host.shape) == (B, 66) and plain.track is None and plain.keep_boxes is None
    heats = []
    for step in range(3):
        src = _source(fmt, 2, step)
        det, K, fi = torch.tensor(dets[step % 2], dtype=torch.float32), _K(B, step), torch.tensor(fidx, dtype=torch.int32)
        s.step(src.pin_memory() if step != 1 else src.cuda(), det, K, frame_idx=fi)
        plain.step(pp.frames_to_rgb(src, fmt, **kw), det, K, frame_idx=fi)
        _same_step(s, plain, (fmt, step))
        assert torch.isfinite(s.rows_host[:, :16]).all()
        heats.append(s.heat.clone())
    assert not torch.equal(heats[0], heats[1]) and not torch.equal(heats[1], heats[2])
    assert s.replays == plain.replays == 3
    with pytest.raises(ValueError, match="frame shape is fixed"):
        s.step(pp.frames_to_rgb(src, fmt, **kw), det, K)            # an RGB frame given to a session of another format
    del s, plain
    gc.collect()


def test_stream_single_frame_forms_and_selecting_tracking_session(hip):
    sh = _shared()
    model = sh["model"]
    # n_frames == 1: a (H * 3 / 2, W) or (H, W, 4) frame is accepted as it is
    bbox_1 = _to_dev(synth.make_batch(seed=51, B=1, T=2))["bbox_3d"][:, 1]
    for fmt in ("nv12", "bgra"):
        s = PoseStream(model, sh["bank"], CASES[(1, 2)][0], bbox_1, frame_shape=(H, W), frame_format=fmt)
        src = _source(fmt, 1, 5)
        det = torch.tensor(CASES[(1, 2)][2][0], dtype=torch.float32)
        a = s.step(src[0], det, _K(1, 0)).clone()
        crops = s.crops.clone()
        b = s.step(src, det, _K(1, 0))
        assert src[0].dim() == s.frames.dim() - 1 and np.array_equal(bits(a.numpy()), bits(b.numpy())) and torch.equal(crops, s.crops)
        assert torch.equal(crops, pp.crop_resize_frames(pp.frames_to_rgb(src, fmt).cuda(), s.windows))
        del s
    # select_k + track_boxes + use_keep_boxes under nv12: none of them looks at pixels
    B, bank, bbox_3d = 2, _bank(model), _bbox_3d(2)
    kw = dict(frame_shape=(H, W), n_frames=2, select_k=K_SEL, select="track", max_rms_px=MAX_RMS, track_boxes=True, use_keep_boxes=True)
    s = PoseStream(model, bank, DATABASES, bbox_3d, frame_format="nv12", **kw)
    plain = PoseStream(model, bank, DATABASES, bbox_3d, **kw)
    dets = CASES[(2, 3)][2]
    for step in range(3):
        src = _source("nv12", 2, 10 + step)
        det = torch.tensor(dets[step % 2], dtype=torch.float32) if step != 1 else None
        fi = torch.tensor([0, 1], dtype=torch.int32)
        s.step(src, det, _K(B, step), frame_idx=fi)
        plain.step(pp.frames_to_rgb(src, "nv12"), det, _K(B, step), frame_idx=fi)
        _same_step(s, plain, ("select + track + keep", step))
        assert torch.equal(s.sel, plain.sel) and torch.equal(s.used, plain.used) and torch.equal(s.keep_boxes, plain.keep_boxes)
        assert np.array_equal(bits(s.track_host.numpy()), bits(plain.track_host.numpy()))
    assert s.replays == plain.replays == 3
    del s, plain
    gc.collect()


def test_forward_from_nv12_frames_matches_forward_from_converted_frames(hip):
    from boxdreamer_amd.model import BoxDreamer
    model = BoxDreamer(_config())
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(1234, 2).items()}, strict=True)
    model = model.cuda().eval()
    B, T = 2, 3
    g = torch.Generator().manual_seed(90)
    yy, xx = np.mgrid[0:360, 0:320]
    smooth = torch.from_numpy(np.rint(127.5 + 100 * np.sin(xx / 17.0 + yy / 29.0)).astype(np.uint8))
    nv12 = ((smooth.int() + torch.randint(0, 24, (360, 320), generator=g)).clamp(0, 255).to(torch.uint8))[None].cuda()      # 240 x 320
    boxes = torch.tensor([[[20, 10, 240, 230], [96, 8, 320, 232], [-30, -40, 300, 290]], [[101, 51, 190, 140], [0, 0, 240, 240], [151, 61, 330, 240]]],
                         dtype=torch.int32, device="cuda")
    fidx = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    base = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(seed=11, B=B, T=T).items() if k != "images"}
    base["query_idx"] = torch.tensor([2, 0])
    for fmt in ("nv12", {"frame_format": "nv12", "colorspace": "bt709", "range": "full"}):
        a = model({**base, "frames": nv12, "crop_boxes": boxes, "frame_idx": fidx, "frame_format": fmt})
        got = {k: a[k].clone() for k in ("images", "pred_bbox", "pred_corners_px", "regression_boxes", "pred_poses")}
        logits = model.decoder.last_logits.clone()
        rgb = pp.frames_to_rgb(nv12, fmt["frame_format"], fmt["colorspace"], fmt["range"]) if isinstance(fmt, dict) else pp.frames_to_rgb(nv12, fmt)
        b = model({**base, "frames": rgb, "crop_boxes": boxes, "frame_idx": fidx})
        for k, v in got.items():
            assert torch.equal(v, b[k]), (fmt, k)
        assert torch.equal(logits, model.decoder.last_logits) and bool(got["images"].any())
