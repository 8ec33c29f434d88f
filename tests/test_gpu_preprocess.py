"""GPU: bd_crop_resize_frames (csrc/preprocess.hip) behind boxdreamer_amd.preprocess and behind BoxDreamer.forward's "frames" keys.

Yardstick: the fp64 restatement of the filter in tests/test_preprocess.py (pinned there to the reference's own output through
tests/golden/preprocess_vectors.npz).  Bound per crop: err_kernel <= max(4e-6, err_reference).  4e-6 is the accumulation bound of an
fp32 implementation with exact tap geometry (two passes of at most 2 ceil(scale) + 2 <= 20 taps for scale <= 9, values and weights in
[0, 1]: 2 x 23 x 2^-24 + 2^-23 < 4e-6); err_reference is the reference's own distance from the exact filter, recorded in the fixture
(its tap centres are fp32).  Where no reference output exists (the randomised sweep) the bound is 4e-6 alone.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from boxdreamer_amd import preprocess as pp
from boxdreamer_amd import synth
from test_preprocess import ACC_BOUND, GOLDEN, cases, exact_fp64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def run_one(frame, box, S, keep=None, dtype=torch.float32):
    f = torch.from_numpy(np.ascontiguousarray(frame))[None].cuda()
    b = torch.tensor([list(map(int, box))], dtype=torch.int32, device="cuda")
    k = None if keep is None else torch.tensor([list(map(int, keep))], dtype=torch.int32, device="cuda")
    return pp.crop_resize_frames(f, b, keep_boxes=k, out_size=S, dtype=dtype)[0]


def test_fixture_cases_against_the_exact_filter_and_the_reference(hip, golden):
    for i, frame, box, S, keep in cases(golden):
        got = run_one(frame, box, S, keep).double().cpu().numpy()
        err_ref = float(golden[f"c{i}_err_ref"])
        err = np.abs(got - golden[f"c{i}_exact"]).max()
        direct = np.abs(got - golden[f"c{i}_ref"].astype(np.float64)).max()
        print(f"[preprocess] case {i:2d} S {S:3d} side {box[2] - box[0]:4d}: err_kernel {err:.2e} err_reference {err_ref:.2e} |kernel - reference| {direct:.2e}")
        assert err <= max(ACC_BOUND, err_ref), (i, err, err_ref)
        assert direct <= max(ACC_BOUND, err_ref) + err_ref, (i, direct)
    # the two crops that share a frame, in ONE launch through frame_idx, and the keep-box cases next to them
    n = int(golden["n_cases"])
    sel = [i for i in range(n) if int(golden[f"c{i}_frame"]) == 1 and int(golden[f"c{i}_out_size"]) == 32]
    assert len(sel) >= 3
    f = torch.from_numpy(golden["frame_1"])[None].cuda()
    b = torch.tensor(np.stack([golden[f"c{i}_int_box"] for i in sel]), dtype=torch.int32, device="cuda")
    out = pp.crop_resize_frames(f, b, frame_idx=torch.zeros(len(sel), dtype=torch.int32, device="cuda"), out_size=32)
    for k, i in enumerate(sel):
        assert np.abs(out[k].double().cpu().numpy() - golden[f"c{i}_exact"]).max() <= max(ACC_BOUND, float(golden[f"c{i}_err_ref"]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_outputs_are_the_fp32_output_rounded_once(hip, golden, dtype):
    for i, frame, box, S, keep in cases(golden):
        want = run_one(frame, box, S, keep).to(dtype)
        got = run_one(frame, box, S, keep, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, want), i


def _strided_frames(rng, n, H, W):
    """[n, H, W, 3] uint8 view into a larger parent: odd row stride, odd frame stride, base pointer off dword alignment."""
    rs, fs = (W + int(rng.integers(1, 6))) * 3 + int(rng.integers(0, 3)), None
    fs = rs * (H + 2) + int(rng.integers(0, 7))
    flat = torch.from_numpy(rng.integers(0, 256, n * fs + 16, dtype=np.uint8))
    # smooth content with an edge in every second frame
    off = int(rng.integers(1, 4))
    view = flat.as_strided((n, H, W, 3), (fs, rs, 3, 1), off)
    for k in range(1, n, 2):
        yy, xx = np.mgrid[0:H, 0:W]
        g = np.stack([255 * xx / W, 255 * yy / H, 127.5 + 127.5 * np.sin(xx / 23.0 + yy / 31.0)], -1)
        g[xx + yy > (H + W) // 2] *= 0.3
        view[k] = torch.from_numpy(np.rint(g).astype(np.uint8))
    dev = flat.cuda().as_strided((n, H, W, 3), (fs, rs, 3, 1), off)
    return view.numpy(), dev


def test_randomised_sweep_against_the_fp64_restatement(hip):
    rng = np.random.default_rng(20261018)
    launches = [(1080, 1920, 3, 224, 44), (480, 640, 4, 224, 60), (333, 517, 5, 224, 60), (97, 161, 4, 57, 50), (720, 1280, 2, 112, 30)]
    worst, total = 0.0, 0
    for H, W, n, S, m in launches:
        host, dev = _strided_frames(rng, n, H, W)
        boxes, fidx = [], []
        for k in range(m):
            kind = k % 6
            if kind == 0:
                s = int(rng.integers(1, 2001))
            elif kind == 1:
                s = int(rng.integers(1, 40))
            else:
                s = int(np.exp(rng.uniform(np.log(8), np.log(2000))))
            if kind == 5:      # anywhere, often partly or fully outside
                x0, y0 = int(rng.integers(-s - 50, W + 50)), int(rng.integers(-s - 50, H + 50))
            else:              # overlapping the frame
                x0, y0 = int(rng.integers(-s // 2, max(W - s // 2, -s // 2 + 1))), int(rng.integers(-s // 2, max(H - s // 2, -s // 2 + 1)))
            boxes.append([x0, y0, x0 + s, y0 + s])
            fidx.append(int(rng.integers(0, n)))
        boxes += [[W + 5, 10, W + 45, 50], [10, 10, 10, 10], [30, 30, 20, 20], [0, 0, 40, 41], [-300, -300, -1, -1]]   # outside / degenerate
        fidx += [0, 0, 0, 0, 0]
        b = torch.tensor(boxes, dtype=torch.int32, device="cuda")
        fi = torch.tensor(fidx, dtype=torch.int32, device="cuda")
        out = pp.crop_resize_frames(dev, b, frame_idx=fi, out_size=S).double().cpu().numpy()
        assert not out[-5:].any(), "a crop outside the frame or with a degenerate box is zeros"
        for k, (box, f) in enumerate(zip(boxes, fidx)):
            want = exact_fp64(host[f], box, S)
            err = np.abs(out[k] - want).max()
            worst = max(worst, err)
            assert err <= ACC_BOUND, (H, W, S, box, f, err)
        total += len(boxes)
    print(f"[preprocess] sweep: {total} crops in {len(launches)} launches, worst err_kernel {worst:.2e} (bound {ACC_BOUND:.0e})")
    assert total >= 200


def test_the_two_rare_forms_of_the_kernel(hip):
    """csrc/preprocess.hip switches per crop to weights evaluated on the fly (out_size x taps beyond its LDS table) and to source bytes
    read straight from global memory (a clipped row beyond its LDS stage: frames wider than 4096 px).  Same arithmetic, same bound:
    the cases stay at scale <= 10, i.e. at most 22 taps per pass (2 x 25 x 2^-24 + 2^-23 = 3.1e-6 < 4e-6)."""
    rng = np.random.default_rng(9)
    host, dev = _strided_frames(rng, 2, 480, 640)
    boxes = [[-1200, -1300, 1500, 1400], [-100, -2000, 2900, 1000], [200, 100, 500, 400]]          # scale 9, 10 (on the fly), 1 (table)
    out = pp.crop_resize_frames(dev, torch.tensor(boxes, dtype=torch.int32, device="cuda"),
                                frame_idx=torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda"), out_size=300).double().cpu().numpy()
    for k, f in enumerate([1, 0, 1]):
        err = np.abs(out[k] - exact_fp64(host[f], boxes[k], 300)).max()
        print(f"[preprocess] on-the-fly weights, box {boxes[k]}: err_kernel {err:.2e}")
        assert err <= ACC_BOUND, (boxes[k], err)
    host, dev = _strided_frames(rng, 2, 6, 4500)
    boxes = [[50, -2200, 4450, 2200], [-3, -1, 4497, 4499], [4000, -100, 4300, 200]]               # scale 8.8, 9 at out_size 500; 0.6
    out = pp.crop_resize_frames(dev, torch.tensor(boxes, dtype=torch.int32, device="cuda"),
                                frame_idx=torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda"), out_size=500).double().cpu().numpy()
    for k, f in enumerate([0, 1, 1]):
        err = np.abs(out[k] - exact_fp64(host[f], boxes[k], 500)).max()
        print(f"[preprocess] direct global reads, box {boxes[k]}: err_kernel {err:.2e}")
        assert err <= ACC_BOUND, (boxes[k], err)
        assert out[k].any()


def test_a_crop_does_not_depend_on_its_launch(hip):
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)).cuda()
    box = [100, -20, 500, 380]
    alone = pp.crop_resize_frames(frames[1:2], torch.tensor([box], dtype=torch.int32, device="cuda"))
    again = pp.crop_resize_frames(frames[1:2], torch.tensor([box], dtype=torch.int32, device="cuda"))
    assert torch.equal(alone, again)
    boxes = []
    for k in range(192):
        s = int(rng.integers(1, 900))
        x0, y0 = int(rng.integers(-100, 600)), int(rng.integers(-100, 440))
        boxes.append([x0, y0, x0 + s, y0 + s])
    boxes[77] = box
    fi = torch.from_numpy(rng.integers(0, 3, 192).astype(np.int32))
    fi[77] = 1
    many = pp.crop_resize_frames(frames, torch.tensor(boxes, dtype=torch.int32, device="cuda"), frame_idx=fi.cuda())
    assert torch.equal(many[77], alone[0])
    shared = pp.crop_resize_frames(frames, torch.tensor([boxes[3], box, box], dtype=torch.int32, device="cuda"),
                                   frame_idx=torch.tensor([int(fi[3]), 1, 1], dtype=torch.int32, device="cuda"))
    assert torch.equal(shared[1], alone[0]) and torch.equal(shared[2], alone[0]) and torch.equal(shared[0], many[3])


def test_out_slice_is_the_only_memory_written(hip):
    rng = np.random.default_rng(6)
    frames = torch.from_numpy(rng.integers(0, 256, (4, 120, 160, 3), dtype=np.uint8)).cuda()
    boxes = torch.tensor([[[0, 0, 100, 100], [30, 10, 130, 110]], [[-10, -10, 90, 90], [50, 20, 150, 120]]], dtype=torch.int32, device="cuda")
    for dtype in (torch.float32, torch.bfloat16):
        big = torch.full((4, 2, 3, 224, 224), -7.0, dtype=dtype, device="cuda")
        ret = pp.crop_resize_frames(frames, boxes, out=big[1:3])
        assert ret.data_ptr() == big[1:3].data_ptr() and ret.shape == (2, 2, 3, 224, 224)
        assert bool((big[0] == -7).all()) and bool((big[3] == -7).all())
        assert torch.equal(big[1:3], pp.crop_resize_frames(frames, boxes, dtype=dtype))
        assert float(big[1:3].min()) >= 0.0
    # the FramePreprocessor's buffers: float boxes in, the same pixels as the two-step form out, nothing re-allocated
    fp = pp.FramePreprocessor(4, 56)
    det = torch.tensor([[10.3, 20.2, 90.7, 70.1], [0.5, 0.5, 40.0, 60.0], [100.0, 50.0, 159.0, 119.0], [-20.0, -5.0, 30.5, 40.25]], device="cuda")
    K = torch.tensor([[500.0, 0, 80], [0, 500, 60], [0, 0, 1]], device="cuda").expand(4, 3, 3)
    img, Kc, bi = fp(frames, det, K)
    ptrs = (img.data_ptr(), bi.data_ptr())
    assert torch.equal(bi.cpu(), pp.square_bbox(det.cpu())) and torch.equal(img, pp.crop_resize_frames(frames, bi, out_size=56))
    assert torch.allclose(Kc.cpu(), pp.crop_intrinsics(K.cpu(), bi.cpu(), 56))
    img2, _, bi2 = fp(frames, det + 3.0, K)
    assert (img2.data_ptr(), bi2.data_ptr()) == ptrs


def test_capture_once_replay_with_new_boxes(hip):
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 240, 320, 3), dtype=np.uint8)).cuda()
    boxes = torch.tensor([[10, 10, 210, 210], [50, -30, 300, 220]], dtype=torch.int32, device="cuda")
    out = torch.zeros((2, 3, 224, 224), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pp.crop_resize_frames(frames, boxes, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pp.crop_resize_frames(frames, boxes, out=out)
    first = pp.crop_resize_frames(frames, boxes)
    g.replay()
    assert torch.equal(out, first)
    new = torch.tensor([[100, 100, 130, 130], [-200, -200, 600, 600]], dtype=torch.int32, device="cuda")
    boxes.copy_(new)                                  # on the device, no re-capture
    g.replay()
    assert torch.equal(out, pp.crop_resize_frames(frames, new)) and not torch.equal(out, first)


def _config(prec="f16c8_qk16", depth=2, **mods):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_modules_config.json")
    m = copy.deepcopy(json.load(open(path))["modules"])
    m["decoder"].update(num_decoder_layers=depth, hip_precision=prec)
    m["encoder"]["dino"]["cfg"].update(synthetic_seed=4321, depth=depth, hip_precision=prec)
    m.update(mods)
    return {"modules": m}


def _host_chain(frame: np.ndarray, box, S: int) -> torch.Tensor:
    """The chain the kernel replaces, on the host: zero-padded integer crop, ToTensor (/ 255 in fp32), antialiased bilinear resize,
    clamp -- the arithmetic of the fixture's stand-ins (the fixture itself holds no 224 x 224 output: it must stay below 1 MiB)."""
    x0, y0, x1, y1 = box
    H, W, _ = frame.shape
    crop = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
    vx0, vx1, vy0, vy1 = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
    crop[vy0 - y0:vy1 - y0, vx0 - x0:vx1 - x0] = frame[vy0:vy1, vx0:vx1]
    t = torch.from_numpy(crop).permute(2, 0, 1).float().div(255)
    return torch.nn.functional.interpolate(t[None], (S, S), mode="bilinear", antialias=True, align_corners=False)[0].clamp(0.0, 1.0)


@pytest.mark.parametrize("graph", [False, True])
def test_forward_from_frames_matches_forward_from_images(hip, golden, graph):
    from boxdreamer_amd.model import BoxDreamer
    model = BoxDreamer(_config(hip_graph=graph))
    model.load_state_dict({"decoder." + k: v for k, v in synth.betr_state_dict(1234, 2).items()}, strict=True)
    model = model.cuda().eval()
    B, T = 2, 3
    frame = golden["frame_0"]
    frames = torch.from_numpy(frame)[None].cuda()
    batches = ([[[20, 10, 240, 230], [96, 8, 320, 232], [-30, -40, 300, 290]], [[100, 50, 190, 140], [0, 0, 240, 240], [150, 60, 330, 240]]],
               [[[25, 12, 240, 227], [90, 8, 314, 232], [-10, -40, 320, 290]], [[100, 50, 200, 150], [0, 0, 239, 239], [150, 60, 320, 230]]])
    for rnd, bl in enumerate(batches):       # (with hip_graph the second round writes into the captured graph's static image buffer)
        boxes = torch.tensor(bl, dtype=torch.int32, device="cuda")
        fidx = torch.zeros((B, T), dtype=torch.int32, device="cuda")
        base = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.make_batch(seed=11 + rnd, B=B, T=T).items() if k != "images"}
        base["query_idx"] = torch.tensor([2, 0])
        images = pp.crop_resize_frames(frames, boxes, frame_idx=fidx)
        a = model({**base, "frames": frames, "crop_boxes": boxes, "frame_idx": fidx})
        got = {k: a[k].clone() for k in ("pred_bbox", "pred_corners_px", "regression_boxes", "pred_poses")}
        assert torch.equal(a["images"], images)
        if graph and rnd == 1:
            assert a["images"].data_ptr() == model._graph.images.data_ptr()
        logits_a = model.decoder.last_logits.clone()
        b = model({**base, "images": images.clone()})
        for k, v in got.items():
            assert torch.equal(v, b[k]), (graph, rnd, k)
        assert torch.equal(logits_a, model.decoder.last_logits)
        host = torch.stack([torch.stack([_host_chain(frame, bx, 224) for bx in row]) for row in bl]).cuda()
        print(f"[preprocess] images: max |kernel - host chain| = {(host - images).abs().max().item():.2e}")
        model({**base, "images": host})
        d = (model.decoder.last_logits - logits_a).abs().max().item()
        print(f"[preprocess] hip_graph={graph} round {rnd}: heat-map logits, frames on the device vs host-made images: max abs diff {d:.2e} (budget 1e-3)")
        assert d <= 1e-3
