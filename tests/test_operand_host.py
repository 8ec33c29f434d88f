"""Host: the operand-buffer layout (boxdreamer_amd/operand.py) and the precision-traits table behind it (_lib.TRAITS), on CPU tensors;
and the reference packer (hip_ops.to_operand) against an integer restatement of its roundings on the steered tables that
tests/test_gpu_range.py feeds to every kernel that stores a 16/8-bit operand."""
import functools

import numpy as np
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, operand, synth

CLASSES = ["bf16", "f16", "fp8", "bf16x3", "f16x3", "f16c8"]
# bytes of one 64-column row over all planes (include/boxdreamer_hip.h): one 16-bit plane; one e4m3 plane; two 16-bit planes; F16C8 =
# an f16 plane + one byte per element -- the "3 bytes per element against 7" of cache.py (the 7: with an fp32 copy next to it)
ROW_BYTES_64 = [128, 128, 64, 256, 256, 192]
bf16, f16, e4m3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# name -> (planes, op_dtype, operand_prec, k_multiple): what the if-chains this table replaced returned for every name
TRAITS = {"bf16": (1, bf16, 0, 64), "fp16": (1, f16, 1, 64), "f16": (1, f16, 1, 64), "bf16x3": (2, bf16, 2, 64), "fp8": (1, e4m3, 4, 128),
          "bf16x3_attn_x3": (2, bf16, 2, 64), "f16c8": (2, f16, 8, 64), "f16c8_qk16": (2, f16, 8, 64), "f16x3": (2, f16, 14, 64),
          "f16x3_attn_x3": (2, f16, 14, 64), "fp8_mixed": (1, e4m3, 4, 128)}


def test_traits_table_matches_the_literal_values():
    assert set(TRAITS) == set(_lib.PREC_NAMES)
    for name, want in TRAITS.items():
        assert (_lib.planes(name), _lib.op_dtype(name), _lib.operand_prec(name), _lib.k_multiple(name)) == want, name
        pid = _lib.prec_id(name)
        assert (_lib.planes(pid), _lib.op_dtype(pid), _lib.operand_prec(pid), _lib.k_multiple(pid)) == want, name
    for attention_only in (3, 5, 9, 10, 16, 17):           # no operand class: the lookups refuse them (the if-chains fell through to bf16)
        assert attention_only not in _lib.TRAITS
        for fn in (_lib.planes, _lib.op_dtype, _lib.operand_prec, _lib.k_multiple):
            with pytest.raises(ValueError):
                fn(attention_only)


@pytest.mark.parametrize("name", CLASSES)
def test_operand_buffers(name):
    cls, cols = _lib.prec_id(name), 64
    x = torch.randn(3, cols) * 3.0
    src = hip_ops.to_operand(x, cls)
    two = _lib.planes(cls) == 2

    t = operand.empty(cls, 3, cols, "cpu")
    assert t.shape == src.shape and t.dtype == src.dtype
    assert operand.empty(cls, 3, cols, "cpu", zero=True).view(torch.uint8).count_nonzero() == 0
    big = operand.empty(cls, 11, cols, "cpu", zero=True)              # more rows than are used: the planes are the CAPACITY apart
    for buf in (t, big):
        assert operand.plane_offset(buf, cls) == (buf[0].numel() if two else 0)
    assert operand.plane_offset(big, cls) == (11 * cols if two else 0)

    views = operand.row_planes(big, cls, 8)
    assert len(views) == _lib.planes(cls) and all(tuple(v.shape) == (8, cols) for v in views)
    assert views[0].dtype == _lib.op_dtype(cls)
    if two:
        assert views[1].dtype == (torch.uint8 if name == "f16c8" else _lib.op_dtype(cls))
        # a view, not a copy, at the head of plane-1 storage
        assert views[1].data_ptr() == big[1].data_ptr()
    assert views[0].data_ptr() == big.data_ptr()

    if name == "f16c8":                                                # the unused tail of the source's plane 1: poison it
        src[1].view(torch.uint8).reshape(-1)[3 * cols:] = 0x7F
    operand.copy_rows(big, 5, src, 3, cls)
    got = operand.empty(cls, 3, cols, "cpu", zero=True)
    for d, s in zip(operand.row_planes(got, cls, 3), operand.row_planes(big, cls, 8)):
        d.copy_(s[5:])
    assert torch.equal(hip_ops.from_operand(got, cls), hip_ops.from_operand(hip_ops.to_operand(x, cls), cls))
    if name == "f16c8":
        assert not (big[1].view(torch.uint8) == 0x7F).any()            # no poisoned byte arrived
    # ... and nothing but rows [5, 8) was written
    for v in operand.row_planes(big, cls, 11):
        raw = v.contiguous().view(torch.uint8).reshape(11, -1)
        assert raw[:5].count_nonzero() == 0 and raw[8:].count_nonzero() == 0 and raw[5:8].count_nonzero() > 0

    assert operand.row_bytes(cls, 64) == ROW_BYTES_64[CLASSES.index(name)]
    assert operand.row_bytes(cls, 64) * 11 <= big.numel() * big.element_size()


# ------------------------------------------------------------------------------------------------------------------ steered tables
# The RANGE contract (csrc/bd_common.h): every fp32 -> 16/8-bit store rounds to nearest even and SATURATES at the class's largest finite
# value.  One table of fp32 values per operand class, steered at the places where a conversion can go wrong; tests/test_gpu_range.py
# puts it in front of every store of every kernel and expects hip_ops.to_operand(table), bit for bit.  Here the packer itself is
# pinned against a second restatement of the rounding, written with integer arithmetic on the fp32 bit patterns.
RANGE_CLASSES = ["bf16", "fp16", "bf16x3", "f16x3", "fp8", "f16c8"]
# element format -> (explicit mantissa bits, exponent of the smallest normal, largest finite value)
FORMATS = {"bf16": (7, -126, float.fromhex("0x1.fep127")), "f16": (10, -14, 65504.0), "e4m3": (3, -6, 448.0)}
BASE_FORMAT = {"bf16": "bf16", "bf16x3": "bf16", "fp16": "f16", "f16x3": "f16", "f16c8": "f16", "fp8": "e4m3"}
# binades (exponent of the lower neighbour) that get a pair of rounding ties: the smallest normal binade, the largest, and some between
BINADES = {"bf16": (-126, -100, -40, -1, 0, 40, 100, 127), "f16": (-14, -9, -4, -1, 0, 3, 9, 15), "e4m3": (-6, -4, -2, -1, 0, 3, 6, 8)}
TABLE_LEN = 768           # 8 x 96: fits the N of every GEMM form; the steered values fill less than the first 192 entries
STEERED_MAX = 192
F32_MAX = float(np.finfo(np.float32).max)


def _around(x):
    """x and its two fp32 neighbours"""
    x = np.float32(x)
    return [x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(np.inf))]


def _steered_positive(prec):
    fmt = BASE_FORMAT[prec]
    m, emin, vmax = FORMATS[fmt]
    sub = 2.0 ** (emin - m)                                    # the smallest subnormal = the subnormal quantum
    v = [0.0, sub, 0.5 * sub, 1.5 * sub, 2.0 ** emin, 2.0 ** emin - sub]
    for j in (2, 3):                                           # ties between two subnormals, lower neighbour even / odd, +- one fp32 ulp
        v += _around((j + 0.5) * sub)
    for e in BINADES[fmt]:
        ulp = 2.0 ** (e - m)
        for j in (2, 3):                                       # ties between two normals of the binade, lower neighbour even / odd
            v += _around((2 ** m + j + 0.5) * ulp)
    v.append(vmax)
    if fmt != "bf16":                                          # (fp32's largest values round to Inf in bf16 in the reference too)
        top = 2.0 ** (int(np.floor(np.log2(vmax))) - m)
        v += _around(vmax + 0.5 * top)                         # 65520 / 464: the first value that rounds past MAX, and its neighbours
        v += [7e4, 1e5, 3e9, F32_MAX]
    if prec == "f16c8":
        v += [511.99, 512.0, 513.0, 1000.0,
              1 + 17 * 2.0 ** -16, 1 + 19 * 2.0 ** -16,        # (x - hi) 2^11 = 17/32, 19/32: e4m3 ties, lower neighbour even / odd
              100 + 34 * 2.0 ** -11, 100 + 38 * 2.0 ** -11,    # ... = 34, 38: ties between 32 | 36 and 36 | 40
              1 + 2.0 ** -20, 1 + 2.0 ** -21,                  # ... = e4m3's smallest subnormal, and half of it (ties to zero)
              512.24, 1024.49, 40015.0]                        # ... beyond 448: the residual an f16 ulp leaves above 512
    if prec in ("bf16x3", "f16x3"):
        hi0 = 2.0 ** (emin + 6)                                # ulp(hi0) = 64 sub: lo below is a subnormal of the class
        v += [np.pi, 1.0 / 3.0, 1 + 2.0 ** -12, 1000.123, 3e-5,          # both planes in use
              hi0 + 8 * sub, hi0 + 2.5 * sub, hi0 + 3.5 * sub]           # lo subnormal: exact, tie (even below), tie (odd below)
    return np.asarray(v, dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _steered_table_np(prec):
    pos = _steered_positive(prec)
    assert 2 * len(pos) <= STEERED_MAX, (prec, len(pos))
    t = np.empty(TABLE_LEN, dtype=np.float32)
    t[0:2 * len(pos):2] = pos
    t[1:2 * len(pos):2] = -pos
    t[2 * len(pos):] = synth.bell_np("range_fill", (TABLE_LEN - 2 * len(pos),), 3.0, 0.0, 17).astype(np.float32)
    assert np.isfinite(t).all()
    return t


def steered_table(prec, n=TABLE_LEN):
    """fp32 [n] (host): the class's steered values with both signs, then bell-shaped filler of a few units; tiled to n > 768.  Any
    n >= 192 holds every steered value."""
    t = _steered_table_np(prec)
    assert n >= STEERED_MAX
    return torch.from_numpy(np.resize(t, n).copy())


def steered_count(prec):
    return 2 * len(_steered_positive(prec))


def round_bits(x, fmt):
    """fp32 array -> float64 array of the values nearest-even rounding to `fmt` gives, saturated at the format's largest finite value:
    integer arithmetic on the fp32 bit patterns (no floating-point conversion is involved until the exact result is written down)."""
    m, emin, vmax = FORMATS[fmt]
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    neg, ex, man = (u >> 31) != 0, (u >> 23) & 0xFF, u & 0x7FFFFF
    assert (ex != 255).all(), "finite inputs only"
    sig = np.where(ex > 0, man | (1 << 23), man)              # |x| = sig 2^e
    e = np.maximum(ex, 1) - 150
    length = np.zeros_like(sig)
    t = sig.copy()
    while t.any():
        length += t > 0
        t >>= 1
    q = np.maximum(length - 1 + e - m, emin - m)              # exponent of the result's last place: normal, or the subnormal quantum
    sh = q - e
    assert (sh >= 1).all()
    sh = np.minimum(sh, 40)                                   # (sig < 2^24: everything from 26 on shifts it out whole)
    quot, rem, half = sig >> sh, sig & ((np.int64(1) << sh) - 1), np.int64(1) << (sh - 1)
    quot = quot + ((rem > half) | ((rem == half) & ((quot & 1) == 1)))
    val = np.minimum(np.ldexp(quot.astype(np.float64), q.astype(np.int64)), vmax)
    return np.where(neg, -val, val) + np.where(neg & (val == 0), -0.0, 0.0)


def restated_planes(x, prec):
    """the planes of the operand class as float64 arrays of exactly representable values (F16C8: plane 1 = the e4m3 value of lo8)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fmt = BASE_FORMAT[prec]
    hi = round_bits(x, fmt)
    if _lib.planes(prec) == 1:
        return [hi]
    rest = (x.astype(np.float64) - hi).astype(np.float32)     # the fp32 subtraction (exact wherever hi did not saturate)
    if prec == "f16c8":
        scaled = np.clip(rest.astype(np.float64) * 2.0 ** _lib.F16C8_D, -448.0, 448.0)
        return [hi, round_bits(scaled.astype(np.float32), "e4m3")]
    return [hi, round_bits(rest, fmt)]


_TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.float8_e4m3fn}


def _plane_bits(t):
    return t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16)


@pytest.mark.parametrize("prec", RANGE_CLASSES)
def test_packer_matches_the_integer_restatement_on_the_steered_table(prec):
    table = steered_table(prec)
    assert table.numel() % 96 == 0 and table.numel() <= 768 and torch.isfinite(table).all()
    fmt = BASE_FORMAT[prec]
    want = [torch.from_numpy(p).float().to(_TORCH[fmt]) for p in restated_planes(table.numpy(), prec)]
    got = hip_ops.to_operand(table[None, :], prec)
    if _lib.planes(prec) == 1:
        got = [got[0]]
    elif prec == "f16c8":
        lo8 = got[1].contiguous().view(torch.uint8).reshape(-1)[:table.numel()]
        # byte 16 h + 8 a + j of every 32-block holds k = 16 a + 8 h + j (csrc/bd_common.h: f16c8_lo_index), stated here on its own
        k_of_byte = torch.tensor([32 * blk + 16 * a + 8 * h + j for blk in range(table.numel() // 32) for h in (0, 1) for a in (0, 1) for j in range(8)])
        want[1] = torch.from_numpy(restated_planes(table.numpy(), prec)[1]).float().to(torch.float8_e4m3fn)[k_of_byte]
        got = [got[0][0], lo8.view(torch.float8_e4m3fn)]
    else:
        got = [got[0][0], got[1][0]]
    for p, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g.float()).all(), f"{prec}: plane {p} of the expectation is not finite"
        bad = (_plane_bits(g) != _plane_bits(w)).nonzero().reshape(-1)
        assert bad.numel() == 0, f"{prec} plane {p}: {bad.numel()} values differ, the first at table[{int(bad[0])}]"
    # the table really holds what it is for: values that saturate, ties, subnormals of the class
    m, emin, vmax = FORMATS[fmt]
    t = table.double().abs()
    assert (t > vmax).any() == (fmt != "bf16") and (t == vmax).any() and ((t > 0) & (t < 2.0 ** emin)).any()
    assert (table[:steered_count(prec):2] == -table[1:steered_count(prec):2]).all()
