"""Host: the operand-buffer layout (boxdreamer_amd/operand.py) and the precision-traits table behind it (_lib.TRAITS), on CPU tensors."""
import pytest
import torch

from boxdreamer_amd import _lib, hip_ops, operand

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
