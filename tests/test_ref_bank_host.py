"""CPU: the reference bank's host side -- the `ref_rows` table helpers next to `packing_index` (_lib.ref_rows_table, check_ref_rows,
gather_sources), the operand-only feature carrier, and bd_gather_view_rows' argument validation, which runs before any launch and so
on a box without a GPU."""
import pytest
import torch

from boxdreamer_amd import _lib, features


def _tables(rows, counts, t_max, bank_len):
    table = _lib.ref_rows_table(rows, len(counts), t_max)
    _lib.check_ref_rows(table, counts, bank_len)
    return _lib.gather_sources(table, counts, t_max)


def test_tables_uniform_batch():
    # B = 2, T = 3, query slot 1 / 2: bank rows elsewhere
    src, encode = _tables([[0, -1, 1], [2, 3, -1]], [3, 3], 3, 4)
    assert src == [0, -1, 1, 2, 3, -2]
    assert encode == [1, 5]                       # flat indices into the B * T padded slots, in the order the encoder packs them


def test_tables_ragged_batch():
    rows = [[0, -1, 1, 9, 9], [-1, 2, 9, 9, 9], [3, 4, 5, 6, -1]]
    src, encode = _tables(rows, [3, 2, 5], 5, 7)
    assert src == [0, -1, 1, -2, 2, 3, 4, 5, 6, -3]
    assert encode == [1, 5, 14]
    assert len(src) == sum([3, 2, 5]) and [s for s in src if s < 0] == [-1, -2, -3]
    # the packed order IS packing_index's order: view v of src sits at padded slot packing_index[v]
    index = _lib.packing_index([3, 2, 5], 5)
    assert [index[v] for v, s in enumerate(src) if s < 0] == encode


def test_tables_bank_row_shared_by_two_samples():
    src, encode = _tables(torch.tensor([[0, 1, -1], [-1, 1, 0]]), [3, 3], 3, 2)
    assert src == [0, 1, -1, -2, 1, 0] and encode == [2, 3]


def test_tables_all_fresh_is_the_identity_over_fresh_views():
    counts = [3, 2, 5]
    src, encode = _tables([[-1] * 5] * 3, counts, 5, 0)
    assert src == [-(k + 1) for k in range(sum(counts))]
    assert encode == _lib.packing_index(counts, 5)


def test_padded_slots_are_ignored_whatever_they_hold():
    junk = [[0, -1, 10 ** 9], [-1, 1, -77]]
    a = _tables(junk, [2, 2], 3, 2)
    b = _tables([[0, -1, -1], [-1, 1, -1]], [2, 2], 3, 2)
    assert a == b == ([0, -1, -2, 1], [1, 3])


def test_validation_errors():
    with pytest.raises(TypeError):                # a tensor that is not on the CPU (checked by device type: a meta tensor stands in)
        _lib.ref_rows_table(torch.zeros((2, 3), dtype=torch.int64, device="meta"), 2, 3)
    with pytest.raises(TypeError):
        _lib.ref_rows_table(torch.zeros((2, 3)), 2, 3)               # floating point
    with pytest.raises(TypeError):
        _lib.ref_rows_table([[0, 1.5, -1], [0, 1, -1]], 2, 3)
    for bad in (torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 3), dtype=torch.int64), torch.zeros(6, dtype=torch.int64),
                [[0, 1, -1]], [[0, 1, -1], [0, 1]]):
        with pytest.raises(ValueError):
            _lib.ref_rows_table(bad, 2, 3)
    table = _lib.ref_rows_table([[0, 4, -1], [0, 1, -1]], 2, 3)
    with pytest.raises(ValueError):
        _lib.check_ref_rows(table, [3, 3], 4)                        # entry == len(bank)
    _lib.check_ref_rows(table, [3, 3], 5)
    with pytest.raises(ValueError):
        _lib.check_ref_rows(_lib.ref_rows_table([[0, -2, -1], [0, 1, -1]], 2, 3), [3, 3], 5)     # < -1 in a valid slot
    with pytest.raises(ValueError):
        _lib.check_ref_rows(_lib.ref_rows_table([[0, -1, -1], [0, -1, -1]], 2, 3), [3, 3], 0)    # an empty bank holds no row 0


def test_operand_only_carrier():
    op = torch.zeros((2, 12, 16), dtype=torch.float16)
    f = features.OperandOnly((3, 4, 16), op, _lib.PREC_F16C8, stamp=("s",))
    assert f.shape == (3, 4, 16) and f.dim() == 3 and f.numel() == 192 and f.device == op.device and f.stamp == ("s",)
    assert f.checked(_lib.PREC_F16C8, 2 * 192, op.device) is op
    with pytest.raises(ValueError, match="operand class"):
        f.checked(_lib.PREC_F16X3, 2 * 192, op.device)               # the adapter's fc1 got promoted: nothing to re-cast from
    with pytest.raises(ValueError):
        f.checked(_lib.PREC_F16C8, 192, op.device)
    with pytest.raises(ValueError):
        f.checked(_lib.PREC_F16C8, 2 * 192, torch.device("meta"))


def _call(lib, bank=0x10000000, bank_plane=0, bank_views=4, fresh=0x20000000, fresh_plane=0, n_fresh=3, src=0x30000000, out=0x40000000, out_plane=0,
          n_views=7, P=256, dim=768, prec=_lib.PREC_BF16, b32=None, f32=None, o32=None):
    # (made-up addresses: every case below is rejected -- or, n_views = 0, accepted -- before anything is launched or dereferenced)
    return lib.bd_gather_view_rows(bank, bank_plane, bank_views, fresh, fresh_plane, n_fresh, src, out, out_plane, n_views, P, dim, prec,
                                   b32, f32, o32, None)


def test_gather_view_rows_validates_before_any_launch():
    lib = _lib.load()
    assert lib.bd_abi_version() == 9
    assert "bd_gather_view_rows" in _lib.EXPORTS
    assert lib.bd_gather_view_rows(None, 0, 0, None, 0, 0, None, None, 0, 0, 0, 0, 0, None, None, None, None) == -5
    assert _call(lib, bank=None) == -5 and _call(lib, fresh=None) == -5 and _call(lib, src=None) == -5 and _call(lib, out=None) == -5
    assert _call(lib, o32=0x50000000) == -5                               # an fp32 output without fp32 sources
    assert _call(lib, bank=None, bank_views=0, n_views=0) == 0        # a table may be NULL when it holds no view
    assert _call(lib, n_views=0) == 0                                 # nothing to do: BD_OK without a launch
    assert _call(lib, P=3, dim=8) == -3                               # P * dim = 24: a view is not whole 16-byte chunks
    assert _call(lib, P=5, dim=48, n_views=0) == 0                    # 240 is
    assert _call(lib, out=0x40000008) == -3 and _call(lib, bank=0x10000004) == -3 and _call(lib, fresh=0x20000002) == -3
    e = 256 * 768
    planes = dict(bank_plane=8 * e, fresh_plane=8 * e, out_plane=8 * e)
    for prec in (_lib.PREC_BF16X3, _lib.PREC_F16X3, _lib.PREC_F16C8):
        assert _call(lib, prec=prec, n_views=0, **planes) == 0
        for k in planes:                                              # a plane offset of 16-bit elements that is not 16-byte aligned
            assert _call(lib, prec=prec, **dict(planes, **{k: 8 * e + 4})) == -3, (prec, k)
    assert _call(lib, prec=_lib.PREC_BF16, n_views=0, bank_plane=3) == 0      # one-plane classes ignore the plane offsets
    assert _call(lib, b32=0x50000004, f32=0x60000000, o32=0x70000000) == -3
    for prec in (_lib.PREC_F16C8_QK16, _lib.PREC_BF16_OUT_FP8, 99, -1):       # whole-path ids and attention codes are not operand classes
        assert _call(lib, prec=prec) == -2
    assert _call(lib, n_views=-1) == -1 and _call(lib, bank_views=-1) == -1 and _call(lib, n_fresh=-2) == -1
    for prec in (_lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_FP8):
        assert _call(lib, prec=prec, n_views=0) == 0
    # out may not overlap a source (its first byte, or its last view reaching into the bank), in either copy; plane 1 may not start
    # inside plane 0
    v = 256 * 768 * 2
    assert _call(lib, out=0x10000000) == -1 and _call(lib, out=0x10000000 + 3 * v) == -1 and _call(lib, out=0x10000000 - 7 * v + 16) == -1
    assert _call(lib, out=0x20000000 + 2 * v) == -1
    assert _call(lib, out=0x10000000 + 4 * v, n_views=0) == 0 and _call(lib, out=0x10000000, bank=0x40000000, n_views=0) == 0
    assert _call(lib, b32=0x50000000, f32=0x60000000, o32=0x60000000 + 2 * v) == -1
    assert _call(lib, prec=_lib.PREC_F16C8, bank_plane=8 * e, fresh_plane=8 * e, out_plane=6 * e) == -1
