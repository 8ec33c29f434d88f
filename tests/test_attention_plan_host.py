"""CPU: bd_attention_plan against what the attention entry points of the commit before plan_attention launched.

tests/golden/attention_forms.json was recorded from that commit by tools/make_golden_attention_forms.py (its docstring describes the
layout); it is never regenerated from the code under test.  A case = (entry point and its integer arguments, pointers, prec,
latency_forms)."""
import ctypes as C
import json
import os

import pytest

from boxdreamer_amd import _lib, build

FAMILIES = (_lib.ATTN_FAMILY_TILED, _lib.ATTN_FAMILY_PP)


@pytest.fixture(scope="module")
def forms(golden_dir):
    with open(os.path.join(golden_dir, "attention_forms.json")) as f:
        return json.load(f)


def instances(lib, family):
    key, rows = (C.c_int * _lib.ATTN_KEY_LEN)(), []
    while lib.bd_attention_instance(family, len(rows), key):
        rows.append(list(key))
    return rows


def cases(forms):
    """(call, pointers, recorded outcome index, description) of every fixture case."""
    for shape, ptrs, lats, idx in forms["groups"]:
        qkv, out, view_start, _ = forms["pointers"][ptrs]
        it = iter(idx)
        for prec in forms["precs"]:
            for lat in lats:
                call = _lib.AttnCall(**{**forms["defaults"], **shape}, prec=prec, latency_forms=lat)
                yield call, (qkv, out, view_start), next(it), (shape, ptrs, prec, lat)


def test_instance_tables_list_every_kernel_once():
    """45 + 12 distinct rows, and together exactly the attn_kernel* entries of the build's resource report."""
    lib = _lib.load()
    key = (C.c_int * _lib.ATTN_KEY_LEN)()
    tables = {}
    for fam, n in zip(FAMILIES, (45, 12)):
        rows = tables[fam] = instances(lib, fam)
        assert len(rows) == n and len({tuple(r) for r in rows}) == n
        assert not lib.bd_attention_instance(fam, n, key) and not lib.bd_attention_instance(fam, -1, key)
    assert not lib.bd_attention_instance(0, 0, key) and not lib.bd_attention_instance(3, 0, key)
    ty, b = ("DF16b", "DF16_"), lambda v: f"Lb{v}E"
    want = {f"attn_kernelI{ty[t]}Li{ns}ELi{hd}ELi{nw}ELi{om}E{b(vl)}E" for t, ns, hd, nw, om, vl in tables[_lib.ATTN_FAMILY_TILED]}
    want |= {f"attn_kernel_ppI{ty[t]}Li{hd}ELi{om}E{b(vl)}E" for t, hd, om, vl, _, _ in tables[_lib.ATTN_FAMILY_PP]}
    with open(build.RESOURCES) as f:
        built = [k for k in json.load(f) if "attn_kernel" in k]
    assert len(built) == 57
    for name in built:                                  # _ZN12_GLOBAL__N_1<len>attn_kernel...I<arguments>EEv<parameter>
        hit = [w for w in want if f"{w}Ev" in name and name.split(w)[0][-1].isdigit()]
        assert len(hit) == 1, name
        want.remove(hit[0])
    assert not want


def test_plan_equals_the_recorded_dispatch(forms):
    """Every fixture case: the recorded return code, or the recorded launch (instance, grid, block, q_len, q_off, out_rows).  The row a
    launch names is the table row with the launch's key; a refusal leaves no launch."""
    lib = _lib.load()
    plan = _lib.AttnPlan()
    tables = {fam: instances(lib, fam) for fam in FAMILIES}
    outcomes = [o if isinstance(o, int) else forms["kernels"][o[0]] + o[1:] for o in forms["outcomes"]]
    n = 0
    for call, ptrs, oc, where in cases(forms):
        plan.n_launches = 7
        rc = lib.bd_attention_plan(C.byref(call), *ptrs, C.byref(plan))
        l = plan.launch[0]
        if rc != 0:
            assert plan.n_launches == 0, where
            got = rc
        else:
            assert plan.n_launches == 1 and tables[l.family][l.row] == list(l.key), where
            got = [l.family, *l.key, l.grid, l.block, l.q_len, l.q_off, l.out_rows]
        assert got == outcomes[oc], where
        n += 1
    assert n == forms["cases"] and n > 6000
    ptrs = forms["pointers"]["ok"][:3]
    assert lib.bd_attention_plan(None, *ptrs, C.byref(plan)) == -5 and plan.n_launches == 0
    assert lib.bd_attention_plan(C.byref(call), *ptrs, None) == -5
    call.entry = 4                                         # no such entry point
    assert lib.bd_attention_plan(C.byref(call), *ptrs, C.byref(plan)) == -1 and plan.n_launches == 0


def test_every_table_row_is_reached(forms):
    """Every instantiated kernel is named by a fixture case: there is no row that the entry points before plan_attention could not
    reach (a row that only latency_forms selects would show here: the tiled 4-wave rows it picks serve other shapes too)."""
    lib = _lib.load()
    reached = {tuple(k) for k in forms["kernels"]}
    assert {(fam, *row) for fam in FAMILIES for row in instances(lib, fam)} == reached


def test_gpu_tests_launch_every_table_row():
    """The rows the GPU tests reach, collected from the plans they assert before their launches (the same functions, called here for
    every parametrisation): tests/test_gpu_range.py's V-row test runs every uniform instance, tests/test_gpu_ragged.py the ragged
    ping-pong instances and the split-bf16 ragged ones, and the remaining six -- the one-plane classes' ragged attn_kernel instance -- are
    the _ROW_CASES of test_attention_online_softmax_steered.  No row is selected by latency_forms alone (that flag moves a call from the
    ping-pong kernel to the 4-wave instance of its class; the forward of tests/test_gpu_path.py's latency test runs it)."""
    import test_gpu_ragged as ragged
    import test_gpu_range as rng
    import test_gpu_steered as steered
    lib = _lib.load()
    fam = {"tiled": _lib.ATTN_FAMILY_TILED, "pp": _lib.ATTN_FAMILY_PP}
    row = lambda p: (fam[p["kernel"]], *p["key"])
    every = {(f, *r) for f in FAMILIES for r in instances(lib, f)}
    uniform = {row(p) for v in rng._PREFIX_VARIANTS for seq, hd in rng.V_ROW_SHAPES for p in rng.v_row_plans(v, seq, hd)}
    assert uniform == {r for r in every if not r[1 + (5 if r[0] == _lib.ATTN_FAMILY_TILED else 3)]}          # (VL is a key's last argument)
    rag = {row(p) for v in ragged.VARIANTS for counts, _ in ragged.VARLEN_BATCHES for p in ragged.varlen_plans(v, counts)}
    rest = every - uniform - rag
    cases = [row(steered.steered_plan(*c)) for c in steered._ROW_CASES]
    assert len(rest) == 6 and sorted(cases) == sorted(rest)
    assert {row(steered.steered_plan(*c)) for c in steered._STEERED} <= every


def test_fixture_covers_the_rules(forms, golden_dir):
    """The grid the fixture must keep when it is recorded again: every entry point, q_view and prefix_queries both ways, the accepted and
    the GEMM-only classes, latency_forms both ways, every return code, and a refusal for each pointer."""
    assert len(forms["revision"]) == 40
    shapes = [{**forms["defaults"], **g[0]} for g in forms["groups"]]
    assert {s["entry"] for s in shapes} == {0, 1, 2, 3}
    assert {(s["entry"], s["has_q_view"]) for s in shapes} >= {(1, 0), (1, 1), (3, 0), (3, 1)}
    assert {s["prefix_queries"] for s in shapes if s["entry"] == 2} == {0, 1}
    assert {s["head_dim"] for s in shapes} >= {64, 96, 80, 0}
    assert set(forms["precs"]) == {0, 1, 2, 3, 5, 9, 10, 16, 17, 4, 8, 14}
    assert {lat for g in forms["groups"] for lat in g[2]} == {0, 1}
    assert {o for o in forms["outcomes"] if isinstance(o, int)} == {-1, -2, -3, -5}
    assert {g[1] for g in forms["groups"]} == set(forms["pointers"])
    assert os.path.getsize(os.path.join(golden_dir, "attention_forms.json")) < 101045
