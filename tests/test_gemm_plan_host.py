"""CPU: bd_gemm_plan against what the dispatch chains of the commit before the plan functions launched.

tests/golden/gemm_forms.json was recorded from that commit by tools/make_golden_gemm_forms.py (its docstring describes the layout); it is
never regenerated from the code under test.  A case = (prec, epilogue variant, N, K, M, cus, concurrent launches)."""
import ctypes as C
import itertools
import json
import os

import pytest

from boxdreamer_amd import _lib

FAMILIES = (_lib.GEMM_FAMILY_PC, _lib.GEMM_FAMILY_GLDS, _lib.GEMM_FAMILY_PC_F16C8)
EP_INDEX = {_lib.GEMM_FAMILY_PC: 8, _lib.GEMM_FAMILY_PC_F16C8: 1}        # where a key holds EP; LNF follows at 12 / 7
LNF_INDEX = {_lib.GEMM_FAMILY_PC: 12, _lib.GEMM_FAMILY_PC_F16C8: 7}


@pytest.fixture(scope="module")
def forms(golden_dir):
    with open(os.path.join(golden_dir, "gemm_forms.json")) as f:
        return json.load(f)


def shapes_of(forms, group):
    """(entry, N, K, M) of every shape of a group (the run-length coding of the entry list undone)."""
    prec, variant, sname, rle = group
    entries = []
    for e in rle:
        entries.extend([entries[-1]] * -e if e < 0 else [e])
    s = forms["shapes"][sname]
    shapes = list(itertools.product(s["N"], s["K"], s["M"]))
    assert len(shapes) == len(entries)
    return [(forms["entries"][e], *nkm) for e, nkm in zip(entries, shapes)]


def gemm_args(forms, variant, N, K, M):
    g = _lib.GemmArgs()
    for k, v in {**forms["base"], **forms["variants"][variant]}.items():
        setattr(g, k, v)
    g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.ldr, g.ln_op_ld = M, N, K, K, K, N, N, N
    g.rms_eps = g.ln_eps = 1e-6
    return g


def plan_of(lib, g, prec, cus, conc, plan):
    """bd_gemm_plan in the fixture's terms: a negative return code, or [[family, key..., grid, block, row0, rows, split_k], ...]."""
    rc = lib.bd_gemm_plan(C.byref(g), prec, cus, conc, C.byref(plan))
    if rc != 0:
        assert plan.n_launches == 0
        return rc
    return [[l.family, *l.key, l.grid, l.block, l.row0, l.rows, l.split_k] for l in plan.launch[:plan.n_launches]]


def instances(lib, family):
    key, rows = (C.c_int * _lib.GEMM_KEY_LEN)(), []
    while lib.bd_gemm_instance(family, len(rows), key):
        rows.append(list(key))
    return rows


def test_instance_tables_list_every_kernel_once():
    lib = _lib.load()
    key = (C.c_int * _lib.GEMM_KEY_LEN)()
    for fam, n in zip(FAMILIES, (39, 28, 50)):                       # the kernels of each family in the build's resource report
        rows = instances(lib, fam)
        assert len(rows) == n and len({tuple(r) for r in rows}) == n
        assert not lib.bd_gemm_instance(fam, n, key) and not lib.bd_gemm_instance(fam, -1, key)
    assert not lib.bd_gemm_instance(0, 0, key) and not lib.bd_gemm_instance(4, 0, key)


def test_plan_equals_the_recorded_dispatch(forms):
    """Every fixture case: the recorded return code or the recorded launches (instance, grid, block, row range, split factor), and both
    predicates' recorded answers.  The row a launch names is the table row with the launch's key."""
    lib = _lib.load()
    plan = _lib.GemmPlan()
    tables = {fam: instances(lib, fam) for fam in FAMILIES}
    outcomes = [o if isinstance(o, int) else [forms["kernels"][l[0]] + l[1:] for l in o] for o in forms["outcomes"]]
    n = 0
    for group in forms["groups"]:
        prec, variant = group[0], group[1]
        for (ln, rms, per_dev), N, K, M in shapes_of(forms, group):
            g = gemm_args(forms, variant, N, K, M)
            where = (prec, variant, N, K, M)
            assert lib.bd_gemm_takes_ln_fold(C.byref(g), prec) == ln, where
            assert lib.bd_gemm_fuses_qk_rmsnorm(C.byref(g), prec) == rms, where
            for (cus, conc), oc in zip(forms["devices"], per_dev):
                got = plan_of(lib, g, prec, cus, conc, plan)
                assert got == outcomes[oc], (where, cus, conc)
                for l in plan.launch[:plan.n_launches]:
                    assert tables[l.family][l.row] == list(l.key)
                n += 1
    assert n == forms["cases"] and n > 50000


def test_every_table_row_is_reached(forms):
    """Every instantiated kernel is named by a fixture case, except the rows no argument set selected before the plan functions either
    (listed here with the reason; they stay instantiated)."""
    lib = _lib.load()
    reached = {tuple(k) for k in forms["kernels"]}
    missing = {(fam, *row) for fam in FAMILIES for row in instances(lib, fam)} - reached
    # gemm_kernel_pc <two-plane or e4m3 class, EP 3, fp32, RING 0>: the fp32-residual epilogue leaves the operand ring only in the one-plane
    # 16-bit classes (ring0_ep3), the template is instantiated for every class
    unreachable = {(_lib.GEMM_FAMILY_PC, tc, ns, bk, 4, 2, 2, 3, 4, 3, 1, 0, 0, 0) for tc, ns, bk in ((0, 2, 32), (1, 2, 32), (2, 1, 128))}
    assert missing == set(unreachable), sorted(missing)


def test_predicate_answers_do_not_depend_on_the_device(forms):
    """bd_gemm_takes_ln_fold / bd_gemm_fuses_qk_rmsnorm answer before a device is involved (forward.hip: plan_stack).  What they ask of a
    plan -- whether one exists, whether a launch has the fused q/k RMSNorm epilogue (EP 2), a LayerNorm-fold producer epilogue (EP 4, 5)
    or the consumer's (LNF) -- is the same for cus in {64, 80, 256, 304} x concurrent launches in {1, 2, 4}, on the whole grid."""
    lib = _lib.load()
    plan = _lib.GemmPlan()
    devices = list(itertools.product((64, 80, 256, 304), (1, 2, 4)))

    def asked(g, prec, cus, conc):
        rc = lib.bd_gemm_plan(C.byref(g), prec, cus, conc, C.byref(plan))
        eps = [(l.key[EP_INDEX[l.family]], l.key[LNF_INDEX[l.family]]) for l in plan.launch[:plan.n_launches] if l.family in EP_INDEX]
        return rc, any(ep == 2 for ep, _ in eps), any(ep in (4, 5) for ep, _ in eps), any(lnf for _, lnf in eps)

    for group in forms["groups"]:
        prec, variant = group[0], group[1]
        for (ln, rms, _), N, K, M in shapes_of(forms, group):
            g = gemm_args(forms, variant, N, K, M)
            where = (prec, variant, N, K, M)
            first = asked(g, prec, *devices[0])
            for cus, conc in devices[1:]:
                assert asked(g, prec, cus, conc) == first, (*where, cus, conc)
            rc, fused, producer, consumer = first
            # a plan with such an epilogue means "yes" (the reverse need not hold: refusals of the operands' layout, and the summary's finding)
            if rc == 0 and (producer or consumer):
                assert ln == 1, where
            if rc == 0 and fused:
                assert rms == 1, where
            fold_asked = bool(g.ln_stats_in or g.ln_colsum or g.ln_stats_out or g.ln_op_out or g.ln_resid_in_op)
            if fold_asked and rc == 0:
                assert producer or consumer, where
