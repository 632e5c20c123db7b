"""GPU: every form of level 1 on inputs placed at its decision boundary (synth.level1_band_case; premises on the oracle alone
in tests/test_level1_band_cases.py): triples whose test (X; Y | S) lies within a few ulp of C[X,Y] and within fractions of
the guard band of the threshold, and planted triples with operands of 0, below 0 and NaN.

One criterion everywhere, all of it exact: adjacency, level counter, (Skeleton) dense separating sets and
canonical_tests[:2] are the oracle's; with validate = 1 no certified verdict contradicts the exact form; the HET form sends
some tests to the exact form and certifies others.  (run_hetcor with a time index does not count the canonical schedule
of level 1: there its level-0 count alone is compared.)"""
import numpy as np
import pytest

from test_gpu_cusk_het import uniform_thresholds
from test_gpu_level1_forms import SKELETON_FORMS, _formid
from test_level1_band_cases import LAYOUTS, THRESHOLDS, band_case, band_ref, time_index

pytestmark = pytest.mark.gpu
ML = 14


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


def _check(e, st, ref, n, sepsets=True, canon=2):
    assert st.level == ref["level"]
    assert np.array_equal(e.adjacency(), ref["G"])
    if sepsets:
        x, y, lv, z, S = e.sepsets()
        assert (S[:, 1:] == -1).all()
        dense = np.full((n, n), -1, np.int32)
        dense[x, y] = S[:, 0]
        assert np.array_equal(dense, ref["sep0"])
    assert list(st.canonical_tests[:canon]) == [int(v) for v in ref["tests"][:canon]]


def _run_skeleton(cg, case, opts=(), offset_bytes=0):
    from cigwas_amd._lib import lib

    c, ref = band_case(*case), band_ref(*case)
    Cm, n = c["C"], c["n"]
    e = cg.Engine(0)
    Cd = cg.DeviceArray(nbytes=Cm.nbytes + 16)
    try:
        assert Cd.ptr % 16 == 0
        assert lib().cusk_dev_upload(Cd.ptr + offset_bytes, Cm.ctypes.data, Cm.nbytes) == 0
        for k, v in opts:
            e.set_option(k, v)
        st = e.run_skeleton(Cd.ptr + offset_bytes, n, c["Th"], 1)
        _check(e, st, ref, n)
        if dict(opts).get("validate"):
            assert st.violations == 0
        return st, e.level1_form()
    finally:
        Cd.free()
        e.close()


HUB = ("hub", "headline", "skeleton")
OTHER_FORMS = {"rows=0": (("rows", 0),), "fast=0": (("fast", 0),)}


@pytest.mark.parametrize("form", SKELETON_FORMS, ids=_formid)
def test_skeleton_hub_every_row_kernel_form(cg, form):
    threads, lds_row, validate = form
    st, kernel = _run_skeleton(cg, HUB, (("l1_threads", threads), ("l1_lds_row", lds_row), ("validate", validate)))
    assert kernel == (4 if not lds_row else 3 if threads == 512 else 2 if threads == 256 else kernel) and kernel in (2, 3, 4)


@pytest.mark.parametrize("name", list(OTHER_FORMS))
def test_skeleton_hub_pair_kernel_and_control(cg, name):
    st, kernel = _run_skeleton(cg, HUB, OTHER_FORMS[name])
    if name == "rows=0":
        assert kernel in (0, 1)


def test_skeleton_hub_misaligned_matrix_takes_the_gather_form(cg):
    st, kernel = _run_skeleton(cg, HUB, offset_bytes=4)
    assert kernel == 4


@pytest.mark.parametrize("name", THRESHOLDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_skeleton_default_form_at_every_threshold(cg, layout, name):
    """below kThMinFilter (below_min) the filter is off and the run must still be the oracle's"""
    for validate in (0, 1):
        st, kernel = _run_skeleton(cg, (layout, name, "skeleton"), (("validate", validate),))
        assert kernel in (2, 3)


@pytest.mark.parametrize("form", [(0, 1), (512, 1)], ids=_formid)
@pytest.mark.parametrize("with_ti", [False, True], ids=["uniform", "uniform-ti"])
@pytest.mark.parametrize("name", ["headline", "biobank"])
def test_hetcor_hub(cg, name, with_ti, form):
    case = ("hub", name, "hetcor")
    c, ref = band_case(*case), band_ref(*case, with_ti)
    Cm, n = c["C"], c["n"]
    e = cg.Engine(0)
    e.set_option("l1_threads", form[0])
    e.set_option("l1_lds_row", form[1])
    Cd = cg.DeviceArray(Cm)
    try:
        st = e.run_hetcor(Cd.ptr, n, c["th"], 1, ess_uniform=float(c["Nval"]), time_index=time_index(*case) if with_ti else None)
        _check(e, st, ref, n, sepsets=False, canon=1 if with_ti else 2)
    finally:
        Cd.free()
        e.close()


def _run_het(cg, case, Nm, ref, opts, sepsets):
    c = band_case(*case)
    Cm, n = c["C"], c["n"]
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        for k, v in opts:
            e.set_option(k, v)
        st = e.run_skeleton_het(Cd.ptr, Nd.ptr, n, c["th"], 1)
        _check(e, st, ref, n, sepsets=sepsets)
        o = dict(opts)
        if o.get("validate"):
            assert st.violations == 0
        if o.get("het_rows"):
            assert e.level1_form() == (4 if o.get("l1_lds_row") == 0 else 2)
            assert 0 < st.rechecks[1] < st.tests[1]
        else:
            assert e.level1_form() == 0
        return st
    finally:
        Cd.free()
        Nd.free()
        e.close()


HET_FORMS = {"default": (), "threads=256,lds_row=0": (("l1_threads", 256), ("l1_lds_row", 0))}
HET_ROWS = {"het_rows=1": (("het_rows", 1),), "het_rows=1,validate": (("het_rows", 1), ("het_filter", 1), ("validate", 1)),
            "het_rows=0": (("het_rows", 0),)}


@pytest.mark.parametrize("rows", list(HET_ROWS))
@pytest.mark.parametrize("form", list(HET_FORMS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_het_uniform_sizes_give_the_skeleton_result(cg, layout, form, rows):
    """the matrix of the Skeleton case at N everywhere: thresholds, and with them graph, separating sets and counts, are
    those of the Skeleton run"""
    case = (layout, "headline", "skeleton")
    c = band_case(*case)
    assert np.array_equal(uniform_thresholds(c["th"], c["Nval"])[:2], c["Th"][:2])
    Nm = np.full((c["n"], c["n"]), c["Nval"], np.float32)
    _run_het(cg, case, Nm, band_ref(*case), HET_FORMS[form] + HET_ROWS[rows], sepsets=True)


@pytest.mark.parametrize("rows", list(HET_ROWS))
@pytest.mark.parametrize("form", list(HET_FORMS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_het_per_triple_sizes(cg, layout, form, rows):
    """sizes on both sides of kHetUMin, kHetUMax and kHetDMin, a NaN, a zero and a negative size; het_rows = 0 runs the same
    input through the work-item kernel"""
    case = (layout, "headline", "het")
    c = band_case(*case)
    st = _run_het(cg, case, c["N"], band_ref(*case), HET_FORMS[form] + HET_ROWS[rows], sepsets=False)
    print(f"{layout} {form} {rows}: tests {st.tests[1]}, sent to the exact form {st.rechecks[1]}, violations {st.violations}")


def test_batched_cliques_equal_their_one_block_runs(cg, oracle, synth):
    """the cliques case twice beside a 70-variable block: bases 0, 2112 and 2240 (multiples of 64), block sizes 2,082 and 70
    (no multiples of 4)"""
    case = ("cliques", "headline", "skeleton")
    c, ref = band_case(*case), band_ref(*case)
    Cm, k, Th = c["C"], c["n"], c["Th"]
    small = synth.random_corr(70, seed=3, k=280)
    ref_small = oracle.skeleton(small, Th, 1)
    assert k % 4 != 0 and ref_small.tests[1] > 0
    mats = [Cm, small, Cm]
    lo, base = [], 0
    for m in mats:
        lo.append(base)
        base += (m.shape[0] + 63) // 64 * 64
    hi = [a + m.shape[0] for a, m in zip(lo, mats)]
    n = base
    big = np.full((n, n), np.nan, np.float32)
    for m, a, b in zip(mats, lo, hi):
        big[a:b, a:b] = m
    e = cg.Engine(0)
    Cd = cg.DeviceArray(big)
    try:
        st = e.run_skeleton_batch(Cd.ptr, n, lo, hi, Th, 1)
        Gs = e.adjacency_blocks()
        x, y, lv, z, S = e.sepsets()
    finally:
        Cd.free()
        e.close()
    assert (S[:, 1:] == -1).all()
    for b, (a, kb) in enumerate(zip(lo, (k, 70, k))):
        want_G, want_sep = (ref_small.G, ref_small.sepset[:, :, 0]) if b == 1 else (ref["G"], ref["sep0"])
        assert np.array_equal(Gs[b], want_G), b
        sel = (x >= a) & (x < a + kb)
        dense = np.full((kb, kb), -1, np.int32)
        dense[x[sel] - a, y[sel] - a] = S[sel, 0] - a
        assert np.array_equal(dense, want_sep), b
    assert list(st.canonical_tests[:2]) == [int(2 * ref["tests"][l] + ref_small.tests[l]) for l in range(2)]
    # ... which is what the one-block run of the same matrix gives (oracle-equal there as well)
    _run_skeleton(cg, case)
