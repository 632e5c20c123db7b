"""Every form of the level-1 row kernel against the oracle: level1_rows2_kernel with the row of C in LDS at 256 and at
512 threads and with the row gathered through the caches, for Skeleton (plain and validating) and hetcor runs.

The input (synth.level1_star_case, checked on the oracle by tests/test_dispatch_cases.py) has one row with 1,300
neighbours at the start of level 1 -- more than two staging rounds of a 512-thread workgroup, so the prefetch of the next
round's records runs and ends inside a row -- and n = 1,301 is not a multiple of 4, so the 16-byte staging of a row clamps
its last piece.  The forms are chosen by the test options "l1_threads" and "l1_lds_row"; a matrix that is not 16-byte
aligned reaches the gather form with no option set."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ML = 14
FORMS = [(t, r) for t in (0, 256, 512) for r in (1, 0)]
# the validating kernels at each forced size, and their gather form
SKELETON_FORMS = [(t, r, 0) for t, r in FORMS] + [(256, 1, 1), (512, 1, 1), (256, 0, 1)]


def _formid(f):
    return f"threads={f[0]},lds_row={f[1]}" + (",validate" if len(f) > 2 and f[2] else "")


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


@functools.lru_cache(maxsize=None)
def _case():
    import cigwas_amd.synth as S
    from oracle import oracle as O

    Cm, info = S.level1_star_case()
    Th = O.threshold_array(info["N"], info["alpha"])
    return Cm, info, Th, O.skeleton(Cm, Th, 1)


@functools.lru_cache(maxsize=None)
def _hetcor_case(with_ti):
    from oracle import oracle as O

    Cm, info, _, _ = _case()
    n = Cm.shape[0]
    ti = np.zeros(n, np.int32)
    if with_ti:
        ti[np.random.default_rng(7).random(n) < 0.25] = 1
        ti[info["hub"]] = 0
    th = O.hetcor_threshold(info["alpha"])
    ref = O.hetcor_skeleton(Cm, np.ones((n, n), np.int32), np.full((n, n), info["N"], np.float32), th, 1, ti)
    return ti, th, ref


def _check_skeleton(e, st, ref, n):
    assert st.level == ref.level
    assert np.array_equal(e.adjacency(), ref.G)
    x, y, lv, z, S = e.sepsets()
    dense = np.full((n, n, ML), -1, np.int32)
    dense[x, y] = S
    assert np.array_equal(dense, ref.sepset)
    assert list(st.canonical_tests[:2]) == [int(ref.tests[0]), int(ref.tests[1])]
    assert st.max_degree[1] == n - 1 and st.tests[1] >= ref.tests[1]


@pytest.mark.parametrize("form", SKELETON_FORMS, ids=_formid)
def test_skeleton_level1_forms(cg, form):
    threads, lds_row, validate = form
    Cm, info, Th, ref = _case()
    n = Cm.shape[0]
    e = cg.Engine(0)
    e.set_option("l1_threads", threads)
    e.set_option("l1_lds_row", lds_row)
    e.set_option("validate", validate)
    Cd = cg.DeviceArray(Cm)
    try:
        st = e.run_skeleton(Cd.ptr, n, Th, 1)
        _check_skeleton(e, st, ref, n)
        if validate:
            assert st.violations == 0
    finally:
        Cd.free()
        e.close()


@pytest.mark.parametrize("with_ti", [False, True], ids=["uniform", "uniform-ti"])
@pytest.mark.parametrize("form", FORMS, ids=_formid)
def test_hetcor_level1_forms(cg, form, with_ti):
    threads, lds_row = form
    Cm, info, _, _ = _case()
    ti, th, ref = _hetcor_case(with_ti)
    n = Cm.shape[0]
    e = cg.Engine(0)
    e.set_option("l1_threads", threads)
    e.set_option("l1_lds_row", lds_row)
    Cd = cg.DeviceArray(Cm)
    try:
        st = e.run_hetcor(Cd.ptr, n, th, 1, ess_uniform=float(info["N"]), time_index=ti if with_ti else None)
        assert st.level == ref.level
        assert np.array_equal(e.adjacency(), ref.G)
        assert st.max_degree[1] == n - 1
    finally:
        Cd.free()
        e.close()


def test_skeleton_level1_misaligned_matrix(cg):
    """the matrix 4 bytes past a 16-byte boundary: the launcher's alignment rule takes the gather form, no option set"""
    from cigwas_amd._lib import lib

    Cm, info, Th, ref = _case()
    n = Cm.shape[0]
    e = cg.Engine(0)
    Cd = cg.DeviceArray(nbytes=Cm.nbytes + 16)
    try:
        assert Cd.ptr % 16 == 0
        assert lib().cusk_dev_upload(Cd.ptr + 4, Cm.ctypes.data, Cm.nbytes) == 0
        st = e.run_skeleton(Cd.ptr + 4, n, Th, 1)
        _check_skeleton(e, st, ref, n)
    finally:
        Cd.free()
        e.close()


def test_level1_options_are_validated(cg):
    e = cg.Engine(0)
    try:
        with pytest.raises(RuntimeError, match="unknown option l1_exp"):
            e.set_option("l1_exp", 1)
        for key, value in (("l1_threads", 384), ("l1_threads", 1024), ("l1_lds_row", 2), ("l1_lds_row", -1)):
            with pytest.raises(RuntimeError, match="unknown option " + key):
                e.set_option(key, value)
        for key, value in (("l1_threads", 256), ("l1_threads", 512), ("l1_threads", 0), ("l1_lds_row", 0), ("l1_lds_row", 1)):
            e.set_option(key, value)
    finally:
        e.close()
