"""The level sweep's kernel families against the oracle, by degree class.

The engine picks a kernel per level and degree class (level_loop.hip, launch_sweeps): the level-1 row / pair /
generic kernels, sweep_vec (64, 128 or 256 threads on class 0), sweep_fast (plain and HET), sweep_tmaj, sweep_exact and
recheck, each staged in LDS or not.  The inputs (synth.dispatch_case, checked on the oracle by
tests/test_dispatch_cases.py) put hub rows at every class boundary, removals at work-item boundaries, second passing
sets in later items and tests inside the filters' guard band; every case runs under each option set that changes the
kernel of its (mode, level, class).  Bars as in test_gpu_parity._check_skeleton; hetcor: adjacency and level."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ML = 14
CAPS = (39, 63, 127, 191, 1 << 30)
SMALL = {"chunk": 256, "chunk0": 64, "chunk0_low": 64}

SKELETON_OPTS = [
    {}, {"vec": 0}, {"vec_threads": 128}, {"vec_threads": 256}, {"fast": 0}, {"validate": 1},
    {"tmaj_min_level": 2}, {"tmaj_min_level": 99},
    {"max_staged_classes": 0}, {"max_staged_classes": 0, "tmaj_min_level": 2}, {"max_staged_classes": 0, "fast": 0},
    {"max_staged_classes": 0, "validate": 1},
    {"rows": 0}, {"pair": 0},
    SMALL, {**SMALL, "vec": 0}, {**SMALL, "tmaj_min_level": 2}, {**SMALL, "vec_threads": 256},
    {"overlap": 0}, {"sync2": 0}, {"assume_symmetric": 1},
    {"l1_threads": 512}, {"l1_lds_row": 0}, {"l1_threads": 512, "validate": 1},
]
CASES = ["l2", "l3", "l4", "l5"]


def _optid(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


@functools.lru_cache(maxsize=None)
def _case(name):
    import cigwas_amd.synth as S
    from oracle import oracle as O

    level, degrees = S.DISPATCH_CASES[name]
    Cm, info = S.dispatch_case(degrees, level, seed=level)
    Th = O.threshold_array(info["N"], info["alpha"])
    dmax = int(O.skeleton(Cm, Th, level - 1).G.sum(1).max())  # largest degree at the start of the level
    return Cm, info, Th, O.skeleton(Cm, Th, level), dmax


@functools.lru_cache(maxsize=None)
def _hetcor_case(name, het, with_ti):
    from oracle import oracle as O

    Cm, info, _, _, _ = _case(name)
    n = Cm.shape[0]
    rng = np.random.default_rng(len(name) + 2 * het + with_ti)
    N = float(info["N"])
    Nm = np.full((n, n), N, np.float32)
    if het:  # a sample size per pair, close enough to N that the near-threshold tests stay inside the guard band
        Nm = (N * (1 + rng.uniform(-1e-5, 1e-5, (n, n)))).astype(np.float32)
        Nm = np.ascontiguousarray(np.maximum(Nm, Nm.T))
    ti = np.zeros(n, np.int32)
    if with_ti:
        ti[rng.random(n) < 0.25] = 1
        keep = [h["h"] for h in info["hubs"]] + [q for h in info["hubs"] for v, T, _ in h["near"] for q in [v] + T]
        ti[keep] = 0  # (the near-threshold tests stay in the schedule)
    th = O.hetcor_threshold(info["alpha"])
    ref = O.hetcor_skeleton(Cm, np.ones((n, n), np.int32), Nm, th, info["level"], ti)
    dmax = int(O.hetcor_skeleton(Cm, np.ones((n, n), np.int32), Nm, th, info["level"] - 1, ti).G.sum(1).max())
    return Nm, ti, th, ref, dmax


def _reached(st, info, opts, dmax):
    """the level of the case ran on the device with the oracle's largest degree (that of the largest hub, or the class
    of it when a time index keeps more edges), and the fast families queued the near-threshold tests for the exact
    recheck"""
    l = info["level"]
    big = max(h["d"] for h in info["hubs"])
    assert st.max_degree[l] == dmax
    assert np.searchsorted(CAPS, dmax) == np.searchsorted(CAPS, big)
    assert st.tests[l] > 0
    if opts.get("fast", 1):
        assert st.rechecks[l] > 0, list(st.rechecks)


@pytest.mark.parametrize("opts", SKELETON_OPTS, ids=_optid)
@pytest.mark.parametrize("name", CASES)
def test_skeleton_dispatch_matrix(cg, name, opts):
    Cm, info, Th, ref, dmax = _case(name)
    n, l = Cm.shape[0], info["level"]
    e = cg.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    Cd = cg.DeviceArray(Cm)
    try:
        st = e.run_skeleton(Cd.ptr, n, Th, l)
        assert st.level == ref.level
        assert np.array_equal(e.adjacency(), ref.G)
        x, y, lv, z, S = e.sepsets()
        dense = np.full((n, n, ML), -1, np.int32)
        dense[x, y] = S
        assert np.array_equal(dense, ref.sepset)
        assert np.allclose(e.pmax(Cd.ptr), ref.pmax, rtol=0, atol=1e-6)
        for k in range(1, ML + 1):
            assert st.tests[k] >= ref.tests[k] or st.tests[k] == 0 == ref.tests[k]
        assert list(st.canonical_tests[: ref.level + 1]) == [int(v) for v in ref.tests[: ref.level + 1]]
        if opts.get("validate"):
            assert st.violations == 0 and st.exact_fallbacks == 0
        _reached(st, info, opts, dmax)
    finally:
        Cd.free()
        e.close()


@pytest.mark.parametrize("opts", [{}, {"fast": 0}, {"max_staged_classes": 0}, {"l1_threads": 512}, {"l1_lds_row": 0}], ids=_optid)
@pytest.mark.parametrize("het,with_ti", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["uniform", "uniform-ti", "het", "het-ti"])
@pytest.mark.parametrize("name", CASES)
def test_hetcor_dispatch_matrix(cg, name, het, with_ti, opts):
    """hetcor with one sample size (sweep_vec / sweep_fast / sweep_tmaj as in Skeleton mode) and with a sample size per
    pair (the HET kernels: the doubled LDS layout stages fewer classes, so rows of degree 128-191 take the unstaged
    kernel of the last class), each with and without a time index"""
    Cm, info, _, _, _ = _case(name)
    Nm, ti, th, ref, dmax = _hetcor_case(name, het, with_ti)
    n = Cm.shape[0]
    e = cg.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        st = e.run_hetcor(Cd.ptr, n, th, info["level"], N_dev=Nd.ptr if het else None, ess_uniform=float(info["N"]),
                          time_index=ti if with_ti else None)
        assert st.level == ref.level
        assert np.array_equal(e.adjacency(), ref.G)
        _reached(st, info, opts, dmax)
    finally:
        Cd.free()
        Nd.free()
        e.close()


@pytest.mark.parametrize("name", CASES)
def test_sepset_z_against_float64(cg, name):
    """the z the engine records for every separating set, against |atanh rho| of the float64 inverse of the same
    sub-matrix (no oracle in between); the bar follows the sub-matrix's condition number and is tight enough to tell
    the winning set from the second passing set of the twin hangers"""
    Cm, info, Th, _, _ = _case(name)
    n, l = Cm.shape[0], info["level"]
    C64 = Cm.astype(np.float64)
    e = cg.Engine(0)
    Cd = cg.DeviceArray(Cm)
    try:
        e.run_skeleton(Cd.ptr, n, Th, l)
        x, y, lv, z, S = e.sepsets()
    finally:
        Cd.free()
        e.close()

    def z64(a, b, s):
        idx = [a, b] + list(s)
        M = C64[np.ix_(idx, idx)]
        P = np.linalg.inv(M)
        r = -P[0, 1] / np.sqrt(P[0, 0] * P[1, 1])
        return abs(float(np.arctanh(r))), float(np.linalg.cond(M))

    bar = {}
    checked = 0
    for i in range(len(x)):
        if lv[i] < 1:
            continue
        s = S[i][S[i] >= 0]
        want, kappa = z64(int(x[i]), int(y[i]), s)
        b = 1e-6 + 32 * kappa * 2.0 ** -24
        assert abs(float(z[i]) - want) <= b, (x[i], y[i], list(s), float(z[i]), want, kappa)
        bar[(int(x[i]), int(y[i]))] = (float(z[i]), b)
        checked += 1
    assert checked > 100
    rejected = total = 0
    for h in info["hubs"]:
        for v, _, T2 in h["twins"]:
            zz, b = bar[(h["h"], v)]
            total += 1
            rejected += abs(zz - z64(h["h"], v, T2)[0]) > b
    assert total >= 4 and rejected >= 0.75 * total
