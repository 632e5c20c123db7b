"""GPU: the kernels that form th / sqrt(mean_ess(x, y, S) - l - 3) -- sweep_kernel<L, *, HET> (ess_threshold_exact),
sweep_fast in HET mode (hoisted sum) and the HET recheck -- with sample sizes that DIFFER, in every degree class and to
level 14, against the oracle's hetcor_skeleton; and every mode at levels 5..14 on a matrix that has removals there.

The inputs and the oracle runs come from tests/test_het_class_cases.py, which checks on the CPU that each of them can
tell a wrong kernel from a right one (the sizes change the graph in the rows of the class, the transposed sizes give
another graph, every level 5..14 removes something)."""
import itertools

import numpy as np
import pytest

import test_gpu_cusk_het as het_mod
from test_gpu_cusk_het import check_records_f64
from test_gpu_parity import _check_skeleton
from test_het_class_cases import (DEEP_LEVELS, FORMS, ML, ODD_LEVELS, TABLE, TABLE_NAMES, deep_case, deep_graphs, degree_class,
                                  odd_case, table_case)

pytestmark = pytest.mark.gpu
RANK_CAP = 3000      # records beyond this rank are not sampled: the float64 restatement enumerates every set up to the rank
SAMPLE = 200
HETCOR_OPTS = [{}, {"fast": 0}, {"max_staged_classes": 0}, {"validate": 1}]


def _optid(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


def _engine(cg, opts):
    e = cg.Engine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def f64_row_tests_oriented(C, Ni, q, nb, x, l, nranks):
    """test_gpu_cusk_het.f64_row_tests with every size read where the reference's mean_ess reads it: N[vix[i]][vix[j]]
    for j < i over vix = [X, Y, S...], i.e. N[Y][X], N[S_a][X], N[S_a][Y], N[S_a][S_b] (b < a).  The original reads
    N[X][S_a] and N[Y][S_a], which is the same number only in a symmetric matrix."""
    d = len(nb)
    Z = np.full((nranks, d), np.nan)
    T = np.full((nranks, d), np.nan)
    npairs = (l + 2) * (l + 1) / 2.0
    for r, idx in enumerate(itertools.islice(itertools.combinations(range(d), l), nranks)):
        S = nb[list(idx)]
        Mi = np.linalg.inv(C[np.ix_(S, S)])
        a = C[x, S]
        B = C[np.ix_(nb, S)]
        num = C[x, nb] - B @ Mi @ a
        with np.errstate(invalid="ignore", divide="ignore"):  # (the members of S themselves: 0 / 0, masked below)
            den = np.sqrt((1.0 - a @ Mi @ a) * (1.0 - np.einsum("ij,jk,ik->i", B, Mi, B)))
            rho = num / den
            z = np.abs(0.5 * np.log(np.abs((1.0 + rho) / (1.0 - rho))))
        common = Ni[S, x].sum() + sum(Ni[S[i], S[j]] for i in range(l) for j in range(i))
        mean = (common + Ni[nb, x] + Ni[np.ix_(S, nb)].sum(0)) / npairs
        with np.errstate(invalid="ignore", divide="ignore"):
            t = q / np.sqrt(mean - l - 3.0)
        keep = np.ones(d, bool)
        keep[list(idx)] = False
        Z[r, keep] = z[keep]
        T[r, keep] = t[keep]
    return Z, T


def _sample_records(synth, rec, start, seed, levels, always=None):
    """up to SAMPLE records of `levels` with a rank of at most RANK_CAP, by a seeded choice, plus those `always` selects"""
    x, y, lv, z, S = rec
    ok = []
    for i in range(len(x)):
        l = int(lv[i])
        if l not in levels:
            continue
        nb = list(np.flatnonzero(start[l][x[i]] == 1))
        if not all(int(v) in nb for v in S[i][:l]):
            ok.append(i)  # (check_records_f64 fails on it)
            continue
        if synth.comb_rank([nb.index(int(v)) for v in S[i][:l]], len(nb)) <= RANK_CAP:
            ok.append(i)
    ok = np.array(ok, np.int64)
    rng = np.random.default_rng(seed)
    pick = set(rng.choice(ok, min(SAMPLE, len(ok)), replace=False).tolist())
    if always is not None:
        pick |= {int(i) for i in ok if always(int(x[i]), int(lv[i]))}
    pick = np.array(sorted(pick), np.int64)
    return tuple(a[pick] for a in rec), len(ok)


def _check_records(monkeypatch, synth, c, Nm, rec, start, levels, always=None, seed=5):
    monkeypatch.setattr(het_mod, "f64_row_tests", f64_row_tests_oriented)
    sub, eligible = _sample_records(synth, rec, start, seed, levels, always)
    count, touched, margin = check_records_f64(c["C"], Nm, float(np.float32(c["th"])), sub, start)
    print(f"records {len(rec[0])}, eligible {eligible}, checked {count}, touched by an undecided test {touched}, "
          f"smallest relative margin {margin:.3e}")
    assert count >= min(SAMPLE, eligible) and count > 0
    assert touched <= 0.02 * count
    return count


# ---------------------------------------------------------------------------------------------------------------------
# a. cusk --het by class
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_cusk_het_by_class_with_sizes_that_differ(cg, synth, monkeypatch, name, form):
    _, levels, named, classes = TABLE[name]
    c = table_case(name, form)
    n = c["n"]
    e = _engine(cg, {})
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"])
    try:
        st = e.run_skeleton_het(Cd.ptr, Nd.ptr, n, c["th"], levels)
        G = e.adjacency()
        rec = e.sepsets()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert st.level == c["level"]
    assert np.array_equal(G, c["G"][levels])
    assert tuple(int(degree_class(st.max_degree[l])) for l in range(1, levels + 1)) == classes[form], st.max_degree[:levels + 1]
    assert sum(st.rechecks) == 0
    x, y, lv, z, S = rec
    assert set(int(v) for v in lv) == set(range(1, levels + 1))
    for a, b in zip(x, y):
        assert G[a, b] == 0 and c["G"][0][a, b] == 1
    start = {l: c["G"][l - 1] for l in range(1, levels + 1)}
    hub = degree_class(c["G"][0].sum(1)) == named[form]
    _check_records(monkeypatch, synth, c, c["N"], rec, start, set(range(1, levels + 1)),
                   always=lambda xx, l: l == 1 and bool(hub[xx]))


# ---------------------------------------------------------------------------------------------------------------------
# b. hetcor with N_dev by class
# ---------------------------------------------------------------------------------------------------------------------
_TI = {}


def _time_index_case(oracle, name):
    """the symmetric form with a time index: a quarter of the variables at 1, none of them a row of the case's class"""
    if name not in _TI:
        c = table_case(name, "sym")
        n = c["n"]
        rng = np.random.default_rng(n)
        ti = np.zeros(n, np.int32)
        ti[rng.random(n) < 0.25] = 1
        ti[degree_class(c["G"][0].sum(1)) == TABLE[name][2]["sym"]] = 0
        ref = oracle.hetcor_skeleton(c["C"], np.ones((n, n), np.int32), c["N"], c["th"], c["levels"], ti)
        assert ti.sum() > 0 and not np.array_equal(ref.G, c["G"][c["levels"]])  # the index changes the schedule
        _TI[name] = (ti, ref)
    return _TI[name]


@pytest.mark.parametrize("opts", HETCOR_OPTS, ids=_optid)
@pytest.mark.parametrize("form", FORMS + ("sym-ti",))
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_hetcor_by_class_with_sizes_that_differ(cg, oracle, name, form, opts):
    c = table_case(name, form.split("-")[0])
    n, levels = c["n"], c["levels"]
    ti, want_G, want_level = None, c["G"][levels], c["level"]
    if form == "sym-ti":
        ti, ref = _time_index_case(oracle, name)
        want_G, want_level = ref.G, ref.level
    e = _engine(cg, opts)
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"])
    try:
        st = e.run_hetcor(Cd.ptr, n, c["th"], levels, N_dev=Nd.ptr, time_index=ti)
        G = e.adjacency()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert st.level == want_level
    assert np.array_equal(G, want_G)
    assert int(degree_class(st.max_degree[1])) == TABLE[name][3][form.split("-")[0]][0]
    assert all(st.tests[l] > 0 for l in range(1, levels + 1))
    if opts.get("validate"):
        assert st.violations == 0 and st.exact_fallbacks == 0


# ---------------------------------------------------------------------------------------------------------------------
# c. levels 5..14 with removals
# ---------------------------------------------------------------------------------------------------------------------
def _ran_to_the_end(st):
    assert st.levels_run == 15
    assert all(st.tests[l] > 0 for l in DEEP_LEVELS), list(st.tests)


@pytest.mark.parametrize("opts", [{}, {"fast": 0}, {"tmaj_min_level": 2}, {"max_staged_classes": 0}], ids=_optid)
def test_deep_removals_skeleton(cg, oracle, opts):
    c = deep_case()
    e = _engine(cg, opts)
    try:
        st, ref = _check_skeleton(cg, e, oracle, c["C"], c["Th"], ML)
        x, y, lv, z, S = e.sepsets()
    finally:
        e.close()
    _ran_to_the_end(st)
    assert ref.level == 15 and set(DEEP_LEVELS) <= set(int(v) for v in lv)


@pytest.mark.parametrize("form,opts", [("uniform", {})] + [(f, o) for f in ("uniform-matrix",) + FORMS for o in ({}, {"fast": 0})],
                         ids=lambda v: v if isinstance(v, str) else _optid(v))
def test_deep_removals_hetcor(cg, form, opts):
    """uniform: one size passed as a number (the kernels without a size matrix); uniform-matrix, sym, asym: N_dev"""
    c = deep_case()
    key = "uniform" if form.startswith("uniform") else form
    G, level = deep_graphs(key)
    e = _engine(cg, opts)
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"][key])
    try:
        if form == "uniform":
            st = e.run_hetcor(Cd.ptr, c["n"], c["th"], ML, ess_uniform=float(c["N"][key][0, 1]))
        else:
            st = e.run_hetcor(Cd.ptr, c["n"], c["th"], ML, N_dev=Nd.ptr)
        got = e.adjacency()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert st.level == level == 15
    assert np.array_equal(got, G[ML])
    _ran_to_the_end(st)


@pytest.mark.parametrize("form", FORMS)
def test_deep_removals_cusk_het(cg, synth, monkeypatch, form):
    c = deep_case()
    G, level = deep_graphs(form)
    e = _engine(cg, {})
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"][form])
    try:
        st = e.run_skeleton_het(Cd.ptr, Nd.ptr, c["n"], c["th"], ML)
        got = e.adjacency()
        rec = e.sepsets()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert st.level == level == 15
    assert np.array_equal(got, G[ML])
    _ran_to_the_end(st)
    assert sum(st.rechecks) == 0
    assert set(DEEP_LEVELS) <= set(int(v) for v in rec[2])
    start = {l: G[l - 1] for l in DEEP_LEVELS}
    _check_records(monkeypatch, synth, c, c["N"][form], rec, start, set(DEEP_LEVELS))


# ---------------------------------------------------------------------------------------------------------------------
# d. unusual sizes inside a sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cusk-het", "hetcor", "hetcor,fast=0"])
def test_unusual_sizes_inside_a_sweep(cg, mode):
    """NaN, 0, negative, non-integer, l + 3 exactly, +inf and values beyond the int range among the sizes of a run: the
    oracle's mean_ess (truncation to int, NaN -> 0, saturation) defines the threshold of every test"""
    c = odd_case()
    e = _engine(cg, {"fast": 0} if mode.endswith("fast=0") else {})
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"])
    try:
        if mode == "cusk-het":
            st = e.run_skeleton_het(Cd.ptr, Nd.ptr, c["n"], c["th"], ODD_LEVELS)
        else:
            st = e.run_hetcor(Cd.ptr, c["n"], c["th"], ODD_LEVELS, N_dev=Nd.ptr)
        G = e.adjacency()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert st.level == c["ref"].level
    assert np.array_equal(G, c["ref"].G)
