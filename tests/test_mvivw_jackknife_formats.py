"""`mvivw --jackknife` without a device: the ABI, the groups, the argument errors, the statuses, the command line and its
four files, and the float64 host form (`mvivw.solve_one_jackknife`, the yardstick of test_gpu_mvivw_jackknife.py) against a
longdouble restatement of the rule of include/cusk_hip.h.

The restatement (`restate`) does not downdate: for every group it sums the complement rows' outer products directly in
np.longdouble, solves that system in longdouble, and evaluates step 5 in the literal forms
theta_J = ng theta - sum (1 - m_g / m) theta_-g and tau_g = h_g theta - (h_g - 1) theta_-g.  It measures what the
subtraction A = G - G_g and float64 rounding do to the result.

Units: theta_-g, theta_J, min and max as d_j value relative to max_j |d_j theta_j| (d_j = sqrt(G_jj) of the full fit), se_J
in the same units, absolute; r_i and PRESS relative to their largest value.

Distances float64 - longdouble over `value_cases()` (k in 1, 7, 39, 127; loo, B = 2, B = 7, unequal label groups; every case
leaves m - m_g >= 2 k rows), measured once, largest per quantity: refit 5.9e-15, theta_J 2.7e-13, se_J 2.1e-15, min / max
5.9e-15, pres 6.2e-15, PRESS 2.1e-15.  theta_J of the k = 127 leave-one-out case (266 groups) is the worst: it adds the
errors of all its refits; every other case stays below 5.1e-14.  MEASURED below is the largest; BOUND_JK =
max(test_mvivw_formats.BOUND, 8 MEASURED) = 1e-9 holds the host form here and the device in test_gpu_mvivw_jackknife.py (the
factor 8 is that of test_gpu_mvivw_robust.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_mvivw_formats import BOUND
from test_mvivw_robust_formats import PARENT_OUTCOMES, PARENT_RESULTS, _small_skeleton
from test_sepselect_het_formats import write_ssz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 2.7e-13
BOUND_JK = max(BOUND, 8 * MEASURED)
L = np.longdouble


def jk_problem(m, k, seed):
    """X, y, w: exposures of unequal scale, weights between 0.5e4 and 1.5e4"""
    rng = np.random.default_rng(seed)
    X = 0.05 * rng.standard_normal((m, k)) * (1.0 + 0.5 * rng.random(k))
    theta = np.array([0.3, -0.2, 0.5, 0.1, -0.4][:k] if k <= 5 else 0.3 * rng.standard_normal(k) / np.sqrt(k))
    w = 1e4 * (0.5 + rng.random(m))
    y = X @ theta + rng.standard_normal(m) / np.sqrt(w)
    return X, y, w


def unequal_bounds(m):
    """label groups of unequal size: 1, 2, 3, ... rows, the rest in the last"""
    b, step = [0], 1
    while b[-1] + step < m - m // 8:
        b.append(b[-1] + step)
        step += 1
    return np.array(b + [m], np.int32)


def value_cases():
    """(name, X, y, w, bounds), every group leaving m - m_g >= 2 k rows"""
    from cigwas_amd import mvivw

    out = []
    for k in (1, 7, 39, 127):
        for name, m in (("loo", 2 * k + 12), ("B2", 4 * k + 9), ("B7", 3 * k + 11), ("labels", 3 * k + 20)):
            X, y, w = jk_problem(m, k, 100 * k + m)
            b = unequal_bounds(m) if name == "labels" else mvivw.groups(np.arange(m), {"loo": "loo", "B2": 2, "B7": 7}[name])
            assert np.all(m - np.diff(b) >= 2 * k) and len(b) >= 3
            out.append((f"k{k}-{name}", X, y, w, b))
    return out


def restate(X, y, w, bounds):
    """the rule in longdouble, the complement rows summed directly -> (theta, d, refit, jk k x 4, press, pres)"""
    from cigwas_amd import mvivw

    X, y, w = X.astype(L), y.astype(L), w.astype(L)
    m, k = X.shape
    Z = np.concatenate([X, y[:, None]], axis=1)
    ng = len(bounds) - 1
    # prefix sums at the boundaries from the front and from the back: the complement of group g is before[g] + after[g + 1]
    before, after = [None] * (ng + 1), [None] * (ng + 1)
    run, at = np.zeros((k + 1, k + 1), L), {int(b): i for i, b in enumerate(bounds)}
    for r in range(m + 1):
        if r in at:
            before[at[r]] = run.copy()
        if r < m:
            run = run + np.outer(Z[r] * w[r], Z[r])
    full = run
    run = np.zeros((k + 1, k + 1), L)
    for r in range(m, -1, -1):
        if r in at:
            after[at[r]] = run.copy()
        if r > 0:
            run = run + np.outer(Z[r - 1] * w[r - 1], Z[r - 1])
    st, theta, _, d, _ = mvivw._solve_sums(full, want_v=False)
    assert st == 0 and theta.dtype == L
    refit, pres = np.zeros((ng, k), L), np.zeros(m, L)
    for g in range(ng):
        st, th, _, _, _ = mvivw._solve_sums(before[g] + after[g + 1], want_v=False)
        assert st == 0
        refit[g] = th
        r0, r1 = bounds[g], bounds[g + 1]
        pres[r0:r1] = np.sqrt(w[r0:r1]) * (y[r0:r1] - X[r0:r1] @ th)
    mg = np.diff(bounds).astype(L)
    h = L(m) / mg
    thj = L(ng) * theta - ((1 - mg / L(m))[:, None] * refit).sum(axis=0)
    tau = h[:, None] * theta[None, :] - (h - 1)[:, None] * refit
    var = ((tau - thj[None, :]) ** 2 / (h - 1)[:, None]).sum(axis=0) / L(ng)
    jk = np.stack([thj, np.sqrt(var), refit.min(axis=0), refit.max(axis=0)], axis=1)
    return theta, d, refit, jk, (pres * pres).sum(), pres


def distances(res, ref):
    """(refit, theta_J, se_J, min / max, pres, PRESS) of a result of solve_one_jackknife against `restate`'s"""
    theta, d, refit, jk, press, pres = ref
    scale = np.max(np.abs(d * theta))
    u = lambda a, b: float(np.max(np.abs(d * (np.asarray(a, L) - b))) / scale)  # noqa: E731
    return np.array([u(res[9], refit), u(res[5][:, 0], jk[:, 0]), u(res[5][:, 1], jk[:, 1]),
                     max(u(res[5][:, 2], jk[:, 2]), u(res[5][:, 3], jk[:, 3])),
                     float(np.max(np.abs(np.asarray(res[8], L) - pres)) / np.max(np.abs(pres))), float(abs(L(res[7][0]) - press) / press)])


# ---- ABI ----
def test_symbol_is_declared_and_exported():
    from cigwas_amd._lib import SO_PATH, SYMBOLS

    _vp, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert SYMBOLS["cusk_mvivw_jackknife"] == (_i, [_vp, _vp, _vp, _ll, _i, _i] + [_vp] * 7 + [_i] + [_vp] * 11)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusk_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int cusk_mvivw_jackknife(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, "
            "const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, "
            "const long long *grp_off, const int *grp, int model, double *theta, double *se, double *stats, int *status, "
            "double *jk, int *jk_arg, double *jk_stats, int *jk_status, double *pres, double *refit, float *kernel_ms);") in hdr
    assert hasattr(ctypes.CDLL(SO_PATH), "cusk_mvivw_jackknife")


# ---- groups ----
def test_groups_of_all_three_specs():
    from cigwas_amd import mvivw

    I = np.array([2, 3, 5, 8, 9, 10, 11])
    assert mvivw.groups(I, "loo").tolist() == list(range(8)) and mvivw.groups(I, "loo").dtype == np.int32
    assert mvivw.groups(I, 2).tolist() == [0, 3, 7] and mvivw.groups(I, 3).tolist() == [0, 2, 4, 7]
    assert mvivw.groups(I, 7).tolist() == mvivw.groups(I, 50).tolist() == list(range(8))  # B capped at m
    for m in (1, 5, 256, 1001):
        for B in (2, 7, 200):
            b = mvivw.groups(np.arange(m), B)
            assert b[0] == 0 and b[-1] == m and np.all(np.diff(b) > 0) and len(b) == min(B, m) + 1
            assert b.tolist() == [g * m // min(B, m) for g in range(min(B, m) + 1)]
    labels = np.array([0, 0, 0, 1, 1, 1, 4, 4, 4, 4, 7, 7])
    assert mvivw.groups(I, "labels", labels).tolist() == [0, 1, 3, 5, 7]  # rows 2 | 3, 5 | 8, 9 | 10, 11 by the labels 0 | 1 | 4 | 7
    assert mvivw.groups(np.array([0, 1, 2]), "labels", labels).tolist() == [0, 3]
    assert mvivw.groups(np.zeros(0, np.int64), "labels", labels).tolist() == [0] == mvivw.groups(np.zeros(0, np.int64), "loo").tolist()
    assert mvivw.groups(np.zeros(0, np.int64), 4).tolist() == [0]
    for bad, word in ((np.array([0, 1, 0] + [2] * 9), "non-decreasing"), (labels[:10], "no group label"), (labels * 0.5, "integers")):
        with pytest.raises(ValueError, match=word):
            mvivw.groups(I, "labels", bad)
    for spec in (1, 0, -3, 2.5, "block", True):
        with pytest.raises(ValueError, match="not loo"):
            mvivw.groups(I, spec)


def test_label_file(tmp_path):
    from cigwas_amd import mvivw

    f = tmp_path / "labels.txt"
    f.write_text("0\n0\n3\n3\n9\n")
    assert mvivw.read_group_labels(str(f), 5).tolist() == [0, 0, 3, 3, 9]
    with pytest.raises(ValueError, match="expected 6 labels"):
        mvivw.read_group_labels(str(f), 6)
    f.write_text("0\n2\n1\n")
    with pytest.raises(ValueError, match="non-decreasing"):
        mvivw.read_group_labels(str(f), 3)
    f.write_text("0\nx\n1\n")
    with pytest.raises(ValueError, match="not an integer"):
        mvivw.read_group_labels(str(f), 3)


# ---- the host form against longdouble ----
def test_host_form_against_the_longdouble_restatement():
    from cigwas_amd import mvivw

    worst = np.zeros(6)
    for name, X, y, w, b in value_cases():
        res = mvivw.solve_one_jackknife(X, y, w, b, 0)
        plain = mvivw.solve_one(X, y, w, 0)
        assert res[0] == 0 and res[4] == 0, name
        assert res[1].tobytes() == plain[1].tobytes() and res[2].tobytes() == plain[2].tobytes(), name  # step 0 is the plain fit
        assert tuple(float(v) for v in res[3]) == tuple(float(v) for v in plain[3]), name
        dist = distances(res, restate(X, y, w, b))
        print(name, dist)
        worst = np.maximum(worst, dist)
    print("float64 - longdouble (refit, theta_J, se_J, min / max, pres, PRESS):", worst)
    assert worst.max() <= BOUND_JK, worst
    assert worst.max() <= 4 * MEASURED, worst  # the header's figure still describes this platform


def test_the_longdouble_form_of_the_rule_agrees_with_the_restatement():
    """solve_one_jackknife handed longdouble arrays (the downdating rule in the wider type) against the direct sums"""
    from cigwas_amd import mvivw

    for name, X, y, w, b in value_cases()[:8]:
        res = mvivw.solve_one_jackknife(X.astype(L), y.astype(L), w.astype(L), b, 0)
        assert res[5].dtype == L and res[9].dtype == L and res[8].dtype == L
        assert distances(res, restate(X, y, w, b)).max() <= 1e-15, name


# ---- identities ----
def test_leave_one_out_residuals_are_e_over_one_minus_h():
    from cigwas_amd import mvivw

    for m, k in ((40, 3), (300, 20)):
        X, y, w = jk_problem(m, k, 7)
        res = mvivw.solve_one_jackknife(X, y, w, np.arange(m + 1), 0)
        Xw = (X * np.sqrt(w)[:, None]).astype(L)
        h = np.einsum("ij,jk,ik->i", Xw, np.linalg.inv((Xw.T @ Xw).astype(np.float64)).astype(L), Xw)
        e = np.sqrt(w) * (y - X @ res[1])
        want = e / (1 - h)
        assert np.max(np.abs(res[8] - want)) / np.max(np.abs(want)) <= 1e-10
        assert float(res[7][0]) == pytest.approx(float(np.sum(want * want)), rel=1e-10)


def test_equal_groups_give_the_textbook_formula():
    from cigwas_amd import mvivw

    X, y, w = jk_problem(120, 4, 3)
    for B in (2, 6, 120):
        res = mvivw.solve_one_jackknife(X, y, w, mvivw.groups(np.arange(120), B), 0)
        refit, ng = res[9], B
        want = np.sqrt((ng - 1) / ng * np.sum((refit - refit.mean(axis=0)) ** 2, axis=0))
        np.testing.assert_allclose(res[5][:, 1], want, rtol=1e-9)
        np.testing.assert_allclose(res[5][:, 0], ng * res[1] - (ng - 1) * refit.mean(axis=0), rtol=1e-9)
        assert np.array_equal(res[5][:, 2], refit.min(axis=0)) and np.array_equal(res[5][:, 3], refit.max(axis=0))
        assert np.array_equal(res[6], np.argmax(np.abs(refit - res[1]), axis=0))


def test_one_exposure_matches_its_closed_form():
    from cigwas_amd import mvivw

    X, y, w = jk_problem(50, 1, 4)
    b = unequal_bounds(50)
    res = mvivw.solve_one_jackknife(X, y, w, b, 0)
    x = X[:, 0]
    G, c = np.sum(w * x * x), np.sum(w * x * y)
    for g in range(len(b) - 1):
        s = slice(b[g], b[g + 1])
        th = (c - np.sum(w[s] * x[s] * y[s])) / (G - np.sum(w[s] * x[s] * x[s]))
        assert res[9][g, 0] == pytest.approx(th, rel=1e-12)
        np.testing.assert_allclose(res[8][s], np.sqrt(w[s]) * (y[s] - x[s] * th), rtol=1e-9, atol=1e-12)


def test_ties_name_the_first_group():
    from cigwas_amd import mvivw

    X, y, w = jk_problem(30, 2, 5)
    X, y, w = np.concatenate([X, X]), np.concatenate([y, y]), np.concatenate([w, w])  # group g and g + 3 hold the same rows
    res = mvivw.solve_one_jackknife(X, y, w, mvivw.groups(np.arange(60), 6), 0)
    np.testing.assert_allclose(res[9][:3], res[9][3:], rtol=1e-9)
    assert np.all(res[6] < 3) or not np.array_equal(np.abs(res[9][:3] - res[1]), np.abs(res[9][3:] - res[1]))


# ---- statuses ----
def status_problems():
    """name -> (X, y, w, bounds, status, jk_status, pivot)"""
    X, y, w = jk_problem(40, 3, 6)
    lost = X.copy()
    lost[:, 1] = 0.0
    lost[17, 1] = 0.05  # without the group of row 17 the second exposure is a column of zeros
    b5 = np.array([0, 10, 20, 30, 40], np.int32)
    return {"one-group": (X, y, w, np.array([0, 40], np.int32), 0, 1, np.nan),
            "leaves-k": (X[:6], y[:6], w[:6], np.array([0, 3, 6], np.int32), 0, 1, np.nan),
            "leaves-k+1": (X[:7], y[:7], w[:7], np.array([0, 3, 5, 7], np.int32), 0, 0, None),
            "lost-column": (lost, y, w, b5, 0, 2, 0.0),
            "lost-column-loo": (lost, y, w, np.arange(41, dtype=np.int32), 0, 2, 0.0),
            "plain-1": (X[:3], y[:3], w[:3], np.array([0, 1, 2, 3], np.int32), 1, 1, np.nan),
            "plain-2": (np.concatenate([X[:, :2], X[:, :1]], axis=1), y, w, b5, 2, 2, np.nan),
            "plain-3": (X, np.where(np.arange(40) == 4, np.inf, y), w, b5, 3, 3, np.nan)}


def test_status_1_2_and_the_plain_statuses():
    from cigwas_amd import mvivw

    for name, (X, y, w, b, st, jst, piv) in status_problems().items():
        res = mvivw.solve_one_jackknife(X, y, w, b, 0)
        plain = mvivw.solve_one(X, y, w, 0)
        assert (res[0], res[4]) == (st, jst) and plain[0] == st, name
        if st == 0:
            assert res[1].tobytes() == plain[1].tobytes() and res[2].tobytes() == plain[2].tobytes(), name
        if jst != 0:
            assert res[5] is None and res[6] is None and res[8] is None and res[9] is None and np.isnan(res[7][0]), name
            assert (np.isnan(res[7][1]) if np.isnan(piv) else res[7][1] == piv), (name, res[7])
        else:
            assert np.isfinite(res[5]).all() and res[7][1] >= 1e-8, name


def batch_call(problems):
    """beta, weight and the call of a list of (X, y, w, bounds): each problem has trait columns and marker rows of its own"""
    from cigwas_amd import mvivw

    M, p = sum(len(q[1]) for q in problems), sum(q[0].shape[1] + 1 for q in problems)
    beta, weight, sel, outcome, bounds = np.zeros((M, p)), np.ones((M, p)), [], [], []
    r = c = 0
    for X, y, w, b in problems:
        m, k = X.shape
        beta[r:r + m, c:c + k], beta[r:r + m, c + k] = X, y
        weight[r:r + m, c + k] = w
        sel.append((np.arange(r, r + m), np.arange(c, c + k)))
        outcome.append(c + k)
        bounds.append(np.asarray(b, np.int32))
        r, c = r + m, c + k + 1
    iv_off, iv, ex_off, ex = mvivw.pack(sel)
    grp_off = np.zeros(len(problems) + 1, np.int64)
    grp_off[1:] = np.cumsum([len(b) for b in bounds])
    return beta, weight, dict(outcome=np.array(outcome, np.int32), iv_off=iv_off, iv=iv, ex_off=ex_off, ex=ex, grp_off=grp_off,
                              grp=np.concatenate(bounds).astype(np.int32))


def test_host_engine_batch_and_argument_errors():
    from cigwas_amd import mvivw

    probs = [v[:4] for v in status_problems().values()]
    want = [(v[4], v[5]) for v in status_problems().values()]
    beta, weight, call = batch_call(probs)
    H = mvivw.HostEngine()
    theta, se, stats, status, jk, jk_arg, jk_stats, jk_status, pres, refit, _ = H.mvivw_jackknife(beta, weight, **call)
    assert list(zip(status.tolist(), jk_status.tolist())) == want
    plain = H.mvivw(beta, weight, **{n: call[n] for n in ("outcome", "iv_off", "iv", "ex_off", "ex")})
    for a, b in zip((theta, se, stats, status), plain):
        assert np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()
    eo, io = call["ex_off"], call["iv_off"]
    rf_off = np.concatenate([[0], np.cumsum((np.diff(call["grp_off"]) - 1) * np.diff(eo))])
    assert refit.shape[0] == rf_off[-1] and jk.shape == (eo[-1], 4) and pres.shape[0] == io[-1]
    for a, (X, y, w, b) in enumerate(probs):
        one = mvivw.solve_one_jackknife(X, y, w, b, 0)
        if one[4] == 0:
            assert np.array_equal(jk[eo[a]:eo[a + 1]], one[5]) and np.array_equal(jk_arg[eo[a]:eo[a + 1]], one[6])
            assert np.array_equal(pres[io[a]:io[a + 1]], one[8]) and np.array_equal(refit[rf_off[a]:rf_off[a + 1]], one[9].reshape(-1))
            assert jk_stats[a].tolist() == [float(v) for v in one[7]]
        else:
            assert np.isnan(jk[eo[a]:eo[a + 1]]).all() and (jk_arg[eo[a]:eo[a + 1]] == -1).all()
            assert np.isnan(pres[io[a]:io[a + 1]]).all() and np.isnan(refit[rf_off[a]:rf_off[a + 1]]).all() and np.isnan(jk_stats[a][0])
    for c, word in argument_errors(call):
        with pytest.raises(ValueError, match=word):
            H.mvivw_jackknife(beta, weight, **c)
    with pytest.raises(ValueError, match="model"):
        H.mvivw_jackknife(beta, weight, **call, model=3)
    data = (np.zeros((5, 5), np.int32), np.eye(5), 2, None)
    for kw in (dict(ld=True), dict(robust="huber")):
        with pytest.raises(ValueError, match="jackknife with ld or robust"):
            mvivw.run("unused", 100, data=data, jackknife="loo", **kw)
    with pytest.raises(ValueError, match="group labels for 3 marker rows"):
        mvivw.run("unused", 100, data=data, jackknife=np.array([0, 1]))


def argument_errors(call):
    """[(call, a word of the message)]: the errors cusk_mvivw_jackknife adds, and two of cusk_mvivw's"""
    g, off = call["grp"], call["grp_off"]

    def grp_with(i, v):
        out = g.copy()
        out[i] = v
        return out

    m0 = int(call["iv_off"][1])  # outcome 0: one group, boundaries (0, m0)
    return [(dict(call, grp_off=None), "no group offsets"),
            (dict(call, grp=grp_with(0, 1)), "strictly ascending from 0 to m"),
            (dict(call, grp=grp_with(1, m0 - 1)), "strictly ascending from 0 to m"),
            (dict(call, grp=grp_with(int(off[3]) + 1, 0)), "strictly ascending from 0 to m"),
            (dict(call, grp=grp_with(int(off[3]) + 2, 41)), "strictly ascending from 0 to m"),
            (dict(call, grp_off=np.concatenate([[0, 1], off[2:]])), "no groups"),
            (dict(call, grp_off=np.concatenate([[0, 0], off[2:]])), "no groups"),
            (dict(call, grp_off=np.concatenate([off[:2], [0], off[3:]])), "not monotone"),
            (dict(call, iv=call["iv"][::-1].copy()), "ascending"),
            (dict(call, outcome=call["outcome"] + 100), "not a trait index")]


# ---- files ----
def test_files_without_the_flag_are_those_of_the_earlier_writer(tmp_path):
    from cigwas_amd import mvivw

    res = mvivw.run("unused", 1000, mode="skeleton", data=_small_skeleton())
    assert "jackknife" not in res and "jk" not in res
    mvivw.write_results(str(tmp_path / "r"), res)
    mvivw.write_outcomes(str(tmp_path / "o"), res)
    assert open(tmp_path / "r").read() == PARENT_RESULTS
    assert open(tmp_path / "o").read() == PARENT_OUTCOMES


def test_files_with_the_flag(tmp_path, capsys):
    from cigwas_amd import mvivw

    res = mvivw.run("unused", 1000, mode="skeleton", data=_small_skeleton(), jackknife="loo")
    assert res["jackknife"] and res["jk_status"].tolist() == [0, 0, 0, 1] and res["status"].tolist() == [0, 0, 0, 1]
    for name, write in (("r", mvivw.write_results), ("o", mvivw.write_outcomes), ("e", mvivw.write_jackknife_residuals),
                        ("t", mvivw.write_jackknife_table)):
        write(str(tmp_path / name), res)
    assert capsys.readouterr().err == ""
    rows = [l.split("\t") for l in open(tmp_path / "r").read().split("\n")[:-1]]
    assert rows[0] == "source sink effect p sk_adj num_snps se jk_effect jk_se jk_p jk_min jk_max jk_marker".split()
    parent = [l.split("\t") for l in PARENT_RESULTS.split("\n")[:-1]]
    assert [r[:7] for r in rows] == parent  # the earlier columns are untouched
    g = lambda v: "%.15g" % v  # noqa: E731
    from scipy.special import ndtr

    for r in rows[1:]:
        e, o = int(r[0]) - 1, int(r[1]) - 1
        I, E = res["selection"][o]
        if e in E.tolist() and res["jk_status"][o] == 0:
            j = E.tolist().index(e)
            tj, sj, lo, hi = res["jk"][o][j]
            assert r[7:12] == [g(tj), g(sj), g(2 * ndtr(-abs(tj / sj))), g(lo), g(hi)]
            assert r[12] == str(int(I[res["bounds"][o][res["jk_arg"][o][j]]]) + 1) and lo <= float(r[2]) <= hi
        else:
            assert r[7:] == ["NA"] * 6
    out = [l.split("\t") for l in open(tmp_path / "o").read().split("\n")[:-1]]
    assert out[0] == "sink n_exposures num_snps sigma q q_p status jk_groups press jk_pivot jk_status".split()
    assert [r[:7] for r in out] == [l.split("\t") for l in PARENT_OUTCOMES.split("\n")[:-1]]
    for o in range(3):
        assert out[1 + o][7:] == [str(len(res["selection"][o][0])), g(res["jk_stats"][o][0]), g(res["jk_stats"][o][1]), "0"]
    assert out[4][7:] == ["3", "NA", "NA", "1"]
    resid = [l.split("\t") for l in open(tmp_path / "e").read().split("\n")[:-1]]
    assert resid[0] == "sink marker group press_residual".split() and len(resid) == 1 + 5 + 7 + 5
    assert resid[1] == ["1", str(int(res["selection"][0][0][0]) + 1), "1", g(res["pres"][0][0])]
    table = [l.split("\t") for l in open(tmp_path / "t").read().split("\n")[:-1]]
    assert table[0] == "sink group first_marker last_marker n source effect".split() and len(table) == 1 + 5 * 1 + 7 * 2 + 5 * 1
    I1, E1 = res["selection"][1]
    assert table[6] == ["2", "1", str(int(I1[0]) + 1), str(int(I1[0]) + 1), "1", str(int(E1[0]) + 1), g(res["refit"][1][0][0])]
    assert table[7][:6] == ["2", "1", str(int(I1[0]) + 1), str(int(I1[0]) + 1), "1", str(int(E1[1]) + 1)]
    # jk_status 1 and 2 print one line each, and their columns are NA
    res["jk_status"][0], res["jk_status"][1] = 1, 2
    mvivw.write_results(str(tmp_path / "r2"), res)
    err = capsys.readouterr().err
    assert "outcome trait 1 (1-based): jackknife status 1" in err and "outcome trait 2 (1-based): jackknife status 2" in err
    rows2 = [l.split("\t") for l in open(tmp_path / "r2").read().split("\n")[1:-1]]
    assert all(r[7:] == ["NA"] * 6 for r in rows2 if r[1] in ("1", "2")) and [r[:7] for r in rows2] == parent[1:]


def write_skeleton(d, N, M=300):
    """a merged skeleton of 6 traits and M markers; trait 6 depends on the others -> (stem, label file)"""
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    p = 6
    rng = np.random.default_rng(9)
    beta = np.clip(0.05 * rng.standard_normal((M, p)), -0.9, 0.9)
    beta[:, 5] = beta[:, :5] @ np.array([0.3, -0.2, 0.4, 0.1, -0.3]) + rng.standard_normal(M) / np.sqrt(N)
    corr = np.eye(p + M)
    corr[p:, :p], corr[:p, p:] = beta, beta.T
    adj = np.zeros((p + M, p + M), np.int32)
    adj[0, 1] = adj[1, 0] = adj[4, 5] = adj[5, 4] = 1
    adj[2, p + 7] = adj[p + 7, 2] = 1
    stem = str(d / "all_merged")
    mmwrite(stem + "_sam.mtx", coo_matrix(adj))
    mmwrite(stem + "_scm.mtx", coo_matrix(corr))
    with open(stem + ".mdim", "w") as f:
        f.write(f"{p + M}\t{p}\t3\n")
    write_ssz(stem, np.full((p + M, p + M), float(N)))
    labels = str(d / "blocks.txt")
    with open(labels, "w") as f:
        f.write("".join(f"{r // 23}\n" for r in range(M)))
    return stem, labels


def test_argparse_surface_and_refusals(capsys):
    from cigwas_amd import cli

    parser = cli.build_parser()
    a = parser.parse_args(["mvivw", "s", "5"])
    assert a.jackknife is None and a.jackknife_groups is None and a.jackknife_residuals is None and a.jackknife_table is None
    a = parser.parse_args(["mvivw", "s", "5", "--jackknife", "loo", "--jackknife-residuals", "r", "--jackknife-table", "t", "--het"])
    assert (a.jackknife, a.jackknife_residuals, a.jackknife_table, a.het) == ("loo", "r", "t", True)
    assert parser.parse_args(["mvivw", "s", "5", "--jackknife", "200"]).jackknife == "200"
    with pytest.raises(SystemExit) as ex:
        parser.parse_args(["mvivw", "s", "5", "--jackknife", "loo", "--jackknife-groups", "f"])
    assert ex.value.code == 2
    capsys.readouterr()
    for argv, word in ((["--jackknife", "loo", "--ld"], "whitening"), (["--jackknife", "7", "--robust"], "another estimator"),
                       (["--jackknife-groups", "f", "--robust", "huber"], "whitening"), (["--jackknife", "1"], "loo or a number"),
                       (["--jackknife", "blocks"], "loo or a number"), (["--jackknife-table", "f"], "need --jackknife"),
                       (["--jackknife-residuals", "f"], "need --jackknife")):
        with pytest.raises(SystemExit) as ex:  # refused before any file is read
            cli.main(["mvivw", "no-such-stem", "5"] + argv)
        assert ex.value.code == 2 and word in capsys.readouterr().err, argv


def test_cli_on_the_host_form(tmp_path, monkeypatch):
    from cigwas_amd import cli, mvivw

    monkeypatch.setattr(cli, "_mvivw_engine", lambda: None)
    N = 10000
    stem, labels = write_skeleton(tmp_path, N)
    cli.main(["mvivw", stem, str(N)])
    plain = open(stem + "_mvivw_results.tsv").read(), open(stem + "_mvivw_outcomes.tsv").read()
    R, T = str(tmp_path / "resid.tsv"), str(tmp_path / "table.tsv")
    for argv, spec in ((["--jackknife", "loo"], "loo"), (["--jackknife", "12"], 12),
                       (["--jackknife-groups", labels], np.arange(300) // 23)):
        cli.main(["mvivw", stem, str(N)] + argv + ["--jackknife-residuals", R, "--jackknife-table", T])
        res = mvivw.run(stem, N, jackknife=spec)
        assert res["jk_status"].tolist() == [0] * 6
        want = {}
        for name, write in (("r", mvivw.write_results), ("o", mvivw.write_outcomes), ("e", mvivw.write_jackknife_residuals),
                            ("t", mvivw.write_jackknife_table)):
            write(str(tmp_path / name), res)
            want[name] = open(tmp_path / name).read()
        got = {"r": open(stem + "_mvivw_results.tsv").read(), "o": open(stem + "_mvivw_outcomes.tsv").read(), "e": open(R).read(),
               "t": open(T).read()}
        assert got == want
        assert ["\t".join(l.split("\t")[:7]) for l in got["r"].split("\n")] == plain[0].split("\n")
        assert ["\t".join(l.split("\t")[:7]) for l in got["o"].split("\n")] == plain[1].split("\n")
        ng = {"loo": 299, 12: 12}.get(spec if not isinstance(spec, np.ndarray) else None)
        if ng:  # trait 3 loses marker 8 as an instrument
            assert got["o"].split("\n")[3].split("\t")[7] == str(ng)
        else:
            assert got["o"].split("\n")[1].split("\t")[7] == "14"
    cli.main(["mvivw", stem, str(N)])  # and without the flag the files are what they were
    assert (open(stem + "_mvivw_results.tsv").read(), open(stem + "_mvivw_outcomes.tsv").read()) == plain
    bad = tmp_path / "bad.txt"
    bad.write_text("".join(f"{-r}\n" for r in range(300)))
    with pytest.raises(ValueError, match="non-decreasing"):
        cli.main(["mvivw", stem, str(N), "--jackknife-groups", str(bad)])
    bad.write_text("0\n1\n")
    with pytest.raises(ValueError, match="expected 300 labels"):
        cli.main(["mvivw", stem, str(N), "--jackknife-groups", str(bad)])


# ---- the plan under the host sanitizers ----
def test_jk_plan_selftest_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mvivw_jk_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "mvivw_jk_plan_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mvivw_jk_plan_selftest: ok" in r.stdout, r.stdout + r.stderr
