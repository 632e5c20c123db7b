"""CPU: `ci-gwas mvivw` (ci-gwas_amd/mvivw.py): the selections, the numpy host form of the rule of include/cusk_hip.h
(`HostEngine`), the two result files and the command line.

The yardstick of the estimates is a numpy LONGDOUBLE solution of the same normal equations by Gauss-Jordan with pivoting,
not R: the reference's robust estimator (`mr_mvivw(..., robust = TRUE)`) is deliberately not reproduced.  The synthetic
problems are built so that the unit-diagonal Gram has a condition number <= 1e4 (asserted per case: a condition on the
inputs); the bound 1e-9 on max|x - x_ref| / max|x_ref| for theta, se and sigma comes from cond * k * eps ~ 1e4 * 128 *
1.1e-16 ~ 1.4e-10.  The device path runs the same cases in test_gpu_mvivw.py, which imports the helpers below."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from test_iv_check_formats import load_kat, materialise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SAMPLES = 50000
BOUND = 1e-9
# (m, k, column correlation)
SHAPES = ((5, 1, 0.0), (9, 7, 0.5), (300, 7, 0.9), (700, 39, 0.9), (1000, 127, 0.9), (257, 127, 0.5), (4097, 127, 0.95))


def synth_problem(m, k, rho, seed):
    """m rows of k exposure columns and one outcome column (the last), as the marker correlations of a skeleton"""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((m, k + 1))
    C = np.linalg.cholesky(rho * np.ones((k + 1, k + 1)) + (1.0 - rho) * np.eye(k + 1))
    Z = (Z @ C.T) * 0.03
    theta0 = 0.2 * rng.standard_normal(k)
    Z[:, k] = Z[:, :k] @ theta0 + 0.01 * rng.standard_normal(m)
    return np.clip(Z, -0.9, 0.9)


@functools.lru_cache(maxsize=None)
def problem(m, k, rho):
    """(beta m x (k + 1), weight m x (k + 1)): exposures are traits 0 .. k-1, the outcome is trait k, every row an instrument"""
    from cigwas_amd import mvivw

    beta = synth_problem(m, k, rho, 1000 * k + m)
    w = mvivw.weights(beta, N_SAMPLES)
    beta.setflags(write=False)
    w.setflags(write=False)
    return beta, w


def one_call(beta, k):
    m = beta.shape[0]
    return dict(outcome=[k], iv_off=[0, m], iv=np.arange(m), ex_off=[0, k], ex=np.arange(k))


def gauss_jordan_ld(A, B):
    """A^-1 B in longdouble, partial pivoting"""
    A, B = np.array(A, np.longdouble), np.array(B, np.longdouble)
    n = A.shape[0]
    for j in range(n):
        r = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, r]], B[[j, r]] = A[[r, j]], B[[r, j]]
        B[j] = B[j] / A[j, j]
        A[j] = A[j] / A[j, j]
        f = A[:, j].copy()
        f[j] = 0
        B -= np.outer(f, B[j])
        A -= np.outer(f, A[j])
    return B


@functools.lru_cache(maxsize=None)
def longdouble_reference(m, k, rho, model=0):
    """(theta, se, sigma, rss, cond of the unit-diagonal Gram) of the rule, in longdouble"""
    beta, w = problem(m, k, rho)
    X, y, wl = (np.array(a, np.longdouble) for a in (beta[:, :k], beta[:, k], w[:, k]))
    G = X.T @ (X * wl[:, None])
    b = X.T @ (wl * y)
    sol = gauss_jordan_ld(G, np.concatenate([b[:, None], np.eye(k, dtype=np.longdouble)], axis=1))
    theta, v = sol[:, 0], np.diag(sol[:, 1:])
    r = y - X @ theta
    rss = (wl * r * r).sum()
    sigma = np.sqrt(rss / (m - k))
    random = model == 1 or (model == 0 and m >= 4)
    se = np.sqrt(v) * (max(sigma, np.longdouble(1)) if random else 1)
    d = np.sqrt(np.diag(G)).astype(np.float64)
    cond = float(np.linalg.cond(G.astype(np.float64) / np.outer(d, d)))
    return theta, se, sigma, rss, cond


def rel(x, ref):
    x, ref = np.asarray(x, np.longdouble), np.asarray(ref, np.longdouble)
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


# ---- selections ----
def small_adjacency():
    """p = 4 traits, 9 markers.  Trait 3 has no marker; trait 2 is adjacent to every marker (status 1 as an outcome under
    `all`); marker row 4 is adjacent to traits 0 and 1; traits 0-1 and 1-2 are adjacent, trait 3 to none."""
    p, M = 4, 9
    adj = np.zeros((p + M, p + M), np.int32)
    for t, rows in ((0, (0, 1, 4)), (1, (4, 5, 6)), (2, range(M))):
        for r in rows:
            adj[t, p + r] = adj[p + r, t] = 1
    for a, b in ((0, 1), (1, 2)):
        adj[a, b] = adj[b, a] = 1
    adj[p + 1, p + 2] = adj[p + 2, p + 1] = 1  # marker-marker entries play no part
    return adj, p, M


def loops_select(adj, p, M, mode, prior=None, iv_rows=None):
    """the four selections as plain loops"""
    out = []
    for o in range(p):
        if mode == "ivs":
            I = sorted({v - 1 for e, oo, v in iv_rows if oo == o + 1})
            E = sorted({e - 1 for e, oo, v in iv_rows if oo == o + 1})
            out.append((I, E))
            continue
        if mode == "all":
            E = [t for t in range(p) if t != o]
            I = [r for r in range(M) if adj[o, p + r] == 0]
        elif mode == "skeleton":
            E = [t for t in range(p) if t != o and adj[t, o] != 0]
            far = [t for t in range(p) if t != o and adj[t, o] == 0]
            I = [r for r in range(M) if adj[o, p + r] == 0 and all(adj[t, p + r] == 0 for t in far)]
        else:
            E = [t for t in range(p) if t != o and prior[o, t] != 1]
            I = [r for r in range(M) if adj[o, p + r] == 0]
        out.append((I, E))
    return out


def same_selection(got, want):
    assert len(got) == len(want)
    for (gi, ge), (wi, we) in zip(got, want):
        assert list(map(int, gi)) == list(wi) and list(map(int, ge)) == list(we)


def test_selections_equal_plain_loops():
    from cigwas_amd import mvivw

    adj, p, M = small_adjacency()
    prior = np.zeros((p, p), np.int32)
    prior[0, 1] = prior[2, 3] = prior[3, 0] = 1
    iv_rows = [(1, 2, 1), (1, 2, 5), (3, 2, 5), (3, 2, 2), (2, 1, 9), (4, 1, 9), (2, 4, 3)]
    for mode, kw in (("all", {}), ("skeleton", {}), ("prior", {"prior": prior}), ("ivs", {"iv_rows": iv_rows})):
        same_selection(mvivw.select(adj, p, mode, **kw), loops_select(adj, p, M, mode, **kw))
    sel = mvivw.select(adj, p, "all")
    assert len(sel[2][0]) == 0 and list(sel[3][0]) == list(range(M))  # adjacent to every marker; adjacent to none
    assert 4 not in sel[0][0] and 4 not in sel[1][0]                  # the marker of two traits
    # a weighted adjacency (any value != 0) selects the same
    same_selection(mvivw.select(adj * 7, p, "skeleton"), loops_select(adj, p, M, "skeleton"))


def test_deviation_skeleton_empty_removal_removes_nothing():
    """the reference's B[-rm_rows, ] with an empty rm_rows selects zero rows in R"""
    from cigwas_amd import mvivw

    p, M = 3, 5
    adj = np.zeros((p + M, p + M), np.int32)
    adj[0, 1] = adj[1, 0] = adj[0, 2] = adj[2, 0] = 1  # every trait is adjacent to outcome 0, no marker is adjacent to anything
    I, E = mvivw.select(adj, p, "skeleton")[0]
    assert list(I) == list(range(M)) and list(E) == [1, 2]


def test_deviation_prior_keeps_marker_rows_numbered_like_traits():
    """the reference removes marker ROWS 1-based-equal to the removed trait numbers and the outcome's number"""
    from cigwas_amd import mvivw

    adj, p, M = small_adjacency()
    prior = np.zeros((p, p), np.int32)
    prior[3, 0] = prior[3, 1] = 1  # outcome 3: traits 0 and 1 are removed; the reference would also drop marker rows 0, 1, 3
    I, E = mvivw.select(adj, p, "prior", prior=prior)[3]
    assert list(I) == list(range(M)) and list(E) == [2]


def test_deviation_num_snps_is_per_outcome(tmp_path):
    """the reference's column carries one recycled value"""
    from cigwas_amd import mvivw

    res = _result_on_small_adjacency(mvivw)
    path = str(tmp_path / "r.tsv")
    mvivw.write_results(path, res)
    rows = [l.rstrip("\n").split("\t") for l in open(path)][1:]
    per_sink = {int(r[1]): int(r[5]) for r in rows}
    assert per_sink == {o + 1: len(res["selection"][o][0]) for o in range(4)} and len(set(per_sink.values())) > 1


# ---- HostEngine ----
@pytest.mark.parametrize("shape", SHAPES)
def test_host_engine_against_longdouble(shape):
    from cigwas_amd import mvivw

    m, k, rho = shape
    beta, w = problem(*shape)
    th_ref, se_ref, sigma_ref, rss_ref, cond = longdouble_reference(*shape)
    assert cond <= 1e4, cond  # worst of these cases: 3.6e3 at (4097, 127, .95)
    theta, se, stats, status, _ = mvivw.HostEngine().mvivw(beta, w, **one_call(beta, k))
    assert status[0] == 0
    worst = max(rel(theta[:k], th_ref), rel(se[:k], se_ref), rel(stats[0, 1], sigma_ref), rel(stats[0, 0], rss_ref))
    print(shape, "cond", cond, "worst", worst)
    # worst observed over the seven cases: 9e-14 at (4097, 127, .95) (float64 against longdouble)
    assert worst <= BOUND, (shape, worst)
    assert PIVOT_OK(stats[0, 2])


def PIVOT_OK(v):
    return 1e-8 <= v <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_host_engine_against_lstsq(shape):
    from cigwas_amd import mvivw

    m, k, rho = shape
    beta, w = problem(*shape)
    sw = np.sqrt(w[:, k])
    A, y = beta[:, :k] * sw[:, None], beta[:, k] * sw
    th_ref = np.linalg.lstsq(A, y, rcond=None)[0]
    r = y - A @ th_ref
    sigma_ref = np.sqrt(r @ r / (m - k))
    v = np.diag(np.linalg.pinv(A.T @ A))
    se_ref = np.sqrt(v) * (max(sigma_ref, 1.0) if m >= 4 else 1.0)
    theta, se, stats, status, _ = mvivw.HostEngine().mvivw(beta, w, **one_call(beta, k))
    assert status[0] == 0
    assert rel(theta[:k], th_ref) <= BOUND and rel(se[:k], se_ref) <= BOUND and rel(stats[0, 1], sigma_ref) <= BOUND


def status_batch(seed=5):
    """p = 12 traits, 600 marker rows; six outcomes with lists of their own: good, m = k, good, k = 0, duplicated column,
    good.  Returns (beta, weight, call) with call the list arguments."""
    from cigwas_amd import mvivw

    beta = synth_problem(600, 11, 0.5, seed)
    beta[:, 7] = beta[:, 3]  # traits 3 and 7 are one column
    w = mvivw.weights(beta, N_SAMPLES)
    rng = np.random.default_rng(seed)
    lists = [
        (0, np.sort(rng.choice(600, 300, replace=False)), [1, 2, 3, 4]),        # good
        (1, np.arange(4), [0, 2, 3, 4]),                                         # m = k: status 1
        (2, np.arange(0, 600, 2), [0, 1, 3]),                                    # good
        (5, np.arange(600), []),                                                 # k = 0: status 1
        (6, np.arange(100, 500), [0, 3, 7]),                                     # duplicated exposure column: status 2
        (11, np.arange(600), [0, 1, 2, 4, 5, 6, 8, 9, 10]),                      # good
    ]
    return beta, w, lists


def call_of(lists):
    from cigwas_amd import mvivw

    iv_off, iv, ex_off, ex = mvivw.pack([(np.asarray(I), np.asarray(E, np.int64)) for _, I, E in lists])
    return dict(outcome=np.array([o for o, _, _ in lists], np.int32), iv_off=iv_off, iv=iv, ex_off=ex_off, ex=ex)


def test_status_1_2_3_and_the_other_outcomes_unchanged():
    from cigwas_amd import mvivw

    beta, w, lists = status_batch()
    call = call_of(lists)
    theta, se, stats, status, _ = mvivw.HostEngine().mvivw(beta, w, **call)
    assert status.tolist() == [0, 1, 0, 1, 2, 0]
    eo = call["ex_off"]
    for a in (1, 3, 4):
        assert np.all(np.isnan(theta[eo[a]:eo[a + 1]])) and np.all(np.isnan(se[eo[a]:eo[a + 1]]))
    assert stats[4, 2] < 1e-8 and np.isnan(stats[4, 0])
    good = [0, 2, 5]
    for bad_value in (np.nan, np.inf, 0.0):
        w2 = w.copy()
        w2[lists[2][1][5], 2] = bad_value  # a row of outcome 2's problem
        t2, s2, st2, status2, _ = mvivw.HostEngine().mvivw(beta, w2, **call)
        assert status2.tolist() == [0, 1, 3, 1, 2, 0]
        assert np.all(np.isnan(t2[eo[2]:eo[3]]))
        for a in (0, 5):  # bit for bit
            assert t2[eo[a]:eo[a + 1]].tobytes() == theta[eo[a]:eo[a + 1]].tobytes()
            assert s2[eo[a]:eo[a + 1]].tobytes() == se[eo[a]:eo[a + 1]].tobytes()
            assert st2[a].tobytes() == stats[a].tobytes()
    b2 = beta.copy()
    odd = int(lists[0][1][lists[0][1] % 2 == 1][0])
    b2[odd, 1] = np.nan  # a value of X of outcomes 0 and 5; outcome 2 has the column but not the row, outcome 4 the row but not the column
    assert mvivw.HostEngine().mvivw(b2, w, **call)[3].tolist() == [3, 1, 0, 1, 2, 3]
    # a bad value outside every problem's rows and columns changes nothing
    w3 = w.copy()
    w3[:, 3] = np.nan  # trait 3 is never an outcome
    t3 = mvivw.HostEngine().mvivw(beta, w3, **call)[0]
    assert t3.tobytes() == theta.tobytes()
    assert good == [a for a in range(6) if status[a] == 0]


def test_model_default_random_fixed():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    # m = 3: default is fixed
    beta, _ = problem(5, 1, 0.0)
    b3 = np.ascontiguousarray(beta[:3])
    w3 = mvivw.weights(b3, N_SAMPLES)
    runs = {mdl: eng.mvivw(b3, w3, **one_call(b3, 1), model=mdl) for mdl in (0, 1, 2)}
    assert runs[0][2][0, 1] > 1 and runs[1][1][0] != runs[2][1][0]  # sigma > 1: random and fixed differ here ...
    assert runs[0][1][0] == runs[2][1][0]                            # ... and default is the fixed one
    # sigma > 1 at N = 50,000 (the noise of the construction is far above byse): random and fixed differ
    beta, w = problem(300, 7, 0.9)
    runs = {mdl: eng.mvivw(beta, w, **one_call(beta, 7), model=mdl) for mdl in (0, 1, 2)}
    sigma = runs[0][2][0, 1]
    assert sigma > 1
    assert np.array_equal(runs[0][1], runs[1][1]) and np.allclose(runs[1][1][:7], runs[2][1][:7] * sigma, rtol=1e-14)
    assert np.array_equal(runs[1][0], runs[2][0])
    # sigma < 1 with small weights (N = 30): random and fixed agree
    wl = mvivw.weights(beta, 30)
    runs = {mdl: eng.mvivw(beta, wl, **one_call(beta, 7), model=mdl) for mdl in (1, 2)}
    assert runs[1][2][0, 1] < 1 and np.array_equal(runs[1][1], runs[2][1])
    with pytest.raises(ValueError, match="model"):
        eng.mvivw(beta, w, **one_call(beta, 7), model=3)


# ---- files ----
def _result_on_small_adjacency(mvivw, model=0):
    """skeleton selection on a chain 0 - 1 - 2 with trait 3 apart: outcomes 0, 1, 2 are estimated on 5, 7 and 5 instruments with
    exposures {1}, {0, 2}, {1}; outcome 3 has no exposure (status 1) and 3 instruments"""
    p, M = 4, 9
    adj = np.zeros((p + M, p + M), np.int32)
    for t, rows in ((0, (0,)), (1, (1, 2)), (2, (3, 4, 5))):
        for r in rows:
            adj[t, p + r] = adj[p + r, t] = 1
    for a, b in ((0, 1), (1, 2)):
        adj[a, b] = adj[b, a] = 1
    rng = np.random.default_rng(3)
    beta = np.clip(0.05 * rng.standard_normal((M, p)), -0.9, 0.9)
    corr = np.eye(p + M)
    corr[p:, :p] = beta
    corr[:p, p:] = beta.T
    return mvivw.run("unused", 1000, mode="skeleton", data=(adj, corr, p, None), model=model)


def test_writer_header_order_and_fills(tmp_path):
    from scipy.special import ndtr

    from cigwas_amd import mvivw

    res = _result_on_small_adjacency(mvivw)
    assert res["status"].tolist() == [0, 0, 0, 1]
    assert [len(I) for I, _ in res["selection"]] == [5, 7, 5, 3]
    path = str(tmp_path / "all_merged_mvivw_results.tsv")
    mvivw.write_results(path, res)
    lines = open(path).read().split("\n")
    assert lines[0] == "source\tsink\teffect\tp\tsk_adj\tnum_snps\tse" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert [(int(r[0]), int(r[1])) for r in rows] == [(e + 1, o + 1) for o in range(4) for e in range(4) if e != o]
    by = {(int(r[0]), int(r[1])): r for r in rows}
    r = by[(2, 1)]  # exposure 1 -> outcome 0: estimated
    th, se = float(res["theta"][0][0]), float(res["se"][0][0])
    assert r[2] == "%.15g" % th and r[6] == "%.15g" % se and r[3] == "%.15g" % (2 * ndtr(-abs(th / se))) and r[4] == "TRUE"
    assert by[(3, 1)][2:5] == ["0", "1", "FALSE"] and by[(3, 1)][6] == "NA"       # not in E
    assert by[(3, 4)][2:5] == ["0", "1", "FALSE"] and by[(3, 4)][6] == "NA"       # status 1
    assert by[(3, 4)][5] == "3" and by[(2, 1)][5] == "5" and by[(1, 2)][5] == "7"
    out = str(tmp_path / "o.tsv")
    mvivw.write_outcomes(out, res)
    olines = open(out).read().split("\n")
    assert olines[0] == "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus"
    first = olines[1].split("\t")
    assert first[0] == "1" and first[1] == "1" and first[6] == "0" and first[4] == "%.15g" % res["stats"][0][0]
    assert olines[4].split("\t") == ["4", "0", "3", "NA", "NA", "NA", "1"]


def test_writer_status_2_gives_na_and_a_line_on_stderr(tmp_path, capsys):
    from cigwas_amd import mvivw

    beta, w, lists = status_batch()
    p = beta.shape[1]
    sel = [(np.arange(600), np.array([t for t in range(p) if t != o])) for o in range(p)]  # 3 and 7 are one column
    iv_off, iv, ex_off, ex = mvivw.pack(sel)
    theta, se, stats, status, _ = mvivw.HostEngine().mvivw(beta, w, np.arange(p), iv_off, iv, ex_off, ex)
    assert status.tolist() == [2] * 3 + [0] + [2] * 3 + [0] + [2] * 4  # only the problems without both columns factor
    res = {"p": p, "selection": sel, "status": status, "stats": stats, "sk_adj": np.zeros((p, p), bool),
           "theta": [theta[ex_off[o]:ex_off[o + 1]] if status[o] == 0 else None for o in range(p)],
           "se": [se[ex_off[o]:ex_off[o + 1]] if status[o] == 0 else None for o in range(p)]}
    path = str(tmp_path / "r.tsv")
    mvivw.write_results(path, res)
    err = capsys.readouterr().err
    assert "outcome trait 1 (1-based): status 2" in err and "outcome trait 4 " not in err
    rows = [l.split("\t") for l in open(path).read().split("\n")[1:-1]]
    assert all(r[2] == r[3] == r[6] == "NA" for r in rows if r[1] == "1")
    assert all(r[2] != "NA" for r in rows if r[1] == "4")


# ---- ABI and CLI ----
def test_symbol_is_declared_and_exported():
    from cigwas_amd._lib import SO_PATH, SYMBOLS

    _vp, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert SYMBOLS["cusk_mvivw"] == (_i, [_vp, _vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusk_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int cusk_mvivw(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, "
            "const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, "
            "double *theta, double *se, double *stats, int *status, float *kernel_ms);") in hdr
    assert hasattr(ctypes.CDLL(SO_PATH), "cusk_mvivw")


def test_argparse_surface():
    from cigwas_amd import cli

    parser = cli.build_parser()
    a = parser.parse_args(["mvivw", "out/stem", "1000"])
    assert (a.cusk_output_stem, a.num_samples, a.s, a.orientation_prior, a.ivs, a.het, a.model, a.out) == \
        ("out/stem", 1000, False, None, None, False, "default", None)
    a = parser.parse_args(["mvivw", "s", "5", "-s", "--het", "--model", "fixed", "--out", "x.tsv"])
    assert a.s and a.het and a.model == "fixed" and a.out == "x.tsv"
    assert parser.parse_args(["mvivw", "s", "5", "--orientation-prior", "p.bin"]).orientation_prior == "p.bin"
    assert parser.parse_args(["mvivw", "s", "5", "--ivs", "t.csv", "--model", "random"]).ivs == "t.csv"
    for bad in (["mvivw", "s", "5", "-s", "--orientation-prior", "p.bin"],  # -s and a prior exclude each other
                ["mvivw", "s", "0"],
                ["mvivw", "s"],
                ["mvivw", "s", "5", "--model", "robust"],
                ["mvivw", "s", "5", "--ivs"]):
        with pytest.raises(SystemExit) as ex:
            parser.parse_args(bad)
        assert ex.value.code == 2


@pytest.fixture()
def host_cli(monkeypatch):
    """the command line on the numpy form: no device"""
    from cigwas_amd import cli

    monkeypatch.setattr(cli, "_mvivw_engine", lambda: None)
    return cli


def parse_results(path):
    rows = [l.split("\t") for l in open(path).read().split("\n")[1:-1]]
    num = lambda s: np.nan if s == "NA" else float(s)  # noqa: E731
    return {(int(r[0]), int(r[1])): (num(r[2]), num(r[3]), r[4], int(r[5]), num(r[6])) for r in rows}


def test_cli_end_to_end_on_a_golden_skeleton(host_cli, tmp_path):
    from cigwas_amd import ivcheck, mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    host_cli.main(["mvivw", stem, str(N)])
    assert open(stem + "_iv_candidates.csv").readline() == "Exposure,Outcome,IV\n"
    got = parse_results(stem + "_mvivw_results.tsv")
    res = mvivw.run(stem, N)
    p = res["p"]
    assert sorted(got) == sorted((e + 1, o + 1) for o in range(p) for e in range(p) if e != o)
    assert (res["status"] == 0).any()
    adj = ivcheck.load(stem)[0]
    for o in range(p):
        I, E = res["selection"][o]
        for j, e in enumerate(E):
            eff, pv, sk, ns, se = got[(int(e) + 1, o + 1)]
            assert ns == len(I) and sk == ("TRUE" if adj[e, o] != 0 else "FALSE")
            if res["status"][o] == 0:
                assert eff == float("%.15g" % res["theta"][o][j]) and se == float("%.15g" % res["se"][o][j]) and 0 <= pv <= 1
    outcomes = open(stem + "_mvivw_outcomes.tsv").read().split("\n")
    assert len(outcomes) == p + 2 and outcomes[0].startswith("sink\t")
    # --out names both files
    host_cli.main(["mvivw", stem, str(N), "-s", "--out", str(tmp_path / "skel_results.tsv")])
    assert os.path.exists(tmp_path / "skel_results.tsv") and os.path.exists(tmp_path / "skel_outcomes.tsv")


def test_cli_ivs_table_written_by_write_csv(host_cli, tmp_path):
    from cigwas_amd import ivcheck, mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    rows = ivcheck.iv_candidates(stem)
    assert rows
    table = str(tmp_path / "ivs.csv")
    ivcheck.write_csv(table, rows)
    assert mvivw.read_ivs(table) == [tuple(r) for r in rows]
    host_cli.main(["mvivw", stem, str(N), "--ivs", table])
    got = parse_results(stem + "_mvivw_results.tsv")
    res = mvivw.run(stem, N, mode="ivs", ivs_path=table)
    for o in range(res["p"]):
        I, E = res["selection"][o]
        assert sorted(I.tolist()) == sorted({v - 1 for e, oo, v in rows if oo == o + 1})
        assert sorted(E.tolist()) == sorted({e - 1 for e, oo, v in rows if oo == o + 1})
        for e in range(res["p"]):
            if e != o:
                assert got[(e + 1, o + 1)][3] == len(I)


def test_cli_het_with_a_missing_ssz_file(host_cli, tmp_path):
    from cigwas_amd import mvivw

    stem = materialise("p6", tmp_path)
    with pytest.raises(FileNotFoundError, match="_ssz.mtx is missing"):
        mvivw.run(stem, 1000, het=True)
    with pytest.raises(FileNotFoundError, match="_ssz.mtx is missing"):
        host_cli.main(["mvivw", stem, "1000", "--het"])
    assert not os.path.exists(stem + "_mvivw_results.tsv")


def test_het_sizes_enter_the_weights(tmp_path):
    from test_sepselect_het_formats import write_ssz

    from cigwas_amd import ivcheck, mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    n = ivcheck.load(stem)[1].shape[0]
    write_ssz(stem, np.full((n, n), N, np.int64))
    plain, het = mvivw.run(stem, N), mvivw.run(stem, 1, het=True)
    for o in range(plain["p"]):
        assert plain["status"][o] == het["status"][o]
        if plain["status"][o] == 0:
            assert plain["theta"][o].tobytes() == het["theta"][o].tobytes() and plain["se"][o].tobytes() == het["se"][o].tobytes()
    sizes = np.full((n, n), N, np.int64)
    sizes[:, 0] = sizes[0, :] = 2  # a size <= 2: the weight is not finite
    write_ssz(stem, sizes)
    assert plain["status"][0] == 0 and mvivw.run(stem, 1, het=True)["status"][0] == 3


# ---- the plan under the host sanitizers ----
def test_plan_selftest_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mvivw_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "mvivw_plan_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mvivw_plan_selftest: ok" in r.stdout, r.stdout + r.stderr
