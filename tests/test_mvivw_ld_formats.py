"""CPU: `ci-gwas mvivw --ld` (ci-gwas_amd/mvivw.py): the numpy host form of the rule of include/cusk_hip.h above
`cusk_mvivw_ld` (`HostEngine.mvivw_ld`, `solve_one_ld`), the `ld_pivot` column and the command line.

The yardstick is a numpy LONGDOUBLE restatement of the DIRECT formula theta = (X' Om^-1 X)^-1 X' Om^-1 y, Om = diag(s) R_l
diag(s), s = 1 / sqrt(w), with v from the inverse's diagonal and rss = r' Om^-1 r, by hand-written Gauss-Jordan elimination
(no whitening, no Cholesky), not R.  Inputs: `synth_problem` for beta, R block-diagonal AR(1), rho^|a-b| in blocks of 50,
rho = 0.6.  Asserted on the inputs: cond(R) <= 100 and the condition of the unit-diagonal X' Om^-1 X <= 1e4.  Bound 1e-7 on
max|x - x_ref| / max|x_ref| for theta, se, sigma and rss, from cond(R) * cond(G) * k * eps = 100 * 1e4 * 128 * 1.1e-16 ~
1.4e-8 with the margin the plain sweep takes over its own product.  The device runs the same cases in test_gpu_mvivw_ld.py.

The instrument lists of the ABI ascend (the argument errors are those of `cusk_mvivw`), so "a permutation of the
instrument list" is a relabelling of the marker rows: the rows of beta and weight and the rows and columns of ld are
permuted together and the list is the ascending one in the new numbering.  The list ORDER of the markers, which the
factorisation walks and the gather indexes by, is what changes."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from test_iv_check_formats import load_kat, materialise
from test_mvivw_formats import N_SAMPLES, gauss_jordan_ld, one_call, problem, rel, synth_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_BOUND = 1e-7
LD_SHAPES = ((5, 1, 0.0), (9, 7, 0.5), (130, 7, 0.9), (300, 7, 0.9), (400, 39, 0.9), (330, 64, 0.5))


def ar1_ld(M, block=50, rho=0.6):
    """block-diagonal AR(1): rho^|a - b| inside blocks of `block` consecutive markers, 0 between blocks"""
    idx = np.arange(M)
    R = rho ** np.abs(idx[:, None] - idx[None, :]).astype(np.float64)
    R[(idx[:, None] // block) != (idx[None, :] // block)] = 0.0
    return R


def with_duplicate(M, i, j):
    """AR(1) blocks over M - 1 distinct markers; marker row j of the M x M result is a copy of marker row i (i < j): equal
    rows of R and R[j, i] = 1"""
    base = ar1_ld(M - 1)
    src = list(range(M - 1))
    src.insert(j, i)
    return base[np.ix_(src, src)]


def conditions(X, w, R):
    """(cond(R), cond of the unit-diagonal X' Om^-1 X)"""
    sw = np.sqrt(w)
    Xs = X * sw[:, None]
    G = Xs.T @ np.linalg.solve(R, Xs)
    d = np.sqrt(np.diag(G))
    return float(np.linalg.cond(R)), float(np.linalg.cond(G / np.outer(d, d)))


@functools.lru_cache(maxsize=None)
def longdouble_direct(m, k, rho, ridge=0.0, model=0):
    """(theta, se, sigma, rss) of the direct formula in longdouble"""
    beta, w = problem(m, k, rho)
    X, y, wl = (np.array(a, np.longdouble) for a in (beta[:, :k], beta[:, k], w[:, k]))
    s = 1 / np.sqrt(wl)
    R = np.array(ar1_ld(m), np.longdouble) * (1 - np.longdouble(ridge))
    R[np.arange(m), np.arange(m)] = 1
    Om = R * s[:, None] * s[None, :]
    Oi = gauss_jordan_ld(Om, np.eye(m, dtype=np.longdouble))
    G = X.T @ Oi @ X
    b = X.T @ (Oi @ y)
    sol = gauss_jordan_ld(G, np.concatenate([b[:, None], np.eye(k, dtype=np.longdouble)], axis=1))
    theta, v = sol[:, 0], np.diag(sol[:, 1:])
    r = y - X @ theta
    rss = r @ (Oi @ r)
    sigma = np.sqrt(rss / (m - k))
    random = model == 1 or (model == 0 and m >= 4)
    se = np.sqrt(v) * (max(sigma, np.longdouble(1)) if random else 1)
    return theta, se, sigma, rss


# ---- the host form against longdouble ----
@pytest.mark.parametrize("shape", LD_SHAPES)
def test_host_form_against_the_direct_formula_in_longdouble(shape):
    """worst distance over the six cases: 2.4e-14 at (400, 39, .9) (float64 whitening against the longdouble direct formula)"""
    from cigwas_amd import mvivw

    m, k, rho = shape
    beta, w = problem(*shape)
    R = ar1_ld(m)
    cr, cg = conditions(beta[:, :k], w[:, k], R)
    assert cr <= 100 and cg <= 1e4, (cr, cg)
    worst = 0.0
    for ridge in (0.0, 0.25):
        th_ref, se_ref, sigma_ref, rss_ref = longdouble_direct(m, k, rho, ridge)
        theta, se, stats, status, _ = mvivw.HostEngine().mvivw_ld(beta, w, R, **one_call(beta, k), ridge=ridge)
        assert status[0] == 0 and 1e-8 <= stats[0, 2] <= 1.0
        worst = max(worst, rel(theta[:k], th_ref), rel(se[:k], se_ref), rel(stats[0, 1], sigma_ref), rel(stats[0, 0], rss_ref))
    print(shape, "cond(R)", cr, "cond(G)", cg, "worst", worst)
    assert worst <= LD_BOUND, (shape, worst)


# ---- reductions ----
def test_identity_ld_is_the_plain_rule():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    for shape in ((9, 7, 0.5), (300, 7, 0.9), (700, 39, 0.9)):
        beta, w = problem(*shape)
        m, k = shape[:2]
        call = one_call(beta, k)
        plain = eng.mvivw(beta, w, **call)
        upper = np.triu(np.full((m, m), np.nan))  # the diagonal and everything above it: never read
        got = eng.mvivw_ld(beta, w, upper, **call)
        assert got[3][0] == 0 and got[2][0, 2] == 1.0
        assert max(rel(got[0][:k], plain[0][:k]), rel(got[1][:k], plain[1][:k]), rel(got[2][0, :2], plain[2][0, :2])) <= 1e-12


def test_ridge_is_the_shrunk_matrix_built_by_hand():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    beta, w = problem(300, 7, 0.9)
    R, lam = ar1_ld(300), 0.3
    hand = (1.0 - lam) * R + lam * np.eye(300)
    a = eng.mvivw_ld(beta, w, R, **one_call(beta, 7), ridge=lam)
    b = eng.mvivw_ld(beta, w, hand, **one_call(beta, 7))
    c = eng.mvivw_ld(beta, w, R, **one_call(beta, 7))
    assert max(rel(a[0][:7], b[0][:7]), rel(a[1][:7], b[1][:7]), rel(a[2][0], b[2][0])) <= 1e-12
    assert rel(a[0][:7], c[0][:7]) > 1e-6  # and the ridge does change the estimates
    for bad in (1.0, -0.1, np.nan, 2.0):
        with pytest.raises(ValueError, match="ridge"):
            eng.mvivw_ld(beta, w, R, **one_call(beta, 7), ridge=bad)


def relabel(beta, w, R, perm):
    """new marker row a is old marker row perm[a]"""
    return np.ascontiguousarray(beta[perm]), np.ascontiguousarray(w[perm]), np.ascontiguousarray(R[np.ix_(perm, perm)])


def test_a_permutation_of_the_instruments_changes_nothing_beyond_the_bound():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    for shape in ((300, 7, 0.9), (130, 7, 0.9)):
        m, k, _ = shape
        beta, w = problem(*shape)
        R = ar1_ld(m)
        first = eng.mvivw_ld(beta, w, R, **one_call(beta, k))
        for seed in (1, 2):
            perm = np.random.default_rng(seed).permutation(m)
            b2, w2, R2 = relabel(beta, w, R, perm)
            got = eng.mvivw_ld(b2, w2, R2, **one_call(b2, k))
            assert got[3][0] == 0
            assert max(rel(got[0][:k], first[0][:k]), rel(got[1][:k], first[1][:k]), rel(got[2][0, 0], first[2][0, 0])) <= LD_BOUND
        # a sub-list: the gather must index by the list, not by position
        I = np.sort(np.random.default_rng(3).choice(m, size=m // 2, replace=False))
        sub = eng.mvivw_ld(beta, w, R, outcome=[k], iv_off=[0, len(I)], iv=I, ex_off=[0, k], ex=np.arange(k))
        own = eng.mvivw_ld(beta[I], w[I], R[np.ix_(I, I)], **one_call(beta[I], k))
        assert sub[0].tobytes() == own[0].tobytes() and sub[1].tobytes() == own[1].tobytes() and sub[2].tobytes() == own[2].tobytes()


# ---- status 4 ----
DUPLICATES = {"early": (0, 1), "middle": (60, 149), "last": (100, 299)}


@pytest.mark.parametrize("where", sorted(DUPLICATES))
def test_a_duplicated_marker_gives_status_4(where):
    from cigwas_amd import mvivw

    beta, w = problem(300, 7, 0.9)
    i, j = DUPLICATES[where]
    R = with_duplicate(300, i, j)
    assert np.array_equal(R[i], R[j]) and R[j, i] == 1.0
    theta, se, stats, status, _ = mvivw.HostEngine().mvivw_ld(beta, w, R, **one_call(beta, 7))
    assert status[0] == 4 and np.all(np.isnan(theta[:7])) and np.all(np.isnan(se[:7]))
    assert np.isnan(stats[0, 0]) and np.isnan(stats[0, 1]) and abs(stats[0, 2]) <= 1e-12
    # without row j the rest factors
    I = np.delete(np.arange(300), j)
    ok = mvivw.HostEngine().mvivw_ld(beta, w, R, outcome=[7], iv_off=[0, 299], iv=I, ex_off=[0, 7], ex=np.arange(7))
    assert ok[3][0] == 0
    # and a ridge makes the whole list factor: the pivot of the copy is 1 - (1 - l)^2 = 0.19 when nothing earlier is in LD
    # with the pair, and a little less otherwise
    shrunk = mvivw.HostEngine().mvivw_ld(beta, w, R, **one_call(beta, 7), ridge=0.1)
    assert shrunk[3][0] == 0 and 0.15 <= shrunk[2][0, 2] <= 0.19 + 1e-12


def pair_ld(M, r, a=3, b=17):
    R = np.zeros((M, M))
    R[b, a] = r
    return R


def test_both_sides_of_the_pivot_rule():
    from cigwas_amd import mvivw

    beta, w = problem(300, 7, 0.9)
    call = one_call(beta, 7)
    ok = mvivw.HostEngine().mvivw_ld(beta, w, pair_ld(300, np.sqrt(1.0 - 2e-8)), **call)
    assert ok[3][0] == 0 and abs(ok[2][0, 2] - 2e-8) <= 1e-12 and np.all(np.isfinite(ok[0][:7]))
    fail = mvivw.HostEngine().mvivw_ld(beta, w, pair_ld(300, np.sqrt(1.0 - 0.5e-8)), **call)
    assert fail[3][0] == 4 and abs(fail[2][0, 2] - 0.5e-8) <= 1e-12 and np.all(np.isnan(fail[0][:7]))
    neg = mvivw.HostEngine().mvivw_ld(beta, w, pair_ld(300, -np.sqrt(1.0 - 0.5e-8)), **call)
    assert neg[3][0] == 4


# ---- status 3 and the order of the statuses ----
def test_status_3_only_for_entries_that_are_read():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    beta, w = problem(300, 7, 0.9)
    R = ar1_ld(300)
    I = np.arange(0, 300, 2)
    call = dict(outcome=[7], iv_off=[0, len(I)], iv=I, ex_off=[0, 7], ex=np.arange(7))
    first = eng.mvivw_ld(beta, w, R, **call)
    assert first[3][0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        R2 = R.copy()
        R2[10, 4] = bad  # both in the list, below the diagonal
        got = eng.mvivw_ld(beta, w, R2, **call)
        assert got[3][0] == 3 and np.all(np.isnan(got[0][:7])) and np.all(np.isnan(got[2][0]))
    R3 = R.copy()
    R3[np.triu_indices(300)] = np.nan  # on and above the diagonal
    R3[11, 4] = R3[10, 5] = R3[299, 1] = np.nan  # below it, but a row or a column outside the list
    same = eng.mvivw_ld(beta, w, R3, **call)
    for a, b in zip(first[:4], same[:4]):
        assert a.tobytes() == b.tobytes()
    b2 = np.array(beta)
    b2[4, 2] = np.nan
    assert eng.mvivw_ld(b2, w, R, **call)[3][0] == 3
    w2 = np.array(w)
    w2[6, 7] = 0.0
    assert eng.mvivw_ld(beta, w2, R, **call)[3][0] == 3


def test_precedence_1_then_3_then_4_then_2():
    from cigwas_amd import mvivw

    eng = mvivw.HostEngine()
    base = synth_problem(300, 8, 0.5, 11)  # traits 0 .. 7, outcome 8
    beta = np.concatenate([base, base[:, :1]], axis=1)  # trait 9 is a copy of trait 0
    w = mvivw.weights(beta, N_SAMPLES)
    dup = with_duplicate(300, 20, 200)
    nan_dup = dup.copy()
    nan_dup[250, 3] = np.nan

    def status(ld, I, E):
        return int(eng.mvivw_ld(beta, w, ld, outcome=[8], iv_off=[0, len(I)], iv=I, ex_off=[0, len(E)], ex=E)[3][0])

    every, cols, twice = np.arange(300), np.arange(8), np.array([0, 1, 2, 9])
    assert status(nan_dup, np.arange(4), twice) == 1    # m <= k: nothing is looked at
    assert status(nan_dup, every, twice) == 3           # a NaN that is read, a duplicated marker and a duplicated column
    assert status(dup, every, twice) == 4               # R fails before the Gram is formed
    assert status(dup, np.delete(every, 200), twice) == 2
    assert status(dup, np.delete(every, 200), cols) == 0
    assert status(nan_dup, np.delete(every, 250), cols) == 4


# ---- files, command line, ABI ----
@pytest.fixture()
def host_cli(monkeypatch):
    """the command line on the numpy form: no device"""
    from cigwas_amd import cli

    monkeypatch.setattr(cli, "_mvivw_engine", lambda: None)
    return cli


def plant_ld(stem, pair=None):
    """rewrite the marker block of <stem>_scm.mtx to the AR(1) blocks, with marker `pair[1]` a copy of marker `pair[0]`"""
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    from cigwas_amd import ivcheck

    _, corr, p, _ = ivcheck.load(stem)
    M = corr.shape[0] - p
    corr[p:, p:] = ar1_ld(M) if pair is None else with_duplicate(M, *pair)
    mmwrite(stem + "_scm.mtx", coo_matrix(corr), precision=17)
    return p, M


def test_argparse_surface_of_ld():
    from cigwas_amd import cli

    parser = cli.build_parser()
    a = parser.parse_args(["mvivw", "s", "5"])
    assert a.ld is False and a.ld_ridge is None
    a = parser.parse_args(["mvivw", "s", "5", "--ld", "--ld-ridge", "0.25", "-s", "--het"])
    assert a.ld and a.ld_ridge == 0.25 and a.s and a.het
    for bad in (["mvivw", "s", "5", "--ld", "--ld-ridge", "-0.1"], ["mvivw", "s", "5", "--ld", "--ld-ridge"],
                ["mvivw", "s", "5", "--ld", "--ld-ridge", "x"]):
        with pytest.raises(SystemExit) as ex:
            parser.parse_args(bad)
        assert ex.value.code == 2


@pytest.mark.parametrize("argv", (["--ld-ridge", "0.1"], ["--ld", "--ld-ridge", "1"], ["--ld", "--ld-ridge", "nan"]))
def test_cli_argument_rules(host_cli, tmp_path, argv):
    stem = materialise("p6", tmp_path)
    with pytest.raises(SystemExit) as ex:
        host_cli.main(["mvivw", stem, "1000"] + argv)
    assert ex.value.code == 2 and not os.path.exists(stem + "_mvivw_results.tsv") and not os.path.exists(stem + "_iv_candidates.csv")


def test_ld_pivot_column_only_with_ld_and_both_files_unchanged_without(host_cli, tmp_path, capsys):
    from cigwas_amd import mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    p, M = plant_ld(stem)
    host_cli.main(["mvivw", stem, str(N)])
    res = mvivw.run(stem, N)
    assert res.pop("ld") is False  # the dictionary the writers were given before there was an `ld`
    mvivw.write_results(str(tmp_path / "r.tsv"), res)
    mvivw.write_outcomes(str(tmp_path / "o.tsv"), res)
    plain_r, plain_o = open(stem + "_mvivw_results.tsv", "rb").read(), open(stem + "_mvivw_outcomes.tsv", "rb").read()
    assert plain_r == open(tmp_path / "r.tsv", "rb").read() and plain_o == open(tmp_path / "o.tsv", "rb").read()
    assert plain_o.split(b"\n")[0] == b"sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus"
    assert plain_r.split(b"\n")[0] == b"source\tsink\teffect\tp\tsk_adj\tnum_snps\tse"
    # a run with --ld in between leaves a later plain run what it was
    out = str(tmp_path / "ld_results.tsv")
    host_cli.main(["mvivw", stem, str(N), "--ld", "--out", out])
    lines = open(tmp_path / "ld_outcomes.tsv").read().split("\n")
    assert lines[0] == "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus\tld_pivot"
    with_ld = mvivw.run(stem, N, ld=True)
    assert (with_ld["status"] == 0).any()
    for o, line in enumerate(lines[1:-1]):
        f = line.split("\t")
        st = int(with_ld["status"][o])
        assert len(f) == 8 and int(f[6]) == st
        assert f[7] == ("%.15g" % with_ld["stats"][o][2] if st in (0, 4) else "NA")
    assert open(out).read().split("\n")[0] == "source\tsink\teffect\tp\tsk_adj\tnum_snps\tse"
    host_cli.main(["mvivw", stem, str(N), "--out", str(tmp_path / "again_results.tsv")])
    assert open(tmp_path / "again_results.tsv", "rb").read() == plain_r and open(tmp_path / "again_outcomes.tsv", "rb").read() == plain_o
    with pytest.raises(ValueError, match="ld_ridge without ld"):
        mvivw.run(stem, N, ld_ridge=0.1)


def test_status_4_rows_are_na_with_a_line_on_stderr(host_cli, tmp_path, capsys):
    from cigwas_amd import mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    res = mvivw.run(stem, N)
    lists = [set(I.tolist()) for I, _ in res["selection"]]
    good = [o for o in range(res["p"]) if res["status"][o] == 0]
    a, b = sorted(set.intersection(*[lists[o] for o in good]))[:2]  # two markers every estimated outcome uses
    plant_ld(stem, (a, b))
    capsys.readouterr()
    out = str(tmp_path / "ld_results.tsv")
    host_cli.main(["mvivw", stem, str(N), "--ld", "--out", out])
    err = capsys.readouterr().err
    with_ld = mvivw.run(stem, N, ld=True)
    assert all(with_ld["status"][o] == 4 for o in good) and good
    assert f"outcome trait {good[0] + 1} (1-based): status 4" in err and "--ld-ridge" in err and "prune-bed" in err
    rows = [l.split("\t") for l in open(out).read().split("\n")[1:-1]]
    hit = [r for r in rows if int(r[1]) == good[0] + 1 and int(r[0]) - 1 in set(res["selection"][good[0]][1].tolist())]
    assert hit and all(r[2] == r[3] == r[6] == "NA" for r in hit)
    orow = open(tmp_path / "ld_outcomes.tsv").read().split("\n")[1 + good[0]].split("\t")
    assert orow[3:7] == ["NA", "NA", "NA", "4"] and abs(float(orow[7])) <= 1e-12
    host_cli.main(["mvivw", stem, str(N), "--ld", "--ld-ridge", "0.1", "--out", out])
    assert all(mvivw.run(stem, N, ld=True, ld_ridge=0.1)["status"][o] == 0 for o in good)
    assert all(l.split("\t")[6] != "4" for l in open(tmp_path / "ld_outcomes.tsv").read().split("\n")[1:-1])


def test_symbol_is_declared_and_exported():
    from cigwas_amd._lib import SO_PATH, SYMBOLS

    _vp, _i, _ll, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    assert SYMBOLS["cusk_mvivw_ld"] == (_i, [_vp, _vp, _vp, _vp, _d, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusk_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int cusk_mvivw_ld(cusk_engine *e, const double *beta, const double *weight, const double *ld, double ridge, "
            "long long M, int p, int nout, const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, "
            "const int *ex, int model, double *theta, double *se, double *stats, int *status, float *kernel_ms);") in hdr
    so = ctypes.CDLL(SO_PATH)
    assert hasattr(so, "cusk_mvivw_ld")
    so.cusk_mvivw_ld.restype = _i
    so.cusk_mvivw_ld.argtypes = SYMBOLS["cusk_mvivw_ld"][1]
    # a null engine is refused before anything else is looked at: no device needed
    assert so.cusk_mvivw_ld(None, None, None, None, 0.0, 1, 1, 0, None, None, None, None, None, 0, None, None, None, None, None) == 2


# ---- the plan under the host sanitizers ----
def test_plan_selftest_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mvivw_ld_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "mvivw_ld_plan_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mvivw_ld_plan_selftest: ok" in r.stdout, r.stdout + r.stderr
