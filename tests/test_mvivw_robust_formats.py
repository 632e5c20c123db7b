"""`mvivw --robust` without a device: the ABI, the argument errors, the command line, the files, and the float64 host form
(`mvivw.solve_one_robust`, the yardstick of test_gpu_mvivw_robust.py) against the same rule evaluated in np.longdouble.

The longdouble form is `solve_one_robust` itself handed longdouble arrays: every operation of the rule then runs in the
wider type (the triangular inverse by plain loops, scipy having no such solver).  It measures what float64 rounding does
to the iteration; it is not a second implementation.

Distances float64 - longdouble over `cases()`, both psi, measured once (largest): theta 3.3e-15 in the units
d_j |theta_j| / (s sqrt(m)), se 2.9e-15, s 4.9e-15, tau 2.7e-15 relative, rho 8.9e-15 absolute: tens of units of 1.1e-16, as
sums of a few hundred terms give.  HOST_DISTANCE below is what the tests hold the host form to (the measured figures with
room for another platform's libm and BLAS); the device bound of test_gpu_mvivw_robust.py is derived from the measured ones."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DISTANCE = 1e-13   # above every measured float64 - longdouble distance of the header
PLANT_SEED = 11         # chosen so that the margins of test_planted_shifts hold by a factor of two (asserted there)
W = 1e4                 # weight of every row: standardised units are 1 / sqrt(W)


def planted(m=400, k=3, frac=0.1, shift=8.0, seed=PLANT_SEED):
    """X, y, w, theta, planted: the rows with the largest first exposure (strong instruments with a direct effect on the
    outcome) have y shifted by `shift` standardised units"""
    rng = np.random.default_rng(seed)
    X = 0.05 * rng.standard_normal((m, k))
    theta = np.array([0.3, -0.2, 0.5, 0.1, -0.4][:k] if k <= 5 else 0.3 * rng.standard_normal(k) / np.sqrt(k))
    w = np.full(m, W)
    y = X @ theta + rng.standard_normal(m) / np.sqrt(w)
    mask = np.zeros(m, bool)
    mask[np.argsort(-X[:, 0])[:int(round(frac * m))]] = True
    y[mask] += shift / np.sqrt(w[mask])
    return X, y, w, theta, mask


def cases():
    """(name, X, y, w) of the problems both test files share: the planted table, one without outliers, and the tile and
    chunk edges with 5 % planted rows"""
    out = [("planted", *planted()[:3]), ("clean", *planted(frac=0.0)[:3])]
    for k, m in ((1, 2), (2, 255), (43, 256), (44, 257), (45, 513)):
        out.append((f"k{k}-m{m}", *planted(m=m, k=k, frac=0.05, seed=100 + k)[:3]))
    return out


def distance(a, b, X, w, m):
    """largest distance of two results of solve_one_robust: theta in the stopping rule's units, the rest relative, rho absolute"""
    d = np.sqrt(np.sum(np.asarray(X, np.float64) ** 2 * np.asarray(w, np.float64)[:, None], axis=0))
    s = float(b[3][1])
    out = [float(np.max(d * np.abs(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64)))) / (s * np.sqrt(m))]
    out.append(float(np.max(np.abs(np.asarray(a[2], np.float64) / np.asarray(b[2], np.float64) - 1))))
    out += [abs(float(a[3][c]) / float(b[3][c]) - 1) for c in (1, 2)]
    out.append(float(np.max(np.abs(np.asarray(a[4], np.float64) - np.asarray(b[4], np.float64)))))
    return out


# ---- ABI ----
def test_symbols_are_declared_and_exported():
    from cigwas_amd._lib import SO_PATH, SYMBOLS

    _vp, _i, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert SYMBOLS["cusk_mvivw_robust"] == (_i, [_vp, _vp, _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp,
                                                 _vp, _vp, _vp])
    assert SYMBOLS["cusk_abs_median"] == (_i, [_vp, _vp, _vp, _i, _vp])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusk_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int cusk_mvivw_robust(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, "
            "const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, int psi, "
            "double *theta, double *se, double *stats, int *status, double *rho, float *kernel_ms);") in hdr
    assert "int cusk_abs_median(cusk_engine *e, const double *vals, const long long *seg_off, int nseg, double *out);" in hdr
    so = ctypes.CDLL(SO_PATH)
    assert hasattr(so, "cusk_mvivw_robust") and hasattr(so, "cusk_abs_median")


# ---- arguments ----
def _one_call():
    X, y, w, _, _ = planted()
    beta = np.concatenate([X, y[:, None]], axis=1)
    return beta, np.tile(w[:, None], (1, 4)), dict(outcome=np.array([3]), iv_off=np.array([0, 400]), iv=np.arange(400),
                                                   ex_off=np.array([0, 3]), ex=np.arange(3))


def test_argument_errors_of_the_host_form():
    from cigwas_amd import mvivw

    beta, w, call = _one_call()
    H = mvivw.HostEngine()
    for psi in (0, 3, -1):
        with pytest.raises(ValueError, match="psi"):
            H.mvivw_robust(beta, w, **call, psi=psi)
    bad = [dict(call, outcome=np.array([4])), dict(call, iv=np.arange(400)[::-1].copy()), dict(call, ex=np.array([0, 1, 3])),
           dict(call, ex=np.array([0, 2, 1])), dict(call, iv_off=np.array([5, 0])), dict(call, iv=np.arange(1, 401))]
    for c in bad:  # every argument error of cusk_mvivw still applies
        with pytest.raises(ValueError):
            H.mvivw_robust(beta, w, **c)
    with pytest.raises(ValueError, match="model"):
        H.mvivw_robust(beta, w, **call, model=3)
    data = (np.zeros((5, 5), np.int32), np.eye(5), 2, None)
    with pytest.raises(ValueError, match="robust with ld"):
        mvivw.run("unused", 100, data=data, ld=True, robust="huber")
    with pytest.raises(ValueError, match="not huber or bisquare"):
        mvivw.run("unused", 100, data=data, robust="tukey")


def test_argparse_surface(capsys):
    from cigwas_amd import cli

    parser = cli.build_parser()
    assert parser.parse_args(["mvivw", "s", "5"]).robust is None
    assert parser.parse_args(["mvivw", "s", "5", "--robust"]).robust == "bisquare"
    assert parser.parse_args(["mvivw", "--robust", "huber", "s", "5"]).robust == "huber"
    a = parser.parse_args(["mvivw", "s", "5", "--robust", "bisquare", "--robust-weights", "w.tsv", "--het", "-s", "--model", "fixed"])
    assert (a.robust, a.robust_weights, a.het, a.s, a.model) == ("bisquare", "w.tsv", True, True, "fixed")
    with pytest.raises(SystemExit) as ex:
        parser.parse_args(["mvivw", "--robust", "lmrob", "s", "5"])
    assert ex.value.code == 2
    for argv, word in ((["mvivw", "s", "5", "--robust", "--ld"], "whitening"), (["mvivw", "s", "5", "--robust-weights", "f"], "needs --robust")):
        with pytest.raises(SystemExit) as ex:  # refused before any file is read
            cli.main(argv)
        assert ex.value.code == 2 and word in capsys.readouterr().err


# ---- files ----
PARENT_RESULTS = (
    "source\tsink\teffect\tp\tsk_adj\tnum_snps\tse\n2\t1\t-0.205009434883199\t0.247276828288404\tTRUE\t5\t0.177192197590602\n"
    "3\t1\t0\t1\tFALSE\t5\tNA\n4\t1\t0\t1\tFALSE\t5\tNA\n1\t2\t-1.01559313921273\t0.0356980455508688\tTRUE\t7\t0.483535143267394\n"
    "3\t2\t0.291244828659912\t0.494502279360118\tTRUE\t7\t0.426316660931882\n4\t2\t0\t1\tFALSE\t7\tNA\n1\t3\t0\t1\tFALSE\t5\tNA\n"
    "2\t3\t0.11164930629625\t0.786670636359143\tTRUE\t5\t0.412543448475428\n4\t3\t0\t1\tFALSE\t5\tNA\n1\t4\t0\t1\tFALSE\t3\tNA\n"
    "2\t4\t0\t1\tFALSE\t3\tNA\n3\t4\t0\t1\tFALSE\t3\tNA\n")
PARENT_OUTCOMES = (
    "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus\n1\t1\t5\t0.898639367811444\t3.23021085352221\t0.520065239917822\t0\n"
    "2\t2\t7\t1.72969393772889\t14.9592055910804\t0.0105380756806654\t0\n"
    "3\t1\t5\t2.32550140430079\t21.6318271256197\t0.000237233342692905\t0\n4\t0\t3\tNA\tNA\tNA\t1\n")


def _small_skeleton():
    """the chain of test_mvivw_formats.py: outcomes 0, 1, 2 on 5, 7 and 5 instruments, outcome 3 without exposures"""
    p, M = 4, 9
    adj = np.zeros((p + M, p + M), np.int32)
    for t, rows in ((0, (0,)), (1, (1, 2)), (2, (3, 4, 5))):
        for r in rows:
            adj[t, p + r] = adj[p + r, t] = 1
    for a, b in ((0, 1), (1, 2)):
        adj[a, b] = adj[b, a] = 1
    beta = np.clip(0.05 * np.random.default_rng(3).standard_normal((M, p)), -0.9, 0.9)
    corr = np.eye(p + M)
    corr[p:, :p] = beta
    corr[:p, p:] = beta.T
    return adj, corr, p, None


def test_files_without_the_flag_are_those_of_the_earlier_writer(tmp_path):
    from cigwas_amd import mvivw

    res = mvivw.run("unused", 1000, mode="skeleton", data=_small_skeleton())
    assert "robust" not in res and "rho" not in res
    mvivw.write_results(str(tmp_path / "r"), res)
    mvivw.write_outcomes(str(tmp_path / "o"), res)
    assert open(tmp_path / "r").read() == PARENT_RESULTS
    assert open(tmp_path / "o").read() == PARENT_OUTCOMES


def test_files_with_the_flag(tmp_path, capsys):
    from cigwas_amd import mvivw

    res = mvivw.run("unused", 1000, mode="skeleton", data=_small_skeleton(), robust="huber")
    assert res["robust"] == "huber" and res["stats"].shape == (4, 6) and res["status"][3] == 1
    mvivw.write_results(str(tmp_path / "r"), res)
    mvivw.write_outcomes(str(tmp_path / "o"), res)
    mvivw.write_weights(str(tmp_path / "w"), res)
    assert open(tmp_path / "r").readline() == "source\tsink\teffect\tp\tsk_adj\tnum_snps\tse\n"
    lines = open(tmp_path / "o").read().split("\n")
    assert lines[0] == "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus\tscale\ttau\titerations\trho_sum"
    assert lines[4].split("\t") == ["4", "0", "3", "NA", "NA", "NA", "1", "NA", "NA", "NA", "NA"]
    for o in range(3):
        row = lines[1 + o].split("\t")
        st = int(res["status"][o])
        assert row[6] == str(st)
        if st == 0:
            assert row[7] == "%.15g" % res["stats"][o][1] and row[9] == str(int(res["stats"][o][4]))
        else:
            assert row[7:] == ["NA"] * 4
    wl = open(tmp_path / "w").read().split("\n")
    assert wl[0] == "sink\tmarker\trho" and wl[-1] == ""
    want = [(o + 1, int(res["selection"][o][0][j]) + 1) for o in range(4) if res["rho"][o] is not None
            for j in np.flatnonzero(res["rho"][o] < 1)]
    assert [(int(l.split("\t")[0]), int(l.split("\t")[1])) for l in wl[1:-1]] == want
    # statuses 5 and 6 print what status 2 prints
    res["status"][0], res["status"][1] = 5, 6
    mvivw.write_results(str(tmp_path / "r2"), res)
    err = capsys.readouterr().err
    assert "outcome trait 1 (1-based): status 5, no estimates" in err and "outcome trait 2 (1-based): status 6" in err
    rows = [l.split("\t") for l in open(tmp_path / "r2").read().split("\n")[1:-1]]
    assert all(r[2] == r[3] == r[6] == "NA" for r in rows if r[1] == "1" and r[0] == "2")


# ---- the host form ----
@pytest.mark.parametrize("psi", (1, 2))
def test_host_form_against_longdouble(psi):
    from cigwas_amd import mvivw

    L = np.longdouble
    worst = np.zeros(5)
    for name, X, y, w in cases():
        a = mvivw.solve_one_robust(X, y, w, 0, psi)
        b = mvivw.solve_one_robust(X.astype(L), y.astype(L), w.astype(L), 0, psi)
        assert a[0] == b[0] == 0 and abs(a[3][4] - b[3][4]) <= 1, name
        assert b[1].dtype == L and b[4].dtype == L
        worst = np.maximum(worst, distance(a, b, X, w, X.shape[0]))
    print("float64 - longdouble (theta, se, s, tau, rho), psi", psi, worst)
    assert np.all(worst <= HOST_DISTANCE), worst


def test_planted_shifts():
    from cigwas_amd import mvivw

    X, y, w, theta, mask = planted()
    st, th, se, stat, rho = mvivw.solve_one_robust(X, y, w, 0, 2)
    st0, th0, se0, _ = mvivw.solve_one(X, y, w, 0)
    assert st == 0 and st0 == 0
    print("planted:", np.abs(th - theta) / se, np.abs(th0 - theta) / se0, rho[mask].max(), np.mean(rho[~mask] < 0.5))
    assert np.all(np.abs(th - theta) <= 3 * se) and np.any(np.abs(th0 - theta) > 3 * se0)
    assert np.all(rho[mask] < 0.5) and np.mean(rho[~mask] < 0.5) <= 0.05
    # the seed leaves a factor of two on every margin
    assert np.all(np.abs(th - theta) <= 1.5 * se) and np.any(np.abs(th0 - theta) > 6 * se0)
    assert np.all(rho[mask] < 0.25) and np.mean(rho[~mask] < 0.5) <= 0.025
    assert stat[0] == pytest.approx(float(np.sum(w * (y - X @ th) ** 2)), rel=1e-12) and stat[5] == pytest.approx(rho.sum(), rel=1e-12)


@pytest.mark.parametrize("psi", (1, 2))
def test_without_outliers_the_robust_estimate_is_the_plain_one(psi):
    from cigwas_amd import mvivw

    X, y, w, _, _ = planted(frac=0.0)
    st, th, se, _, _ = mvivw.solve_one_robust(X, y, w, 0, psi)
    _, th0, _, _ = mvivw.solve_one(X, y, w, 0)
    assert st == 0 and np.all(np.abs(th - th0) <= 0.5 * se)


def status_tables():
    """name -> (X, y, w, psi, status): 6 more than half the rows fitted exactly; 2 the rows that survive the bisquare stage
    have lost the second column (its six rows carry residuals of +-1000 units that no coefficient can fit)"""
    X, y, w, _, _ = planted(m=200, k=2, frac=0.0, seed=5)
    X6, y6 = X.copy(), y.copy()
    X6[:120], y6[:120] = 0.0, 0.0
    X2, y2 = X.copy(), y.copy()
    X2[:, 1] = 0.0
    X2[:6, 1] = 0.05
    y2[:6] += np.array([1, -1, 1, -1, 1, -1]) * 1000.0 / np.sqrt(W)
    return {"exact": (X6, y6, w, 2, 6), "lost-column": (X2, y2, w, 2, 2)}


def test_status_6_2_and_5():
    from cigwas_amd import mvivw

    for name, (X, y, w, psi, want) in status_tables().items():
        st, th, se, stat, rho = mvivw.solve_one_robust(X, y, w, 0, psi)
        assert st == want and th is None and se is None and rho is None, name
        assert np.isnan(stat[0]) and (stat[3] == 0.0 if want == 2 else np.isnan(stat[3])), name
    X2, y2, w, _, _ = status_tables()["lost-column"]
    assert mvivw.solve_one_robust(X2, y2, w, 0, 1)[0] == 0  # Huber weights never vanish
    X, y, w, _, _ = planted()
    full = mvivw.solve_one_robust(X, y, w, 0, 2)
    assert full[0] == 0 and 4 < full[3][4] < 100
    assert mvivw.solve_one_robust(X, y, w, 0, 2, max_updates=2)[0] == 5  # the cap, lowered through the host form's argument
    assert mvivw.solve_one_robust(X, y, w, 0, 2, max_updates=int(full[3][4]))[0] == 0


def test_host_engine_batch_leaves_neighbours_alone():
    from cigwas_amd import mvivw

    X, y, w, _, _ = planted()
    X6, y6, w6, _, _ = status_tables()["exact"]
    M = 400
    beta = np.zeros((M, 8))
    beta[:, :3], beta[:, 3] = X, y
    beta[:200, 4:6], beta[:200, 6] = X6, y6
    wt = np.full((M, 8), W)
    sel = [(np.arange(400), np.arange(3)), (np.arange(200), np.array([4, 5])), (np.arange(400), np.arange(3)), (np.arange(2), np.arange(3))]
    iv_off, iv, ex_off, ex = mvivw.pack(sel)
    theta, se, stats, status, rho, _ = mvivw.HostEngine().mvivw_robust(beta, wt, np.array([3, 6, 3, 7]), iv_off, iv, ex_off, ex, psi=2)
    one = mvivw.solve_one_robust(X, y, w, 0, 2)
    assert status.tolist() == [0, 6, 0, 1] and stats.shape == (4, 6)
    for a in (0, 2):
        assert np.array_equal(theta[ex_off[a]:ex_off[a + 1]], one[1]) and np.array_equal(rho[iv_off[a]:iv_off[a + 1]], one[4])
        assert np.array_equal(stats[a], np.array(one[3], np.float64))
    assert np.isnan(theta[3:5]).all() and np.isnan(rho[400:600]).all() and np.isnan(stats[1]).all()
