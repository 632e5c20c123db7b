"""GPU: `cusk_mvivw_robust` and `cusk_abs_median` (`Engine.mvivw_robust`, `Engine.abs_median`, `ci-gwas mvivw --robust`)
against the float64 host form (`mvivw.HostEngine.mvivw_robust`), which test_mvivw_robust_formats.py holds against longdouble.

1. The selection kernel against np.sort by equality, every segment length and content of the list below in one call.
2. Shape sweep: k at the tile-class edges of the Gram kernel, m at the chunk edges and one m = 5,000, both psi, all three
   models, 5 % planted rows (m = k + 1: a residual of equal size in every row, see shape_problem).  For m < 4 k the exposure columns are orthonormalised over the rows, as in test_gpu_mvivw.py.
   Status and the set {rho = 0} by equality (rows whose |u| is within BOUND of 1 in the host form set aside, at most 1 % of
   a case), updates +- 1, the rest within BOUND.
   BOUND = 1e-7 = max(1,000 x the stopping tolerance 1e-10, 8 x 8.9e-15), 8.9e-15 being the largest distance between the
   float64 and the longdouble host form measured over `cases()` of test_mvivw_robust_formats.py (its header; theta in the
   units d_j theta_j / (s sqrt(m)), se, s and tau relative, rho absolute).  The stopping rule bounds a step, not the distance
   to the fixed point, and the float64 host form is the only thing the device can be expected to match.
3. One call that mixes outcomes of different k and m with one outcome each of status 1, 2, 3 and 6 between good ones.
   Status 5 between good outcomes comes from the sweep: with m near 2 k the updates contract slowly, and at k = 127 the
   problems of m = 255, 256 and 257 do not converge within 100 updates in the host form (k = 87, m = 256 and k = 88,
   m = 255 at psi = 2 likewise), each in one call with problems that do.
4. Two runs, an outcome alone or among 40, and a small "mvivw_part_bytes" (several groups) give the same bytes.
5. The command line on a merged skeleton written here, with and without --het."""
import numpy as np
import pytest

from test_mvivw_robust_formats import W, planted, status_tables
from test_sepselect_het_formats import write_ssz

pytestmark = pytest.mark.gpu

BOUND = 1e-7
KS = (1, 2, 43, 44, 45, 87, 88, 89, 127)


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


# ---- 1. selection ----
def test_abs_median_equals_np_sort(eng):
    rng = np.random.default_rng(2)
    big = np.finfo(np.float64).max
    segs = []
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 20001):
        ties = rng.standard_normal(n)
        ties[n // 4:n - n // 4] = -0.75
        zeros = np.zeros(n)
        zeros[::2] = -0.0
        segs += [rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n), np.full(n, -3.25), zeros, ties,
                 rng.integers(1, 1 << 40, n).astype(np.int64).view(np.float64) * rng.choice([-1.0, 1.0], n),  # subnormals
                 -big * (0.25 + 0.2 * rng.random(n)), np.sort(rng.standard_normal(n))[::-1].copy()]  # the last: descending
    off = np.zeros(len(segs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in segs])
    vals = np.concatenate(segs)
    want = []
    for s in segs:
        a = np.sort(np.abs(s))
        n = len(a)
        want.append(a[n // 2] if n & 1 else (a[n // 2 - 1] + a[n // 2]) * 0.5)
    want = np.array(want)
    assert np.isfinite(want).all() and (want[4::7] < 1e-300).all() and (want[5::7] > 1e307).all()
    out = np.full(len(segs) + 1, -777.0)
    got = eng.abs_median(vals, off, out=out)
    assert out[-1] == -777.0  # the guard word
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)
    assert np.isnan(eng.abs_median(vals, np.array([3, 3]))[0])


# ---- 2. shape sweep ----
def shape_problem(m, k):
    X, y, w, theta, mask = planted(m=m, k=k, frac=0.05, seed=1000 * k + m)
    if m == k + 1 and k > 1:
        # one residual degree of freedom: e is a multiple of the one direction n orthogonal to the columns, and reweighting
        # such a system has no stable fixed point in general (the host form ends in status 5 or 2 by rounding).  With
        # |n_i| all equal every rho is equal, so the update reproduces theta and both stages converge at once.
        rng = np.random.default_rng(m + k)
        n = rng.choice([-1.0, 1.0], m) / np.sqrt(m)
        Q = np.linalg.qr(np.concatenate([n[:, None], rng.standard_normal((m, k))], axis=1))[0][:, 1:]
        return 0.05 * np.sqrt(m) * Q, 0.05 * np.sqrt(m) * Q @ theta + 3.0 * np.sqrt(m) * n / np.sqrt(W)
    if m < 4 * k:
        rng = np.random.default_rng(m + k)
        X = 0.05 * np.sqrt(m) * np.linalg.qr(rng.standard_normal((m, k)))[0]
        y = X @ theta + rng.standard_normal(m) / np.sqrt(W)
        y[mask] += 8.0 / np.sqrt(W)
    return X, y


def batch(problems):
    """beta, weight and the call of a list of (X, y): each problem has trait columns and marker rows of its own"""
    from cigwas_amd import mvivw

    M, p = sum(len(y) for _, y in problems), sum(X.shape[1] + 1 for X, _ in problems)
    beta, sel, outcome = np.zeros((M, p)), [], []
    r = c = 0
    for X, y in problems:
        m, k = X.shape
        beta[r:r + m, c:c + k], beta[r:r + m, c + k] = X, y
        sel.append((np.arange(r, r + m), np.arange(c, c + k)))
        outcome.append(c + k)
        r, c = r + m, c + k + 1
    iv_off, iv, ex_off, ex = mvivw.pack(sel)
    return beta, np.full((M, p), W), dict(outcome=np.array(outcome, np.int32), iv_off=iv_off, iv=iv, ex_off=ex_off, ex=ex)


def compare(dev, host, beta, call, psi):
    theta, se, stats, status, rho, _ = dev
    th, sh, sth, status_h, rh, _ = host
    assert status.tolist() == status_h.tolist(), (status.tolist(), status_h.tolist())
    worst = 0.0
    for a, st in enumerate(status_h):
        i0, i1, e0, e1 = call["iv_off"][a], call["iv_off"][a + 1], call["ex_off"][a], call["ex_off"][a + 1]
        if st != 0:
            assert np.isnan(theta[e0:e1]).all() and np.isnan(se[e0:e1]).all() and np.isnan(rho[i0:i1]).all()
            assert np.isnan(stats[a][[0, 1, 2, 4, 5]]).all()
            assert stats[a][3] == sth[a][3] if st == 2 else np.isnan(stats[a][3])
            continue
        I, E, o, m = call["iv"][i0:i1], call["ex"][e0:e1], call["outcome"][a], i1 - i0
        assert abs(stats[a][4] - sth[a][4]) <= 1, (a, stats[a][4], sth[a][4])
        s = sth[a][1]
        d = np.sqrt(np.sum(beta[np.ix_(I, E)] ** 2 * W, axis=0))
        dist = [np.max(d * np.abs(theta[e0:e1] - th[e0:e1])) / (s * np.sqrt(m)), np.max(np.abs(se[e0:e1] / sh[e0:e1] - 1)),
                abs(stats[a][1] / s - 1), abs(stats[a][2] / sth[a][2] - 1), np.max(np.abs(rho[i0:i1] - rh[i0:i1])),
                abs(stats[a][0] / sth[a][0] - 1), abs(stats[a][5] / sth[a][5] - 1)]
        worst = max(worst, *dist)
        assert max(dist) <= BOUND, (a, m, len(E), dist)
        if psi == 2:
            e = np.sqrt(W) * (beta[I, o] - beta[np.ix_(I, E)] @ th[e0:e1])
            near = np.abs(np.abs(e / (4.685 * s)) - 1) <= BOUND
            assert near.sum() <= 0.01 * m
            assert np.array_equal((rho[i0:i1] == 0)[~near], (rh[i0:i1] == 0)[~near])
    return worst


@pytest.fixture(scope="module")
def shape_calls():
    """per k: the batch of its problems, built once"""
    out = {}
    for k in KS:
        ms = sorted({k + 1, 255, 256, 257, 513} | ({5000} if k == 45 else set()))
        out[k] = batch([shape_problem(m, k) for m in ms if m > k])
    return out


@pytest.mark.parametrize("psi", (1, 2))
@pytest.mark.parametrize("k", KS)
def test_shape_sweep_against_the_host_form(k, psi, eng, shape_calls):
    from cigwas_amd import mvivw

    beta, w, call = shape_calls[k]
    # the host form of the widest problems takes seconds per call: from k = 87 on a case runs one model, and the cases
    # between them all three
    for model in ((0, 1, 2) if k <= 45 else ((KS.index(k) + psi) % 3,)):
        host = mvivw.HostEngine().mvivw_robust(beta, w, **call, model=model, psi=psi)
        dev = eng.mvivw_robust(beta, w, **call, model=model, psi=psi)
        worst = compare(dev, host, beta, call, psi)
        print(f"k {k} psi {psi} model {model}: status {host[3].tolist()} updates {host[2][:, 4].tolist()} distance {worst:.3g}")
    assert (host[3] == 0).any()  # the sweep compares estimates, not only failures


# ---- 3. statuses between good outcomes ----
def mixed_call():
    X6, y6, _, _, _ = status_tables()["exact"]
    X2, y2, _, _, _ = status_tables()["lost-column"]
    good = [shape_problem(300, 3), shape_problem(513, 45), shape_problem(257, 89)]
    probs = [good[0], (good[0][0][:3], good[0][1][:3]), good[1], (X2, y2), good[2], (X6, y6), good[0], shape_problem(256, 2), good[1]]
    beta, w, call = batch(probs)
    w[call["iv"][call["iv_off"][7]], call["outcome"][7]] = np.inf  # status 3
    return beta, w, call


def test_failed_outcomes_leave_their_neighbours_untouched(eng):
    from cigwas_amd import mvivw

    beta, w, call = mixed_call()
    host = mvivw.HostEngine().mvivw_robust(beta, w, **call, psi=2)
    assert host[3].tolist() == [0, 1, 0, 2, 0, 6, 0, 3, 0]
    dev = eng.mvivw_robust(beta, w, **call, psi=2)
    compare(dev, host, beta, call, 2)
    theta, _, stats, _, rho, _ = dev
    eo, io = call["ex_off"], call["iv_off"]
    assert theta[eo[0]:eo[1]].tobytes() == theta[eo[6]:eo[7]].tobytes() and stats[0].tobytes() == stats[6].tobytes()
    assert rho[io[2]:io[3]].tobytes() == rho[io[8]:io[9]].tobytes() and stats[2].tobytes() == stats[8].tobytes()
    with pytest.raises(Exception, match="psi"):
        eng.mvivw_robust(beta, w, **call, psi=3)
    with pytest.raises(Exception, match="ascending"):
        eng.mvivw_robust(beta, w, **dict(call, iv=call["iv"][::-1].copy()), psi=2)
    assert eng.mvivw_robust(beta, w, **call, psi=2)[0].tobytes() == theta.tobytes()  # the engine is still usable


# ---- 4. determinism and independence ----
def as_bytes(res, a=None, call=None):
    theta, se, stats, status, rho, _ = res
    if a is None:
        return theta.tobytes() + se.tobytes() + stats.tobytes() + rho.tobytes() + status.tobytes()
    e0, e1, i0, i1 = call["ex_off"][a], call["ex_off"][a + 1], call["iv_off"][a], call["iv_off"][a + 1]
    return theta[e0:e1].tobytes() + se[e0:e1].tobytes() + stats[a].tobytes() + rho[i0:i1].tobytes()


def test_same_bytes_twice_alone_and_in_groups(eng):
    from cigwas_amd.skeleton import Engine

    target = shape_problem(513, 45)
    probs = [shape_problem(100 + 17 * j, 1 + (5 * j) % 60) for j in range(39)]
    probs.insert(20, target)
    beta, w, call = batch(probs)
    first = eng.mvivw_robust(beta, w, **call, psi=2)
    assert (first[3] == 0).all() and len(set(first[2][:, 4].tolist())) > 3  # the outcomes freeze at different updates
    assert as_bytes(eng.mvivw_robust(beta, w, **call, psi=2)) == as_bytes(first)
    b1, w1, c1 = batch([target])
    alone = eng.mvivw_robust(b1, w1, **c1, psi=2)
    assert as_bytes(alone, 0, c1) == as_bytes(first, 20, call)
    small = Engine(0)
    try:
        small.set_option("mvivw_part_bytes", 1 << 20)  # the target's partials alone are larger: many groups
        assert as_bytes(small.mvivw_robust(beta, w, **call, psi=2)) == as_bytes(first)
    finally:
        small.close()


# ---- 5. command line ----
def write_skeleton(d, N):
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    p, M = 6, 300
    rng = np.random.default_rng(9)
    beta = np.clip(0.05 * rng.standard_normal((M, p)), -0.9, 0.9)
    beta[:, 5] = beta[:, :5] @ np.array([0.3, -0.2, 0.4, 0.1, -0.3]) + rng.standard_normal(M) / np.sqrt(N)
    plantedrows = np.arange(0, 300, 20)
    beta[plantedrows, 5] += 8.0 / np.sqrt(N)  # direct effects on trait 6
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
    return stem, plantedrows


def numbers(path):
    num = lambda s: np.nan if s in ("NA", "TRUE", "FALSE") else float(s)  # noqa: E731
    return np.array([[num(v) for v in l.split("\t")] for l in open(path).read().split("\n")[1:-1]])


@pytest.mark.parametrize("het", (False, True))
def test_cli_files_equal_the_host_form_s(het, tmp_path):
    from cigwas_amd import cli, mvivw

    N = 10000
    stem, plantedrows = write_skeleton(tmp_path, N)
    F = str(tmp_path / "weights.tsv")
    cli.main(["mvivw", stem, str(N), "--robust", "--robust-weights", F] + (["--het"] if het else []))
    res = mvivw.run(stem, N, het=het, robust="bisquare")
    assert res["status"][5] == 0  # the outcome with the planted markers; whatever the others are, the files must agree
    hr, ho, hw = str(tmp_path / "h_results.tsv"), str(tmp_path / "h_outcomes.tsv"), str(tmp_path / "h_weights.tsv")
    mvivw.write_results(hr, res)
    mvivw.write_outcomes(ho, res)
    mvivw.write_weights(hw, res)
    # effect and se: theta within BOUND s sqrt(m) / d_j, here s sqrt(m) / d_j < 1 and |theta| > 1e-3, so 1e-4 relative holds
    # with room; p is a function of the two; the outcome columns compare like se
    got, want = numbers(stem + "_mvivw_results.tsv"), numbers(hr)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[:, [0, 1, 2, 5, 6]], want[:, [0, 1, 2, 5, 6]], rtol=1e-6, atol=1e-9)
    got, want = numbers(stem + "_mvivw_outcomes.tsv"), numbers(ho)
    assert open(stem + "_mvivw_outcomes.tsv").readline().endswith("\tscale\ttau\titerations\trho_sum\n")
    np.testing.assert_allclose(np.delete(got, [5, 9], 1), np.delete(want, [5, 9], 1), rtol=1e-6)
    assert np.array_equal(np.isnan(got[:, 9]), np.isnan(want[:, 9])) and not np.any(np.abs(got[:, 9] - want[:, 9]) > 1)
    gw, ww = numbers(F), numbers(hw)
    sure = ww[np.abs(ww[:, 2] - 0.5) < 0.49]  # rows whose rho is not within rounding of 0 | 1 are in both files
    have = {(int(r[0]), int(r[1])): r[2] for r in gw}
    assert all(abs(have[int(r[0]), int(r[1])] - r[2]) <= 1e-6 for r in sure)
    listed = {int(r[1]) for r in gw if int(r[0]) == 6}
    assert set((plantedrows + 1).tolist()) <= listed
