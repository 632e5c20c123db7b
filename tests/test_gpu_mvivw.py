"""GPU: the multivariable IVW regressions on the device (`cusk_mvivw`, `Engine.mvivw`, `ci-gwas mvivw`) against the numpy
host form (`mvivw.HostEngine`), which test_mvivw_formats.py holds against longdouble.

1. Shape sweep: the seven shapes of test_mvivw_formats.py, and m in {k+1, 255, 256, 257, 511, 513} at k in {1, 2, 63, 64,
   127} (the chunk edges, the just-sufficient system, both ends of the triangle), and m = 257 at k in {43, 44, 87, 88}
   (k + 1 = 44 | 45 and 88 | 89: the last problem of a tile class and the first of the next).  All outcomes of
   a shape go in ONE call with lists of their own, outcomes with status 1, 2 and 3 between the good ones.  Bound: 1e-9 on
   max|x - x_host| / max|x_host| for theta, se, sigma and rss, from cond * k * eps ~ 1e4 * 128 * 1.1e-16; the condition
   number of every good problem is asserted <= 1e4 (a condition on the inputs: in the added shapes with m < 4 k the
   exposure columns are orthonormalised over the rows, since a random (k+1) x k system has no bounded condition number).
2. Identical calls give identical bytes; permuting the outcomes permutes the results bit for bit; guard words and unused
   exposure slots stay untouched; argument errors write nothing and leave the engine usable.
3. The four selections and --het through the command line on golden skeletons, against the host form's files."""
import os

import numpy as np
import pytest

from test_iv_check_formats import load_kat, materialise
from test_mvivw_formats import BOUND, N_SAMPLES, SHAPES, parse_results, rel, synth_problem
from test_sepselect_het_formats import write_ssz

pytestmark = pytest.mark.gpu

POISON, I_POISON = -777.0, -12345
EDGES = tuple((m, k, 0.5) for k in (1, 2, 63, 64, 127) for m in sorted({k + 1, 255, 256, 257, 511, 513})
              if m > k and (m, k, 0.5) not in SHAPES) + tuple((257, k, 0.5) for k in (43, 44, 87, 88))


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def shape_batch(m, k, rho):
    """beta (m + 40) x (k + 4), weight, [(outcome, I, E)], indices of the good outcomes.  Traits 0 .. k-1 are exposures,
    k and k + 1 outcomes, k + 2 is a copy of trait 0, k + 3 is zero.  The last row carries an infinite weight."""
    from cigwas_amd import mvivw

    M, p = m + 40, k + 4
    rng = np.random.default_rng(7 * m + k)
    orth = m < 4 * k and (m, k, rho) not in SHAPES  # the seven shapes are built as in test_mvivw_formats.py
    Z = synth_problem(M, k + 1, rho, 31 * m + k)  # columns 0 .. k + 1
    if orth:
        Q = np.linalg.qr(rng.standard_normal((m, k)))[0]
        Z[:m, :k] = 0.03 * np.sqrt(m) * Q
        Z[:m, k] = Z[:m, :k] @ (0.2 * rng.standard_normal(k)) + 0.01 * rng.standard_normal(m)
        Z = np.clip(Z, -0.9, 0.9)
    beta = np.zeros((M, p))
    beta[:, :k + 2] = Z
    beta[:, k + 2] = beta[:, 0]
    w = mvivw.weights(beta, N_SAMPLES)
    w[M - 1, :] = np.inf
    head = np.arange(m)
    if orth:
        second = (k + 1, head, np.arange(1, k) if k > 1 else np.arange(1))
        last = (k, head, np.arange(k - 1) if k > 1 else np.arange(1))
    else:
        second = (k + 1, np.sort(rng.choice(M - 1, size=max(3 * m // 4, k + 1), replace=False)),
                  np.sort(rng.choice(k, size=max(k - 3, 1), replace=False)))
        last = (k, np.arange(20, m + 20), np.arange(k))
    dup = [k + 3] if k == 1 else [0] + list(range(2, k)) + [k + 2]
    lists = [
        (k, head, np.arange(k)),                                      # the shape itself
        (k + 1, np.arange(k), np.arange(k)),                          # m = k: status 1
        second,
        (k + 1, head, np.array(dup)),                                 # a zero or a duplicated column: status 2
        (k, np.concatenate([np.arange(1, m), [M - 1]]), np.arange(k)),  # an infinite weight: status 3
        last,
    ]
    return beta, w, lists, (0, 2, 5)


def call_of(lists):
    from cigwas_amd import mvivw

    iv_off, iv, ex_off, ex = mvivw.pack([(np.asarray(I), np.asarray(E, np.int64)) for _, I, E in lists])
    return dict(outcome=np.array([o for o, _, _ in lists], np.int32), iv_off=iv_off, iv=iv, ex_off=ex_off, ex=ex)


def gram_cond(beta, w, o, I, E):
    X = beta[np.ix_(I, E)]
    G = X.T @ (X * w[I, o][:, None])
    d = np.sqrt(np.diag(G))
    return float(np.linalg.cond(G / np.outer(d, d)))


# ---- 1. shape sweep ----
@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=lambda s: f"m{s[0]}-k{s[1]}-r{s[2]}")
def test_shape_sweep_against_the_host_form(shape, eng):
    from cigwas_amd import mvivw

    m, k, rho = shape
    beta, w, lists, good = shape_batch(m, k, rho)
    call = call_of(lists)
    for a in good:
        if len(lists[a][2]) and len(lists[a][1]) > len(lists[a][2]):
            assert gram_cond(beta, w, *lists[a]) <= 1e4
    th, seh, sth, status_h, _ = mvivw.HostEngine().mvivw(beta, w, **call)
    nex = int(call["ex_off"][-1])
    tb, sb = np.full(nex + 5, POISON), np.full(nex + 5, POISON)
    stb, fb = np.full((len(lists) + 2, 3), POISON), np.full(len(lists) + 3, I_POISON, np.int32)
    theta, se, stats, status, ms = eng.mvivw(beta, w, **call, theta=tb, se=sb, stats=stb, status=fb)
    assert np.all(tb[nex:] == POISON) and np.all(sb[nex:] == POISON) and np.all(stb[len(lists):] == POISON)
    assert np.all(fb[len(lists):] == I_POISON) and not np.any(tb[:nex] == POISON) and not np.any(stb[:len(lists)] == POISON)
    assert status.tolist() == status_h.tolist(), (status.tolist(), status_h.tolist())
    assert status[1] == 1 and status[3] == 2 and status[4] == 3 and status[0] == 0 and status[5] == 0 and ms > 0
    eo = call["ex_off"]
    worst = 0.0
    for a in range(len(lists)):
        sl = slice(eo[a], eo[a + 1])
        if status[a] != 0:
            assert np.all(np.isnan(theta[sl])) and np.all(np.isnan(se[sl])) and np.isnan(stats[a, 0]) and np.isnan(stats[a, 1])
            continue
        worst = max(worst, rel(theta[sl], th[sl]), rel(se[sl], seh[sl]), rel(stats[a, 1], sth[a, 1]), rel(stats[a, 0], sth[a, 0]))
        assert abs(stats[a, 2] - sth[a, 2]) <= 1e-9
    print(shape, "worst", worst)
    assert worst <= BOUND, (shape, worst)


# ---- 2. bytes, order, guards, errors ----
def test_identical_calls_and_permuted_outcomes_give_identical_bytes(eng):
    for shape in ((700, 39, 0.9), (513, 127, 0.5), (300, 7, 0.9)):
        beta, w, lists, _ = shape_batch(*shape)
        call = call_of(lists)
        first = eng.mvivw(beta, w, **call)
        again = eng.mvivw(beta, w, **call)
        for a, b in zip(first[:4], again[:4]):
            assert a.tobytes() == b.tobytes()
        perm = [4, 2, 0, 5, 3, 1]
        pcall = call_of([lists[a] for a in perm])
        theta, se, stats, status, _ = eng.mvivw(beta, w, **pcall)
        eo, po = call["ex_off"], pcall["ex_off"]
        for pos, a in enumerate(perm):
            assert theta[po[pos]:po[pos + 1]].tobytes() == first[0][eo[a]:eo[a + 1]].tobytes()
            assert se[po[pos]:po[pos + 1]].tobytes() == first[1][eo[a]:eo[a + 1]].tobytes()
            assert stats[pos].tobytes() == first[2][a].tobytes() and status[pos] == first[3][a]


def test_groups_of_outcomes_give_the_bytes_of_one_group(eng):
    """engine option "mvivw_part_bytes": the outcomes run in groups whose chunk partials fit the bound, one buffer reused
    group after group.  1 byte puts every outcome in a group of its own; the middle values cut the call in two and three."""
    try:
        for shape in ((700, 39, 0.9), (513, 127, 0.5)):
            beta, w, lists, _ = shape_batch(*shape)
            call = call_of(lists + lists[::-1])  # 12 outcomes, 8 of them on the device
            eng.set_option("mvivw_part_bytes", 256 << 20)
            whole = eng.mvivw(beta, w, **call)
            assert whole[3].tolist() == [0, 1, 0, 2, 3, 0, 0, 3, 2, 0, 1, 0]
            m, k, _ = shape
            one = 8 * ((m + 255) // 256) * (k + 1) * (k + 2) // 2  # the partials of the shape's own problem
            for bound in (1, 2 * one, 3 * one + 8):
                eng.set_option("mvivw_part_bytes", bound)
                cut = eng.mvivw(beta, w, **call)
                for a, b in zip(whole[:4], cut[:4]):
                    assert a.tobytes() == b.tobytes(), (shape, bound)
        with pytest.raises(RuntimeError):
            eng.set_option("mvivw_part_bytes", 0)
    finally:
        eng.set_option("mvivw_part_bytes", 256 << 20)


def test_unused_exposure_slots_are_untouched(eng):
    from cigwas_amd import mvivw

    beta, w, lists, _ = shape_batch(300, 7, 0.9)
    call = call_of(lists)
    shift = 3  # the lists start at slot 3
    call["ex_off"] = call["ex_off"] + shift
    call["ex"] = np.concatenate([np.full(shift, 999, np.int32), call["ex"]])
    nex = int(call["ex_off"][-1])
    tb, sb = np.full(nex + 4, POISON), np.full(nex + 4, POISON)
    theta, se, stats, status, _ = eng.mvivw(beta, w, **call, theta=tb, se=sb)
    assert np.all(tb[:shift] == POISON) and np.all(sb[:shift] == POISON) and np.all(tb[nex:] == POISON) and np.all(sb[nex:] == POISON)
    th, seh, _, status_h, _ = mvivw.HostEngine().mvivw(beta, w, **call)
    assert status.tolist() == status_h.tolist()
    ok = ~np.isnan(th[shift:nex])
    assert rel(theta[shift:nex][ok], th[shift:nex][ok]) <= BOUND and np.array_equal(np.isnan(theta[shift:nex]), ~ok)


def test_argument_errors_write_nothing(eng):
    beta, w, lists, _ = shape_batch(300, 7, 0.9)
    M, p = beta.shape
    good = dict(outcome=[7, 8], iv_off=[0, 100, 300], iv=np.concatenate([np.arange(100), np.arange(200)]), ex_off=[0, 3, 5],
                ex=[0, 1, 2, 3, 4])

    def bad(msg, model=0, **change):
        call = {**good, **change}
        tb, sb, stb, fb = np.full(9, POISON), np.full(9, POISON), np.full((4, 3), POISON), np.full(4, I_POISON, np.int32)
        with pytest.raises(RuntimeError, match=f"error 2: cusk_mvivw: .*{msg}"):  # CUSK_ERR_ARG
            eng.mvivw(beta, w, **call, model=model, theta=tb, se=sb, stats=stb, status=fb)
        assert np.all(tb == POISON) and np.all(sb == POISON) and np.all(stb == POISON) and np.all(fb == I_POISON)

    iv = good["iv"]
    bad("not a trait index", outcome=[7, p])
    bad("not a trait index", outcome=[-1, 8])
    bad("not a marker row", iv=np.where(np.arange(300) == 99, M, iv))
    bad("not a marker row", iv=np.where(np.arange(300) == 0, -1, iv))
    bad("instrument list is not strictly ascending", iv=np.where(np.arange(300) == 50, 49, iv))
    bad("exposure list is not strictly ascending", ex=[0, 2, 1, 3, 4])
    bad("exposure list is not strictly ascending", ex=[0, 1, 1, 3, 4])
    bad("own exposures", ex=[0, 1, 7, 3, 4])
    bad("not a trait index", ex=[0, 1, 2, 3, p])
    bad("not monotone", iv_off=[0, 300, 100])
    bad("not monotone", ex_off=[0, 5, 3])
    bad("model", model=3)
    bad("model", model=-1)
    wide = np.zeros((300, 140))
    with pytest.raises(RuntimeError, match="more than 127 exposures"):
        eng.mvivw(wide, np.ones_like(wide), [139], [0, 300], np.arange(300), [0, 128], np.arange(128))
    theta, se, stats, status, _ = eng.mvivw(beta, w, **good)  # the engine is fine afterwards
    assert status.tolist() == [0, 0] and np.all(np.isfinite(theta[:5]))


# ---- 3. the command line on golden skeletons ----
def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= BOUND * max(abs(b), 1e-300) or a == b


def compare_files(dev_path, host_path):
    dev, host = parse_results(dev_path), parse_results(host_path)
    assert sorted(dev) == sorted(host)
    estimated = 0
    for key, (eff, pv, sk, ns, se) in host.items():
        d = dev[key]
        assert d[2] == sk and d[3] == ns and _close(d[0], eff) and _close(d[4], se), (key, d, host[key])
        assert (np.isnan(d[1]) and np.isnan(pv)) or abs(d[1] - pv) <= BOUND  # a probability: absolute
        estimated += int(np.isfinite(se))
    return estimated


def parse_outcomes(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus" and lines[-1] == ""
    num = lambda s: np.nan if s == "NA" else float(s)  # noqa: E731
    return [(int(r[0]), int(r[1]), int(r[2]), num(r[3]), num(r[4]), num(r[5]), int(r[6])) for r in (l.split("\t") for l in lines[1:-1])]


def compare_outcomes(dev_path, host_path):
    """every column of the per-outcome file: sigma and q to 1e-9 relative, q_p to 1e-9 absolute, the rest equal"""
    dev, host = parse_outcomes(dev_path), parse_outcomes(host_path)
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        assert d[:3] == h[:3] and d[6] == h[6], (d, h)
        assert _close(d[3], h[3]) and _close(d[4], h[4]), (d, h)
        assert (np.isnan(d[5]) and np.isnan(h[5])) or abs(d[5] - h[5]) <= BOUND, (d, h)
        assert np.isfinite(d[3]) == (d[6] == 0) and np.isfinite(d[5]) == (d[6] == 0)
    return sum(1 for d in dev if d[6] == 0)


@pytest.mark.parametrize("name", ("p6", "p40"))
def test_cli_selections_against_the_host_form(name, tmp_path):
    from cigwas_amd import cli, ivcheck, mvivw

    stem = materialise(name, tmp_path)
    N = load_kat()[name]["num_samples"]
    adj, corr, p, _ = ivcheck.load(stem)
    prior = np.zeros((p, p), np.int32)
    prior[0, 1:3] = 1
    prior[p - 1, 0] = 1
    prior_path = str(tmp_path / "prior.bin")
    prior.tofile(prior_path)
    table = str(tmp_path / "ivs.csv")
    ivcheck.write_csv(table, ivcheck.iv_candidates(stem))
    total = estimated = 0
    for tag, flags, kw in (("all", [], {}), ("skeleton", ["-s"], {}), ("prior", ["--orientation-prior", prior_path], {"prior_path": prior_path}),
                           ("ivs", ["--ivs", table], {"ivs_path": table})):
        for model in ("default", "fixed"):
            out = str(tmp_path / f"dev_{tag}_{model}_results.tsv")
            cli.main(["mvivw", stem, str(N), "--model", model, "--out", out] + flags)
            res = mvivw.run(stem, N, mode=tag, model=mvivw.MODELS[model], **kw)
            host = str(tmp_path / f"host_{tag}_{model}_results.tsv")
            mvivw.write_results(host, res)
            total += compare_files(out, host)
            mvivw.write_outcomes(host + ".o", res)
            estimated += compare_outcomes(out[:-len("_results.tsv")] + "_outcomes.tsv", host + ".o")
    assert total > 0 and estimated > 0


def test_cli_het(tmp_path):
    from cigwas_amd import cli, ivcheck, mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    n = ivcheck.load(stem)[1].shape[0]
    plain = str(tmp_path / "plain_results.tsv")
    cli.main(["mvivw", stem, str(N), "--out", plain])
    write_ssz(stem, np.full((n, n), N, np.int64))
    uniform = str(tmp_path / "uniform_results.tsv")
    cli.main(["mvivw", stem, "1", "--het", "--out", uniform])
    assert open(uniform, "rb").read() == open(plain, "rb").read()  # uniform sizes: the plain run bit for bit
    sizes = np.full((n, n), N, np.int64)
    sizes[:, 1] = sizes[1, :] = N // 4  # trait 1 is observed on a quarter
    write_ssz(stem, sizes)
    quarter = str(tmp_path / "quarter_results.tsv")
    cli.main(["mvivw", stem, "1", "--het", "--out", quarter])
    res = mvivw.run(stem, 1, het=True)
    host = str(tmp_path / "host_results.tsv")
    mvivw.write_results(host, res)
    assert compare_files(quarter, host) > 0
    mvivw.write_outcomes(host + ".o", res)
    assert compare_outcomes(str(tmp_path / "quarter_outcomes.tsv"), host + ".o") > 0
    # Under random effects with sigma > 1 a common factor of an outcome's weights cancels in se (v ~ 1 / c, sigma^2 ~ c), so
    # the change shows under the fixed model: se of the quartered outcome grows by sqrt((N - 2) / (N / 4 - 2)).
    fixed_plain, fixed_quarter = str(tmp_path / "fp_results.tsv"), str(tmp_path / "fq_results.tsv")
    cli.main(["mvivw", stem, "1", "--het", "--model", "fixed", "--out", fixed_quarter])
    mvivw.write_results(host, mvivw.run(stem, 1, het=True, model=mvivw.MODELS["fixed"]))
    assert compare_files(fixed_quarter, host) > 0
    cli.main(["mvivw", stem, str(N), "--model", "fixed", "--out", fixed_plain])
    q, pl = parse_results(fixed_quarter), parse_results(fixed_plain)
    assert res["status"][1] == 0
    factor = np.sqrt((N - 2.0) / (N // 4 - 2.0))
    moved = [key for key in q if key[1] == 2 and np.isfinite(q[key][4])]
    assert moved and all(abs(q[key][4] / pl[key][4] - factor) <= 1e-9 * factor for key in moved)
    assert all(q[key][4] == pl[key][4] or (np.isnan(q[key][4]) and np.isnan(pl[key][4])) for key in q if key[1] != 2)
    assert not os.path.exists(stem + "_mvivw_results.tsv")
