"""GPU: the generalised-least-squares regressions on the device (`cusk_mvivw_ld`, `Engine.mvivw_ld`, `ci-gwas mvivw --ld`)
against the numpy host form (`mvivw.HostEngine.mvivw_ld`), which test_mvivw_ld_formats.py holds against the direct formula
in longdouble.

1. Shape sweep: m in {k+1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1025} at k in {1, 2, 64, 127} where m > k.  The
   panel is 64 columns wide, the trailing tiles 64 x 64, the panel solve takes 32 rows and a chunk of the regression 256:
   both sides of every edge are in the list (m + k + 1 rows stand in the workspace, so the row edges move with k).  All
   outcomes of a shape go in ONE call with lists of their own; outcomes of status 1, 2, 3 (an infinite weight; a NaN of
   the LD that is read) and 4 (a duplicated marker) sit between the good ones.  Bound 1e-7 on max|x - x_host| /
   max|x_host| for theta, se, sigma and rss (cond(R) * cond(G) * k * eps = 100 * 1e4 * 128 * 1.1e-16 ~ 1.4e-8 with the
   margin of the plain sweep); cond(R) <= 100 and cond(G) <= 1e4 are asserted on every good problem.
2. Both sides of the pivot rule and the three positions of a duplicate, with the pivot within 1e-12 of the host's.
3. Identical calls give identical bytes; permuting the outcomes permutes the results bit for bit; the workspace bound is
   an argument error that writes nothing; R = I gives `Engine.mvivw`.
4. The four selections, --het and --ld-ridge through the command line on golden skeletons whose marker block is rewritten
   to the AR(1) blocks with one planted duplicate pair, against the host form's files."""
import numpy as np
import pytest

from test_gpu_mvivw import I_POISON, POISON, call_of, shape_batch
from test_iv_check_formats import load_kat, materialise
from test_mvivw_formats import one_call, parse_results, problem, rel
from test_mvivw_ld_formats import DUPLICATES, LD_BOUND, ar1_ld, conditions, pair_ld, plant_ld, with_duplicate
from test_sepselect_het_formats import write_ssz

pytestmark = pytest.mark.gpu

SWEEP = tuple((m, k) for k in (1, 2, 64, 127) for m in sorted({k + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1025}) if m > k)


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host():
    from cigwas_amd import mvivw

    return mvivw.HostEngine()


def ld_shape_batch(m, k):
    """`shape_batch` of test_gpu_mvivw.py (six outcomes: good, status 1, good, status 2, status 3, good) with an LD matrix
    over its M = m + 40 markers: AR(1) blocks in which marker M - 2 is a copy of marker 0 and ld[M - 3, 0] is NaN, and two
    more outcomes: the first m - 1 rows with marker M - 2 (status 4) and with marker M - 3 (status 3)."""
    beta, w, lists, _ = shape_batch(m, k, 0.5)
    M = beta.shape[0]
    ld = with_duplicate(M, 0, M - 2)
    ld[M - 3, 0] = np.nan
    lists = list(lists)
    lists.append((k, np.concatenate([np.arange(m - 1), [M - 2]]), np.arange(k)))
    lists.append((k, np.concatenate([np.arange(m - 1), [M - 3]]), np.arange(k)))
    return beta, w, ld, lists


# ---- 1. shape sweep ----
@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: f"m{s[0]}-k{s[1]}")
def test_shape_sweep_against_the_host_form(shape, eng, host):
    m, k = shape
    beta, w, ld, lists = ld_shape_batch(m, k)
    call = call_of(lists)
    th, seh, sth, status_h, _ = host.mvivw_ld(beta, w, ld, **call)
    nex = int(call["ex_off"][-1])
    tb, sb = np.full(nex + 5, POISON), np.full(nex + 5, POISON)
    stb, fb = np.full((len(lists) + 2, 3), POISON), np.full(len(lists) + 3, I_POISON, np.int32)
    theta, se, stats, status, ms = eng.mvivw_ld(beta, w, ld, **call, theta=tb, se=sb, stats=stb, status=fb)
    assert np.all(tb[nex:] == POISON) and np.all(sb[nex:] == POISON) and np.all(stb[len(lists):] == POISON)
    assert np.all(fb[len(lists):] == I_POISON) and not np.any(tb[:nex] == POISON) and not np.any(stb[:len(lists)] == POISON)
    assert status.tolist() == status_h.tolist(), (status.tolist(), status_h.tolist())
    # the second list is drawn at random and may hold the planted pair or the NaN; every other status is fixed
    assert [int(status[a]) for a in (0, 1, 3, 4, 5, 6, 7)] == [0, 1, 2, 3, 0, 4, 3] and status[2] in (0, 3, 4) and ms > 0
    eo = call["ex_off"]
    worst = 0.0
    for a, (o, I, E) in enumerate(lists):
        sl = slice(eo[a], eo[a + 1])
        if status[a] != 0:
            assert np.all(np.isnan(theta[sl])) and np.all(np.isnan(se[sl])) and np.isnan(stats[a, 0]) and np.isnan(stats[a, 1])
            assert np.isnan(stats[a, 2]) if status[a] in (1, 3) else abs(stats[a, 2] - sth[a, 2]) <= 1e-9
            continue
        cr, cg = conditions(beta[np.ix_(I, E)], w[I, o], ld[np.ix_(I, I)])
        assert cr <= 100 and cg <= 1e4, (shape, a, cr, cg)
        worst = max(worst, rel(theta[sl], th[sl]), rel(se[sl], seh[sl]), rel(stats[a, 1], sth[a, 1]), rel(stats[a, 0], sth[a, 0]))
        assert abs(stats[a, 2] - sth[a, 2]) <= 1e-9
    print(shape, "worst", worst)
    assert worst <= LD_BOUND, (shape, worst)


# ---- 2. the pivot rule ----
def test_both_sides_of_the_pivot_rule_and_the_three_duplicates(eng, host):
    beta, w = problem(300, 7, 0.9)
    call = one_call(beta, 7)
    cases = [("above", pair_ld(300, np.sqrt(1.0 - 2e-8)), 0), ("below", pair_ld(300, np.sqrt(1.0 - 0.5e-8)), 4)]
    cases += [(where, with_duplicate(300, *DUPLICATES[where]), 4) for where in sorted(DUPLICATES)]
    for tag, ld, want in cases:
        h = host.mvivw_ld(beta, w, ld, **call)
        d = eng.mvivw_ld(beta, w, ld, **call)
        assert h[3][0] == want and d[3][0] == want, (tag, h[3][0], d[3][0])
        assert abs(d[2][0, 2] - h[2][0, 2]) <= 1e-12, (tag, d[2][0, 2], h[2][0, 2])
        if want == 4:
            assert np.all(np.isnan(d[0][:7])) and np.all(np.isnan(d[1][:7])) and np.isnan(d[2][0, 0]) and np.isnan(d[2][0, 1])
        else:
            assert abs(d[2][0, 2] - 2e-8) <= 1e-12 and np.all(np.isfinite(d[0][:7]))


# ---- 3. bytes, order, the bound, the plain rule ----
def test_identical_calls_and_permuted_outcomes_give_identical_bytes(eng):
    for shape in ((257, 64), (513, 2), (129, 127)):
        beta, w, ld, lists = ld_shape_batch(*shape)
        call = call_of(lists)
        first = eng.mvivw_ld(beta, w, ld, **call)
        again = eng.mvivw_ld(beta, w, ld, **call)
        for a, b in zip(first[:4], again[:4]):
            assert a.tobytes() == b.tobytes()
        perm = [4, 6, 2, 0, 7, 5, 3, 1]
        pcall = call_of([lists[a] for a in perm])
        theta, se, stats, status, _ = eng.mvivw_ld(beta, w, ld, **pcall)
        eo, po = call["ex_off"], pcall["ex_off"]
        for pos, a in enumerate(perm):
            assert theta[po[pos]:po[pos + 1]].tobytes() == first[0][eo[a]:eo[a + 1]].tobytes()
            assert se[po[pos]:po[pos + 1]].tobytes() == first[1][eo[a]:eo[a + 1]].tobytes()
            assert stats[pos].tobytes() == first[2][a].tobytes() and status[pos] == first[3][a]


def test_the_workspace_bound_is_an_argument_error_that_writes_nothing(eng):
    beta, w = problem(300, 7, 0.9)
    ld = ar1_ld(300)
    lists = [(7, np.arange(100), np.arange(7)), (7, np.arange(300), np.arange(7)), (7, np.arange(50, 250), np.arange(7))]
    call = call_of(lists)
    try:
        eng.set_option("mvivw_ld_bytes", 100 * 100 * 8)  # only the smallest outcome fits
        tb, sb, stb, fb = np.full(30, POISON), np.full(30, POISON), np.full((5, 3), POISON), np.full(5, I_POISON, np.int32)
        with pytest.raises(RuntimeError, match="error 2: cusk_mvivw_ld: outcome 1: .*mvivw_ld_bytes"):
            eng.mvivw_ld(beta, w, ld, **call, theta=tb, se=sb, stats=stb, status=fb)
        assert np.all(tb == POISON) and np.all(sb == POISON) and np.all(stb == POISON) and np.all(fb == I_POISON)
        small = eng.mvivw_ld(beta, w, ld, **call_of(lists[:1]))  # the engine is fine, and what fits runs
        assert small[3].tolist() == [0]
        with pytest.raises(RuntimeError):
            eng.set_option("mvivw_ld_bytes", 0)
    finally:
        eng.set_option("mvivw_ld_bytes", 8 << 30)
    whole = eng.mvivw_ld(beta, w, ld, **call)
    assert whole[3].tolist() == [0, 0, 0] and whole[0][:7].tobytes() == small[0][:7].tobytes()
    for bad in (1.0, -0.5, np.nan):
        with pytest.raises(RuntimeError, match="error 2: cusk_mvivw_ld: ridge"):
            eng.mvivw_ld(beta, w, ld, **call, ridge=bad, theta=tb, se=sb, stats=stb, status=fb)
    with pytest.raises(RuntimeError, match="error 2: cusk_mvivw_ld: .*strictly ascending"):
        eng.mvivw_ld(beta, w, ld, outcome=[7], iv_off=[0, 3], iv=[2, 1, 5], ex_off=[0, 1], ex=[0], theta=tb, se=sb, stats=stb, status=fb)
    assert np.all(tb == POISON) and np.all(sb == POISON) and np.all(stb == POISON) and np.all(fb == I_POISON)


def test_identity_ld_gives_the_plain_rule(eng):
    for shape in ((300, 7, 0.9), (700, 39, 0.9), (257, 127, 0.5)):
        beta, w = problem(*shape)
        m, k = shape[:2]
        call = one_call(beta, k)
        plain = eng.mvivw(beta, w, **call)
        got = eng.mvivw_ld(beta, w, np.triu(np.full((m, m), np.nan)), **call)  # the diagonal and above: never read
        assert got[3][0] == 0 and plain[3][0] == 0 and got[2][0, 2] == 1.0
        assert max(rel(got[0][:k], plain[0][:k]), rel(got[1][:k], plain[1][:k]), rel(got[2][0, :2], plain[2][0, :2])) <= 1e-12


# ---- 4. the command line on golden skeletons ----
def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= LD_BOUND * max(abs(b), 1e-300) or a == b


def compare_results(dev_path, host_path):
    dev, host = parse_results(dev_path), parse_results(host_path)
    assert sorted(dev) == sorted(host)
    estimated = 0
    for key, (eff, pv, sk, ns, se) in host.items():
        d = dev[key]
        assert d[2] == sk and d[3] == ns and _close(d[0], eff) and _close(d[4], se), (key, d, host[key])
        assert (np.isnan(d[1]) and np.isnan(pv)) or abs(d[1] - pv) <= LD_BOUND  # a probability: absolute
        estimated += int(np.isfinite(se))
    return estimated


def parse_ld_outcomes(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus\tld_pivot" and lines[-1] == ""
    num = lambda s: np.nan if s == "NA" else float(s)  # noqa: E731
    return [(int(r[0]), int(r[1]), int(r[2]), num(r[3]), num(r[4]), num(r[5]), int(r[6]), num(r[7])) for r in (l.split("\t") for l in lines[1:-1])]


def compare_outcomes(dev_path, host_path):
    dev, host = parse_ld_outcomes(dev_path), parse_ld_outcomes(host_path)
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        assert d[:3] == h[:3] and d[6] == h[6], (d, h)
        assert _close(d[3], h[3]) and _close(d[4], h[4]), (d, h)
        assert (np.isnan(d[5]) and np.isnan(h[5])) or abs(d[5] - h[5]) <= LD_BOUND, (d, h)
        assert (np.isnan(d[7]) and np.isnan(h[7])) or abs(d[7] - h[7]) <= 1e-9, (d, h)
        assert np.isfinite(d[3]) == (d[6] == 0) and np.isfinite(d[7]) == (d[6] in (0, 4))
    return [d[6] for d in dev]


def planted_pair(stem, N):
    """the two markers that most instrument lists of the selection `all` hold"""
    from cigwas_amd import mvivw

    sel = mvivw.run(stem, N)["selection"]
    M = max(int(I.max()) for I, _ in sel) + 1
    count = np.zeros(M, int)
    for I, _ in sel:
        count[I] += 1
    a, b = sorted(np.argsort(-count, kind="stable")[:2].tolist())
    return a, b


@pytest.mark.parametrize("name", ("p6", "p40"))
def test_cli_selections_against_the_host_form(name, tmp_path):
    from cigwas_amd import cli, ivcheck, mvivw

    stem = materialise(name, tmp_path)
    N = load_kat()[name]["num_samples"]
    pair = planted_pair(stem, N)
    p, M = plant_ld(stem, pair)
    prior = np.zeros((p, p), np.int32)
    prior[0, 1:3] = 1
    prior[p - 1, 0] = 1
    prior_path = str(tmp_path / "prior.bin")
    prior.tofile(prior_path)
    table = str(tmp_path / "ivs.csv")
    ivcheck.write_csv(table, ivcheck.iv_candidates(stem))
    fours = estimated = 0
    for tag, flags, kw in (("all", [], {}), ("skeleton", ["-s"], {}), ("prior", ["--orientation-prior", prior_path], {"prior_path": prior_path}),
                           ("ivs", ["--ivs", table], {"ivs_path": table})):
        for ridge in (None, 0.1):
            out = str(tmp_path / f"dev_{tag}_{ridge}_results.tsv")
            cli.main(["mvivw", stem, str(N), "--ld", "--out", out] + flags + ([] if ridge is None else ["--ld-ridge", str(ridge)]))
            res = mvivw.run(stem, N, mode=tag, ld=True, ld_ridge=ridge or 0.0, **kw)
            host_path = str(tmp_path / f"host_{tag}_{ridge}_results.tsv")
            mvivw.write_results(host_path, res)
            estimated += compare_results(out, host_path)
            mvivw.write_outcomes(host_path + ".o", res)
            statuses = compare_outcomes(out[:-len("_results.tsv")] + "_outcomes.tsv", host_path + ".o")
            both = [int(pair[0] in I and pair[1] in I) for I, _ in res["selection"]]
            if ridge is None:  # exactly the outcomes whose lists hold both copies fail, every other one is estimated
                assert statuses == [4 * b for b in both], (tag, statuses, both)
                fours += sum(both)
            else:              # and the ridge turns every status 4 into 0
                assert statuses == [0] * p, (tag, statuses)
    assert fours > 0 and estimated > 0


def test_cli_ld_with_het(tmp_path):
    from cigwas_amd import cli, ivcheck, mvivw

    stem = materialise("p6", tmp_path)
    N = load_kat()["p6"]["num_samples"]
    plant_ld(stem)
    n = ivcheck.load(stem)[1].shape[0]
    sizes = np.full((n, n), N, np.int64)
    sizes[:, 1] = sizes[1, :] = N // 4  # trait 1 is observed on a quarter
    write_ssz(stem, sizes)
    out = str(tmp_path / "het_results.tsv")
    cli.main(["mvivw", stem, "1", "--ld", "--het", "--model", "fixed", "--out", out])
    res = mvivw.run(stem, 1, het=True, ld=True, model=mvivw.MODELS["fixed"])
    host_path = str(tmp_path / "host_results.tsv")
    mvivw.write_results(host_path, res)
    assert compare_results(out, host_path) > 0
    mvivw.write_outcomes(host_path + ".o", res)
    assert compare_outcomes(str(tmp_path / "het_outcomes.tsv"), host_path + ".o") == [0] * 6
    plain = str(tmp_path / "plain_results.tsv")
    cli.main(["mvivw", stem, str(N), "--ld", "--model", "fixed", "--out", plain])
    q, pl = parse_results(out), parse_results(plain)
    moved = [key for key in q if key[1] == 2 and np.isfinite(q[key][4])]
    assert moved and all(q[key][4] > pl[key][4] for key in moved)  # the sizes enter through w: fewer samples, wider se
