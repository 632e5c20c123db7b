"""GPU: `cusk_mvivw_jackknife` (`Engine.mvivw_jackknife`, `ci-gwas mvivw --jackknife`) against the float64 host form
(`mvivw.HostEngine.mvivw_jackknife`), which test_mvivw_jackknife_formats.py holds against a longdouble restatement.

1. Shape sweep: k at the tile-class edges of the refit kernel (1, 2, 43, 44, 45, 87, 88, 127).  Per k one call of three
   problems: groups of 1, 2, slab, slab + 1, 255, 256, 257 rows and one of several slabs (slab = 32 rows, 16 from 88
   columns on), where every refit keeps more than 2 k rows; ng = 2 on m = 4 k + 9; and equal groups B = 5.  Leave-one-out
   at m = 300, and the largest case m = 4,097, k = 127, B = 7.  Everything within BOUND_JK of the host form in the units of
   test_mvivw_jackknife_formats.py; jk_status and jk_arg by equality, the exposures whose two largest moves differ by less
   than BOUND_JK in the host form set aside (at most 1 % of a case, asserted).
2. theta, se, stats and status bit for bit those of `Engine.mvivw` on the same call, in every case of 1.
3. One call that mixes plain status 1, 2, 3 and jk_status 1, 2 between good outcomes of different k and m.
4. Two runs, an outcome alone or among 40, and a small "mvivw_jk_bytes" (several batches) give the same bytes.
5. Guard words behind every output array in every call here (`guard=4`); pres and refit absent or present.
6. The command line on a merged skeleton written here, with and without --het."""
import numpy as np
import pytest

from test_mvivw_jackknife_formats import BOUND_JK, argument_errors, batch_call, jk_problem, status_problems, write_skeleton

pytestmark = pytest.mark.gpu

KS = (1, 2, 43, 44, 45, 87, 88, 127)
PLAIN = ("outcome", "iv_off", "iv", "ex_off", "ex")


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def edge_bounds(k):
    """group sizes at every edge of the refit kernel, and the m that leaves every refit more than 2 k rows"""
    slab = 32 if k + 1 <= 88 else 16
    sizes = [1, 2, slab, slab + 1, 255, 256, 257, 3 * slab + 5, 2 * k + 40]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), slab


def shape_problems(k):
    from cigwas_amd import mvivw

    b, _ = edge_bounds(k)
    out = [(*jk_problem(int(b[-1]), k, 11 * k + 1), b)]
    for m, B in ((4 * k + 9, 2), (5 * (k + 9), 5)):
        out.append((*jk_problem(m, k, 11 * k + B), mvivw.groups(np.arange(m), B)))
    return out


def run(eng, beta, weight, call, **kw):
    return eng.mvivw_jackknife(beta, weight, **call, guard=4, **kw)


def compare(dev, host, beta, weight, call):
    """every output of the device against the host form; returns the largest distance"""
    theta, se, stats, status, jk, jk_arg, jk_stats, jk_status, pres, refit, _ = dev
    th, _, _, status_h, jkh, argh, jsh, jstatus_h, ph, rh, _ = host
    assert status.tolist() == status_h.tolist() and jk_status.tolist() == jstatus_h.tolist(), (jk_status.tolist(), jstatus_h.tolist())
    eo, io, go = call["ex_off"], call["iv_off"], call["grp_off"]
    rf_off = np.concatenate([[0], np.cumsum(np.maximum(np.diff(go) - 1, 0) * np.diff(eo))])
    worst = 0.0
    for a, st in enumerate(jstatus_h):
        e0, e1, i0, i1, r0, r1 = eo[a], eo[a + 1], io[a], io[a + 1], rf_off[a], rf_off[a + 1]
        if st != 0:
            assert np.isnan(jk[e0:e1]).all() and (jk_arg[e0:e1] == -1).all() and np.isnan(pres[i0:i1]).all()
            assert np.isnan(refit[r0:r1]).all() and np.isnan(jk_stats[a][0])
            assert jk_stats[a][1] == jsh[a][1] if (st == 2 and status_h[a] == 0) else np.isnan(jk_stats[a][1]), (a, jk_stats[a])
            continue
        I, E, o, k = call["iv"][i0:i1], call["ex"][e0:e1], call["outcome"][a], e1 - e0
        d = np.sqrt(np.sum(beta[np.ix_(I, E)] ** 2 * weight[I, o][:, None], axis=0))
        scale = np.max(np.abs(d * th[e0:e1]))
        R, Rh = refit[r0:r1].reshape(-1, k), rh[r0:r1].reshape(-1, k)
        dist = [np.max(np.abs(d * (R - Rh))) / scale, np.max(np.abs(d[:, None] * (jk[e0:e1] - jkh[e0:e1]))) / scale,
                np.max(np.abs(pres[i0:i1] - ph[i0:i1])) / np.max(np.abs(ph[i0:i1])), abs(jk_stats[a][0] / jsh[a][0] - 1),
                abs(jk_stats[a][1] / jsh[a][1] - 1)]
        worst = max(worst, *dist)
        assert max(dist) <= BOUND_JK, (a, i1 - i0, k, dist)
        moves = np.sort(np.abs(d * (Rh - th[e0:e1])) / scale, axis=0)
        near = moves[-1] - moves[-2] < BOUND_JK
        assert near.sum() <= 0.01 * k, (a, near.sum())
        assert np.array_equal(jk_arg[e0:e1][~near], argh[e0:e1][~near]), a
    return worst


def check_case(eng, problems, **kw):
    from cigwas_amd import mvivw

    beta, weight, call = batch_call(problems)
    host = mvivw.HostEngine().mvivw_jackknife(beta, weight, **call)
    dev = run(eng, beta, weight, call, **kw)
    worst = compare(dev, host, beta, weight, call)
    plain = eng.mvivw(beta, weight, **{n: call[n] for n in PLAIN})
    for name, a, b in zip(("theta", "se", "stats", "status"), dev[:4], plain[:4]):
        assert a.tobytes() == b.tobytes(), name  # step 0 is cusk_mvivw bit for bit
    return dev, host, worst


# ---- 1, 2. shapes ----
@pytest.mark.parametrize("k", KS)
def test_shape_sweep_against_the_host_form(k, eng):
    b, slab = edge_bounds(k)
    assert np.diff(b).tolist()[:8] == [1, 2, slab, slab + 1, 255, 256, 257, 3 * slab + 5] and np.all(b[-1] - np.diff(b) > 2 * k)
    dev, host, worst = check_case(eng, shape_problems(k))
    assert host[7].tolist() == [0, 0, 0]
    print(f"k {k}: m {np.diff(batch_call(shape_problems(k))[2]['iv_off']).tolist()} distance {worst:.3g}")


@pytest.mark.parametrize("k", (3, 45))
def test_leave_one_out_at_300(k, eng):
    dev, host, worst = check_case(eng, [(*jk_problem(300, k, 300 + k), np.arange(301, dtype=np.int32))])
    assert host[7].tolist() == [0] and dev[9].shape[0] == 300 * k
    print(f"loo m 300 k {k}: distance {worst:.3g}")


def test_the_largest_case(eng):
    from cigwas_amd import mvivw

    dev, host, worst = check_case(eng, [(*jk_problem(4097, 127, 4097), mvivw.groups(np.arange(4097), 7))])
    assert host[7].tolist() == [0]
    print(f"m 4097 k 127 B 7: distance {worst:.3g}")


# ---- 3. statuses between good outcomes ----
def mixed_problems():
    from cigwas_amd import mvivw

    bad = status_problems()
    good = [(*jk_problem(300, 3, 1), mvivw.groups(np.arange(300), 9)), (*jk_problem(513, 45, 2), mvivw.groups(np.arange(513), 4)),
            (*jk_problem(400, 88, 3), mvivw.groups(np.arange(400), 3))]
    order = [good[0], "plain-1", good[1], "lost-column", good[2], "plain-2", "one-group", good[0], "plain-3", "leaves-k", good[1],
             "lost-column-loo"]
    return [q if isinstance(q, tuple) else bad[q][:4] for q in order]


def test_failed_outcomes_leave_their_neighbours_untouched(eng):
    dev, host, _ = check_case(eng, mixed_problems())
    assert host[3].tolist() == [0, 1, 0, 0, 0, 2, 0, 0, 3, 0, 0, 0]
    assert host[7].tolist() == [0, 1, 0, 2, 0, 2, 1, 0, 3, 1, 0, 2]
    beta, weight, call = batch_call(mixed_problems())
    eo, io = call["ex_off"], call["iv_off"]
    jk, pres, jk_stats = dev[4], dev[8], dev[6]
    assert jk[eo[0]:eo[1]].tobytes() == jk[eo[7]:eo[8]].tobytes() and jk_stats[0].tobytes() == jk_stats[7].tobytes()
    assert pres[io[2]:io[3]].tobytes() == pres[io[10]:io[11]].tobytes() and jk_stats[2].tobytes() == jk_stats[10].tobytes()
    for c, word in argument_errors(call):
        with pytest.raises(Exception, match=word if c.get("grp_off", 0) is not None else "bad arguments"):
            run(eng, beta, weight, c)  # the guard words also show that nothing was written
    with pytest.raises(Exception, match="model"):
        run(eng, beta, weight, call, model=3)
    assert run(eng, beta, weight, call)[4].tobytes() == jk.tobytes()  # the engine is still usable


# ---- 4, 5. determinism, independence, absent outputs ----
def as_bytes(res, a=None, call=None):
    if a is None:
        return b"".join(np.ascontiguousarray(v).tobytes() for v in res[:10] if v is not None)
    eo, io, go = call["ex_off"], call["iv_off"], call["grp_off"]
    rf_off = np.concatenate([[0], np.cumsum(np.maximum(np.diff(go) - 1, 0) * np.diff(eo))])
    e, i, r = slice(eo[a], eo[a + 1]), slice(io[a], io[a + 1]), slice(rf_off[a], rf_off[a + 1])
    parts = [res[0][e], res[1][e], res[2][a], res[3][a:a + 1], res[4][e], res[5][e], res[6][a], res[7][a:a + 1], res[8][i], res[9][r]]
    return b"".join(np.ascontiguousarray(v).tobytes() for v in parts)


def test_same_bytes_twice_alone_in_batches_and_without_the_optional_outputs(eng):
    from cigwas_amd import mvivw
    from cigwas_amd.skeleton import Engine

    target = (*jk_problem(513, 45, 2), mvivw.groups(np.arange(513), 40))
    probs = [(*jk_problem(100 + 17 * j, 1 + (5 * j) % 60, j), mvivw.groups(np.arange(100 + 17 * j), 2 + j % 9)) for j in range(39)]
    probs.insert(20, target)
    beta, weight, call = batch_call(probs)
    first = run(eng, beta, weight, call)
    assert (first[7] == 0).all()
    assert as_bytes(run(eng, beta, weight, call)) == as_bytes(first)
    b1, w1, c1 = batch_call([target])
    assert as_bytes(run(eng, b1, w1, c1), 0, c1) == as_bytes(first, 20, call)
    for kw in (dict(want_pres=False), dict(want_refit=False), dict(want_pres=False, want_refit=False)):
        res = run(eng, beta, weight, call, **kw)
        assert (res[8] is None) == (not kw.get("want_pres", True)) and (res[9] is None) == (not kw.get("want_refit", True))
        assert as_bytes(res[:8]) == as_bytes(first[:8])
        assert res[8] is None or res[8].tobytes() == first[8].tobytes()
        assert res[9] is None or res[9].tobytes() == first[9].tobytes()
    small = Engine(0)
    try:
        small.set_option("mvivw_jk_bytes", 4096)  # the target's refits alone are larger: many batches
        assert as_bytes(run(small, beta, weight, call)) == as_bytes(first)
        small.set_option("mvivw_part_bytes", 1 << 16)
        assert as_bytes(run(small, beta, weight, call)) == as_bytes(first)
    finally:
        small.close()


# ---- 6. command line ----
def numbers(path):
    num = lambda s: np.nan if s in ("NA", "TRUE", "FALSE") else float(s)  # noqa: E731
    return np.array([[num(v) for v in l.split("\t")] for l in open(path).read().split("\n")[1:-1]])


@pytest.mark.parametrize("het", (False, True))
def test_cli_files_equal_the_host_form_s(het, tmp_path):
    from cigwas_amd import cli, mvivw

    N = 10000
    stem, labels = write_skeleton(tmp_path, N)
    R, T = str(tmp_path / "resid.tsv"), str(tmp_path / "table.tsv")
    cli.main(["mvivw", stem, str(N), "--jackknife-groups", labels, "--jackknife-residuals", R, "--jackknife-table", T]
             + (["--het"] if het else []))
    res = mvivw.run(stem, N, het=het, jackknife=np.arange(300) // 23)
    assert res["jk_status"].tolist() == [0] * 6
    want = {}
    for name, write in (("r", mvivw.write_results), ("o", mvivw.write_outcomes), ("e", mvivw.write_jackknife_residuals),
                        ("t", mvivw.write_jackknife_table)):
        write(str(tmp_path / name), res)
        want[name] = numbers(str(tmp_path / name))
    got = {"r": numbers(stem + "_mvivw_results.tsv"), "o": numbers(stem + "_mvivw_outcomes.tsv"), "e": numbers(R), "t": numbers(T)}
    assert open(stem + "_mvivw_results.tsv").readline().endswith("\tjk_effect\tjk_se\tjk_p\tjk_min\tjk_max\tjk_marker\n")
    assert open(stem + "_mvivw_outcomes.tsv").readline().endswith("\tjk_groups\tpress\tjk_pivot\tjk_status\n")
    # estimates agree within BOUND_JK in standardised units, here far below 1e-6 relative of values above 1e-3; the p-values
    # are functions of them
    for name in "roet":
        assert got[name].shape == want[name].shape and np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
        np.testing.assert_allclose(got[name], want[name], rtol=1e-6, atol=1e-9, err_msg=name)
    assert np.array_equal(got["r"][:, 12], want["r"][:, 12]) and np.array_equal(got["t"][:, :6], want["t"][:, :6])
