"""GPU: the instrument filter's tests on the device (`cusk_iv_check`, `cusk_iv_check_het`, `check-ivs`).

1. Goldens through the ABI: every test the reference performed (tests/golden/iv_check_<case>.npz).  Per case the generator
   asserted margin = min |z_ref - thr| >= 1000 d, so a kernel z within margin / 2 of z_ref cannot flip a verdict: flags
   must equal the reference's verdicts for EVERY recorded test.  Second bound: |z - z_ref| <= p max(d, 2^-52 (1 + |z_ref|)),
   the same formula in the same precision with another summation order over at most p terms.
2. Goldens through the files: `check_ivs(engine=...)` and the command line write the reference's rows.
3. Shape sweep against the numpy host form: item counts around the tile (64) and set sizes around every LDS class.
4. Argument errors, a singular set, an indefinite set, NaN.
5. Het: uniform sizes reproduce the table call bit for bit; sizes that differ by trait agree with the in-test oracle."""
import os

import numpy as np
import pytest
from scipy.stats import norm

from test_iv_check_formats import (CASES, HET_CASE, HET_QUARTER, flag_sets, het_oracle, load_kat, load_tests, materialise,
                                   rows_of, trait_corr_of, trait_sizes)
from test_sepselect_het_formats import write_ssz

pytestmark = pytest.mark.gpu

Z_POISON, F_POISON = -777.0, -12345


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def poisoned(n, guard=7):
    return np.full(n + guard, Z_POISON), np.full(n + guard, F_POISON, np.int32)


def check_guard(z, flags, n):
    assert np.all(z[n:] == Z_POISON) and np.all(flags[n:] == F_POISON)
    assert not np.any(flags[:n] == F_POISON) and not np.any(z[:n] == Z_POISON)


# ---- 1. goldens through the ABI ----
@pytest.mark.parametrize("name", CASES)
def test_goldens_through_the_abi(name, eng, tmp_path):
    from cigwas_amd import ivcheck

    case, t = load_kat()[name], load_tests(name)
    tc = trait_corr_of(name, tmp_path)
    p = case["traits"]
    worst = 0.0
    for alpha_id, alpha in enumerate((case["accept_alpha"], case["reject_alpha"])):
        pick = t["alpha_id"] == alpha_id
        n = int(pick.sum())
        zb, fb = poisoned(n)
        z, flags, _ = eng.iv_check(tc, t["set_off"], t["sets"], t["x"][pick], t["y"][pick], t["set"][pick],
                                   ivcheck.thresholds(alpha, case["num_samples"], p), z=zb, flags=fb)
        check_guard(zb, fb, n)
        zr = t["z"][pick]
        dev = np.abs(z - zr)
        worst = max(worst, float(dev.max()))
        print(f"{name} alpha {alpha}: {n} tests, max |z - z_ref| {dev.max():.3e} (margin {case['margin']:.3e}, d {case['d']:.3e})")
        assert not (flags >> 8).any()
        assert np.array_equal(flags & 1, (zr < t["thr"][pick]).astype(np.int32))
        assert dev.max() <= case["margin"] / 2
        assert np.all(dev <= p * np.maximum(case["d"], 2.0 ** -52 * (1 + np.abs(zr))))
    print(f"{name}: measured maximum deviation {worst:.3e}")


# ---- 2. goldens through the files ----
@pytest.mark.parametrize("name", CASES)
def test_goldens_through_the_files(name, eng, tmp_path):
    from cigwas_amd import cli, ivcheck

    case = load_kat()[name]
    stem = materialise(name, tmp_path)
    read = lambda path: [tuple(int(v) for v in ln.split(",")) for ln in open(path).read().splitlines()[1:]]  # noqa: E731
    for key, relaxed, reverse in flag_sets(case):
        stats = {}
        rows = ivcheck.check_ivs(stem, case["num_samples"], case["accept_alpha"], case["reject_alpha"],
                                 relaxed_local_faithfulness=relaxed, check_reverse_causality=reverse, engine=eng, stats=stats)
        assert rows == rows_of(name, key), key
        assert stats["calls"] <= 4 and stats["kernel_ms"] > 0
        out = os.path.join(str(tmp_path), "ivs.csv")
        cli.main(["check-ivs", stem, str(case["num_samples"]), "--accept-alpha", repr(case["accept_alpha"]), "--reject-alpha",
                  repr(case["reject_alpha"]), "--out", out] + (["--relaxed-local-faithfulness"] if relaxed else []) +
                 (["--check-reverse-causality"] if reverse else []))
        assert open(out).readline() == "Exposure,Outcome,IV\n" and read(out) == rows_of(name, key), key
    # default output name, and uniform sizes through --het
    n = case["traits"] + case["markers"]
    write_ssz(stem, np.full((n, n), case["num_samples"]))
    key, relaxed, reverse = flag_sets(case)[0]
    cli.main(["check-ivs", stem, "1", "--accept-alpha", repr(case["accept_alpha"]), "--reject-alpha", repr(case["reject_alpha"]),
              "--het"] + (["--relaxed-local-faithfulness"] if relaxed else []) + (["--check-reverse-causality"] if reverse else []))
    assert read(stem + "_ivs.csv") == rows_of(name, key)


# ---- 3. shape sweep ----
SWEEP_P, SWEEP_M = 130, 90


@pytest.fixture(scope="module")
def sweep_corr():
    """sample correlations of 220 variables on 6000 draws: well conditioned, nothing structural"""
    rng = np.random.default_rng(5)
    n = SWEEP_P + SWEEP_M
    F = rng.normal(size=(6000, 8))
    X = F @ (rng.normal(size=(8, n)) * 0.25) + rng.normal(size=(6000, n))
    corr = np.corrcoef(X.T)
    corr = 0.5 * (corr + corr.T)
    np.fill_diagonal(corr, 1.0)
    return np.ascontiguousarray(corr[:, :SWEEP_P]), float(np.linalg.cond(corr[:SWEEP_P, :SWEEP_P]))


def sweep_items(rng, nitems, set_lists, n, p):
    """items spread over the sets and the empty set, a few y per set, x any variable outside {y} + S; shuffled"""
    xs, ys, iset = [], [], []
    for k in range(nitems):
        s = int(rng.integers(-1, len(set_lists)))
        S = set(set_lists[s]) if s >= 0 else set()
        free = [t for t in range(p) if t not in S]
        y = free[int(rng.integers(0, min(3, len(free))))]
        while True:
            x = int(rng.integers(0, n))
            if x != y and x not in S:
                break
        xs.append(x), ys.append(y), iset.append(s)
    order = rng.permutation(nitems)
    return (np.array(a, np.int32)[order] for a in (xs, ys, iset))


@pytest.mark.parametrize("s", (0, 1, 2, 31, 32, 33, 63, 64, 65, 127))
def test_shape_sweep_against_the_host_form(s, eng, sweep_corr):
    from cigwas_amd import ivcheck

    tc, cond = sweep_corr
    n, p = tc.shape
    rng = np.random.default_rng(100 + s)
    set_lists = [sorted(rng.choice(p, size=s, replace=False).tolist()) for _ in range(3)] if s else []
    set_off = np.zeros(len(set_lists) + 1, np.int32)
    set_off[1:] = np.cumsum([len(v) for v in set_lists])
    sets = np.array([t for v in set_lists for t in v], np.int32)
    # both compute the same sums in float64 in another order: s^2 products against W (norm <= cond) and entries <= 1
    tol = 64 * max(s, 1) ** 2 * 2.0 ** -52 * cond
    for nitems in (1, 63, 64, 65, 4097):
        xs, ys, iset = sweep_items(rng, nitems, set_lists, n, p)
        zh, status = ivcheck.host_z(tc, set_off, sets, xs, ys, iset)
        assert not status.any()
        thr = np.full(p, np.median(zh))  # both verdicts occur
        zb, fb = poisoned(nitems)
        z, flags, ms = eng.iv_check(tc, set_off, sets, xs, ys, iset, thr, z=zb, flags=fb)
        check_guard(zb, fb, nitems)
        assert not (flags >> 8).any() and ms > 0
        assert np.max(np.abs(z - zh)) <= tol, (s, nitems, float(np.max(np.abs(z - zh))), tol)
        far = np.abs(zh - thr[0]) > tol
        assert np.array_equal((flags & 1)[far], (zh < thr[0])[far].astype(np.int32))
        if nitems >= 63:
            assert (flags & 1).any() and not (flags & 1).all()


# ---- 4. errors and edges ----
def test_argument_errors_launch_nothing(eng, sweep_corr):
    tc, _ = sweep_corr
    n, p = tc.shape
    thr = np.ones(p)
    big = list(range(128))
    cases = [
        ("longer than 127", [0, 128], big, [p], [129], [0]),
        ("twice", [0, 3], [1, 2, 1], [p], [0], [0]),
        ("not a trait index", [0, 2], [1, p], [p + 1], [0], [0]),
        ("not a trait index", [0, 2], [1, -1], [p + 1], [0], [0]),
        ("own conditioning set", [0, 2], [1, 2], [1], [0], [0]),
        ("own conditioning set", [0, 2], [1, 2], [p], [2], [0]),
        ("not a variable index", [0, 1], [1], [n], [0], [0]),
        ("not a variable index", [0, 1], [1], [p], [-1], [0]),
        ("x equals y", [0, 1], [1], [5], [5], [0]),
        ("neither x nor y is a trait", [0, 1], [1], [p], [p + 1], [0]),
        ("set index out of range", [0, 1], [1], [p], [0], [1]),
    ]
    for msg, set_off, sets, xs, ys, iset in cases:
        zb, fb = poisoned(1)
        with pytest.raises(RuntimeError, match=msg):
            eng.iv_check(tc, set_off, sets, xs, ys, iset, thr, z=zb, flags=fb)
        assert np.all(zb == Z_POISON) and np.all(fb == F_POISON)
    z, flags, _ = eng.iv_check(tc, [0, 1], [1], [p], [0], [0], thr)  # the engine is fine afterwards
    assert flags[0] >> 8 == 0 and np.isfinite(z[0])


def test_singular_set_marks_its_items_only(eng, sweep_corr):
    from cigwas_amd import ivcheck

    tc = sweep_corr[0].copy()
    n, p = tc.shape
    tc[:, 7] = tc[:, 3]  # trait 7 becomes a copy of trait 3
    tc[7, :] = tc[3, :]
    tc[3, 7] = tc[7, 3] = 1.0
    set_lists = [[1, 2, 4], [3, 5, 7, 9], [6, 8], [0, 3, 7] + list(range(10, 50))]
    set_off = np.cumsum([0] + [len(v) for v in set_lists]).astype(np.int32)
    sets = np.array([t for v in set_lists for t in v], np.int32)
    rng = np.random.default_rng(1)
    iset = rng.integers(-1, 4, size=300).astype(np.int32)
    xs = rng.integers(p, n, size=300).astype(np.int32)
    ys = np.full(300, 60, np.int32)
    z, flags, _ = eng.iv_check(tc, set_off, sets, xs, ys, iset, np.full(p, 0.01))
    bad = (iset == 1) | (iset == 3)
    assert bad.any() and (~bad).any()
    assert np.all(flags[bad] == 2 << 8) and np.all(np.isnan(z[bad]))
    assert not (flags[~bad] >> 8).any()
    zh, _ = ivcheck.host_z(tc, set_off, sets, xs[~bad], ys[~bad], iset[~bad])
    assert np.max(np.abs(z[~bad] - zh)) <= 1e-12


def test_indefinite_set_agrees_with_the_inverse(eng):
    """pairwise-complete correlations need not be positive definite: the first pivot candidates are exchanged"""
    p, n = 5, 9
    rng = np.random.default_rng(2)
    corr = np.eye(n)
    corr[0, 1] = corr[1, 0] = 0.9
    corr[0, 2] = corr[2, 0] = 0.9
    corr[1, 2] = corr[2, 1] = -0.9
    for a in range(n):
        for b in range(max(a + 1, 3), n):
            if a < p or b < p:
                corr[a, b] = corr[b, a] = rng.uniform(-0.2, 0.2)
    assert np.linalg.eigvalsh(corr[:3, :3]).min() < -0.1
    tc = np.ascontiguousarray(corr[:, :p])
    xs = np.arange(5, 9, dtype=np.int32)
    ys = np.array([3, 4, 3, 4], np.int32)
    z, flags, _ = eng.iv_check(tc, [0, 3], [0, 1, 2], xs, ys, [0] * 4, np.full(p, 0.05))
    zo, _ = het_oracle(tc, np.ones((n, p), np.int64), [0, 3], [0, 1, 2], xs, ys, [0] * 4, 1.0)
    assert not (flags >> 8).any()
    assert np.max(np.abs(z - zo)) <= 1e-13
    assert np.array_equal(flags & 1, (zo < 0.05).astype(np.int32))


def test_nan_is_dependent(eng, sweep_corr):
    tc = sweep_corr[0].copy()
    n, p = tc.shape
    tc[p + 1, 4] = np.nan  # a set member's correlation with one marker
    tc[p + 2, 0] = np.nan  # a raw correlation
    z, flags, _ = eng.iv_check(tc, [0, 3], [2, 4, 6], [p + 1, p + 3, p + 2, p + 3], [0, 0, 0, 0], [0, 0, -1, -1], np.full(p, 1e9))
    assert np.isnan(z[0]) and flags[0] == 0
    assert np.isnan(z[2]) and flags[2] == 0
    assert np.isfinite(z[1]) and flags[1] == 1 and np.isfinite(z[3]) and flags[3] == 1


# ---- 5. het ----
@pytest.mark.parametrize("name", CASES)
def test_het_at_uniform_sizes_is_the_table_call_bit_for_bit(name, eng, tmp_path):
    from cigwas_amd import ivcheck

    case, t = load_kat()[name], load_tests(name)
    tc = trait_corr_of(name, tmp_path)
    n, p, N = tc.shape[0], case["traits"], case["num_samples"]
    for alpha in (case["accept_alpha"], case["reject_alpha"]):
        z0, f0, _ = eng.iv_check(tc, t["set_off"], t["sets"], t["x"], t["y"], t["set"], ivcheck.thresholds(alpha, N, p))
        z1, f1, _ = eng.iv_check_het(tc, t["set_off"], t["sets"], t["x"], t["y"], t["set"], np.full((n, p), N, np.int32),
                                     norm.ppf(1 - alpha / 2))
        assert np.array_equal(z0.view(np.int64), z1.view(np.int64)) and np.array_equal(f0, f1)
        assert (f0 & 1).any() and not (f0 & 1).all()


def test_check_ivs_on_a_duplicated_trait_names_the_outcome(eng, tmp_path):
    """device and host form call the same sets singular (the kernel's exact-zero pivot rule, restated in ivcheck.exactly_singular)"""
    from cigwas_amd import ivcheck

    from test_iv_check_formats import duplicated_trait_stem

    stem = duplicated_trait_stem(tmp_path)
    for engine in (eng, None):
        with pytest.raises(ivcheck.SingularSetError, match=r"outcome trait 1 \(1-based\)"):
            ivcheck.check_ivs(stem, 20000, 1e-4, 1e-3, relaxed_local_faithfulness=True, engine=engine)


def test_het_with_differing_sizes_agrees_with_the_oracle(eng, tmp_path):
    from cigwas_amd import ivcheck

    case, t = load_kat()[HET_CASE], load_tests(HET_CASE)
    stem = materialise(HET_CASE, tmp_path)
    tc = trait_corr_of(HET_CASE, tmp_path)
    n, p, N = tc.shape[0], case["traits"], case["num_samples"]
    ssz = trait_sizes(n, p, N, HET_QUARTER)
    tn = ssz[:, :p].astype(np.int32)
    for alpha in (case["accept_alpha"], case["reject_alpha"]):
        q = norm.ppf(1 - alpha / 2)
        zb, fb = poisoned(t["x"].size)
        z, flags, _ = eng.iv_check_het(tc, t["set_off"], t["sets"], t["x"], t["y"], t["set"], tn, q, z=zb, flags=fb)
        check_guard(zb, fb, t["x"].size)
        zo, thr = het_oracle(tc, tn, t["set_off"], t["sets"], t["x"], t["y"], t["set"], q)
        assert np.min(np.abs(zo - thr)) > 1e3 * max(case["d"], 1e-15)  # condition on the inputs (also asserted on the CPU)
        assert np.max(np.abs(z - zo)) <= p * max(case["d"], 2.0 ** -52 * (1 + np.abs(zo).max()))
        assert np.array_equal(flags, (zo < thr).astype(np.int32))
    bad = tn.copy()
    bad[0, 1] += 1
    with pytest.raises(RuntimeError, match="not symmetric"):
        eng.iv_check_het(tc, t["set_off"], t["sets"], t["x"], t["y"], t["set"], bad, 2.0)
    # through the files: the host form's rows (pinned to the oracle on the CPU)
    write_ssz(stem, ssz)
    for key, relaxed, reverse in flag_sets(case):
        kw = dict(relaxed_local_faithfulness=relaxed, check_reverse_causality=reverse, het=True)
        assert ivcheck.check_ivs(stem, 0, case["accept_alpha"], case["reject_alpha"], engine=eng, **kw) == \
            ivcheck.check_ivs(stem, 0, case["accept_alpha"], case["reject_alpha"], **kw)
