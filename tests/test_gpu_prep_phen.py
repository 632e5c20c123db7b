"""GPU: cusk_phen_adjust / cusk_phen_moments against the rule restated in float64 (tests/test_prep_phen_formats.py:
np.linalg.lstsq on the raw covariates with an intercept, rounded to float32), and `prep-phen` / `check-phen` through the CLI.

The bound on `out` is ONE float32 ulp.  Where it comes from: the device solves the normal equations in double on the scaled
design, so its relative error is of order kappa^2 c n 2^-53; every case asserts that premise on the design it drew
(kappa(scaled design)^2 c n 2^-53 < 2^-26), and what is left is a value that lands on a float32 rounding boundary.  n, status
and the NaN pattern are compared by equality.  sd and r2 are held to 1e-9 relative.  mean and beta are held to 1e-9 of their
natural unit plus their own size: the mean of a residual is zero in exact arithmetic and a coefficient may be, so neither
has a relative error of its own; the unit is sd(y) for the mean, sd(y) / sd(x_j) for a slope and sd(y) (1 + sum |mu_j| /
sd(x_j)) for the intercept."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_prep_phen_formats import CHUNK, OK, SINGULAR, TOO_FEW, adjust_restated, draw, premise_holds
from test_prune_cases import pack_bed, planted_genotypes, write_fileset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NS = (1, 2, 63, 64, 65, 257, 1027, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
CS = (0, 1, 2, 7, 8, 9, 31, 32, 63)
PS = (1, 3, 9)
GAPS = (None, "random", "first_chunk", "covar", "all_nan")


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def compare(got, ref, Y, X, c, label):
    assert premise_holds(ref, c), label
    assert np.array_equal(got["status"], ref["status"]), (label, got["status"], ref["status"])
    assert np.array_equal(got["n"], ref["n"]), label
    assert np.array_equal(np.isnan(got["out"]), np.isnan(ref["out"])), label
    seen = ~np.isnan(ref["out"])
    ulps = np.abs(got["out"][seen].astype(np.float64) - ref["out"][seen]) / np.spacing(np.abs(ref["out"][seen]))
    worst = float(ulps.max()) if ulps.size else 0.0
    print(f"{label}: max |out - float64| = {worst:g} ulp, {int((ulps > 0).sum())} of {ulps.size} values differ")
    assert worst <= 1.0, label
    A = np.all(np.isfinite(X), axis=0) if c else None
    for t in range(Y.shape[0]):
        if ref["status"][t] != OK:
            assert np.isnan(got["mean"][t]) and np.isnan(got["sd"][t]) and np.all(np.isnan(got["beta"][t])) and np.isnan(got["r2"][t])
            continue
        fitted = np.isfinite(ref["r2"][t])
        U = np.isfinite(Y[t]) & (A if fitted else True)
        sy = Y[t, U].astype(np.float64).std()
        assert abs(got["sd"][t] - ref["sd"][t]) <= 1e-9 * ref["sd"][t], (label, t)
        assert abs(got["mean"][t] - ref["mean"][t]) <= 1e-9 * (abs(ref["mean"][t]) + sy), (label, t)
        if not fitted:
            assert np.isnan(got["r2"][t]) and np.all(np.isnan(got["beta"][t]))
            continue
        assert abs(got["r2"][t] - ref["r2"][t]) <= 1e-9 * abs(ref["r2"][t]), (label, t, got["r2"][t], ref["r2"][t])
        x = X[:, U].astype(np.float64)
        mu, sx = x.mean(axis=1), x.std(axis=1)
        unit = np.concatenate([[sy * (1.0 + np.sum(np.abs(mu) / sx))], sy / sx])
        err = np.abs(got["beta"][t] - ref["beta"][t]) / (np.abs(ref["beta"][t]) + unit)
        assert np.all(err <= 1e-9), (label, t, err.max())


def shapes_for(N):
    """every c that leaves n_t >= c + 2 with room after 30 % gaps, p and the missingness pattern rotating"""
    out = []
    for k, c in enumerate(CS):
        if c and N < 4 * (c + 2):
            continue
        out.append((c, PS[(k + N) % 3], GAPS[(k + N) % 5]))
    return out


@pytest.mark.parametrize("N", NS)
def test_adjust_equals_float64_within_one_ulp(eng, N):
    for c, p, gaps in shapes_for(N):
        Y, X = draw(N, p, c, 1000 * N + c, gaps=gaps)
        ref = adjust_restated(Y, X)
        got = eng.phen_adjust(Y, X if c else None, N, p, c)
        compare(got, ref, Y, X, c, f"N={N} c={c} p={p} gaps={gaps}")
        if gaps == "all_nan":
            assert got["status"][-1] == TOO_FEW and got["n"][-1] == 0
        again = eng.phen_adjust(Y, X if c else None, N, p, c)
        for key in ("out", "mean", "sd", "beta", "r2"):
            assert np.array_equal(_bits(got[key]), _bits(again[key])), (N, c, key)  # the same bytes


def test_age_and_age_squared_in_raw_units(eng):
    """raw condition number in the millions, scaled one moderate: the case the scaling is there for"""
    N, p, c = 3001, 3, 4
    Y, X = draw(N, p, c, 77, gaps="random", age=True)
    Y = (Y + 0.02 * (X[0] - 55.0) + 0.001 * (X[1] - 3025.0)).astype(np.float32)
    U = np.isfinite(Y[0])
    raw = np.linalg.cond(np.vstack([np.ones(U.sum()), X[:, U].astype(np.float64)]).T)
    ref = adjust_restated(Y, X)
    print(f"age design: condition number raw {raw:.3g}, scaled {ref['cond'].max():.3g}")
    assert raw > 1e5 and ref["cond"].max() < 1e3
    compare(eng.phen_adjust(Y, X, N, p, c), ref, Y, X, c, "age, age^2")


def test_adjust_flags_status_and_guards(eng):
    N, p, c = CHUNK + 77, 4, 3
    Y, X = draw(N, p, c, 5, gaps="random")
    X = np.vstack([X[:2], X[:1]]).astype(np.float32)  # covariate 2 duplicates covariate 0: every adjusted trait is singular
    adjust = np.array([1, 0, 1, 0], np.uint8)
    ref = adjust_restated(Y, X, adjust)
    assert list(ref["status"]) == [SINGULAR, OK, SINGULAR, OK]
    out = np.full(p * N + GUARD, -7.0, np.float32)
    stats = {"n": np.full(p + GUARD, -5, np.int32), "mean": np.full(p + GUARD, -5.0), "sd": np.full(p + GUARD, -5.0),
             "beta": np.full(p * (c + 1) + GUARD, -5.0), "r2": np.full(p + GUARD, -5.0), "status": np.full(p + GUARD, -5, np.int32)}
    keep = {k: v for k, v in stats.items()}
    got = eng.phen_adjust(Y, X, N, p, c, adjust=adjust, out=out, stats=stats)
    compare(got, ref, Y, X, c, "flags")
    assert np.all(np.isnan(got["out"][[0, 2]]))
    assert np.all(out[p * N:] == -7.0)
    for key, arr in keep.items():
        used = p * (c + 1) if key == "beta" else p
        assert np.all(arr[used:] == -5), key
    # a covariate that does not vary where one trait lives: that trait alone is singular
    Y2, X2 = draw(N, 3, 2, 6)
    X2[0, :300] = 2.0
    Y2[1, 300:] = np.nan
    ref2 = adjust_restated(Y2, X2)
    assert list(ref2["status"]) == [OK, SINGULAR, OK]
    compare(eng.phen_adjust(Y2, X2, N, 3, 2), ref2, Y2, X2, 2, "constant within one trait")
    # n_t = c + 1 is too few, c + 2 is enough
    Y3, X3 = draw(200, 2, 5, 8)
    Y3[0, 6:] = np.nan
    Y3[1, 7:] = np.nan
    ref3 = adjust_restated(Y3, X3)
    got3 = eng.phen_adjust(Y3, X3, 200, 2, 5)
    assert list(ref3["status"]) == [TOO_FEW, OK] and np.array_equal(got3["status"], ref3["status"]) and list(got3["n"]) == [6, 7]


def test_host_and_device_inputs_and_moments(eng):
    from cigwas_amd.skeleton import DeviceArray

    N, p, c = 2 * CHUNK + 3, 3, 7
    Y, X = draw(N, p, c, 21, gaps="random")
    host = eng.phen_adjust(Y, X, N, p, c)
    # resident copies with poison behind them: nothing past row ends may be read
    Yd = DeviceArray(np.concatenate([Y.reshape(-1), np.full(GUARD, 1e30, np.float32)]))
    Xd = DeviceArray(np.concatenate([X.reshape(-1), np.full(GUARD, np.nan, np.float32)]))
    dev = eng.phen_adjust(Yd, Xd, N, p, c)
    for key in ("out", "mean", "sd", "beta", "r2"):
        assert np.array_equal(_bits(host[key]), _bits(dev[key])), key
    assert np.array_equal(host["n"], dev["n"]) and np.array_equal(host["status"], dev["status"])
    # the moments alone = the moments of an adjustment without covariates
    plain = eng.phen_adjust(Y, None, N, p, 0)
    for src in (Y, Yd):
        n, mean, sd = eng.phen_moments(src, N, p)
        assert np.array_equal(n, plain["n"]) and np.array_equal(_bits(mean), _bits(plain["mean"])) and np.array_equal(_bits(sd), _bits(plain["sd"]))
    z = plain["out"].astype(np.float64)
    n2, mean2, sd2 = eng.phen_moments(plain["out"], N, p)
    assert np.all(np.abs(mean2) < 1e-6) and np.all(np.abs(sd2 - 1) < 1e-6) and np.array_equal(n2, np.isfinite(z).sum(axis=1))
    Yd.free()
    Xd.free()


def test_argument_errors_launch_nothing(eng):
    from cigwas_amd._lib import lib

    L = lib()
    N, p = 50, 2
    Y, X = draw(N, p, 2, 3)
    big = np.zeros((64, N), np.float32)
    adjust = np.ones(p, np.uint8)
    out = np.full(p * N, -7.0, np.float32)
    n = np.full(p, -5, np.int32)
    ARG = 2
    assert L.cusk_phen_adjust(eng.h, _ptr(Y), _ptr(big), N, p, 64, _ptr(adjust), _ptr(out), _ptr(n), None, None, None, None, None) == ARG
    assert "63" in L.cusk_last_error(eng.h).decode()
    for args in ((None, _ptr(X), N, p, 2, _ptr(adjust), _ptr(out)), (_ptr(Y), None, N, p, 2, _ptr(adjust), _ptr(out)),
                 (_ptr(Y), _ptr(X), 0, p, 2, _ptr(adjust), _ptr(out)), (_ptr(Y), _ptr(X), N, 0, 2, _ptr(adjust), _ptr(out)),
                 (_ptr(Y), _ptr(X), N, p, 2, None, _ptr(out)), (_ptr(Y), _ptr(X), N, p, 2, _ptr(adjust), None)):
        assert L.cusk_phen_adjust(eng.h, *args, _ptr(n), None, None, None, None, None) == ARG
    assert L.cusk_phen_moments(eng.h, None, N, p, _ptr(n), None, None) == ARG
    assert np.all(out == -7.0) and np.all(n == -5)
    # a constant covariate is an argument error that names it, and nothing is written
    Xc = X.copy()
    Xc[1] = 4.0
    with pytest.raises(RuntimeError, match="covariate 1"):
        eng.phen_adjust(Y, Xc, N, p, 2, out=out)
    assert np.all(out == -7.0)
    compare(eng.phen_adjust(Y, X, N, p, 2), adjust_restated(Y, X), Y, X, 2, "after the errors")


# ---- through the command line ---------------------------------------------------------------------------------------

def _cli(*argv):
    return subprocess.run([sys.executable, "-c", "import sys, cigwas_amd.cli as c; c.main(sys.argv[1:])", *argv], cwd=ROOT,
                          capture_output=True, text=True)


FLAG_N, FLAG_ALPHA = 2000, 1e-4


def planted_cohort(seed=3):
    """Two continuous traits that share the covariate `age` and nothing else, and two graded traits.
    Margins, in float64 on the CPU (asserted in the test before anything runs on the device): the level-0 threshold of cuskss
    at N = 1940 observed individuals and alpha = 1e-4 is |atanh r| >= 3.89 / sqrt(N - 3) = 0.0884; the traits are
    0.5 age_z + noise, so their raw correlation is 0.25 / 1.25 = 0.2 (atanh 0.203: more than twice the threshold), and the
    correlation of their residuals is that of two independent noises, sd 1 / sqrt(N) = 0.023 (asserted: below half the
    threshold)."""
    rng = np.random.default_rng(seed)
    N = FLAG_N
    age = rng.uniform(40, 70, N)
    sex = rng.integers(0, 2, N).astype(np.float64)
    az = (age - age.mean()) / age.std()
    t0 = 100 + 8 * (0.5 * az + rng.standard_normal(N))
    t1 = -3 + 0.1 * (0.5 * az + rng.standard_normal(N))
    lat = rng.standard_normal((2, N)) + 0.8 * rng.standard_normal(N)
    o0 = np.digitize(lat[0], [-0.5, 0.7]).astype(np.float64) + 1  # levels 1, 2, 3
    o1 = (lat[1] > 0.2).astype(np.float64)                         # 0 / 1
    Y = np.vstack([t0, t1, o0, o1]).astype(np.float32)
    X = np.vstack([age, age ** 2, sex]).astype(np.float32)
    absent = rng.random(N) < 0.03
    return Y, X, absent, ["t0", "t1", "o0", "o1"], ["age", "age2", "sex"]


def write_shuffled(path, ids, names, M, absent, rng):
    order = rng.permutation(len(ids))
    with open(path, "w") as f:
        f.write("IID\tFID\t" + "\t".join(names) + "\n")
        for i in order:
            if not absent[i]:
                f.write(f"{ids[i][1]}\t{ids[i][0]}\t" + "\t".join("NA" if np.isnan(v) else repr(float(v)) for v in M[:, i]) + "\n")
        f.write("nobody\tx\t" + "\t".join(["1"] * len(names)) + "\n")


def test_cli_prep_check_sumstats_and_the_flag(eng, oracle, tmp_path):
    import cigwas_amd as cg
    from cigwas_amd import cli

    Y, X, absent, names, cnames = planted_cohort()
    N, m = FLAG_N, 24
    stem = str(tmp_path / "set")
    write_fileset(stem, pack_bed(planted_genotypes(m, N, 8, 4)), N, ["1"] * m)
    ids = [(f"f{i}", f"i{i}") for i in range(N)]
    rng = np.random.default_rng(9)
    table, covar = str(tmp_path / "traits.tsv"), str(tmp_path / "covar.tsv")
    write_shuffled(table, ids, names, Y, absent, rng)
    write_shuffled(covar, ids, cnames, X, np.zeros(N, bool), rng)
    Ya, Xa = Y.copy(), X.copy()
    Ya[:, absent] = np.nan
    adjust = np.array([1, 1, 0, 0], np.uint8)
    ref_adj, ref_std = adjust_restated(Ya, Xa, adjust), adjust_restated(Ya)
    # the margins of the docstring, in float64, before the device is asked
    th0 = float(cg.threshold_array(int((~absent).sum()), FLAG_ALPHA)[0])
    seen = ~absent
    r_std = np.corrcoef(ref_std["out"][0, seen].astype(np.float64), ref_std["out"][1, seen].astype(np.float64))[0, 1]
    r_adj = np.corrcoef(ref_adj["out"][0, seen].astype(np.float64), ref_adj["out"][1, seen].astype(np.float64))[0, 1]
    print(f"flag: level-0 threshold {th0:.4f}; atanh r unadjusted {np.arctanh(r_std):.4f}, adjusted {np.arctanh(r_adj):.4f}")
    assert abs(np.arctanh(r_std)) > 2 * th0 and abs(np.arctanh(r_adj)) < 0.5 * th0

    out_adj, out_std = str(tmp_path / "adj.phen"), str(tmp_path / "std.phen")
    r = _cli("prep-phen", stem, table, out_adj, "--covar", covar, "--ordinal", "o0,o1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{int((~absent).sum())} of {N} individuals of the .fam found, 1 rows of the table dropped" in r.stdout
    r = _cli("prep-phen", stem, table, out_std)
    assert r.returncode == 0, r.stdout + r.stderr
    # row-aligned, and the values of the engine on the aligned arrays, bit for bit
    for path, ref, kw in ((out_adj, ref_adj, dict(covar=Xa, c=3, adjust=adjust)), (out_std, ref_std, dict(covar=None, c=0))):
        got_names, data, info = cg.phen_table_load(path, stem + ".fam")
        assert got_names == names and info == {"matched": N, "dropped": 0, "in_order": True}
        lines = open(path).read().splitlines()
        assert lines[0] == "FID\tIID\t" + "\t".join(names) and [ln.split("\t")[:2] for ln in lines[1:]] == [list(x) for x in ids]
        want = eng.phen_adjust(Ya, kw["covar"], N, 4, kw["c"], adjust=kw.get("adjust"))
        assert np.all((_bits(data) == _bits(want["out"])) | (np.isnan(data) & np.isnan(want["out"])))
        assert np.array_equal(np.isnan(data), np.isnan(ref["out"]))
        assert np.all(np.abs(data - ref["out"])[~np.isnan(data)] <= np.spacing(np.abs(ref["out"][~np.isnan(data)])))
        rep = [ln.split("\t") for ln in open(path + ".prep.tsv").read().splitlines()]
        assert rep[0] == ["trait", "mode", "n", "mean", "sd", "r2"] and [x[0] for x in rep[1:]] == names
        assert [x[1] for x in rep[1:]] == [("adjusted" if kw["c"] and adjust[t] else "standardised") for t in range(4)]
        assert [int(x[2]) for x in rep[1:]] == list(ref["n"])
        # the ordinal traits keep their levels: as many distinct values, in the same order
        for t in (2, 3):
            ok = ~np.isnan(data[t])
            assert len(np.unique(data[t, ok])) == len(np.unique(Ya[t, ok])) and np.array_equal(np.argsort(data[t, ok], kind="stable"),
                                                                                              np.argsort(Ya[t, ok], kind="stable"))
        r = _cli("check-phen", stem, path)
        assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("check-phen", stem, table)
    assert r.returncode == 1 and "rows:" in r.stdout
    for nm in ("t0", "t1", "o0"):
        assert f"trait {nm}:" in r.stdout, r.stdout
    # argument errors before the device is asked for
    assert _cli("prep-phen", stem, table, table).returncode != 0
    assert _cli("prep-phen", stem, table, covar, "--covar", covar).returncode != 0

    # sumstats on both files: the pair of traits that shares only `age`
    cli.main(["prep-bed", stem])
    th_atanh = {}
    for label, path, ref in (("adj", out_adj, ref_adj), ("std", out_std, ref_std)):
        outdir = tmp_path / f"ss_{label}"
        outdir.mkdir()
        cli.main(["sumstats", stem, path, str(outdir)])
        _names, pxp, _ = oracle.load_pxp(str(outdir / "pxp.txt"), sample_size=float(N))
        want = np.corrcoef(ref["out"][0, seen].astype(np.float64), ref["out"][1, seen].astype(np.float64))[0, 1]
        print(f"sumstats on {label}: pxp[t0, t1] = {pxp[0, 1]:.6f}, float64 correlation of the restated residuals {want:.6f}")
        assert abs(float(pxp[0, 1]) - want) <= 1e-5  # the tolerance of tests/test_gpu_sumstats.py for pxp
        th_atanh[label] = abs(np.arctanh(float(pxp[0, 1])))
    assert th_atanh["std"] >= th0 > th_atanh["adj"]  # level 0 of cuskss keeps the edge on the unadjusted file, removes it on the adjusted

    # sumstats --ordinal takes the prepared file: the polychoric correlation of the two graded traits is the one of their
    # raw levels (it depends on the table of levels alone)
    raw_levels = str(tmp_path / "levels.phen")
    _n, data, _i = cg.phen_table_load(out_adj, stem + ".fam")
    data[2:] = Ya[2:]
    cg.phen_write(raw_levels, stem + ".fam", names, data)
    poly = []
    for label, path in (("prepared", out_adj), ("levels", raw_levels)):
        outdir = tmp_path / f"ord_{label}"
        outdir.mkdir()
        cli.main(["sumstats", stem, path, str(outdir), "--ordinal", "o0,o1"])
        _names, pxp, _ = oracle.load_pxp(str(outdir / "pxp.txt"), sample_size=float(N))
        poly.append(pxp)
    assert np.array_equal(_bits(poly[0][2:, 2:]), _bits(poly[1][2:, 2:])) and abs(poly[0][2, 3]) > 0.2
