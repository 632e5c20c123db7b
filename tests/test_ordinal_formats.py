"""No GPU: `--ordinal` from the command line to the native argv on both routes and every argument error; the new ABI entries;
the standard-error writer read back through the loaders' float and cusk_ess_from_se; and the float64 oracle of
ordinal_ref64.py against closed forms and on a planted effect at 5 % prevalence."""
import ctypes as C

import numpy as np
import pytest

import ordinal_cases
import ordinal_ref64 as R


# ------------------------------------------------------------------------------------------------ command line
@pytest.fixture()
def phen_file(tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    n = 40
    cols = {"height": rng.standard_normal(n), "disease": (rng.random(n) < 0.3).astype(float), "grade": rng.integers(0, 4, n).astype(float),
            "nine": np.arange(n) % 9.0, "flat": np.ones(n), "bmi": rng.standard_normal(n)}
    lines = ["FID IID " + " ".join(cols)]
    for i in range(n):
        vals = ["NA" if (name == "disease" and i % 7 == 0) else repr(float(v[i])) for name, v in cols.items()]
        lines.append(f"f{i} i{i} " + " ".join(vals))
    path = tmp_path / "y.phen"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _parse(argv):
    from cigwas_amd import cli

    return cli.build_parser().parse_args(argv)


def test_sumstats_ordinal_argv(phen_file):
    from cigwas_amd import cli

    args = _parse(["sumstats", "stem", phen_file, "out", "--ordinal", "disease,3"])
    assert cli.sumstats_argv(args)[1:] == ["sumstats", phen_file, "stem", "NULL", "out", "se", "ordinal=2,3"]
    args = _parse(["sumstats", "stem", phen_file, "out", "--se", "--marker-indices", "ix", "--ordinal", "grade"])
    assert cli.sumstats_argv(args)[1:] == ["sumstats", phen_file, "stem", "ix", "out", "se", "ordinal=3"]
    # without the option: what it was
    assert cli.sumstats_argv(_parse(["sumstats", "stem", phen_file, "out"]))[1:] == ["sumstats", phen_file, "stem", "NULL", "out"]
    assert cli.sumstats_argv(_parse(["sumstats", "stem", phen_file, "out", "--se"]))[-1] == "se"


def _merged(phen_file, extra):
    return _parse(["cuskss-merged", "--marker-indices", "ix", "--alpha", "1e-3", "--bfiles", "stem", "--phen", phen_file] + extra)


def test_cuskss_merged_ordinal_argv(phen_file):
    from cigwas_amd import cli

    argv = cli.cuskss_argv(_merged(phen_file, ["--het", "--ordinal", "2,grade"]))
    assert argv[1] == "cuskss-bed" and argv[-2:] == ["het", "ordinal=2,3"]
    argv = cli.cuskss_argv(_merged(phen_file, ["--het", "--het-markers", "--ordinal", "disease"]))
    assert argv[-3:] == ["het", "markers", "ordinal=2"]
    assert cli.cuskss_argv(_merged(phen_file, ["--het"]))[-1] == "het"


@pytest.mark.parametrize("names, message", [
    ("nosuch", "unknown trait 'nosuch'"),
    ("0", "out of range"),
    ("7", "out of range"),
    ("nine", "nine has 9 distinct values"),
    ("flat", "flat has 1 distinct values"),
    ("disease,4", "nine has 9 distinct values"),
])
def test_ordinal_argument_errors(phen_file, names, message):
    from cigwas_amd import cli

    with pytest.raises(SystemExit) as ex:
        cli.sumstats_argv(_parse(["sumstats", "stem", phen_file, "out", "--ordinal", names]))
    assert message in str(ex.value)
    with pytest.raises(SystemExit) as ex:
        cli.cuskss_argv(_merged(phen_file, ["--het", "--ordinal", names]))
    assert message in str(ex.value)


def test_ordinal_needs_het_and_genotypes(phen_file):
    from cigwas_amd import cli

    with pytest.raises(SystemExit) as ex:
        cli.cuskss_argv(_merged(phen_file, ["--ordinal", "disease"]))
    assert "--het" in str(ex.value)
    with pytest.raises(SystemExit) as ex:
        cli.cuskss_argv(_parse(["cuskss-merged", "--marker-indices", "ix", "--alpha", "1e-3", "--pxp", "pxp.txt", "--num-samples", "10",
                                "--ordinal", "disease"]))
    assert "--ordinal needs --bfiles" in str(ex.value)


# ------------------------------------------------------------------------------------------------ ABI and writer
def test_abi_symbols():
    from cigwas_amd._lib import SYMBOLS, lib

    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    want = {
        "cusk_ordinal_tables": (i, [vp, vp, vp, vp, sz, sz, sz, sz, vp, sz, vp, vp, vp, vp]),
        "cusk_polychoric_fit": (i, [vp, vp, sz, i, i, vp, vp, vp]),
        "cusk_polyserial_fit": (i, [vp, vp, sz, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp]),
        "cusk_sumstats_write_se_values": (i, [C.c_char_p, vp, sz, sz, vp, vp, vp, vp, vp, C.c_char_p, sz]),
        "cusk_matrix_set_cross": (i, [vp, vp, sz, sz, vp]),
    }
    L = lib()
    for name, (res, args) in want.items():
        assert SYMBOLS[name] == (res, args)
        assert getattr(L, name).argtypes == args
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "cusk_hip.h")).read()
    for name in want:
        assert f"int {name}(" in header


def test_se_values_round_trip(tmp_path):
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(11))
    m, p = 17, 3
    r = rng.uniform(-0.95, 0.95, (m, p)).astype(np.float32)
    se = (rng.uniform(0.001, 0.2, (m, p))).astype(np.float32)
    se[2, 1] = np.nan  # a boundary estimate: r without se
    r[5, 0] = se[5, 0] = np.nan  # a degenerate one
    pr = np.eye(p, dtype=np.float32)
    pse = np.full((p, p), np.nan, np.float32)
    pr[0, 1] = pr[1, 0] = 0.4321
    pse[0, 1] = pse[1, 0] = 0.0123
    pr[0, 2] = pr[2, 0] = -0.9999
    names, ids = ["a", "b", "c"], [str(v) for v in range(m)]
    cg.sumstats_write(str(tmp_path), np.ones(1, np.float32), r, pr, ids, ids, ids, names)
    cg.sumstats_write_se_values(str(tmp_path), se, pse, ids, ids, ids, names)
    rows_r = [ln.split()[3:] for ln in open(tmp_path / "mxp.txt").read().splitlines()[1:]]
    rows_s = [ln.split()[3:] for ln in open(tmp_path / "mxp_se.txt").read().splitlines()[1:]]
    assert rows_s[2][1] == "NA" and rows_r[2][1] != "NA" and rows_r[5][0] == "NA" and rows_s[5][0] == "NA"
    for i in range(m):
        for t in range(p):
            if np.isnan(se[i, t]):
                continue
            rf, sf = np.float32(rows_r[i][t]), np.float32(rows_s[i][t])  # text -> the loaders' float
            assert rf == r[i, t] and sf == se[i, t]
            assert cg.ess_from_se(float(rf), float(sf)) == cg.ess_from_se(float(r[i, t]), float(se[i, t]))
    prow = open(tmp_path / "pxp_se.txt").read().splitlines()
    assert prow[0] == "a b c" and prow[1].split()[1] == "nan" and np.float32(prow[1].split()[2]) == np.float32(0.0123)
    assert np.isnan(cg.ess_from_se(-0.9999, float("nan")))


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("p11", [0.25, 0.3, 0.45, 0.1])
def test_oracle_two_by_two_with_even_margins(p11):
    n = 100000
    a = int(round(p11 * n))
    t = np.array([[a, n // 2 - a], [n // 2 - a, a]])
    rho, se, status = R.polychoric(t)
    assert status == R.OK and abs(rho - np.sin(np.pi / 2 * (4 * a / n - 1))) < 1e-10 and se > 0


def test_oracle_symmetries():
    assert abs(R.polychoric(np.outer([20, 30, 50], [10, 40]))[0]) < 1e-10  # independence
    t = np.array([[30, 12, 5], [14, 22, 9], [4, 11, 28]])
    rho, se, status = R.polychoric(t)
    assert status == R.OK and 0.3 < rho < 0.9
    rt, st_, _ = R.polychoric(t.T)
    assert abs(rt - rho) < 1e-10 and abs(st_ / se - 1) < 1e-8
    rr, sr, _ = R.polychoric(t[::-1])
    assert abs(rr + rho) < 1e-10 and abs(sr / se - 1) < 1e-8
    assert R.polychoric([[5, 0], [0, 5]])[2] == R.BOUNDARY and R.polychoric([[5, 5], [0, 0]])[2] == R.DEGENERATE


def test_planted_effect_at_five_percent_prevalence():
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(2024))
    n, rho0 = 20000, 0.5
    x = rng.standard_normal(n)
    liab = rho0 * x + np.sqrt(1 - rho0 ** 2) * rng.standard_normal(n)
    case = (liab > np.quantile(liab, 0.95)).astype(np.int64)
    grade = np.searchsorted([-0.5, 0.8], x)  # the partner as a three-class variable, as a marker is
    rho, se, status = R.polychoric(R.pair_table(grade, case, 3, 2))
    assert status == R.OK and abs(rho - rho0) < 4 * se
    pearson = np.corrcoef(grade, case)[0, 1]
    assert pearson < 0.35
    assert cg.ess_from_se(float(np.float32(rho)), float(np.float32(se))) < n / 2
    # and polyserial on the continuous partner itself
    rho_s, se_s, status = R.polyserial(x, case)
    assert status == R.OK and abs(rho_s - rho0) < 4 * se_s and np.corrcoef(x, case)[0, 1] < 0.35


def test_fit_cases_stay_within_the_oracles_share():
    """the random tables test_gpu_ordinal.py compares the fit kernel on: the oracle alone calls at most 2 % of them
    boundary or degenerate, so the seed and the ranges of the generator leave the comparison its cases"""
    cases = ordinal_cases.fit_cases()
    assert 280 <= len(cases) <= 320
    random_tables = [t for _, t, is_random in cases if is_random]
    left_out = sum(R.polychoric(t)[2] != R.OK for t in random_tables)
    assert left_out <= 0.02 * len(random_tables), (left_out, len(random_tables))
    assert {t.sum() for t in random_tables} == {50, 1000, 500000}
    assert {s for s, _, _ in cases} == {(3, 2), (3, 3), (3, 8), (8, 8), (2, 2)}
    special = [R.polychoric(t)[2] for _, t, is_random in cases if not is_random]
    assert special.count(R.BOUNDARY) >= 5 and special.count(R.DEGENERATE) >= 3


def test_planted_alpha_is_chosen_with_the_oracle(oracle):
    """the CPU oracle's cuskss pipeline on the planted set: at PLANTED_ALPHA, and a decade to either side, the
    marker-disease edge is removed on Pearson values at N and kept on the oracle's polychoric / polyserial values"""
    G, phen = ordinal_cases.planted_set()
    k, p = ordinal_cases.PLANTED_K, ordinal_cases.PLANTED_TRAITS
    C, E, Co, Eo = ordinal_cases.planted_squares(G, phen)
    a, b = ordinal_cases.PLANTED_MARKER, k + ordinal_cases.PLANTED_DISEASE
    assert C[a, b] < 0.35 and abs(float(Co[a, b]) - 0.5) < 0.1 and Eo[a, b] < ordinal_cases.PLANTED_N / 2
    for alpha in (ordinal_cases.PLANTED_ALPHA * 10, ordinal_cases.PLANTED_ALPHA, ordinal_cases.PLANTED_ALPHA / 10):
        plain = oracle.cuskss_from_square(C, E, p, alpha, ordinal_cases.PLANTED_L1, ordinal_cases.PLANTED_L2, 1)
        latent = oracle.cuskss_from_square(Co, Eo, p, alpha, ordinal_cases.PLANTED_L1, ordinal_cases.PLANTED_L2, 1)
        assert not ordinal_cases.has_edge(plain.num_var, plain.new_to_old, plain.G, a, b), alpha
        assert ordinal_cases.has_edge(latent.num_var, latent.new_to_old, latent.G, a, b), alpha
