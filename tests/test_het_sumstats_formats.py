"""CPU: per-pair sample sizes on the summary-statistic route -- the standard error written for a pair observed on `count`
individuals (cusk_se_from_count) must give back exactly `count` through the loaders' ess = ((1 - r^2) / se)^2
(cusk_ess_from_se) and the sweep's truncation to int; the two se files (cusk_sumstats_write_se) are read back with the
oracle's restatement of the reference's loaders; the CLI marshals `sumstats --se` and `cuskss-merged --bfiles --het` into
a trailing word of the `mps` argv and leaves both lists alone without the flags."""
import numpy as np
import pytest

M_TOTAL, P = 83, 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _word(x):
    return int(np.float32(x).view(np.uint32))


def _ess_numpy(r, se):
    """host_io.h:307-311: float product, double quotient, rounded to float, squared in float"""
    r, se = np.float32(r), np.float32(se)
    with np.errstate(all="ignore"):
        ss = np.float32((np.float64(1.0) - np.float64(r * r)) / np.float64(se))
        return np.float32(ss * ss)


@pytest.mark.parametrize("lo, hi", [(4, 100), (100, 10_000), (10_000, 500_000), (500_000, 2_000_000)])
def test_se_from_count_recovers_the_count(lo, hi):
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(hi))
    r = rng.uniform(-0.95, 0.95, 5000).astype(np.float32)
    count = rng.integers(lo, hi, 5000, endpoint=True)
    r[:4], count[:4] = [0.0, 0.95, -0.95, 0.5], [lo, hi, hi, hi]
    wrong = 0
    for ri, ci in zip(r, count):
        se = cg.se_from_count(ri, int(ci))
        ess = cg.ess_from_se(ri, se)
        assert _word(ess) == _word(_ess_numpy(ri, se))
        plain = np.float32((1.0 - float(ri * ri)) / np.sqrt(float(ci)))
        assert abs(_word(se) - _word(plain)) <= 1  # at most one ulp from the formula
        wrong += int(ess) != ci
    assert wrong == 0


def test_ess_from_se_is_the_loaders_formula_bit_for_bit():
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(3))
    for r, se in zip(rng.uniform(-1, 1, 2000).astype(np.float32), rng.uniform(1e-4, 0.5, 2000).astype(np.float32)):
        assert _word(cg.ess_from_se(r, se)) == _word(_ess_numpy(r, se))
    assert np.isnan(cg.ess_from_se(1.0, 0.0)) and np.isnan(cg.ess_from_se(0.3, np.nan))
    assert cg.ess_from_se(1.0, 0.25) == 0.0


def test_se_from_count_refuses_what_has_no_standard_error():
    import cigwas_amd as cg

    for r, count in [(np.nan, 100), (0.3, 0), (0.3, -5), (1.0, 100), (-1.0, 100)]:
        assert np.isnan(cg.se_from_count(r, count)), (r, count)
    assert cg.se_from_count(0.0, 4) == 0.5


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(20250102))
    mxp = rng.uniform(-0.95, 0.95, (M_TOTAL, P)).astype(np.float32)
    mxp_n = rng.integers(4, 2_000_000, (M_TOTAL, P), endpoint=True).astype(np.int32)
    mxp_n[:, 1] = rng.integers(4, 300, M_TOTAL)
    mxp[7, 2], mxp_n[7, 2] = np.nan, 0  # a pair never observed together: no correlation, count zero
    mxp[80, 0] = np.nan                 # a marker without variance: no correlation whatever the count
    pxp = rng.uniform(-0.95, 0.95, (P, P)).astype(np.float32)
    pxp = np.triu(pxp, 1) + np.triu(pxp, 1).T + np.eye(P, dtype=np.float32)
    pxp_n = rng.integers(4, 2_000_000, (P, P), endpoint=True).astype(np.int32)
    pxp_n = np.triu(pxp_n) + np.triu(pxp_n, 1).T
    pxp[0, 3] = pxp[3, 0] = np.nan
    pxp_n[0, 3] = pxp_n[3, 0] = 0
    chr_ids = ["2"] * 40 + ["X"] * (M_TOTAL - 40)
    snps = [f"rs{11 * i}" for i in range(M_TOTAL)]
    refs = ["ACGT"[i % 4] for i in range(M_TOTAL)]
    names = ["bmi", "T1", "height_cm", "ldl"]
    d = tmp_path_factory.mktemp("het_formats")
    tri = np.ones(1, np.float32)
    cg.sumstats_write(str(d), tri, mxp, pxp, chr_ids, snps, refs, names)
    cg.sumstats_write_se(str(d), mxp, mxp_n, pxp, pxp_n, chr_ids, snps, refs, names)
    return dict(dir=d, mxp=mxp, mxp_n=mxp_n, pxp=pxp, pxp_n=pxp_n, names=names)


def test_mxp_se_file_gives_back_the_counts(written, oracle):
    d = written["dir"]
    for rows in (list(range(M_TOTAL)), [0, 7, 33, 80, 82]):
        corr, ess = oracle.load_mxp(str(d / "mxp.txt"), rows, se_path=str(d / "mxp_se.txt"))
        want_r, want_n = written["mxp"][rows], written["mxp_n"][rows]
        nan = np.isnan(want_r)
        assert np.array_equal(_bits(corr), _bits(np.where(nan, np.float32(0), want_r)))
        assert np.array_equal(np.isnan(ess), nan)  # no sample size exactly where there is no correlation
        assert np.array_equal(ess[~nan].astype(np.int64), want_n[~nan])
    a, b = open(d / "mxp.txt").read().split("\n"), open(d / "mxp_se.txt").read().split("\n")
    assert len(a) == len(b) == M_TOTAL + 2 and a[0] == b[0] and b[-1] == ""
    assert [ln.split()[:3] for ln in a[1:-1]] == [ln.split()[:3] for ln in b[1:-1]]
    assert b[8].split()[5] == "NA" and b[81].split()[3] == "NA"


def test_pxp_se_file_gives_back_the_counts(written, oracle):
    d = written["dir"]
    names, corr, ess = oracle.load_pxp(str(d / "pxp.txt"), se_path=str(d / "pxp_se.txt"))
    assert list(names) == written["names"]
    want_r, want_n = written["pxp"], written["pxp_n"]
    off = ~np.eye(P, dtype=bool)
    nan = np.isnan(want_r)
    assert np.array_equal(_bits(corr), _bits(np.where(nan, np.float32(0), want_r)))
    assert np.array_equal(np.isnan(ess)[off], nan[off])
    assert np.array_equal(ess[off & ~nan].astype(np.int64), want_n[off & ~nan])
    assert np.isnan(np.diag(ess)).all()  # the convention of the diagonal: nan in the file, no sample size
    a, b = open(d / "pxp.txt").read().split("\n"), open(d / "pxp_se.txt").read().split("\n")
    assert a[0] == b[0] and [ln.split()[:1] for ln in a[1:P + 1]] == [ln.split()[:1] for ln in b[1:P + 1]]
    assert all(b[1 + i].split()[1 + i] == "nan" for i in range(P)) and b[1].split()[4] == "nan"


def test_se_writer_reports_a_directory_it_cannot_write(tmp_path):
    import cigwas_amd as cg
    from cigwas_amd._lib import lib
    import ctypes as C

    with pytest.raises(RuntimeError, match="cannot write"):
        cg.sumstats_write_se(str(tmp_path / "missing_dir"), np.full((2, 1), 0.5, np.float32), np.full((2, 1), 9, np.int32),
                             np.ones((1, 1), np.float32), np.full((1, 1), 9, np.int32), ["1", "1"], ["a", "b"], ["A", "C"], ["t"])
    err = C.create_string_buffer(64)
    assert lib().cusk_sumstats_write_se(b"x", None, None, 0, 0, None, None, None, None, None, None, err, len(err)) != 0
    assert b"bad arguments" in err.value


def test_sumstats_se_argv():
    from cigwas_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["sumstats", "stem", "y.phen", "out", "--marker-indices", "merged_blocks.ixs", "--se"])
    assert cli.sumstats_argv(a) == [cli.MPS_PATH, "sumstats", "y.phen", "stem", "merged_blocks.ixs", "out", "se"]
    a = p.parse_args(["sumstats", "stem", "y.phen", "out", "--marker-indices", "merged_blocks.ixs"])
    assert a.se is False
    assert cli.sumstats_argv(a) == [cli.MPS_PATH, "sumstats", "y.phen", "stem", "merged_blocks.ixs", "out"]


def test_cuskss_merged_het_argv():
    from cigwas_amd import cli

    p = cli.build_parser()
    base = ["cuskss-merged", "--bfiles", "stem", "--phen", "y.phen", "--marker-indices", "ix.bin", "--alpha", "0.0001",
            "--max-level-one", "3", "--max-level-two", "2", "--time-index", "t.txt", "--outdir", "o"]
    plain = [cli.MPS_PATH, "cuskss-bed", "y.phen", "stem", "ix.bin", "t.txt", "0.0001", "3", "2", "1", "o"]
    a = p.parse_args(base)
    assert a.het is False and cli.cuskss_argv(a) == plain
    assert cli.cuskss_argv(p.parse_args(base + ["--het"])) == plain + ["het"]


def test_het_without_bfiles_exits_with_a_message():
    from cigwas_amd import cli

    a = cli.build_parser().parse_args(["cuskss-merged", "--mxm", "m.bin", "--mxp", "mxp.txt", "--pxp", "pxp.txt", "--marker-indices",
                                       "ix.bin", "--alpha", "0.0001", "--num-samples", "5000", "--het"])
    with pytest.raises(SystemExit) as ei:
        cli.cuskss_argv(a)
    assert isinstance(ei.value.code, str) and "--het" in ei.value.code and "--bfiles" in ei.value.code
    # the standard-error files stay refused beside --bfiles, with or without --het
    a = cli.build_parser().parse_args(["cuskss-merged", "--bfiles", "stem", "--phen", "y.phen", "--marker-indices", "ix.bin",
                                       "--alpha", "0.0001", "--het", "--mxp-se", "a", "--pxp-se", "b"])
    with pytest.raises(SystemExit) as ei:
        cli.cuskss_argv(a)
    assert "--mxp-se" in ei.value.code
    for name in ("cuskss", "cuskss-het"):  # --het belongs to cuskss-merged alone
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([name, "--pxp", "p", "--marker-indices", "ix.bin", "--alpha", "0.0001",
                                           "--num-samples", "5", "--het"])
