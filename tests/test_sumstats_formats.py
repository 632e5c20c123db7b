"""CPU: the summary-statistic route from genotypes -- the CLI marshals `sumstats` and `cuskss-merged --bfiles` into the
positional argv of `mps sumstats` / `mps cuskss-bed`, and the host-only writer (cusk_sumstats_write) produces files that
the loaders of `cuskss` (oracle.load_mxm / load_mxp / load_pxp, restating the reference's) read back bit for bit."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")


def test_sumstats_argv():
    from cigwas_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["sumstats", "stem", "y.phen", "out", "--marker-indices", "merged_blocks.ixs"])
    assert a.func is cli.sumstats
    assert cli.sumstats_argv(a) == [cli.MPS_PATH, "sumstats", "y.phen", "stem", "merged_blocks.ixs", "out"]
    a = p.parse_args(["sumstats", "stem", "y.phen", "out"])
    assert cli.sumstats_argv(a) == [cli.MPS_PATH, "sumstats", "y.phen", "stem", "NULL", "out"]


def test_cuskss_merged_bfiles_argv(tmp_path):
    from cigwas_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["cuskss-merged", "--bfiles", "stem", "--phen", "y.phen", "--marker-indices", "ix.bin", "--alpha", "0.0001",
                      "--max-level-one", "3", "--max-level-two", "2", "--time-index", "t.txt", "--outdir", "o"])
    assert a.func is cli.cuskss
    assert cli.cuskss_argv(a) == [cli.MPS_PATH, "cuskss-bed", "y.phen", "stem", "ix.bin", "t.txt", "0.0001", "3", "2", "1", "o"]
    # --num-samples is optional on this route and, if given, must be the .dim's
    stem = str(tmp_path / "geno")
    with open(stem + ".dim", "w") as f:
        f.write("4321\t17\n")
    base = ["cuskss-merged", "--bfiles", stem, "--phen", "y.phen", "--marker-indices", "ix.bin", "--alpha", "0.0001"]
    a = p.parse_args(base + ["--num-samples", "4321"])
    assert cli.cuskss_argv(a) == [cli.MPS_PATH, "cuskss-bed", "y.phen", stem, "ix.bin", "NULL", "0.0001", "3", "14", "1", "./"]
    with pytest.raises(SystemExit) as ei:
        cli.cuskss_argv(p.parse_args(base + ["--num-samples", "4320"]))
    assert "4320" in str(ei.value.code) and "4321" in str(ei.value.code)


@pytest.mark.parametrize("extra, needle", [
    (["--bfiles", "stem", "--phen", "y.phen", "--pxp", "pxp.txt"], "not both"),
    (["--bfiles", "stem", "--phen", "y.phen", "--mxm", "m.bin", "--mxp", "mxp.txt"], "not both"),
    (["--bfiles", "stem"], "--phen"),
    (["--phen", "y.phen"], "--bfiles"),
    (["--bfiles", "stem", "--phen", "y.phen", "--mxp-se", "a", "--pxp-se", "b"], "--mxp-se"),
    (["--bfiles", "stem", "--phen", "y.phen", "--num-samples", "10"], ".dim"),  # no such .dim file
    ([], "--pxp"),  # neither route
    (["--pxp", "pxp.txt"], "--num-samples"),  # the file route still needs the sample size
])
def test_cuskss_merged_bfiles_errors_exit_with_a_message(extra, needle):
    from cigwas_amd import cli

    a = cli.build_parser().parse_args(["cuskss-merged", "--marker-indices", "ix.bin", "--alpha", "0.0001"] + extra)
    with pytest.raises(SystemExit) as ei:
        cli.cuskss_argv(a)
    assert isinstance(ei.value.code, str) and needle in ei.value.code


def test_cuskss_merged_needs_marker_indices_on_the_bfiles_route():
    from cigwas_amd import cli

    a = cli.build_parser().parse_args(["cuskss-merged", "--bfiles", "stem", "--phen", "y.phen", "--alpha", "0.0001"])
    with pytest.raises(SystemExit) as ei:
        cli.cuskss_argv(a)
    assert "--marker-indices" in ei.value.code


def test_bfiles_is_an_option_of_cuskss_merged_only():
    from cigwas_amd import cli

    for name in ("cuskss", "cuskss-het"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([name, "--bfiles", "stem", "--phen", "y.phen", "--marker-indices", "ix.bin",
                                           "--alpha", "0.0001", "--pxp", "p", "--num-samples", "5"])
        with pytest.raises(SystemExit):  # --pxp stays required there
            cli.build_parser().parse_args([name, "--marker-indices", "ix.bin", "--alpha", "0.0001", "--num-samples", "5"])


def test_cuskss_merged_file_route_argv_is_unchanged():
    from cigwas_amd import cli

    a = cli.build_parser().parse_args(["cuskss-merged", "--mxm", "m.bin", "--mxp", "mxp.txt", "--pxp", "pxp.txt", "--marker-indices",
                                       "ix.bin", "--alpha", "0.0001", "--num-samples", "500000", "--max-level-two", "1", "--outdir",
                                       "o"])
    assert cli.cuskss_argv(a) == [cli.MPS_PATH, "cuskss", "m.bin", "mxp.txt", "NULL", "pxp.txt", "NULL", "NULL", "0", "NULL",
                                  "ix.bin", "0.0001", "3", "1", "1", "500000", "o"]


K, M_TOTAL, P = 37, 101, 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """random arrays with the awkward values in them, written by cusk_sumstats_write"""
    if not os.path.exists(SO):
        pytest.skip("libcusk_hip.so not built (run __graft_entry__.build())")
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(20240611))
    special = np.array([1.0, -1.0, 0.0, -0.0, 1e-8, -3.25e-8, 0.1, 1.0 / 3.0, np.nextafter(np.float32(1), np.float32(0)),
                        1.17549435e-38, 3.4e38], np.float32)
    tri = rng.uniform(-1, 1, K * (K + 1) // 2).astype(np.float32)
    tri[np.cumsum(np.arange(1, K + 1)) - 1] = 1.0  # the diagonal
    tri[5:5 + special.size] = special
    tri[100] = np.nan
    tri[-1] = np.nan  # a NaN on the diagonal as well
    mxp = rng.uniform(-1, 1, (M_TOTAL, P)).astype(np.float32)
    mxp[:special.size, 1] = special
    mxp[50, 2] = np.nan
    mxp[100, 0] = np.nan
    pxp = rng.uniform(-1, 1, (P, P)).astype(np.float32)
    pxp = np.triu(pxp, 1) + np.triu(pxp, 1).T + np.eye(P, dtype=np.float32)
    pxp[0, 1] = pxp[1, 0] = 1e-8
    pxp[0, 2] = pxp[2, 0] = np.nan
    chr_ids = ["1"] * 60 + ["X"] * (M_TOTAL - 60)
    snps = [f"rs{7 * i}" for i in range(M_TOTAL)]
    refs = ["ACGT"[i % 4] for i in range(M_TOTAL)]
    names = ["bmi", "T1", "height_cm"]
    d = tmp_path_factory.mktemp("sumstats_formats")
    cg.sumstats_write(str(d), tri, mxp, pxp, chr_ids, snps, refs, names)
    return dict(dir=d, tri=tri, mxp=mxp, pxp=pxp, chr=chr_ids, snp=snps, ref=refs, names=names)


def test_mxm_file_reads_back_bit_for_bit(written, oracle):
    path = str(written["dir"] / "mxm.bin")
    assert os.path.getsize(path) == 4 * K * (K + 1) // 2
    raw = np.fromfile(path, np.float32)
    assert not np.isnan(raw).any()  # NaN -> 0 at the source
    want = np.where(np.isnan(written["tri"]), np.float32(0), written["tri"])
    assert np.array_equal(_bits(raw), _bits(want))
    full = oracle.load_mxm(path)
    assert full.shape == (K, K)
    il = np.tril_indices(K)
    assert np.array_equal(_bits(full[il]), _bits(want)) and np.array_equal(_bits(full.T[il]), _bits(want))


def test_mxp_file_reads_back_bit_for_bit(written, oracle):
    path = str(written["dir"] / "mxp.txt")
    want = np.where(np.isnan(written["mxp"]), np.float32(0), written["mxp"])
    got, _ = oracle.load_mxp(path, list(range(M_TOTAL)))
    assert np.array_equal(_bits(np.asarray(got, np.float32).reshape(M_TOTAL, P)), _bits(want))
    rows = [0, 3, 50, 77, 100]
    got, _ = oracle.load_mxp(path, rows)
    assert np.array_equal(_bits(np.asarray(got, np.float32).reshape(len(rows), P)), _bits(want[rows]))
    lines = open(path).read().split("\n")
    assert lines[0].split() == ["chr", "snp", "ref"] + written["names"] and lines[-1] == "" and len(lines) == M_TOTAL + 2
    for i, ln in enumerate(lines[1:-1]):
        assert ln.split()[:3] == [written["chr"][i], written["snp"][i], written["ref"][i]]
    assert lines[51].split()[5] == "NA" and lines[101].split()[3] == "NA"  # the token the mxp loaders map to 0


def test_pxp_file_reads_back_bit_for_bit(written, oracle):
    path = str(written["dir"] / "pxp.txt")
    want = np.where(np.isnan(written["pxp"]), np.float32(0), written["pxp"])
    names, got, _ = oracle.load_pxp(path, sample_size=1000.0)
    assert list(names) == written["names"]
    assert np.array_equal(_bits(got), _bits(want))
    lines = open(path).read().split("\n")
    assert [ln.split()[0] for ln in lines[1:P + 1]] == written["names"]
    assert lines[1].split()[3] == "nan"  # NA would not parse as a number in a pxp file


def test_writer_reports_a_directory_it_cannot_write(tmp_path):
    if not os.path.exists(SO):
        pytest.skip("libcusk_hip.so not built (run __graft_entry__.build())")
    import cigwas_amd as cg

    with pytest.raises(RuntimeError, match="cannot write"):
        cg.sumstats_write(str(tmp_path / "missing_dir"), np.ones(1, np.float32), np.zeros((2, 1), np.float32),
                          np.ones((1, 1), np.float32), ["1", "1"], ["a", "b"], ["A", "C"], ["t"])
