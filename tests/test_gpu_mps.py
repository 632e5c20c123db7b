"""GPU: the `mps`-compatible host program end to end (argv in, result files out)."""
import os
import subprocess

import numpy as np
import pytest

from test_blocking_cases import BANDED_EDGE_CASES, SMALL_CHROMOSOMES, SMALL_MAXB, SMALL_N, SMALL_WIDTH, is_cover

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPS = os.path.join(ROOT, "ci-gwas_amd", "csrc", "mps")


def _run(argv, env=None):
    r = subprocess.run([MPS] + argv, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("case", ["cuskss_trait_only", "cuskss_two_stage_merged", "cuskss_two_stage_block"])
def test_cuskss_reference_fixtures(kat, golden_dir, tmp_path, case):
    """the three end-to-end cases of the reference's tests/cuskss_tests.cpp"""
    k = kat[case]
    g = lambda f: os.path.join(golden_dir, f)
    # through argv "trait only" means mxm == NULL, which the reference's mps.cpp:60-63 only accepts together with a
    # block file (a merged run insists on mxm/mxp); the reference's test builds CuskssArgs by hand instead
    merged = k["merged"] and not k["trait_only"]
    argv = ["cuskss",
            "NULL" if k["trait_only"] else g(k["mxm"]), "NULL" if k["trait_only"] else g(k["mxp"]), "NULL",
            g(k["pxp"]), "NULL", "NULL", str(k.get("block_index", 0)),
            g(k.get("blocks", "blocks.txt")) if not merged else "NULL", g(k["marker_ixs"]) if merged else "NULL",
            str(k["alpha"]), str(k["max_level_one"]), str(k["max_level_two"]), str(k["depth"]), str(k["num_samples"]),
            str(tmp_path)]
    _run(argv)
    base = str(tmp_path / k["stem"])
    assert list(np.fromfile(base + ".adj", np.int32)) == k["exp_adj"]
    assert np.allclose(np.fromfile(base + ".corr", np.float32), k["exp_corr"], atol=k["tol"], rtol=0)
    if "exp_ixs" in k:
        assert list(np.fromfile(base + ".ixs", np.int32)) == k["exp_ixs"]
    nv, nph, ml = [int(v) for v in open(base + ".mdim").read().split()]
    assert nph == 3 and ml == 14 and nv * nv == len(k["exp_adj"])
    assert not os.path.exists(base + ".sep")


def _write_cuskss_inputs(tmp_path, oracle, synth, m, p, het, seed):
    rng = np.random.default_rng(seed)
    Cm = synth.synth_corr_block(m, p, N=4096, block_index=seed)
    names = [f"T{k}" for k in range(p)]
    # mxm: lower triangle incl. diagonal
    il = np.tril_indices(m)
    Cm[:m, :m][il].astype(np.float32).tofile(tmp_path / "mxm.bin")
    se_mp = rng.uniform(0.012, 0.02, (m, p))
    se_pp = rng.uniform(0.012, 0.02, (p, p))
    with open(tmp_path / "mxp.txt", "w") as f, open(tmp_path / "mxp_se.txt", "w") as g:
        f.write("chr snp ref " + " ".join(names) + "\n")
        g.write("chr snp ref " + " ".join(names) + "\n")
        for i in range(m):
            vals = [repr(float(Cm[i, m + k])) for k in range(p)]
            if i == 7:
                vals[1] = "NA"
            f.write(f"1 rs{i} A " + " ".join(vals) + "\n")
            g.write(f"1 rs{i} A " + " ".join(repr(float(se_mp[i, k])) for k in range(p)) + "\n")
    with open(tmp_path / "pxp.txt", "w") as f, open(tmp_path / "pxp_se.txt", "w") as g:
        f.write(" ".join(names) + "\n")
        g.write(" ".join(names) + "\n")
        for a in range(p):
            f.write(names[a] + " " + " ".join(repr(float(Cm[m + a, m + b])) for b in range(p)) + "\n")
            g.write(names[a] + " " + " ".join(repr(float(se_pp[a, b])) for b in range(p)) + "\n")
    with open(tmp_path / "blocks.txt", "w") as f:
        f.write(f"1\t0\t{m - 1}\n")
    with open(tmp_path / "time_index.txt", "w") as f:
        for k in range(p):
            f.write(f"{1 + k % 3}\n")


@pytest.mark.parametrize("het", [False, True])
def test_cuskss_files_match_oracle_pipeline(oracle, synth, tmp_path, het):
    m, p = 250, 6
    _write_cuskss_inputs(tmp_path, oracle, synth, m, p, het, seed=91)
    t = lambda f: str(tmp_path / f)
    out = tmp_path / "out"
    out.mkdir()
    _run(["cuskss", t("mxm.bin"), t("mxp.txt"), t("mxp_se.txt") if het else "NULL", t("pxp.txt"),
          t("pxp_se.txt") if het else "NULL", t("time_index.txt"), "0", t("blocks.txt"), "NULL", "0.0001", "3", "2", "1",
          "4096", str(out)])
    # oracle pipeline on the same files
    mxm = oracle.load_mxm(t("mxm.bin"))
    _, pxp, ess_p = oracle.load_pxp(t("pxp.txt"), sample_size=4096.0, se_path=t("pxp_se.txt") if het else None)
    mxp, ess_mp = oracle.load_mxp(t("mxp.txt"), range(m), se_path=t("mxp_se.txt") if het else None)
    sq, es = oracle.make_square_cuskss_inputs(mxm, mxp, pxp, 4096.0, ess_mp if het else None, ess_p if het else None)
    ti = np.loadtxt(t("time_index.txt"), dtype=np.int32)
    ref = oracle.cuskss_from_square(sq, es, p, 1e-4, 3, 2, 1, ti)
    oracle.write_reduced(ref, t("ref"), with_sep=False)
    for ext in (".mdim", ".ixs", ".adj", ".corr"):
        assert open(str(out / f"1_0_{m - 1}") + ext, "rb").read() == open(t("ref") + ext, "rb").read(), ext


def test_cusk_block_files_match_oracle_pipeline(oracle, synth, tmp_path):
    m, N, p = 300, 2000, 4
    bed, phen, means, stds, G = synth.synth_bed_block(m, N, p, block_index=17, miss=0.003)
    phen = phen.copy()
    phen[5] = np.nan
    stem = str(tmp_path / "geno")
    chr_ids = ["1"] * 100 + ["2"] * 200  # the block sits on the second chromosome
    synth.write_bfiles(stem, bed, N, means, stds, chr_ids)
    synth.write_phen(str(tmp_path / "y.phen"), phen, N, p)
    with open(tmp_path / "b.blocks", "w") as f:
        f.write("1\t0\t99\n2\t10\t159\n")
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, CUSK_WRITE_FULL_CORRMATS="1")
    _run(["cusk", str(tmp_path / "y.phen"), stem, str(tmp_path / "b.blocks"), "0.001", "3", "14", "1", str(out), "1"], env)
    base = str(out / "2_10_159")
    mb = 150
    n = mb + p
    sq = np.fromfile(base + ".all_corrs", np.float32).reshape(n, n)
    # the matrix the sweep ran on vs the oracle's correlation build on the same block
    sel = slice(110, 260)
    phen_rt = oracle.load_phen(str(tmp_path / "y.phen"))[2]
    o_mxm, o_mxp, o_pxp = oracle.corr_pearson_npn(bed[sel], phen_rt, mb, N, p, means[sel], stds[sel])
    want = oracle.square_from_cusk_corrs(o_mxm, o_mxp, o_pxp, mb, p)
    assert np.array_equal(sq[:mb, :mb], want[:mb, :mb])
    assert np.allclose(sq, want, atol=1e-5, rtol=0)
    # result files vs the oracle's two-stage pipeline on that very matrix
    Th = oracle.threshold_array(N, 0.001)
    ref = oracle.cusk_from_corr(sq, p, Th, 3, 14, 1)
    oracle.write_reduced(ref, str(tmp_path / "ref"), with_sep=True)
    for ext in (".mdim", ".ixs", ".adj", ".corr", ".sep"):
        assert open(base + ext, "rb").read() == open(str(tmp_path / "ref") + ext, "rb").read(), ext


def test_cusk_skips_block_without_signal(synth, tmp_path):
    m, N, p = 64, 500, 2
    bed, phen, means, stds, G = synth.synth_bed_block(m, N, p, block_index=3)
    rng = np.random.default_rng(0)
    phen = rng.standard_normal(p * N).astype(np.float32)  # traits unrelated to the markers
    stem = str(tmp_path / "g")
    synth.write_bfiles(stem, bed, N, means, stds)
    synth.write_phen(str(tmp_path / "y.phen"), phen, N, p)
    with open(tmp_path / "b.blocks", "w") as f:
        f.write("1\t0\t63\n")
    out = tmp_path / "out"
    out.mkdir()
    txt = _run(["cusk", str(tmp_path / "y.phen"), stem, str(tmp_path / "b.blocks"), "1e-12", "2", "2", "1", str(out), "0"])
    assert "Skipping block" in txt and not list(out.iterdir())


def test_error_paths(tmp_path):
    r = subprocess.run([MPS, "cusk", "nope.phen", "nope", "nope.blocks", "0.1", "1", "1", "1", str(tmp_path), "0"],
                       capture_output=True, text=True)
    assert r.returncode == 1
    r = subprocess.run([MPS, "prep", "x"], capture_output=True, text=True)
    assert r.returncode != 0


@pytest.mark.parametrize("m,N,width", [(700, 600, 150), (333, 1001, 64), (130, 256, 129)] + BANDED_EDGE_CASES)
def test_banded_correlations_match_oracle(oracle, synth, m, N, width):
    """cusk_corr_banded (the FP4 contingency kernel restricted to a band) against the oracle: band and forward row
    sums bit-exact; widths that do and do not divide the tile, N with and without partial K blocks; and the shapes
    at which the number of band tiles per row tile and the clamps at the last marker change (BANDED_EDGE_CASES: width 1,
    one marker, less than / exactly / just over one and two tiles, widths around 64 and 128, bands wider than the
    chromosome), where the entries past the last marker are exactly 0"""
    import cigwas_amd as cg

    bed, _phen, _means, _stds, _G = synth.synth_bed_block(m, N, 1, block_index=23, miss=0.01)
    e = cg.Engine(0)
    sums, band = e.corr_banded(bed, m, N, width, want_band=True)
    e.close()
    want = oracle.marker_corr_banded(bed, m, N, width)
    assert np.array_equal(band, want, equal_nan=True)
    assert np.array_equal(sums, oracle.banded_row_abs_sums(want))
    if width >= m - 1:
        past = np.arange(m)[:, None] + 1 + np.arange(width)[None, :] >= m
        assert past.any() and np.array_equal(band[past].view(np.int32), np.zeros(int(past.sum()), np.int32))


def test_mps_block_file_matches_oracle_pipeline(oracle, synth, tmp_path):
    """`mps block` end to end on two chromosomes: the .blocks file equals the oracle's pipeline (banded npn
    correlations -> row sums -> Hanning smoothing -> minima -> bisection), and a second run appends (io.cpp:266-277)"""
    m1, m2, N = 1500, 900, 400
    bed, _phen, means, stds, _G = synth.synth_bed_block(m1 + m2, N, 1, block_index=31)
    chr_ids = ["3"] * m1 + ["7"] * m2
    stem = str(tmp_path / "g")
    synth.write_bfiles(stem, bed, N, means, stds, chr_ids)
    txt = _run(["block", stem, "300", "1", "200"])
    assert "[Chr 3]: Partitioned into" in txt and "[Chr 7]: Partitioned into" in txt
    want = oracle.make_blocks(bed, chr_ids, N, 300, 200)
    path = stem + "_m300.blocks"
    got = open(path).read().splitlines()
    assert got == want and len(want) > 4
    # every chromosome is covered exactly once, in order
    for cid, mm in (("3", m1), ("7", m2)):
        rows = [tuple(map(int, l.split("\t")[1:])) for l in got if l.split("\t")[0] == cid]
        assert rows[0][0] == 0 and rows[-1][1] == mm - 1 and all(rows[i + 1][0] == rows[i][1] + 1 for i in range(len(rows) - 1))
    _run(["block", stem, "300", "1", "200"])
    assert open(path).read().splitlines() == want + want
    # the block file drives `mps cusk` unchanged
    assert oracle.read_blocks(path)[: len(want)] is not None


def test_mps_block_file_at_small_chromosomes(oracle, synth, tmp_path):
    """`mps block` on chromosomes of 3, 64, 65 and 400 markers whose ids are not in sorted order, band width 2, and an N
    that is no multiple of 64 (rows that are not 16-byte multiples: the banded kernel without the prefetch): the .blocks
    file equals the oracle's, chromosome after chromosome in .bim order (inputs checked in test_blocking_cases.py)"""
    sizes = [m for _, m in SMALL_CHROMOSOMES]
    bed, _phen, means, stds, _G = synth.synth_bed_block(sum(sizes), SMALL_N, 1, block_index=37)
    chr_ids = [c for c, m in SMALL_CHROMOSOMES for _ in range(m)]
    stem = str(tmp_path / "g")
    synth.write_bfiles(stem, bed, SMALL_N, means, stds, chr_ids)
    txt = _run(["block", stem, str(SMALL_MAXB), "1", str(SMALL_WIDTH)])
    for c, m in SMALL_CHROMOSOMES:
        assert f"[Chr {c}]: Loading bed data for {m} markers." in txt
    want = oracle.make_blocks(bed, chr_ids, SMALL_N, SMALL_MAXB, SMALL_WIDTH)
    got = open(f"{stem}_m{SMALL_MAXB}.blocks").read().splitlines()
    assert got == want and len(want) > len(sizes)
    for c, m in SMALL_CHROMOSOMES:
        assert is_cover([tuple(map(int, l.split("\t")[1:])) for l in got if l.split("\t")[0] == c], m)


def test_mps_block_refuses_band_wider_than_the_chromosome(synth, tmp_path):
    bed, _phen, means, stds, _G = synth.synth_bed_block(100, 200, 1, block_index=2)
    stem = str(tmp_path / "g")
    synth.write_bfiles(stem, bed, 200, means, stds)
    r = subprocess.run([MPS, "block", stem, "50", "1", "500"], capture_output=True, text=True)
    assert r.returncode == 1 and "corr width" in r.stdout

