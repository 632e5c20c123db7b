"""GPU: per-pair sample sizes from genotypes -- the pair-count kernel (cusk_pair_counts) against a boolean matrix product
in numpy, `sumstats --se` (the two standard-error files) and `cuskss-merged --bfiles --phen --het` (the same sample sizes
without the files), on a .phen with gaps.

Everything here is exact: counts are integers, the se files must give back those integers through the loaders'
ess = ((1 - r^2) / se)^2 and the sweep's truncation, the two routes of `cuskss-merged` are compared byte for byte, and the
result files equal the oracle's hetcor pipeline on the matrices the loaders make of the files `sumstats --se` wrote.
The last test shows that the flag matters: on this data the oracle's skeleton with per-pair sample sizes differs from
its skeleton at the uniform N, `--het` gives the first and the plain `--bfiles` run the second."""
import os
import pathlib
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M, M1, N, P = 1200, 700, 4001, 6  # N is not a multiple of 4: rows end inside a byte and start at any alignment
K_SEL = 150
ALPHA, L1, L2, DEPTH = 1e-4, 3, 3, 1
NAN_RATE = (0.0, 0.1, 0.7, 0.67, 0.75, 0.3)  # three traits observed in a third of the cohort or less
SEED = 9090
FILES = ("cuskss_merged.mdim", "cuskss_merged.ixs", "cuskss_merged.adj", "cuskss_merged.corr", "cuskss_merged_sam.mtx",
         "cuskss_merged_scm.mtx")


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


def _reference_counts(bed, phen, n_ind, p):
    """(markers x traits, traits x traits) counts of complete observations: boolean matrix products"""
    codes = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :n_ind]
    present = (codes != 1).astype(np.int64)
    seen = (~np.isnan(np.asarray(phen, np.float32).reshape(p, n_ind))).astype(np.int64)
    return present @ seen.T, seen @ seen.T


def _case(n_ind, m, p, seed):
    """random .bed rows and phenotypes with every awkward column: NaN rates from 0 to 70 %, an all-NaN trait, an
    all-missing marker, a marker without a missing call, random bits in the padding of each row's last byte"""
    rng = np.random.Generator(np.random.PCG64(seed))
    clb = (n_ind + 3) // 4
    bed = rng.integers(0, 256, (m, clb), dtype=np.uint8)  # all four codes, a quarter of the calls missing, padding random
    if m > 2:
        bed[1] = 0x55  # every call missing
        b = bed[2]
        miss = (b & 0x55) & ~((b >> 1) & 0x55)
        bed[2] = b | (miss << 1)  # 01 -> 11: no missing call
    phen = rng.standard_normal((p, n_ind)).astype(np.float32)
    for t, rate in enumerate(np.linspace(0.0, 0.7, p)):
        phen[t, rng.random(n_ind) < rate] = np.nan
    if p > 2:
        phen[p - 2] = np.nan
    return bed, np.ascontiguousarray(phen).reshape(-1)


@pytest.mark.parametrize("n_ind, m, p", [(1, 5, 3), (3, 7, 4), (4001, 230, 11), (16384, 150, 20), (70001, 37, 9)])
def test_pair_counts_equal_a_boolean_matrix_product(n_ind, m, p):
    import cigwas_amd as cg

    bed, phen = _case(n_ind, m, p, 1000 + n_ind)
    want_mxp, want_pxp = _reference_counts(bed, phen, n_ind, p)
    eng = cg.Engine(0)
    got_mxp, got_pxp = eng.pair_counts(bed, phen, n_ind, p)
    assert got_mxp.dtype == np.int32 and got_mxp.shape == (m, p) and got_pxp.shape == (p, p)
    assert np.array_equal(got_mxp, want_mxp) and np.array_equal(got_pxp, want_pxp)
    assert np.array_equal(got_pxp, got_pxp.T)
    if m > 2:
        assert not got_mxp[1].any() and np.array_equal(got_mxp[2], np.diag(want_pxp))
    # device-resident inputs: the same counts
    bed_d, phen_d = cg.DeviceArray(bed), cg.DeviceArray(phen)
    dev_mxp, dev_pxp = eng.pair_counts(bed_d, phen_d, n_ind, p)
    assert np.array_equal(dev_mxp, want_mxp) and np.array_equal(dev_pxp, want_pxp)
    # the first rows only, and the result does not depend on what follows them
    few_mxp, _ = eng.pair_counts(bed_d, phen_d, n_ind, p, k=max(m // 2, 1))
    assert np.array_equal(few_mxp, want_mxp[:max(m // 2, 1)])
    # a scattered index list, from host and from resident rows, against the same rows made contiguous
    ix = np.sort(np.random.Generator(np.random.PCG64(n_ind)).choice(m, size=max(m // 3, 1), replace=False)).astype(np.int32)
    ix[-1] = m - 1
    ix = np.unique(ix)
    con_mxp, con_pxp = eng.pair_counts(bed[ix], phen, n_ind, p)
    for b, ph in ((bed, phen), (bed_d, phen_d), (bed_d, phen)):
        ix_mxp, ix_pxp = eng.pair_counts(b, ph, n_ind, p, marker_ix=ix, m_total=m)
        assert np.array_equal(ix_mxp, con_mxp) and np.array_equal(ix_mxp, want_mxp[ix]) and np.array_equal(ix_pxp, con_pxp)
    for bad in ([1, 1], [2, 1], [0, m], [-1, 0]):
        with pytest.raises(RuntimeError, match="ascending"):
            eng.pair_counts(bed, phen, n_ind, p, marker_ix=bad, m_total=m)
    bed_d.free()
    phen_d.free()
    eng.close()


def make_genotypes_and_traits(synth, seed):
    """genotypes, traits with 8 planted marker effects each and a trait DAG, gaps at NAN_RATE per trait, and a marker
    selection that holds the planted markers"""
    rng = synth.rng_for(seed)
    G = synth.make_genotypes(M, N, rng, miss=0.01)
    g = G.astype(np.float64)
    g[G < 0] = np.nan
    gs = np.nan_to_num((g - np.nanmean(g, 1, keepdims=True)) / np.nanstd(g, 1, keepdims=True))
    Y = np.zeros((P, N))
    planted = []
    for k in range(P):
        idx = rng.choice(M, size=8, replace=False)
        planted.extend(int(v) for v in idx)
        y = (rng.uniform(0.08, 0.2, 8) * rng.choice([-1.0, 1.0], 8)) @ gs[idx]
        for k2 in range(k):
            if rng.random() < 0.6:
                y = y + rng.uniform(0.08, 0.25) * rng.choice([-1.0, 1.0]) * Y[k2]
        y = y + rng.standard_normal(N)
        Y[k] = (y - y.mean()) / y.std()
    Y = Y.astype(np.float32)
    for k, rate in enumerate(NAN_RATE):
        Y[k, rng.random(N) < rate] = np.nan
    rest = np.setdiff1d(np.arange(M), planted)
    ixs = np.sort(np.concatenate([np.unique(planted), rng.choice(rest, size=K_SEL - len(set(planted)), replace=False)])).astype(np.int32)
    assert len(ixs) == K_SEL and (ixs < M1).any() and (ixs >= M1).any()
    return G, np.ascontiguousarray(Y).reshape(-1), ixs


def oracle_skeletons(oracle, mxm, mxp, pxp, mxp_ess, pxp_ess):
    """the oracle's cuskss pipeline on the same correlations, with per-pair sample sizes and at the uniform N"""
    sq, es = oracle.make_square_cuskss_inputs(mxm, mxp, pxp, float(N), mxp_ess, pxp_ess)
    het = oracle.cuskss_from_square(sq, es, P, ALPHA, L1, L2, DEPTH)
    sq, es = oracle.make_square_cuskss_inputs(mxm, mxp, pxp, float(N))
    return het, oracle.cuskss_from_square(sq, es, P, ALPHA, L1, L2, DEPTH)


def skeletons_differ(a, b):
    return a.num_var != b.num_var or not np.array_equal(a.new_to_old, b.new_to_old) or not np.array_equal(a.G, b.G)


@pytest.fixture(scope="module")
def data(tmp_path_factory, synth, oracle):
    from cigwas_amd import cli

    d = pathlib.Path(tmp_path_factory.mktemp("het_sumstats"))
    G, phen, ixs = make_genotypes_and_traits(synth, SEED)
    stem = str(d / "geno")
    bed = synth.pack_bed(G)
    synth.write_bfiles(stem, bed, N, np.zeros(M), np.zeros(M), ["1"] * M1 + ["2"] * (M - M1))
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    synth.write_phen(str(d / "y.phen"), phen, N, P)
    cli.main(["prep-bed", stem])
    ixs.tofile(str(d / "merged_blocks.ixs"))
    mxp_n, pxp_n = _reference_counts(bed, phen, N, P)
    # the files of `sumstats`, with and without --se
    plain, se = d / "plain", d / "se"
    plain.mkdir()
    se.mkdir()
    cli.main(["sumstats", stem, str(d / "y.phen"), str(plain), "--marker-indices", str(d / "merged_blocks.ixs")])
    cli.main(["sumstats", stem, str(d / "y.phen"), str(se), "--marker-indices", str(d / "merged_blocks.ixs"), "--se"])
    return dict(dir=d, stem=stem, phen_path=str(d / "y.phen"), ixs_path=str(d / "merged_blocks.ixs"), ixs=ixs, plain=plain, se=se,
                mxp_n=mxp_n, pxp_n=pxp_n)


def test_sumstats_se_files(data, oracle):
    for f in ("mxm.bin", "mxp.txt", "pxp.txt"):
        _same(str(data["plain"] / f), str(data["se"] / f))
    assert sorted(os.listdir(data["plain"])) == ["mxm.bin", "mxp.txt", "pxp.txt"]
    assert sorted(os.listdir(data["se"])) == ["mxm.bin", "mxp.txt", "mxp_se.txt", "pxp.txt", "pxp_se.txt"]
    se = data["se"]
    raw = [ln.split()[3:] for ln in open(se / "mxp.txt").read().splitlines()[1:]]
    finite = np.array([[tok != "NA" for tok in row] for row in raw])
    _, ess = oracle.load_mxp(str(se / "mxp.txt"), list(range(M)), se_path=str(se / "mxp_se.txt"))
    assert finite.shape == (M, P) and finite.mean() > 0.99
    assert np.array_equal(np.isnan(ess), ~finite)
    assert np.array_equal(ess[finite].astype(np.int64), data["mxp_n"][finite])
    _, pxp, pess = oracle.load_pxp(str(se / "pxp.txt"), se_path=str(se / "pxp_se.txt"))
    off = ~np.eye(P, dtype=bool)
    assert not np.isnan(pess[off]).any() and np.array_equal(pess[off].astype(np.int64), data["pxp_n"][off])
    assert np.isnan(np.diag(pess)).all()
    assert data["pxp_n"].min() < 0.15 * N and data["mxp_n"].min() < 0.3 * N  # the gaps are there


def _merged(cli, data, outdir, extra):
    outdir.mkdir()
    shutil.copy(data["ixs_path"], outdir)
    cli.main(["cuskss-merged", "--marker-indices", str(outdir / "merged_blocks.ixs"), "--alpha", str(ALPHA), "--max-level-one", str(L1),
              "--max-level-two", str(L2), "--max-depth", str(DEPTH), "--outdir", str(outdir)] + extra)


@pytest.fixture(scope="module")
def oracle_results(data, oracle, tmp_path_factory):
    """the oracle's result files from the matrices the loaders make of the files of `sumstats --se`"""
    se = data["se"]
    rows = [int(v) for v in data["ixs"]]
    mxm = oracle.load_mxm(str(se / "mxm.bin"))
    _, pxp, pxp_ess = oracle.load_pxp(str(se / "pxp.txt"), se_path=str(se / "pxp_se.txt"))
    mxp, mxp_ess = oracle.load_mxp(str(se / "mxp.txt"), rows, se_path=str(se / "mxp_se.txt"))
    het, uniform = oracle_skeletons(oracle, mxm, mxp, pxp, mxp_ess, pxp_ess)
    d = pathlib.Path(tmp_path_factory.mktemp("het_oracle"))
    for name, red in (("het", het), ("uniform", uniform)):
        (d / name).mkdir()
        oracle.write_reduced(red, str(d / name / "cuskss_merged"), with_sep=False)
    return dict(dir=d, het=het, uniform=uniform)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("time_index", [False, True])
def test_het_from_genotypes_equals_the_file_route(data, oracle, oracle_results, tmp_path, time_index):
    from cigwas_amd import cli

    extra = []
    if time_index:
        ti = tmp_path / "time_index.txt"
        ti.write_text("".join(f"{v}\n" for v in (1, 1, 2, 2, 3, 3)))
        extra = ["--time-index", str(ti)]
    se = data["se"]
    _merged(cli, data, tmp_path / "direct", ["--bfiles", data["stem"], "--phen", data["phen_path"], "--het"] + extra)
    _merged(cli, data, tmp_path / "files", ["--mxm", str(se / "mxm.bin"), "--mxp", str(se / "mxp.txt"), "--pxp", str(se / "pxp.txt"),
                                            "--mxp-se", str(se / "mxp_se.txt"), "--pxp-se", str(se / "pxp_se.txt"),
                                            "--num-samples", str(N)] + extra)
    for f in FILES:
        _same(str(tmp_path / "direct" / f), str(tmp_path / "files" / f))
    if not time_index:
        for ext in (".mdim", ".adj", ".corr"):
            _same(str(tmp_path / "direct" / "cuskss_merged") + ext, str(oracle_results["dir"] / "het" / "cuskss_merged") + ext)
        assert oracle_results["het"].num_var > P + 5  # a graph with markers in it


@pytest.mark.timeout(1500)
def test_the_flag_matters(data, oracle, oracle_results, tmp_path):
    from cigwas_amd import cli

    het, uniform = oracle_results["het"], oracle_results["uniform"]
    print(f"oracle: {het.num_var} variables / {int(het.G.sum()) // 2} edges with per-pair sample sizes, "
          f"{uniform.num_var} / {int(uniform.G.sum()) // 2} at the uniform N")
    assert skeletons_differ(het, uniform)
    assert het.num_var > P + 5 and uniform.num_var > P + 5
    _merged(cli, data, tmp_path / "het", ["--bfiles", data["stem"], "--phen", data["phen_path"], "--het"])
    _merged(cli, data, tmp_path / "plain", ["--bfiles", data["stem"], "--phen", data["phen_path"]])
    for ext in (".mdim", ".adj", ".corr"):
        _same(str(tmp_path / "het" / "cuskss_merged") + ext, str(oracle_results["dir"] / "het" / "cuskss_merged") + ext)
        _same(str(tmp_path / "plain" / "cuskss_merged") + ext, str(oracle_results["dir"] / "uniform" / "cuskss_merged") + ext)
    assert open(tmp_path / "het" / "cuskss_merged.adj", "rb").read() != open(tmp_path / "plain" / "cuskss_merged.adj", "rb").read() \
        or open(tmp_path / "het" / "cuskss_merged.mdim", "rb").read() != open(tmp_path / "plain" / "cuskss_merged.mdim", "rb").read()
