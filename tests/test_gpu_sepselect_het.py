"""GPU: sepselect at per-pair sample sizes (`cusk_sepselect_greedy_het`, `sepselect --het`, `orient-v-structs --het`).

1. With every size equal to N the het path writes, byte for byte, the files the reference wrote for the goldens.
2. On seeded skeletons with estimated correlations and sizes that follow each trait's observed fraction, every LDS class
   of the kernel (8/16/32/64/84 candidates) and the HBM work-space path give the sets, PAG and files of the in-test
   oracle (test_sepselect_het_formats.py: the oracle's greedy loop with the threshold rule of the header).
3. On the small graph the het result differs from the run at the uniform N: the flag matters.
4. End to end from a PLINK set with a 60 % NA trait: `cuskss-merged --het` writes the sizes (`.ess`, `_ssz.mtx`), the
   file route on `sumstats --se` writes the same bytes, `sepselect --het` on that stem equals the oracle, and the non-het
   run writes neither file.

The comparisons are exact.  That is a condition on the inputs, asserted on the CPU by the generator: no decision of the
oracle lies within 1e-9 (relative) of its threshold and no round has two candidates with the same z, so the last bits in
which the kernel's downdates differ from a matrix inverse cannot change a decision."""
import os
import pathlib
import shutil

import numpy as np
import pytest
from scipy.stats import norm

from test_sepselect_het_formats import CASES, het_run, write_ssz
from test_sepselect_oracle import check_outputs, load_cases, materialise

pytestmark = pytest.mark.gpu

CAPS = (8, 16, 32, 64, 84)  # candidate-count classes served from LDS; longer lists run in the HBM work space
FRACTIONS = (1.0, 0.6, 0.2)
OUT_FILES = (".mdim", "_sam.mtx", "_scm.mtx", "_spm.mtx", ".ssm", ".ut", ".atr")


def storage_class(t):
    return next((c for c in CAPS if t <= c), "hbm")


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


# ---- 1. uniform sizes: the reference-written goldens ----
@pytest.mark.parametrize("name", CASES)
def test_uniform_sizes_write_the_reference_files(name, tmp_path):
    from cigwas_amd import sepselect as SS

    case = load_cases()[name]
    stem, prior = materialise(case, str(tmp_path))
    n = int(case["input"]["mdim"].split()[0])
    write_ssz(stem, np.full((n, n), case["num_samples"]))
    res = SS.orient_v_structures_merged(stem, case["alpha"], 0, orientation_prior_file=prior, het=True)  # num_samples unused
    assert len(res.min_sepsets) == case["pairs_with_minimum"]
    ostem = os.path.join(str(tmp_path), "max_sep_min_pc")
    res.to_file(ostem)
    check_outputs(case, ostem)


# ---- 2. / 3. seeded skeletons, every kernel class ----
def make_skeleton(seed, p, marker_lists, n_obs, trait_edge_prob):
    """A merged skeleton (traits 0..p-1, then one marker per entry of `marker_lists`, adjacent to that many traits) with
    the sample correlations of `n_obs` draws of a linear model, and sample sizes: each trait is observed on a fraction
    of the N = n_obs individuals, a pair on about N times the smaller fraction (a little less, pair by pair)."""
    rng = np.random.default_rng(seed)
    m = len(marker_lists)
    n = p + m
    X = rng.normal(size=(n_obs, m))
    F = rng.normal(size=(n_obs, 6))
    Y = F @ (rng.normal(size=(6, p)) * 0.5) + X @ (rng.normal(size=(m, p)) * 0.15) + rng.normal(size=(n_obs, p))
    corr = np.corrcoef(np.hstack([Y, X]).T)
    corr = 0.5 * (corr + corr.T)
    np.fill_diagonal(corr, 1.0)
    adj = np.zeros((n, n), dtype=bool)
    tt = np.triu(rng.random((p, p)) < trait_edge_prob, 1)
    adj[:p, :p] = tt | tt.T
    for k, t in enumerate(marker_lists):
        nb = rng.choice(p, size=t, replace=False)
        adj[p + k, nb] = adj[nb, p + k] = True
    frac = np.concatenate([rng.permutation(np.resize(FRACTIONS, p)), np.ones(m)])
    ssz = np.floor(n_obs * np.minimum.outer(frac, frac)).astype(np.int64) - np.triu(rng.integers(0, n_obs // 50, size=(n, n)), 1)
    ssz = np.triu(ssz, 1) + np.triu(ssz, 1).T
    ssz[p:, p:] = n_obs  # marker x marker: the cohort
    np.fill_diagonal(ssz, 0)
    return adj, corr, ssz


def write_skeleton(stem, adj, corr, ssz, p):
    import scipy.sparse as sp
    from scipy.io import mmwrite

    n = adj.shape[0]
    mmwrite(stem + "_sam.mtx", sp.coo_matrix(adj.astype(np.int32)))
    mmwrite(stem + "_scm.mtx", sp.coo_matrix(corr))
    write_ssz(stem, ssz)
    with open(stem + ".mdim", "w") as f:
        f.write(f"{n}\t{p}\t3\n")
    np.arange(n - p, dtype=np.int32).tofile(stem + ".ixs")


def oracle_at(stem, ssz, alpha):
    """the het oracle on a written skeleton, with the conditions under which an exact comparison is meaningful"""
    from oracle import sepselect_oracle as SO

    g = SO.load_merged(stem)
    assert g["num_var"] == ssz.shape[0]  # no collinear marker in these graphs
    log = []
    exp = het_run(g, ssz, alpha, log=log)
    assert log and all(abs(best - thr) / thr > 1e-9 for best, thr, _ in log), "a decision sits on its threshold: other seed"
    assert not any(tie for _, _, tie in log), "two candidates with the same z: other seed"
    assert exp["min_sepsets"] and any(exp["max_sepsets"].values())
    return g, exp


SMALL = dict(seed=11, p=12, marker_lists=[2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12] * 3, n_obs=1000, trait_edge_prob=0.5, alpha=1e-2)
LARGE = dict(seed=12, p=90, marker_lists=[20, 40, 70, 84, 88, 30], n_obs=2000, trait_edge_prob=0.02, alpha=1e-2)


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    """both graphs written once, with the oracle's result at the per-pair sizes (and, for the small one, at the uniform N)"""
    out = {}
    for name, par in (("small", SMALL), ("large", LARGE)):
        d = pathlib.Path(tmp_path_factory.mktemp("sepselect_het_" + name))
        adj, corr, ssz = make_skeleton(par["seed"], par["p"], par["marker_lists"], par["n_obs"], par["trait_edge_prob"])
        stem = str(d / "cuskss_merged")
        write_skeleton(stem, adj, corr, ssz, par["p"])
        g, exp = oracle_at(stem, ssz, par["alpha"])
        out[name] = dict(dir=d, stem=stem, par=par, adj=adj, ssz=ssz, g=g, exp=exp)
    return out


def _lists(gr):
    """candidate-list length of every outer pair (i, j): the trait neighbours of i"""
    p = gr["par"]["p"]
    return {(i, j): int(np.count_nonzero(gr["adj"][i, :p])) for (i, j) in gr["exp"]["max_sepsets"]}


@pytest.mark.parametrize("name", ["small", "large"])
def test_every_kernel_class_equals_the_het_oracle(name, graphs, tmp_path):
    from cigwas_amd import sepselect as SS
    from oracle import sepselect_oracle as SO

    gr = graphs[name]
    par, exp = gr["par"], gr["exp"]
    p = par["p"]
    lists = _lists(gr)
    classes = {k: storage_class(t) for k, t in lists.items()}
    if name == "small":
        assert set(classes.values()) == {8, 16} and max(lists.values()) == 12
    else:  # pairs led by marker k run in the class of its list: 20 -> 32, 40 -> 64, 70 and 84 -> 84, 88 -> work space
        by_marker = {k: {c for (i, _), c in classes.items() if i == p + k} for k in range(len(par["marker_lists"]))}
        assert by_marker == {0: {32}, 1: {64}, 2: {84}, 3: {84}, 4: {"hbm"}, 5: {32}}
        assert {lists[k] for k in lists if k[0] >= p} == set(par["marker_lists"])
        assert set(classes.values()) >= {32, 64, 84, "hbm"}
    res = SS.orient_v_structures_merged(gr["stem"], par["alpha"], 0, het=True)
    assert {k: [int(v) for v in s] for k, s in exp["max_sepsets"].items()} == res.max_sepsets
    assert set(exp["min_sepsets"]) == set(res.min_sepsets)
    assert np.array_equal(exp["rel"], res.get_rfci_relevant_unshielded_triples())
    assert np.array_equal(exp["ambiguous"], res.ambiguous_triples)
    assert np.array_equal(exp["pag"], res.pag)
    (tmp_path / "dev").mkdir()
    (tmp_path / "cpu").mkdir()
    res.to_file(str(tmp_path / "dev" / "max_sep_min_pc"))
    SO.write(exp, str(tmp_path / "cpu" / "max_sep_min_pc"))
    for sfx in OUT_FILES:
        _same(str(tmp_path / "dev" / "max_sep_min_pc") + sfx, str(tmp_path / "cpu" / "max_sep_min_pc") + sfx)


def test_the_flag_matters(graphs):
    from cigwas_amd import sepselect as SS
    from oracle import sepselect_oracle as SO

    gr = graphs["small"]
    par, het = gr["par"], gr["exp"]
    N = par["n_obs"]
    # first on the two oracles, so that the device comparison below cannot pass vacuously
    uni = SO.run(gr["stem"], par["alpha"], N)
    assert set(uni["max_sepsets"]) == set(het["max_sepsets"])
    differing = [k for k in het["max_sepsets"] if het["max_sepsets"][k] != uni["max_sepsets"][k]]
    assert differing and not np.array_equal(het["pag"], uni["pag"])
    plain = SS.orient_v_structures_merged(gr["stem"], par["alpha"], N)
    flagged = SS.orient_v_structures_merged(gr["stem"], par["alpha"], N, het=True)
    assert plain.max_sepsets == {k: [int(v) for v in s] for k, s in uni["max_sepsets"].items()}
    assert np.array_equal(plain.pag, uni["pag"])
    # the same pairs differ on the device (the two dicts list the pairs in different orders)
    assert {k for k in flagged.max_sepsets if flagged.max_sepsets[k] != plain.max_sepsets[k]} == {(int(i), int(j)) for i, j in differing}
    assert flagged.max_sepsets == {k: [int(v) for v in s] for k, s in het["max_sepsets"].items()}
    assert np.array_equal(flagged.pag, het["pag"]) and not np.array_equal(flagged.pag, plain.pag)


def test_bad_het_arguments_are_refused():
    import cigwas_amd as cg

    eng = cg.Engine(0)
    corr = np.eye(4)
    tn = np.full((4, 2), 100, np.int32)
    ok = eng.sepselect_greedy_het(corr[:, :2], [2], [3], [0.0], [0, 2], [0, 1], tn, [100], 2.0)
    assert ok[2][0] >> 8 == 0
    bad = tn.copy()
    bad[0, 1] = 99  # trait x trait block not symmetric
    with pytest.raises(Exception, match="symmetric"):
        eng.sepselect_greedy_het(corr[:, :2], [2], [3], [0.0], [0, 2], [0, 1], bad, [100], 2.0)
    with pytest.raises(Exception):  # candidate 7 is not a trait index
        eng.sepselect_greedy_het(corr[:, :2], [2], [3], [0.0], [0, 1], [7], tn, [100], 2.0)
    # sizes too small for any test (negative radicand, NaN threshold): nothing is independent
    tiny = np.full((4, 2), 2, np.int32)
    sel, sel_len, flags, _ = eng.sepselect_greedy_het(corr[:, :2], [2], [3], [0.0], [0, 2], [0, 1], tiny, [2], 2.0)
    assert flags[0] >> 8 == 0 and sel_len[0] == 2  # never separated: the loop runs to the end of the list, as the oracle's does
    eng.close()


# ---- 4. end to end ----
E_M, E_N, E_P, E_SEL = 400, 301, 6, 60
E_NAN = (0.0, 0.05, 0.6, 0.0, 0.1, 0.0)  # trait 2 is observed on 40 % of the cohort
E_ALPHA, E_L1, E_L2, E_DEPTH = 1e-2, 3, 3, 1
E_SEED = 4242


def make_plink_case(synth, seed):
    """genotypes, six traits with planted marker effects and a trait chain, gaps at E_NAN per trait, a marker selection
    that holds the planted markers"""
    rng = synth.rng_for(seed)
    G = synth.make_genotypes(E_M, E_N, rng, window=8, rho=0.5, miss=0.01)
    g = G.astype(np.float64)
    g[G < 0] = np.nan
    gs = np.nan_to_num((g - np.nanmean(g, 1, keepdims=True)) / np.nanstd(g, 1, keepdims=True))
    Y = np.zeros((E_P, E_N))
    planted = []
    for k in range(E_P):
        idx = rng.choice(E_M, size=3, replace=False)
        planted.extend(int(v) for v in idx)
        y = (rng.uniform(0.35, 0.5, 3) * rng.choice([-1.0, 1.0], 3)) @ gs[idx]
        for k2 in range(k):
            if k2 == k - 1 or rng.random() < 0.3:
                y = y + rng.uniform(0.35, 0.6) * rng.choice([-1.0, 1.0]) * Y[k2]
        y = y + rng.standard_normal(E_N)
        Y[k] = (y - y.mean()) / y.std()
    Y = Y.astype(np.float32)
    for k, rate in enumerate(E_NAN):
        Y[k, rng.random(E_N) < rate] = np.nan
    rest = np.setdiff1d(np.arange(E_M), planted)
    ixs = np.sort(np.concatenate([np.unique(planted), rng.choice(rest, size=E_SEL - len(set(planted)), replace=False)]))
    return G, np.ascontiguousarray(Y).reshape(-1), ixs.astype(np.int32)


def pair_counts(bed, phen):
    codes = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :E_N]
    present = (codes != 1).astype(np.int64)
    seen = (~np.isnan(np.asarray(phen, np.float32).reshape(E_P, E_N))).astype(np.int64)
    return present @ seen.T, seen @ seen.T


def run_end_to_end(synth, d, seed):
    """every command of the chain, once; returns the directories and what numpy says the sizes are"""
    from cigwas_amd import cli

    G, phen, ixs = make_plink_case(synth, seed)
    stem = str(d / "geno")
    bed = synth.pack_bed(G)
    synth.write_bfiles(stem, bed, E_N, np.zeros(E_M), np.zeros(E_M))
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    synth.write_phen(str(d / "y.phen"), phen, E_N, E_P)
    cli.main(["prep-bed", stem])
    ixs.tofile(str(d / "merged_blocks.ixs"))
    (d / "se").mkdir()
    cli.main(["sumstats", stem, str(d / "y.phen"), str(d / "se"), "--marker-indices", str(d / "merged_blocks.ixs"), "--se"])
    se = d / "se"
    routes = {"direct": ["--bfiles", stem, "--phen", str(d / "y.phen"), "--het"],
              "files": ["--mxm", str(se / "mxm.bin"), "--mxp", str(se / "mxp.txt"), "--pxp", str(se / "pxp.txt"), "--mxp-se",
                        str(se / "mxp_se.txt"), "--pxp-se", str(se / "pxp_se.txt"), "--num-samples", str(E_N)],
              "plain": ["--bfiles", stem, "--phen", str(d / "y.phen")]}
    for name, extra in routes.items():
        (d / name).mkdir()
        shutil.copy(d / "merged_blocks.ixs", d / name)
        cli.main(["cuskss-merged", "--marker-indices", str(d / name / "merged_blocks.ixs"), "--alpha", str(E_ALPHA),
                  "--max-level-one", str(E_L1), "--max-level-two", str(E_L2), "--max-depth", str(E_DEPTH), "--outdir",
                  str(d / name)] + extra)
    mxp_n, pxp_n = pair_counts(bed, phen)
    return dict(dir=d, mxp_n=mxp_n, pxp_n=pxp_n)


@pytest.fixture(scope="module")
def chain(tmp_path_factory, synth):
    return run_end_to_end(synth, pathlib.Path(tmp_path_factory.mktemp("sepselect_het_e2e")), E_SEED)


def test_cuskss_het_writes_the_sample_sizes(chain):
    d = chain["dir"]
    with open(d / "direct" / "cuskss_merged.mdim") as f:
        n, p, _ = (int(v) for v in f.readline().split())
    m = n - p
    assert p == E_P and m > 3  # a graph with markers in it
    glob = np.fromfile(d / "direct" / "cuskss_merged.ixs", dtype=np.int32)  # after the post-step: .bim rows of the markers
    assert glob.shape[0] == m
    ess = np.fromfile(d / "direct" / "cuskss_merged.ess", dtype=np.float32)
    assert ess.shape[0] == n * n
    ess = ess.reshape(n, n)
    want = np.full((n, n), float(E_N))  # markers first, then the traits; N between markers
    want[:m, m:] = chain["mxp_n"][glob]
    want[m:, :m] = chain["mxp_n"][glob].T
    want[m:, m:] = chain["pxp_n"]
    want[m:, m:][np.eye(p, dtype=bool)] = np.nan  # the diagonal as the pipeline has it (pxp_se holds nan there)
    assert np.array_equal(np.isnan(ess), np.isnan(want))
    assert np.array_equal(np.trunc(ess[~np.isnan(want)]), want[~np.isnan(want)])
    assert want[m:, m:][0, 2] < 0.5 * E_N  # the gap is there
    # the file route on the files of `sumstats --se`: the same bytes, sizes included
    for f in ("cuskss_merged.ess", "cuskss_merged_ssz.mtx", "cuskss_merged.corr", "cuskss_merged.adj", "cuskss_merged.mdim",
              "cuskss_merged.ixs", "cuskss_merged_sam.mtx", "cuskss_merged_scm.mtx"):
        _same(str(d / "direct" / f), str(d / "files" / f))
    # the post-step: the sizes in the merged order (traits first), whole numbers
    from scipy.io import mmread

    ssz = mmread(str(d / "direct" / "cuskss_merged_ssz.mtx")).toarray()
    order = np.concatenate([np.arange(m, n), np.arange(m)])
    assert np.array_equal(ssz, np.nan_to_num(want, nan=0.0)[np.ix_(order, order)])
    # without --het: neither file
    assert not os.path.exists(d / "plain" / "cuskss_merged.ess") and not os.path.exists(d / "plain" / "cuskss_merged_ssz.mtx")
    assert os.path.exists(d / "plain" / "cuskss_merged_scm.mtx")


def test_sepselect_het_on_that_stem_equals_the_oracle(chain, tmp_path):
    from scipy.io import mmread

    from cigwas_amd import cli
    from oracle import sepselect_oracle as SO

    d = chain["dir"] / "direct"
    stem = str(d / "cuskss_merged")
    g = SO.load_merged(stem)
    ssz = mmread(stem + "_ssz.mtx").toarray().astype(np.int64)
    kept = np.isin(np.fromfile(stem + ".ixs", dtype=np.int32), g["ixs"])  # the collinear-marker cut, applied to the sizes
    keep = np.concatenate([np.ones(g["num_phen"], dtype=bool), kept])
    ssz = ssz[np.ix_(keep, keep)]
    log = []
    exp = het_run(g, ssz, E_ALPHA, log=log)
    assert exp["min_sepsets"] and any(exp["max_sepsets"].values())  # otherwise there is nothing to write: other seed
    assert all(abs(best - thr) / thr > 1e-9 for best, thr, _ in log) and not any(tie for _, _, tie in log)  # as in oracle_at
    uni = SO.greedy_sepsets(g, SO.outer_pairs(exp["rel"]), E_ALPHA, E_N)[0]
    print(f"{len(exp['max_sepsets'])} outer pairs, {sum(exp['max_sepsets'][k] != uni[k] for k in uni)} differ from the run at N")
    cli.main(["sepselect", stem, str(E_ALPHA), str(E_N), "--het"])
    SO.write(exp, str(tmp_path / "max_sep_min_pc"))
    for sfx in OUT_FILES:
        if sfx != "_spm.mtx":  # sepselect orients nothing
            _same(str(d / "max_sep_min_pc") + sfx, str(tmp_path / "max_sep_min_pc") + sfx)
    assert not os.path.exists(str(d / "max_sep_min_pc") + "_spm.mtx")
