"""CPU: sepselect at per-pair sample sizes -- the rule, the files and the command line, without a device.

The rule (include/cusk_hip.h, cusk_sepselect_greedy_het): a decision over the variables V = {i, j} + S + {t},
|S + {t}| = l, is taken against q / sqrt(mean - l - 3), mean = (sum of the sizes of the (l + 2)(l + 1) / 2 unordered
pairs of V) / that count, q = norm.ppf(1 - alpha / 2).  `het_greedy_pair` / `het_greedy_sepsets` below restate
`greedy_pair` / `greedy_sepsets` of oracle/sepselect_oracle.py with that rule and nothing else changed; the GPU tests
(test_gpu_sepselect_het.py) compare the device against them.  Here they are pinned to the reference-written goldens:
with every size equal to N they must return what the oracle returns at N.

Files: a heterogeneous `cuskss` run writes `cuskss_merged.ess` (float32, layout of `.corr`); the post-step turns it into
`cuskss_merged_ssz.mtx` through the index mapping and writer of `_scm.mtx`; `MergedCuskResults` loads it and cuts it with
the collinear markers."""
import os
import shutil

import numpy as np
import pytest
from scipy.stats import norm

from conftest import GOLDEN
from test_sepselect_oracle import load_cases, materialise

CASES = ["small", "prior", "collinear", "wide", "dense_traits"]


# ---- the het oracle ----
def het_threshold(q, ssz, variables):
    """q / sqrt(mean - l - 3) over the unordered pairs of `variables` (the first two are the outer pair)"""
    l = len(variables) - 2
    total = sum(int(ssz[a, b]) for k, a in enumerate(variables) for b in variables[:k])  # exact: Python integers
    mean = np.float64(total) / np.float64((l + 2) * (l + 1) // 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / np.sqrt(mean - l - 3)


def het_greedy_pair(corr, ssz, i, j, pool, q, log=None):
    """sepselect_oracle.greedy_pair with the threshold of every decision from `ssz`.  `log`, if given, receives one
    (best z, threshold, some two candidates had the same z) per decision, for the input conditions of the GPU tests."""
    from oracle import sepselect_oracle as SO

    chosen = []
    z0, thr0 = SO.partial_z(corr, [i, j]), het_threshold(q, ssz, [i, j])
    if log is not None:
        log.append((z0, thr0, False))
    separated = z0 < thr0
    seen_minimum = False
    previous = np.inf
    for size in range(1, len(pool) + 1):
        best, pick, zs = np.inf, None, []
        for t in pool:
            z = SO.partial_z(corr, [i, j] + chosen + [t])
            zs.append(z)
            if z <= best:
                best, pick = z, t
        if best > previous and separated and not seen_minimum:
            seen_minimum = True
        thr = het_threshold(q, ssz, [i, j] + chosen + [pick])
        if log is not None:
            log.append((best, thr, len(set(zs)) < len(zs)))
        indep = best < thr
        if separated and not indep:
            break
        separated = separated or indep
        previous = best
        chosen.append(pick)
        pool.remove(pick)
    return chosen, seen_minimum


def het_greedy_sepsets(g, ssz, pairs, alpha, log=None):
    """sepselect_oracle.greedy_sepsets at the sample sizes `ssz` (num_var x num_var, the layout of g["corr"])"""
    q = norm.ppf(1 - (alpha / 2))
    grown, with_minimum = {}, {}
    for (i, j) in pairs:
        row = np.flatnonzero(g["adj"][i])
        chosen, seen = het_greedy_pair(g["corr"], ssz, i, j, set(row[row < g["num_phen"]]), q, log)
        grown[(i, j)] = chosen
        if seen:
            with_minimum[(i, j)] = chosen
    return grown, with_minimum


def het_run(g, ssz, alpha, prior_file=None, log=None):
    """sepselect_oracle.run on a loaded graph, at the sample sizes `ssz`"""
    from oracle import sepselect_oracle as SO

    triples = SO.unshielded_triples(g["adj"])
    rel = SO.relevant_triples(triples, g["num_phen"])
    grown, with_minimum = het_greedy_sepsets(g, ssz, SO.outer_pairs(rel), alpha, log)
    pag = SO.orient(g, rel, grown, SO.orientation_prior(g, prior_file))
    return {"g": g, "triples": triples, "rel": rel, "max_sepsets": grown, "min_sepsets": with_minimum, "pag": pag,
            "ambiguous": SO.ambiguous_triples(triples, grown, with_minimum)}


def write_ssz(stem, ssz):
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    mmwrite(stem + "_ssz.mtx", coo_matrix(np.asarray(ssz, dtype=np.float64)))


def read_mtx_entries(path):
    """[(i, j, value text)] of a coordinate file in file order, and its size line"""
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("%%MatrixMarket matrix coordinate")
    return [tuple(ln.split("\t")) for ln in lines[2:]], lines[1]


@pytest.mark.parametrize("name", CASES)
def test_het_oracle_at_uniform_sizes_is_the_oracle(name, tmp_path):
    from oracle import sepselect_oracle as SO

    case = load_cases()[name]
    stem, _ = materialise(case, str(tmp_path))
    g = SO.load_merged(stem)
    pairs = SO.outer_pairs(SO.relevant_triples(SO.unshielded_triples(g["adj"]), g["num_phen"]))
    want = SO.greedy_sepsets(g, pairs, case["alpha"], case["num_samples"])
    got = het_greedy_sepsets(g, np.full(g["corr"].shape, case["num_samples"], dtype=np.int64), pairs, case["alpha"])
    assert got == want and len(got[1]) == case["pairs_with_minimum"]
    assert list(got[0]) == list(want[0])  # same pair order too
    # the threshold itself, bit for bit, at every level a golden reaches
    q = norm.ppf(1 - (case["alpha"] / 2))
    ssz = np.full((40, 40), case["num_samples"], dtype=np.int64)
    for l in range(0, 30):
        assert het_threshold(q, ssz, list(range(l + 2))) == SO.z_threshold(case["alpha"], case["num_samples"], l)


def test_het_threshold_is_the_mean_over_all_pairs():
    ssz = np.array([[0, 10, 20, 30], [10, 0, 40, 50], [20, 40, 0, 60], [30, 50, 60, 0]])
    q = 2.0
    assert het_threshold(q, ssz, [0, 1]) == q / np.sqrt(10.0 - 0 - 3)
    assert het_threshold(q, ssz, [1, 0, 2]) == q / np.sqrt(np.float64(70) / 3 - 1 - 3)
    assert het_threshold(q, ssz, [3, 1, 0, 2]) == q / np.sqrt(np.float64(210) / 6 - 2 - 3)
    assert not 0.0 < het_threshold(q, np.full((4, 4), 4), [0, 1, 2, 3])  # negative radicand: NaN, nothing is below it


# ---- .ess -> _ssz.mtx ----
def _merged_dir(tmp_path, name="cm"):
    G = os.path.join(GOLDEN, "merge")
    d = tmp_path / name
    shutil.copytree(os.path.join(G, "cuskss_merged_raw"), d)
    shutil.copy(os.path.join(G, "merged", "merged_blocks.ixs"), d)
    with open(d / "cuskss_merged.mdim") as f:
        num_var, num_p, _ = (int(v) for v in f.readline().split())
    return G, d, num_var, num_p


def test_ess_goes_through_the_mapping_and_writer_of_corr(tmp_path):
    from cigwas_amd import merge

    G, d, n, p = _merged_dir(tmp_path)
    m = n - p
    r, c = np.indices((n, n))
    code = (1000 * (r + 1) + c + 1).astype(np.float32)  # every entry names its own dense (row, column)
    code.tofile(d / "cuskss_merged.corr")  # the same code through the correlation route, for the comparison
    ess = code.copy()
    ess[m:, m:][np.eye(p, dtype=bool)] = np.nan  # the trait diagonal as the pipeline has it
    ess[0, m + 1] = ess[m + 1, 0] = np.nan  # a NaN correlation
    ess[1, m] += 0.5  # the se -> size chain lands in [count, count + 1)
    ess.tofile(d / "cuskss_merged.ess")
    merge.reformat_cuskss_merged_output(str(d)).write_mm(f"{d}/cuskss_merged")
    scm, scm_size = read_mtx_entries(d / "cuskss_merged_scm.mtx")
    ssz, ssz_size = read_mtx_entries(d / "cuskss_merged_ssz.mtx")
    assert open(d / "cuskss_merged_ssz.mtx").readline() == open(d / "cuskss_merged_scm.mtx").readline()
    assert len(scm) == n * n and len(ssz) == n * n - p - 2
    assert scm_size.split("\t")[:2] == ssz_size.split("\t")[:2] and int(ssz_size.split("\t")[2]) == len(ssz)
    where = {v: (i, j) for i, j, v in scm}  # code -> merged (row, column), as the correlation route maps it
    assert len(where) == n * n
    for i, j, v in ssz:
        assert v.endswith(".0") and where[v] == (i, j)  # whole numbers written as floats, at the place corr has them
    assert [(i, j) for i, j, _ in ssz] == [(i, j) for i, j, v in scm if v in {e[2] for e in ssz}]  # same entry order
    # dense marker 1 x trait 0 -> merged (p + 2, 1): truncated, not rounded up
    assert (str(p + 2), "1", f"{float(code[1, m])}") in ssz
    # traits first in the merged order: dense (m + a, m + b) -> (a + 1, b + 1)
    assert where[f"{float(code[m, m + 1])}"] == ("1", "2") and where[f"{float(code[0, m])}"] == (str(p + 1), "1")


def test_without_ess_the_post_step_writes_what_it_wrote(tmp_path):
    from cigwas_amd import merge

    G, d, n, p = _merged_dir(tmp_path)
    merge.reformat_cuskss_merged_output(str(d)).write_mm(f"{d}/cuskss_merged")
    assert not os.path.exists(d / "cuskss_merged_ssz.mtx")
    # with it: one more file, the others keep their bytes (the goldens the reference's own post-step wrote)
    G, d, n, p = _merged_dir(tmp_path, "cm_het")
    np.full((n, n), 1234, np.float32).tofile(d / "cuskss_merged.ess")
    merge.reformat_cuskss_merged_output(str(d)).write_mm(f"{d}/cuskss_merged")
    assert os.path.exists(d / "cuskss_merged_ssz.mtx")
    for f in sorted(os.listdir(os.path.join(G, "cuskss_merged"))):
        assert open(d / f, "rb").read() == open(os.path.join(G, "cuskss_merged", f), "rb").read(), f


# ---- the loader ----
def test_sizes_are_loaded_and_cut_with_the_collinear_markers(tmp_path):
    from cigwas_amd import sepselect as SS
    from oracle import sepselect_oracle as SO

    case = load_cases()["collinear"]
    stem, _ = materialise(case, str(tmp_path))
    assert SS.MergedCuskResults(stem).ssz is None  # optional
    n_in, p, _ = (int(v) for v in case["input"]["mdim"].split())
    r, c = np.indices((n_in, n_in))
    full = 100 * (r + 1) + c + 1  # every entry names its own (row, column) before the cut
    full[2, 3] = full[3, 2] = 0  # an entry without a size is not in the file and reads as 0
    write_ssz(stem, full)
    cr = SS.MergedCuskResults(stem, het=True)
    g = SO.load_merged(stem)
    assert cr.num_var == g["num_var"] < n_in  # markers were dropped
    kept = np.concatenate([np.arange(p), p + np.flatnonzero(np.isin(np.array(case["input"]["ixs"]), g["ixs"]))])
    assert len(kept) == cr.num_var
    assert cr.ssz.shape == cr.corr.shape and np.array_equal(cr.ssz, full[np.ix_(kept, kept)])
    assert cr.ssz[2, 3] == 0 and cr.ssz.dtype == np.float64


def test_asymmetric_sizes_are_refused_before_any_device_work(tmp_path):
    from cigwas_amd import sepselect as SS

    case = load_cases()["small"]
    stem, _ = materialise(case, str(tmp_path))
    n = int(case["input"]["mdim"].split()[0])
    write_ssz(stem, np.full((n, n), case["num_samples"]))
    cr = SS.MergedCuskResults(stem, het=True)
    cr.ssz[0, 1] += 1
    with pytest.raises(ValueError, match="not symmetric"):
        cr.find_maximal_and_min_pcorr_sepsets_incr(case["alpha"], case["num_samples"], het=True)


# ---- command line ----
def test_het_flags_parse():
    from cigwas_amd import cli

    p = cli.build_parser()
    a = p.parse_args(["sepselect", "out/cuskss_merged", "0.001", "1000", "--het"])
    assert a.func is cli.run_sepselect and a.het is True and a.num_samples == 1000
    a = p.parse_args(["orient-v-structs", "out/cuskss_merged", "0.001", "1000", "--het", "--orientation-prior", "prior.bin"])
    assert a.func is cli.run_v_struct and a.het is True and a.orientation_prior == "prior.bin"
    for cmd in ("sepselect", "orient-v-structs"):
        assert p.parse_args([cmd, "out/cuskss_merged", "0.001", "1000"]).het is False
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "out/cuskss_merged", "0.001", "--het"])  # num-samples stays positional


@pytest.mark.parametrize("cmd", ["sepselect", "orient-v-structs"])
def test_missing_sizes_are_a_clear_error_before_any_engine(cmd, tmp_path, monkeypatch):
    from cigwas_amd import cli
    from cigwas_amd import sepselect as SS

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(SS, "Engine", no_engine)
    case = load_cases()["small"]
    stem, _ = materialise(case, str(tmp_path))
    with pytest.raises(FileNotFoundError) as err:
        cli.main([cmd, stem, str(case["alpha"]), str(case["num_samples"]), "--het"])
    assert stem + "_ssz.mtx" in str(err.value) and "cuskss-merged --het" in str(err.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "max_sep_min_pc.mdim"))
