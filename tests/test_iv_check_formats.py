"""CPU: `iv-candidates` / `check-ivs` (ci-gwas_amd/ivcheck.py) against what the reference itself produced.

tests/golden/iv_check_kat.json (metadata) and iv_check_<case>.npz (data) were written by tests/golden/make_iv_check_golden.py from the
reference's `get_iv_candidates` / `check_ivs`: input files, candidate rows, the rows of the flag combinations, and every
distinct test the reference performed as (x, y, S, z_ref, thr).  Per case the generator recorded margin = min |z_ref - thr|
and asserted margin >= 1000 d (d = the float64 Schur form's largest deviation from z_ref), so a z within margin / 2 of
z_ref cannot flip a verdict and no item is left out anywhere.

Subject here: the numpy host form (`check_ivs(engine=None)`, `HostEngine`), the file formats and the command line.  The
device path runs the same cases in test_gpu_iv_check.py, which imports the helpers below."""
import ctypes
import functools
import itertools
import json
import os
import re

import numpy as np
import pytest

from test_sepselect_het_formats import write_ssz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("p2", "p6", "p14", "p40", "p66", "p128")


@functools.lru_cache(maxsize=None)
def load_kat():
    with open(os.path.join(GOLDEN, "iv_check_kat.json")) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def load_tests(name):
    with np.load(os.path.join(GOLDEN, f"iv_check_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def flag_sets(case):
    """[(key, relaxed, reverse)] of the stored combinations"""
    out = []
    for key in case["row_counts"]:
        relaxed, reverse = (int(v) for v in re.fullmatch(r"relaxed=(\d),reverse=(\d)", key).groups())
        out.append((key, bool(relaxed), bool(reverse)))
    return out


def materialise(name, d):
    """write the case's three input files; returns the stem"""
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    case = load_kat()[name]
    stem = os.path.join(str(d), "all_merged")
    t = load_tests(name)
    if case["input_as_text"]:
        for key, suffix in (("mdim", ".mdim"), ("sam", "_sam.mtx"), ("scm", "_scm.mtx")):
            with open(stem + suffix, "wb") as f:
                f.write(t["input_" + key].tobytes())
    else:
        mmwrite(stem + "_sam.mtx", coo_matrix(t["adj"].astype(np.int32)))
        mmwrite(stem + "_scm.mtx", coo_matrix(t["corr"]))
        with open(stem + ".mdim", "w") as f:
            f.write(f"{case['traits'] + case['markers']}\t{case['traits']}\t3\n")
    return stem


def trait_corr_of(name, d):
    from cigwas_amd import ivcheck

    _, corr, p, _ = ivcheck.load(materialise(name, d))
    return np.ascontiguousarray(corr[:, :p])


def rows_of(name, key):
    case = load_kat()[name]
    rows = load_tests(name)["rows_" + key].tolist()
    assert len(rows) == case["row_counts"][key]
    return [tuple(r) for r in rows]


def candidates_of(name):
    case = load_kat()[name]
    rows = load_tests(name)["candidates"].tolist()
    assert len(rows) == case["candidate_count"]
    return [tuple(r) for r in rows]


def het_oracle(tc, tn, set_off, sets, xs, ys, iset, q):
    """per item: the inverse over [x, y] + S, and the mean rule of the header -- nothing shared with the package"""
    p = tc.shape[1]
    full = lambda tab, a, b: tab[a, b] if b < p else tab[b, a]  # noqa: E731
    z, thr = np.empty(len(xs)), np.empty(len(xs))
    for k, (x, y, s) in enumerate(zip(xs, ys, iset)):
        S = [int(t) for t in sets[set_off[s]:set_off[s + 1]]] if s >= 0 else []
        V = [int(x), int(y)] + S
        M = np.array([[1.0 if a == b else full(tc, a, b) for b in V] for a in V])
        m = np.linalg.inv(M)
        r = -m[0, 1] / np.sqrt(abs(m[0, 0] * m[1, 1]))
        z[k] = abs(0.5 * np.log(abs((1 + r) / (1 - r))))
        nsum = sum(int(full(tn, a, b)) for a, b in itertools.combinations(V, 2))
        mean = nsum / (len(V) * (len(V) - 1) // 2)
        with np.errstate(invalid="ignore"):
            thr[k] = q / np.sqrt(np.float64(mean - len(S) - 3))
    return z, thr


def trait_sizes(n, p, N, quarter_trait):
    """sizes that differ by trait: trait t is observed on a share of the N individuals, one trait on a quarter; a pair
    on the smaller share"""
    share = np.ones(n)
    share[:p] = np.linspace(1.0, 0.7, p)
    share[quarter_trait] = 0.25
    return np.floor(N * np.minimum(share[:, None], share[None, :])).astype(np.int64)


# ---- ABI ----
def test_symbols_are_declared_and_exported():
    from cigwas_amd._lib import SO_PATH, SYMBOLS

    _vp, _i, _ll, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    assert SYMBOLS["cusk_iv_check"] == (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    assert SYMBOLS["cusk_iv_check_het"] == (_i, [_vp, _vp, _ll, _i, _i, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cusk_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert ("int cusk_iv_check(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off, "
            "const int *set, long long nitems, const int *item_x, const int *item_y, const int *item_set, const double *thr, "
            "double *z, int *flags, float *kernel_ms);") in hdr
    assert ("int cusk_iv_check_het(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, "
            "const int *set_off, const int *set, long long nitems, const int *item_x, const int *item_y, const int *item_set, "
            "const int *trait_n, double q, double *z, int *flags, float *kernel_ms);") in hdr
    lib = ctypes.CDLL(SO_PATH)
    assert hasattr(lib, "cusk_iv_check") and hasattr(lib, "cusk_iv_check_het")


# ---- the host form against the reference ----
@pytest.mark.parametrize("name", CASES)
def test_host_form_reproduces_the_reference_rows(name, tmp_path):
    from cigwas_amd import ivcheck

    case = load_kat()[name]
    stem = materialise(name, tmp_path)
    assert ivcheck.iv_candidates(stem) == candidates_of(name)
    for key, relaxed, reverse in flag_sets(case):
        stats = {}
        rows = ivcheck.check_ivs(stem, case["num_samples"], case["accept_alpha"], case["reject_alpha"],
                                 relaxed_local_faithfulness=relaxed, check_reverse_causality=reverse, stats=stats)
        assert rows == rows_of(name, key), key
        assert stats["calls"] <= 4


@pytest.mark.parametrize("name", CASES)
def test_host_form_reproduces_every_recorded_z(name, tmp_path):
    from cigwas_amd import ivcheck

    case, t = load_kat()[name], load_tests(name)
    tc = trait_corr_of(name, tmp_path)
    assert t["z"].size == case["tests"] and case["margin"] >= 1000 * case["d"]
    for alpha_id, alpha in enumerate((case["accept_alpha"], case["reject_alpha"])):
        pick = t["alpha_id"] == alpha_id
        z, flags, _ = ivcheck.HostEngine().iv_check(tc, t["set_off"], t["sets"], t["x"][pick], t["y"][pick], t["set"][pick],
                                                    ivcheck.thresholds(alpha, case["num_samples"], case["traits"]))
        dev = np.abs(z - t["z"][pick])
        print(f"{name} alpha {alpha}: {int(pick.sum())} tests, max |z - z_ref| {dev.max():.3e}, margin {case['margin']:.3e}")
        assert dev.max() <= case["margin"] / 2
        assert np.array_equal(flags & 1, (t["z"][pick] < t["thr"][pick]).astype(np.int32))
        assert not (flags >> 8).any()


def test_first_marker_is_never_a_candidate(tmp_path):
    """`v > p`: variable p, the first marker, is adjacent to traits here and must appear in neither table"""
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    from cigwas_amd import ivcheck
    from cigwas_amd.synth import merged_skeleton

    p, m = 4, 12
    adj, corr, _, _ = merged_skeleton(7, p, m, noise=0.002)
    adj[:p, p] = adj[p, :p] = True  # the first marker touches every trait
    corr[:p, p] = corr[p, :p] = 0.3
    stem = os.path.join(str(tmp_path), "m")
    mmwrite(stem + "_sam.mtx", coo_matrix(adj.astype(np.int32)))
    mmwrite(stem + "_scm.mtx", coo_matrix(corr))
    with open(stem + ".mdim", "w") as f:
        f.write(f"{p + m}\t{p}\t3\n")
    cand = ivcheck.iv_candidates(stem)
    assert cand and all(iv >= 2 for _, _, iv in cand)  # IV 1 is variable p
    assert {iv for _, _, iv in cand} >= {int(v) + 1 - p for v in np.flatnonzero(adj[0]) if v > p}
    rows = ivcheck.check_ivs(stem, 20000, 1e-2, 1e-3, relaxed_local_faithfulness=True)
    assert all(iv >= 2 for _, _, iv in rows)


def duplicated_trait_stem(d):
    """the p6 skeleton with trait 4 made an exact copy of trait 1: the conditioning set of every other outcome is singular"""
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    from cigwas_amd import ivcheck

    adj, corr, p, _ = ivcheck.load(materialise("p6", d))
    corr[4, :], corr[:, 4] = corr[1, :].copy(), corr[:, 1].copy()
    corr[1, 4] = corr[4, 1] = corr[4, 4] = 1.0
    stem = os.path.join(str(d), "dup")
    mmwrite(stem + "_sam.mtx", coo_matrix(adj.astype(np.int32)))
    mmwrite(stem + "_scm.mtx", coo_matrix(corr))
    with open(stem + ".mdim", "w") as f:
        f.write(f"{corr.shape[0]}\t{p}\t3\n")
    return stem


def test_singular_set_raises_and_names_the_outcome(tmp_path):
    from cigwas_amd import ivcheck

    stem = duplicated_trait_stem(tmp_path)
    with pytest.raises(ivcheck.SingularSetError, match=r"outcome trait 1 \(1-based\)"):  # the first outcome whose set holds both
        ivcheck.check_ivs(stem, 20000, 1e-4, 1e-3, relaxed_local_faithfulness=True)
    _, corr, p, _ = ivcheck.load(stem)
    assert ivcheck.exactly_singular(corr[np.ix_([1, 2, 4], [1, 2, 4])])
    assert not ivcheck.exactly_singular(corr[np.ix_([0, 1, 2, 3], [0, 1, 2, 3])])
    assert not ivcheck.exactly_singular(np.array([[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]]))  # indefinite, regular


# ---- CSV ----
def test_csv_text(tmp_path):
    from cigwas_amd import ivcheck

    path = os.path.join(str(tmp_path), "t.csv")
    ivcheck.write_csv(path, [(1, 2, 3), (np.int64(1), np.int32(2), 17), (2, 1, 4)])
    assert open(path).read() == "Exposure,Outcome,IV\n1,2,3\n1,2,17\n2,1,4\n"
    ivcheck.write_csv(path, [])
    assert open(path).read() == "Exposure,Outcome,IV\n"  # the reference's empty frame has no columns; the header is kept here
    # row order: exposure outer, outcome inner, ascending IV inside a pair
    stem = materialise("p6", tmp_path)
    rows = ivcheck.iv_candidates(stem)
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    import pandas as pd

    ivcheck.write_csv(path, rows)
    ref_path = os.path.join(str(tmp_path), "pandas.csv")
    pd.DataFrame([{"Exposure": e, "Outcome": o, "IV": v} for e, o, v in rows]).to_csv(ref_path, index=False)
    assert open(path).read() == open(ref_path).read()


# ---- command line ----
def test_cli_argument_rules(tmp_path):
    from cigwas_amd import cli

    parser = cli.build_parser()
    a = parser.parse_args(["iv-candidates", "out/stem"])
    assert a.cusk_output_stem == "out/stem" and a.func is cli.run_iv_candidates
    a = parser.parse_args(["check-ivs", "out/stem", "1000", "--accept-alpha", "0.01", "--reject-alpha", "1e-3"])
    assert (a.cusk_output_stem, a.num_samples, a.accept_alpha, a.reject_alpha) == ("out/stem", 1000, 0.01, 1e-3)
    assert not (a.relaxed_local_faithfulness or a.check_reverse_causality or a.het) and a.out is None
    a = parser.parse_args(["check-ivs", "s", "5", "--accept-alpha", "0.5", "--reject-alpha", "0.5", "--het", "--out", "x.csv",
                           "--relaxed-local-faithfulness", "--check-reverse-causality"])
    assert a.relaxed_local_faithfulness and a.check_reverse_causality and a.het and a.out == "x.csv"
    for bad in (["check-ivs", "s", "1000", "--accept-alpha", "0.01"],  # both alphas are required
                ["check-ivs", "s", "1000", "--reject-alpha", "0.01"],
                ["check-ivs", "s", "0", "--accept-alpha", "0.01", "--reject-alpha", "0.01"],
                ["check-ivs", "s", "1000", "--accept-alpha", "1.5", "--reject-alpha", "0.01"],
                ["check-ivs", "s", "1000", "--accept-alpha", "0.1", "--reject-alpha", "-0.01"],
                ["check-ivs", "s", "--accept-alpha", "0.1", "--reject-alpha", "0.01"],
                ["iv-candidates"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    # iv-candidates needs no device
    stem = materialise("p6", tmp_path)
    cli.main(["iv-candidates", stem])
    lines = open(stem + "_iv_candidates.csv").read().splitlines()
    assert lines[0] == "Exposure,Outcome,IV"
    assert [tuple(int(v) for v in ln.split(",")) for ln in lines[1:]] == candidates_of("p6")


def test_het_without_sizes_names_the_file(tmp_path):
    from cigwas_amd import cli, ivcheck

    stem = materialise("p6", tmp_path)
    with pytest.raises(FileNotFoundError, match=re.escape(stem + "_ssz.mtx")):
        ivcheck.check_ivs(stem, 1000, 0.01, 0.01, het=True)
    with pytest.raises(FileNotFoundError, match=re.escape(stem + "_ssz.mtx")):  # raised before any engine exists
        cli.main(["check-ivs", stem, "1000", "--accept-alpha", "0.01", "--reject-alpha", "0.01", "--het"])
    assert not os.path.exists(stem + "_ivs.csv")


# ---- het ----
@pytest.mark.parametrize("name", CASES)
def test_het_host_form_at_uniform_sizes_equals_the_reference_rows(name, tmp_path):
    from cigwas_amd import ivcheck

    case = load_kat()[name]
    stem = materialise(name, tmp_path)
    n = case["traits"] + case["markers"]
    write_ssz(stem, np.full((n, n), case["num_samples"]))
    for key, relaxed, reverse in flag_sets(case):
        rows = ivcheck.check_ivs(stem, 0, case["accept_alpha"], case["reject_alpha"], relaxed_local_faithfulness=relaxed,
                                 check_reverse_causality=reverse, het=True)  # num_samples is not used
        assert rows == rows_of(name, key), key


HET_CASE, HET_QUARTER = "p6", 2


def test_het_host_form_agrees_with_the_oracle_and_the_flag_matters(tmp_path):
    from scipy.stats import norm

    from cigwas_amd import ivcheck

    case, t = load_kat()[HET_CASE], load_tests(HET_CASE)
    stem = materialise(HET_CASE, tmp_path)
    tc = trait_corr_of(HET_CASE, tmp_path)
    n, p, N = tc.shape[0], case["traits"], case["num_samples"]
    ssz = trait_sizes(n, p, N, HET_QUARTER)
    tn = ssz[:, :p]
    for alpha in (case["accept_alpha"], case["reject_alpha"]):
        q = norm.ppf(1 - alpha / 2)
        z, flags, _ = ivcheck.HostEngine().iv_check_het(tc, t["set_off"], t["sets"], t["x"], t["y"], t["set"], tn, q)
        zo, thr = het_oracle(tc, tn, t["set_off"], t["sets"], t["x"], t["y"], t["set"], q)
        assert np.min(np.abs(zo - thr)) > 1e3 * max(case["d"], 1e-15)  # a condition on these inputs: no verdict hangs on the last bits
        assert np.max(np.abs(z - zo)) <= 10 * max(case["d"], 1e-15)
        assert np.allclose(ivcheck.het_thresholds(tn, t["set_off"], t["sets"], t["x"], t["y"], t["set"], q), thr, rtol=1e-15, atol=0)
        assert np.array_equal(flags, (zo < thr).astype(np.int32))
    write_ssz(stem, ssz)
    changed = 0
    for key, relaxed, reverse in flag_sets(case):
        rows = ivcheck.check_ivs(stem, 0, case["accept_alpha"], case["reject_alpha"], relaxed_local_faithfulness=relaxed,
                                 check_reverse_causality=reverse, het=True)
        changed += rows != rows_of(HET_CASE, key)
    assert changed >= 1
