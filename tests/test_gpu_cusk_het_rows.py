"""GPU: engine option het_rows -- level 1 of cusk_run_skeleton_het / cusk_run_skeleton_batch_het on the HET forms of the
row-streaming kernel (level1_rows2_kernel<0, V, T, LDSROW, true>).

With the option the adjacency, the level counter, the separating-set records, pMax and the canonical test counts of
levels 0 and 1 must be those of the run without it (the exact sweep), and adjacency and level those of the oracle's
hetcor_skeleton; cusk_engine_level1_form tells the row-kernel run from a fall-back.  tests/test_cusk_het_rows_formats.py
checks the filter's band on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cusk_het import B_ALPHA, B_DEPTH, B_L1, B_L2, B_SIZES, MPS
from test_gpu_cusk_het_filter import _run, _same_files, _same_result, dataset  # noqa: F401  (dataset: the het files)
from test_het_class_cases import ML, deep_case, deep_graphs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 1e-4


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


def _oracle(oracle, Cm, Nm, th, level):
    n = Cm.shape[0]
    return oracle.hetcor_skeleton(Cm, np.ones((n, n), np.int32), Nm, th, level, np.zeros(n, np.int32))


def _pair(cg, Cm, Nm, th, levels, opts=(), before=None, c_offset=0):
    """-> (run with het_rows = 0, run with het_rows = 1 and `opts`, level1_form of the second) on one engine"""
    n = Cm.shape[0]
    e = cg.Engine(0)
    if c_offset:
        flat = np.zeros(n * n + c_offset, np.float32)
        flat[c_offset:] = Cm.reshape(-1)
        Cd = cg.DeviceArray(flat)
    else:
        Cd = cg.DeviceArray(Cm)
    Nd = cg.DeviceArray(Nm)

    class P:  # the matrix as the engine sees it
        ptr = Cd.ptr + 4 * c_offset

    try:
        base = _run(cg, e, P, Nd, n, th, levels)
        assert e.level1_form() == (0 if levels >= 1 else -1)
        e.set_option("het_rows", 1)
        for k, v in opts:
            e.set_option(k, v)
        if before:
            before(e)
        got = _run(cg, e, P, Nd, n, th, levels)
        form = e.level1_form()
    finally:
        Cd.free()
        Nd.free()
        e.close()
    return base, got, form


def _same(got, base):
    _same_result(got, base)
    assert list(got["st"].canonical_tests[:2]) == list(base["st"].canonical_tests[:2])
    assert got["st"].removed[1] == base["st"].removed[1]


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the forms on the star case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(cg, oracle, synth):
    """level1_star_case (n = 1,301) with a symmetric size matrix that differs by pair: two trait columns at 25 % and 60 %
    of N, the rest at N, NaN on the diagonal; the oracle's graph after level 1"""
    Cm, info = synth.level1_star_case()
    n = Cm.shape[0]
    N = float(info["N"])
    Nm = np.full((n, n), N, np.float32)
    for col, share in ((n - 2, 0.25), (n - 1, 0.60)):
        Nm[:, col] = Nm[col, :] = np.floor(share * N)
    np.fill_diagonal(Nm, np.nan)
    th = cg.hetcor_threshold(info["alpha"])
    return dict(C=Cm, N=Nm, n=n, th=th, ref=_oracle(oracle, Cm, Nm, th, 1))


FORM_OF = {(0, 1): 2, (256, 1): 2, (512, 1): 3, (0, 0): 4, (256, 0): 4, (512, 0): 4}


@pytest.mark.parametrize("validate", (0, 1))
@pytest.mark.parametrize("lds", (1, 0))
@pytest.mark.parametrize("threads", (0, 256, 512))
def test_forms_give_the_exact_het_run(cg, star, threads, lds, validate):
    opts = [("l1_threads", threads), ("l1_lds_row", lds)]
    if validate:
        opts += [("het_filter", 1), ("validate", 1)]
    base, got, form = _pair(cg, star["C"], star["N"], star["th"], 1, opts)
    st = got["st"]
    print(f"threads {threads} lds {lds} validate {validate}: form {form}, tests {list(st.tests[:2])}, removed {st.removed[1]}, "
          f"violations {st.violations}, sent to the exact form {st.rechecks[1]} ({st.rechecks[1] / st.tests[1]:.2e})")
    assert base["st"].rechecks[1] == 0 and base["st"].subsets[1] > 0 and st.subsets[1] == 0 and st.rechecks[1] < st.tests[1] // 100
    assert form == FORM_OF[(threads, lds)]
    _same(got, base)
    assert st.level == star["ref"].level and np.array_equal(got["G"], star["ref"].G)
    assert st.removed[1] > 0 and st.violations == 0


def test_misaligned_matrix_runs_the_gather_form(cg, star):
    base, got, form = _pair(cg, star["C"], star["N"], star["th"], 1, c_offset=1)
    assert form == 4
    _same(got, base)
    assert np.array_equal(got["G"], star["ref"].G)


# ---------------------------------------------------------------------------------------------------------------------
# 3: small shapes where segments go wrong
# ---------------------------------------------------------------------------------------------------------------------
def _small_case(synth, n, seed):
    """sample correlations of a synthetic LD block of n - 5 markers and 5 traits (level 1 removes most of what level 0
    keeps) and symmetric sizes; variable 0 is tied to the last variable alone (a row of degree 1), and the last variable's
    neighbours all precede it"""
    Cm = synth.synth_corr_block(n - 5, 5, N=4096, block_index=seed).astype(np.float32).copy()
    Cm[0, :] = Cm[:, 0] = 0.0
    Cm[0, n - 1] = Cm[n - 1, 0] = 0.3
    np.fill_diagonal(Cm, 1.0)
    Nm = synth.het_sizes(n, seed, 4096.0, lo=0.25)
    return np.ascontiguousarray(Cm), Nm


@pytest.mark.parametrize("n", (63, 65, 257))
def test_small_shapes(cg, oracle, synth, n):
    Cm, Nm = _small_case(synth, n, 100 + n)
    th = cg.hetcor_threshold(ALPHA)
    g0 = _oracle(oracle, Cm, Nm, th, 0).G
    deg = g0.sum(1)
    # segment of neighbour X of row ya: the positions behind ya in X's list
    odd = sum(1 for ya in range(n) for X in np.flatnonzero(g0[ya]) if int(g0[X, ya + 1:].sum()) % 2 == 1)
    print(f"n {n}: degrees min {deg.min()} max {deg.max()}, rows of degree 1: {int((deg == 1).sum())}, odd segments {odd}, "
          f"last row's degree {deg[n - 1]}")
    assert (deg == 1).sum() >= 1 and odd > 0 and deg[n - 1] >= 1 and g0[n - 1, :n - 1].sum() == deg[n - 1]
    ref = _oracle(oracle, Cm, Nm, th, 1)
    for opts in ([], [("l1_lds_row", 0)], [("l1_threads", 512)]):
        base, got, form = _pair(cg, Cm, Nm, th, 1, opts)
        assert form in (2, 3, 4)
        _same(got, base)
        assert np.array_equal(got["G"], ref.G) and got["st"].level == ref.level


# ---------------------------------------------------------------------------------------------------------------------
# 4: unusual sizes
# ---------------------------------------------------------------------------------------------------------------------
QUIET = tuple(range(10, 18))  # variables of the 3-4-5 case whose every pair has no usable size


def unusual_case(synth, values):
    """_small_case(65) with `values` scattered over the size matrix (symmetric).  The 3-4-5 case also has the eight QUIET
    variables: every pair that touches one has size NaN or 2 (alternating), which level 0 cannot judge (NaN or negative
    radicand: the edge stays), so level 1 meets triples whose mean size is below 4 on edges that are still there -- among
    them the triples (X quiet; ya, yb) whose N[ya, yb] is one of 3 / 4 / 5."""
    n = 65
    Cm, Nm = _small_case(synth, n, 7)
    rng = np.random.default_rng(3)
    iu = np.triu_indices(n, 1)
    pick = rng.integers(0, len(values), len(iu[0]))
    unusual = rng.uniform(size=len(iu[0])) < (0.5 if len(values) > 1 else 0.1)
    vals = np.where(unusual, np.array(values, np.float32)[pick], Nm[iu])
    if values[0] == 3.0:
        quiet = np.isin(iu[0], QUIET) | np.isin(iu[1], QUIET)
        vals = np.where(quiet, np.where((iu[0] + iu[1]) % 2 == 0, np.float32(np.nan), np.float32(2.0)), vals)
    Nm[iu] = vals
    Nm.T[iu] = vals
    return Cm, Nm


def level1_radicands(g0, Nm):
    """over the level-1 tests of the graph g0 (X, unordered neighbours ya < yb: two tests each): (tests, tests whose
    radicand me - 4 is negative, i.e. whose threshold is NaN, those of them with N[ya, yb] in {3, 4, 5}), in the kernels'
    arithmetic: int-truncated sizes (NaN -> 0), float sum, float division by 3"""
    with np.errstate(invalid="ignore"):
        Ni = np.nan_to_num(np.trunc(Nm), nan=0.0).astype(np.float32)
    tests = nan_th = nan_345 = 0
    for X in range(g0.shape[0]):
        nb = np.flatnonzero(g0[X])
        if len(nb) < 2:
            continue
        a, b = np.triu_indices(len(nb), 1)
        ya, yb = nb[a], nb[b]
        s = np.float32(Ni[X, ya] + Ni[X, yb]) + Ni[ya, yb]
        neg = (s / np.float32(3.0)).astype(np.float64) - 4.0 < 0.0
        tests += 2 * len(a)
        nan_th += 2 * int(neg.sum())
        nan_345 += 2 * int((neg & np.isin(Nm[ya, yb], (3.0, 4.0, 5.0))).sum())
    return tests, nan_th, nan_345


@pytest.mark.parametrize("values", ([3.0, 4.0, 5.0], [np.nan], [8388607.0, 8388609.0, 10000000.0]), ids=("3-4-5", "nan", "2^23"))
def test_unusual_sizes(cg, oracle, synth, values):
    """realised (CPU oracle's level-0 graph): 3-4-5: 45,162 level-1 tests, 22,984 with a NaN threshold, 13,072 of those
    with N[ya, yb] in {3, 4, 5}, and the 28 edges among the quiet variables, all of whose tests have a NaN threshold, stay;
    nan: 32,250 tests, 264 with a NaN threshold; 2^23: none"""
    Cm, Nm = unusual_case(synth, values)
    th = cg.hetcor_threshold(ALPHA)
    g0 = _oracle(oracle, Cm, Nm, th, 0).G
    tests, nan_th, nan_345 = level1_radicands(g0, Nm)
    print(f"{tests} level-1 tests, {nan_th} with a NaN threshold, {nan_345} of those with N[ya, yb] in 3 / 4 / 5")
    ref = _oracle(oracle, Cm, Nm, th, 1)
    base, got, form = _pair(cg, Cm, Nm, th, 1)
    assert form in (2, 3)
    _same(got, base)
    assert np.array_equal(got["G"], ref.G) and got["st"].level == ref.level
    assert got["st"].removed[1] > 0
    if values[0] == 3.0:
        assert nan_th > 1000 and nan_345 > 1000
        # every test of an edge between two quiet variables has three sizes of at most 2: NaN threshold, the edge stays
        q = np.array(QUIET)
        sub = np.ix_(q, q)
        off = ~np.eye(len(q), dtype=bool)
        assert np.all(g0[sub][off] == 1) and np.all(got["G"][sub][off] == 1)
        print(f"{int(off.sum()) // 2} edges among the quiet variables have NaN thresholds only and stay")
    elif np.isnan(values[0]):
        assert nan_th > 0
    # the tests with a NaN threshold are among those the filter hands to the exact form
    assert got["st"].rechecks[1] >= nan_th and got["st"].subsets[1] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5: fall-backs
# ---------------------------------------------------------------------------------------------------------------------
def test_fall_backs(cg, star):
    Cm, Nm, th = star["C"], star["N"], star["th"]
    asym = Nm.copy()
    asym[5, 9] = asym[5, 9] - 1.0
    base, got, form = _pair(cg, Cm, asym, th, 1)
    assert form == 0
    _same(got, base)
    for key in ("fast", "rows", "pair"):
        base, got, form = _pair(cg, Cm, Nm, th, 1, [(key, 0)])
        assert form == 0, key
        _same(got, base)
        assert np.array_equal(got["G"], star["ref"].G)
    n = star["n"]
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        Th = cg.threshold_array(4096, ALPHA)
        a = e.run_skeleton(Cd.ptr, n, Th, 1)
        Ga, fa = e.adjacency_bits(), e.level1_form()
        e.set_option("het_rows", 1)
        b = e.run_skeleton(Cd.ptr, n, Th, 1)
        assert fa == e.level1_form() and fa in (2, 3) and np.array_equal(Ga, e.adjacency_bits()) and list(a.tests[:2]) == list(b.tests[:2])
        e.set_option("validate", 1)
        with pytest.raises(RuntimeError, match="validate"):
            e.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, 1)
        e.set_option("validate", 0)
        e.set_row_shard(0, 2, exchange=lambda *a: 0)
        with pytest.raises(RuntimeError, match="row-sharded"):
            e.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, 1)
        with pytest.raises(RuntimeError, match="unknown option het_rows"):
            e.set_option("het_rows", 2)
    finally:
        Cd.free()
        Nd.free()
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6: batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("het_filter", (0, 1))
def test_batch_is_the_single_block_run_per_block(cg, synth, het_filter):
    spans, maxlevel = (70, 257, 130), 3
    th = cg.hetcor_threshold(ALPHA)
    mats = [_small_case(synth, k, 40 + k) for k in spans]
    e = cg.Engine(0)
    singles = []
    try:
        for Cm, Nm in mats:
            Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
            singles.append(_run(cg, e, Cd, Nd, Cm.shape[0], th, maxlevel))
            assert e.level1_form() == 0
            Cd.free()
            Nd.free()
        e.set_option("het_rows", 1)
        e.set_option("het_filter", het_filter)
        lo, pos = [], 0
        for k in spans:
            lo.append(pos)
            pos += (k + 63) // 64 * 64
        hi = [a + k for a, k in zip(lo, spans)]
        n = pos + 64
        big = np.full((n, n), np.nan, np.float32)
        bigN = np.full((n, n), 2.0, np.float32)
        bigN[np.triu_indices(n, 1)] = 3.0  # asymmetric outside the blocks: the symmetry kernel does not look there
        for (Cm, Nm), a, b in zip(mats, lo, hi):
            big[a:b, a:b], bigN[a:b, a:b] = Cm, Nm
        Cd, Nd = cg.DeviceArray(big), cg.DeviceArray(bigN)
        st = e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, n, lo, hi, th, maxlevel)
        form = e.level1_form()
        Gs = e.adjacency_blocks()
        x, y, lv, z, S = e.sepsets()
        Cd.free()
        Nd.free()
    finally:
        e.close()
    assert form in (2, 3, 4) and st.removed[1] > 0
    for a, b, G, one in zip(lo, hi, Gs, singles):
        assert np.array_equal(G, one["G"])
        sel = (x >= a) & (x < b)
        x1, y1, lv1, _z1, S1 = one["rec"]
        assert len(x1) > 0
        assert np.array_equal(x[sel] - a, x1) and np.array_equal(y[sel] - a, y1) and np.array_equal(lv[sel], lv1)
        assert np.array_equal(np.where(S[sel] >= 0, S[sel] - a, -1), S1)


# ---------------------------------------------------------------------------------------------------------------------
# 7: deep run
# ---------------------------------------------------------------------------------------------------------------------
def test_deep_run_to_level_14(cg):
    c = deep_case()
    G, level = deep_graphs("sym")
    base, got, form = _pair(cg, c["C"], c["N"]["sym"], c["th"], ML, [("het_filter", 1), ("validate", 1)])
    assert form in (2, 3)
    _same(got, base)
    assert got["st"].violations == 0 and got["st"].level == level and np.array_equal(got["G"], G[ML])


# ---------------------------------------------------------------------------------------------------------------------
# 8: files
# ---------------------------------------------------------------------------------------------------------------------
def test_blockset_set_het_rows_writes_the_het_files(cg, dataset, tmp_path):  # noqa: F811
    import cigwas_amd._lib as L
    from cigwas_amd import run_blocks as rb

    e = cg.Engine(0)
    bs = rb.BlockSet(dataset["gaps"], dataset["stem"], dataset["blocks"], float(B_ALPHA), int(B_L1), int(B_L2), int(B_DEPTH))
    bs.set_het(True)
    bs.set_het_rows(True)
    forms = []
    for b in range(len(B_SIZES)):
        res, st = bs.run_block(e, b)
        forms.append(e.level1_form())
        if res is not None:
            res.write(str(tmp_path))
    L.lib().cusk_blockset_release_engine(bs.h, e.h)
    bs.close()
    e.close()
    _same_files(str(dataset["want"]), str(tmp_path))
    assert any(f in (2, 3, 4) for f in forms), forms  # the option reached the engine


def test_mps_cusk_het_filter_rows_writes_the_het_files(dataset, tmp_path):  # noqa: F811
    for b in range(len(B_SIZES)):
        argv = [MPS, "cusk", dataset["gaps"], dataset["stem"], dataset["blocks"], B_ALPHA, B_L1, B_L2, B_DEPTH, str(tmp_path), str(b),
                "het", "filter", "rows"]
        r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, CUSK_OPTIONS="validate=1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "level 1 on the row kernel" in r.stdout
        # the option reached the engine: stage one's level 1 formed no conditioning sets
        assert "het rows: stage 1 level 1 on the row kernel" in r.stdout, r.stdout[-2000:]
    _same_files(str(dataset["want"]), str(tmp_path))


def test_run_blocks_het_batch_vars_filter_rows_writes_the_het_files(dataset, tmp_path):  # noqa: F811
    cmd = [sys.executable, os.path.join(ROOT, "ci-gwas_amd", "run_blocks.py"), dataset["gaps"], dataset["stem"], dataset["blocks"],
           B_ALPHA, B_L1, B_L2, B_DEPTH, str(tmp_path), "--het-batch-vars", "256", "--het-filter", "--het-rows", "--writer", "local"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["CUSK_OPTIONS"] = "validate=1"
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _same_files(str(dataset["want"]), str(tmp_path))
    # the option reached the engines of the batches: every stage-one run had its level 1 on the row kernel
    import re

    m = re.search(r"het rows: level 1 on the row kernel in (\d+) of (\d+) stage-one", r.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) > 0, r.stdout[-2000:]
