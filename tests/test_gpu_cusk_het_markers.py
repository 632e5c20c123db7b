"""GPU: per-pair sample sizes between markers -- cusk_marker_pair_sizes / _batch against the numpy restatement of
test_cusk_het_markers_formats.py (bitwise), the engine on the size matrix they complete against the oracle, and the flag
through `mps cusk ... het markers`, the block set, run_blocks.py and `cuskss-merged --bfiles --het --het-markers`.

The data set (`array_dataset`) has the two-array pattern: every third marker is genotyped on one 30 % of the individuals,
the others on 80 %, the two sets sharing 10 %; two traits have gaps.  Its seed was chosen on the CPU (oracle only, the
correlations from the oracle's restatement of the build) so that the premises asserted below hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cusk_het_formats import ess_square_expected
from test_cusk_het_markers_formats import marker_pair_counts
from test_gpu_cusk_het import EXTS, ML, MPS, _dense, _same_files, prefilter_het

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


@pytest.fixture(scope="module")
def eng(cg):
    e = cg.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the count kernel
# ---------------------------------------------------------------------------------------------------------------------
RATES = (0.0, 0.001, 0.1, 0.9, 1.0)


def count_case(k, N, seed):
    """.bed rows of 2 k + 3 markers x N individuals, marker i missing at rate RATES[(i + seed) % 5] (from k = 5 on every
    case holds a wholly missing marker, with it pairs of count 0); random bits where the last byte holds no individual"""
    rng = np.random.default_rng(1000 * k + N + seed)
    mt = 2 * k + 3
    clb = (N + 3) // 4
    codes = rng.choice(np.array([0, 2, 3], np.uint8), (mt, 4 * clb))
    for i in range(mt):
        codes[i, rng.random(4 * clb) < RATES[(i + seed) % 5]] = 1
    codes[:, N:] = rng.integers(0, 4, (mt, 4 * clb - N))
    bed = (codes[:, 0::4] | (codes[:, 1::4] << 2) | (codes[:, 2::4] << 4) | (codes[:, 3::4] << 6)).astype(np.uint8)
    ix = np.sort(rng.choice(mt, k, replace=False)).astype(np.int32)
    return bed, ix


def _poisoned(bed):
    """the rows, one byte of slack in front (rows then start at every residue of 16) and 64 bytes of 0x55 -- all codes
    `missing` -- behind the last"""
    flat = np.full(1 + bed.size + 64, 0x55, np.uint8)
    flat[1:1 + bed.size] = bed.reshape(-1)
    return flat


def _run_single(cg, eng, flat, on_device, ix, k, m_total, N, ld):
    """-> ld x ld float32: cusk_marker_pair_sizes over a matrix of sentinels; the rows start one byte into `flat`"""
    import ctypes as C

    from cigwas_amd._lib import lib

    out = cg.DeviceArray(np.full((ld, ld), SENTINEL, np.float32))
    dev = cg.DeviceArray(flat) if on_device else None
    bed_p = dev.ptr + 1 if on_device else flat.ctypes.data + 1
    ix_p = ix.ctypes.data_as(C.c_void_p) if ix is not None else None
    eng._check(lib().cusk_marker_pair_sizes(eng.h, bed_p, ix_p, k, m_total, N, out.ptr, ld))
    got = out.download(np.float32, (ld, ld))
    out.free()
    if dev is not None:
        dev.free()
    return got


@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130])
def test_counts_are_the_numpy_restatement_bitwise(cg, eng, k, N):
    bed, ix = count_case(k, N, seed=k + N)
    mt = bed.shape[0]
    ld = k + 3
    for rows, sel in ((ix, ix), (None, np.arange(k))):
        src = bed if rows is not None else bed[:k]  # NULL: the poison follows row k - 1
        want = marker_pair_counts(bed[sel], N)
        assert want.max() <= N and (k < 5 or want.min() == 0)
        flat = _poisoned(src)
        for on_device in (False, True):
            got = _run_single(cg, eng, flat, on_device, rows, k, src.shape[0], N, ld)
            assert np.array_equal(got[:k, :k].view(np.uint32), want.astype(np.float32).view(np.uint32)), (rows is None, on_device)
            assert np.array_equal(got[:k, :k].view(np.uint32), got[:k, :k].T.view(np.uint32))
            assert np.all(got[k:, :] == SENTINEL) and np.all(got[:, k:] == SENTINEL)
    assert mt == 2 * k + 3


def test_argument_errors_have_messages(cg, eng):
    bed = np.zeros((4, 1), np.uint8)
    out = cg.DeviceArray(np.zeros((4, 4), np.float32))
    with pytest.raises(RuntimeError, match="2\\^24"):
        eng.marker_pair_sizes(bed, 1 << 24, out.ptr, 4, k=4, m_total=4)
    with pytest.raises(RuntimeError, match="ascending"):
        eng.marker_pair_sizes(bed, 4, out.ptr, 4, marker_ix=[2, 1])
    with pytest.raises(RuntimeError, match="multiples of 64"):
        eng.marker_pair_sizes_batch(bed, 4, [2, 2], [0, 32], 128, out.ptr)
    eng.marker_pair_sizes(bed, 4, out.ptr, 4)
    assert np.all(out.download(np.float32, (4, 4)) == 4.0)
    out.free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the batch form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_batch_blocks_are_the_single_block_calls(cg, eng, on_device):
    """three blocks of 5 / 64 / 70 markers and 3 traits at bases 0 / 64 / 192 of a 320 x 320 allocation, the 70-marker block
    named a second time at base 320 of a 448 x 448 one"""
    N, p = 517, 3
    bed, _ = count_case(80, N, seed=3)
    rng = np.random.default_rng(5)
    lists = [np.sort(rng.choice(bed.shape[0], mb, replace=False)).astype(np.int32) for mb in (5, 64, 70)]
    lists.append(lists[2])
    m, base, n = [5, 64, 70, 70], [0, 64, 192, 320], 448
    assert all(b % 64 == 0 and b + mb + p <= nb for b, mb, nb in zip(base, m, base[1:] + [n]))
    src = cg.DeviceArray(bed) if on_device else bed
    out = cg.DeviceArray(np.full((n, n), SENTINEL, np.float32))
    eng.marker_pair_sizes_batch(src, N, m, base, n, out.ptr, marker_ix=np.concatenate(lists), m_total=bed.shape[0])
    got = out.download(np.float32, (n, n))
    out.free()
    inside = np.zeros((n, n), bool)
    for b, mb, ix in zip(base, m, lists):
        one = cg.DeviceArray(np.zeros((mb, mb), np.float32))
        eng.marker_pair_sizes(src, N, one.ptr, mb, marker_ix=ix, m_total=bed.shape[0])
        single = one.download(np.float32, (mb, mb))
        one.free()
        assert np.array_equal(single, marker_pair_counts(bed[ix], N).astype(np.float32))
        assert np.array_equal(got[b:b + mb, b:b + mb].view(np.uint32), single.view(np.uint32))
        inside[b:b + mb, b:b + mb] = True
    assert np.all(got[~inside] == SENTINEL)
    assert np.array_equal(got[192:262, 192:262], got[320:390, 320:390])
    if on_device:
        src.free()


# ---------------------------------------------------------------------------------------------------------------------
# the data set of 3. - 6.
# ---------------------------------------------------------------------------------------------------------------------
A_N, A_P = 2000, 4
A_SIZES = [40, 40, 40]
A_ALPHA, A_L1, A_L2, A_DEPTH = "0.0001", "3", "6", "1"
PLANT_A, PLANT_B = 4, 7   # two markers of the small array, block 0
DATA_SEED = 11   # chosen among seeds 0-39 on the CPU, see test_the_flag_matters and test 3


def array_dataset(synth, seed=DATA_SEED):
    """-> G (120 x 2000 int8, -1 = missing), Yg (4 x 2000 float32 with NaN).  Markers i % 3 == 1 are genotyped on the small
    array (individuals of rank 1,400 - 1,999 of a permutation), the others on the big one (rank 0 - 1,599): 600 common
    individuals inside the small array, 200 across the arrays, none of the pairs without any.  PLANT_B repeats PLANT_A on
    eight individuals in a hundred, and both act on trait 0, so both stay in the block's result."""
    N, p, m = A_N, A_P, sum(A_SIZES)
    rng = synth.rng_for(9500 + seed)
    G = synth.make_genotypes(m, N, rng, window=10, rho=0.6, miss=0.0)
    fresh = rng.binomial(2, 0.4, (2, N)).astype(np.int8)
    G[PLANT_A] = fresh[0]
    G[PLANT_B] = np.where(rng.random(N) < 0.08, fresh[0], fresh[1])
    g = G.astype(np.float64)
    gs = (g - g.mean(1, keepdims=True)) / g.std(1, keepdims=True)
    Y = rng.standard_normal((p, N))
    Y[0] += 0.40 * gs[PLANT_A] - 0.40 * gs[PLANT_B] + 0.30 * gs[50]
    Y[1] += 0.30 * gs[20] - 0.30 * gs[95]
    Y[2] += 0.30 * gs[62] + 0.25 * Y[0]
    Y[3] += 0.32 * gs[110] - 0.30 * gs[30]
    Y = ((Y - Y.mean(1, keepdims=True)) / Y.std(1, keepdims=True)).astype(np.float32)
    rank = rng.permutation(N)
    small, big = rank >= 1400, rank < 1600
    for i in range(m):
        G[i, ~(small if i % 3 == 1 else big)] = -1
    Y[1, rng.permutation(N)[int(0.5 * N):]] = np.nan
    Y[3, rng.permutation(N)[int(0.7 * N):]] = np.nan
    return G, Y


def size_matrix(mxp_ess, pxp_ess, counts, m, p, N):
    """cusk_ess_square, then the marker x marker counts over its corner (None: N stays there)"""
    S = ess_square_expected(mxp_ess, pxp_ess, m, p, float(N))
    if counts is not None:
        S[:m, :m] = counts.astype(np.float32)
    return S


def oracle_levels(oracle, C, Nsz, th, maxlevel):
    n = C.shape[0]
    ones, ti = np.ones((n, n), np.int32), np.zeros(n, np.int32)
    return [oracle.hetcor_skeleton(C, ones, Nsz, th, l, ti).G for l in range(maxlevel + 1)]


def pair_premise(C, counts, N, q, a, b):
    """|z| sqrt(size - 3) / q of the pair at N and at its own count"""
    z = abs(float(np.arctanh(np.float64(C[a, b]))))
    return z * np.sqrt(N - 3.0) / q, z * np.sqrt(float(counts[a, b]) - 3.0) / q


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, synth):
    d = tmp_path_factory.mktemp("cusk_het_markers")
    G, Yg = array_dataset(synth)
    means, stds = synth.bed_stats(G)
    stem = str(d / "geno")
    bed = synth.pack_bed(G)
    synth.write_bfiles(stem, bed, A_N, means, stds)
    synth.write_phen(str(d / "gaps.phen"), Yg.reshape(-1), A_N, A_P)
    bounds, first = [], 0
    with open(d / "b.blocks", "w") as f:
        for s in A_SIZES:
            f.write(f"1\t{first}\t{first + s - 1}\n")
            bounds.append((first, first + s - 1))
            first += s
    return dict(dir=d, stem=stem, gaps=str(d / "gaps.phen"), blocks=str(d / "b.blocks"), bounds=bounds, G=G, Yg=Yg, bed=bed,
                means=means, stds=stds)


def block_inputs(cg, eng, ds, f, l):
    """correlations (device + host), the m x p and p x p sizes of the het chain, and the numpy counts of markers f .. l"""
    N, p = A_N, A_P
    mb = l - f + 1
    n = mb + p
    sel = slice(f, l + 1)
    ess_of = lambda r, c: np.float32(np.nan) if np.isnan(r) else np.float32(cg.ess_from_se(float(r), cg.se_from_count(float(r), int(c))))
    Cd = cg.DeviceArray(nbytes=4 * n * n)
    mxp = eng.corr_build(ds["bed"][sel], ds["Yg"], mb, N, p, ds["means"][sel], ds["stds"][sel], Cd.ptr, want_mxp=True).reshape(mb, p)
    sq = Cd.download(np.float32, (n, n))
    mxp_n, pxp_n = eng.pair_counts(ds["bed"][sel], ds["Yg"], N, p)
    mxp_ess = np.array([[ess_of(mxp[i, t], mxp_n[i, t]) for t in range(p)] for i in range(mb)], np.float32)
    pxp_ess = np.full((p, p), np.nan, np.float32)
    for a in range(p):
        for c in range(a + 1, p):
            pxp_ess[a, c] = pxp_ess[c, a] = ess_of(sq[mb + a, mb + c], pxp_n[a, c])
    return Cd, sq, mxp, mxp_ess, pxp_ess, marker_pair_counts(ds["bed"][sel], N)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the engine on the completed size matrix
# ---------------------------------------------------------------------------------------------------------------------
def test_engine_run_on_the_completed_matrix_is_the_oracles(cg, eng, oracle, dataset):
    """all 120 markers as one block + 4 traits, level 3.  Size matrix = cusk_ess_square + cusk_marker_pair_sizes."""
    ds = dataset
    m, p, N = sum(A_SIZES), A_P, A_N
    n = m + p
    th = cg.hetcor_threshold(float(A_ALPHA))
    Cd, sq, mxp, mxp_ess, pxp_ess, counts = block_inputs(cg, eng, ds, 0, m - 1)
    assert not np.isnan(sq[:m, :m]).any() and counts.min() >= 190  # no pair without common individuals, no NaN correlation
    Nd = cg.DeviceArray(nbytes=4 * n * n)
    eng.ess_square(mxp_ess, pxp_ess, m, p, float(N), Nd.ptr)
    eng.marker_pair_sizes(ds["bed"], N, Nd.ptr, n)
    Nsz = Nd.download(np.float32, (n, n))
    want = size_matrix(mxp_ess, pxp_ess, counts, m, p, N)
    assert np.array_equal(Nsz.view(np.uint32), want.view(np.uint32))
    # the premise, oracle alone: the counts remove marker-marker edges at level 0 and at a later level that N keeps
    mine = oracle_levels(oracle, sq, Nsz, th, 3)
    flat = oracle_levels(oracle, sq, size_matrix(mxp_ess, pxp_ess, None, m, p, N), th, 3)
    mm = np.zeros((n, n), bool)
    mm[:m, :m] = True
    lost0 = (flat[0] == 1) & (mine[0] == 0) & mm
    lost_later = (flat[3] == 1) & (mine[0] == 1) & (mine[3] == 0) & mm
    print(f"marker-marker edges kept at N and removed at the counts: {lost0.sum() // 2} at level 0, {lost_later.sum() // 2} at levels 1-3")
    assert lost0.sum() >= 2 and lost_later.sum() >= 2
    # exact het run
    for key in ("het_filter", "het_rows"):
        eng.set_option(key, 0)
    st = eng.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, 3)
    G, rec = eng.adjacency(), eng.sepsets()
    ref = oracle.hetcor_skeleton(sq, np.ones((n, n), np.int32), Nsz, th, 3, np.zeros(n, np.int32))
    assert np.array_equal(G, ref.G) and np.array_equal(ref.G, mine[3]) and st.level == ref.level
    # filter and row kernel: the same bytes, and the row kernel ran -- the matrix passed the device's symmetry check
    eng.set_option("het_filter", 1)
    eng.set_option("het_rows", 1)
    eng.set_option("validate", 1)
    try:
        st2 = eng.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, 3)
        form = eng.level1_form()
        G2, rec2 = eng.adjacency(), eng.sepsets()
    finally:
        for key in ("het_filter", "het_rows", "validate"):
            eng.set_option(key, 0)
    assert form in (2, 3, 4), form
    assert st2.violations == 0
    assert np.array_equal(G2, G) and all(np.array_equal(a, b) for a, b in zip(rec, rec2))
    Cd.free()
    Nd.free()


# ---------------------------------------------------------------------------------------------------------------------
# 4. - 6. files
# ---------------------------------------------------------------------------------------------------------------------
def compose(ds, cg, eng, oracle, out, het_markers):
    """every block through the steps of the het branch: numpy counts -> size matrix -> both stages (the engine's exact het
    run, its adjacency held to the oracle's hetcor_skeleton) -> the oracle's prune / reduce / write functions"""
    N, p = A_N, A_P
    th = cg.hetcor_threshold(float(A_ALPHA))
    for key in ("het_filter", "het_rows"):
        eng.set_option(key, 0)
    info = {}
    for b, (f, l) in enumerate(ds["bounds"]):
        mb = l - f + 1
        n = mb + p
        Cd, sq, mxp, mxp_ess, pxp_ess, counts = block_inputs(cg, eng, ds, f, l)
        num_sig = prefilter_het(mxp, mxp_ess, th)
        info[b] = dict(num_sig=num_sig, stem=f"1_{f}_{l}", C=sq, counts=counts)
        if num_sig == 0:
            Cd.free()
            continue
        Nsq = size_matrix(mxp_ess, pxp_ess, counts if het_markers else None, mb, p, N)
        Nd = cg.DeviceArray(Nsq)
        eng.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, int(A_L1))
        G1 = eng.adjacency()
        assert np.array_equal(G1, oracle_levels(oracle, sq, Nsq, th, int(A_L1))[-1])
        x, y, lv, z, S = eng.sepsets()
        P = oracle.subset_variables(G1, n, mb, int(A_DEPTH))
        gcs = oracle.reduce_gcs(G1, sq, _dense(n, x, y, S), P, n, p, int(A_L1))
        k = gcs.num_var
        C2, N2 = np.ascontiguousarray(gcs.C, np.float32).reshape(k, k), np.ascontiguousarray(Nsq[np.ix_(P, P)])
        C2d, N2d = cg.DeviceArray(C2), cg.DeviceArray(N2)
        eng.run_skeleton_het(C2d.ptr, N2d.ptr, k, th, int(A_L2))
        G2 = eng.adjacency()
        assert np.array_equal(G2, oracle_levels(oracle, C2, N2, th, int(A_L2))[-1])
        x, y, lv, z, S = eng.sepsets()
        P2 = oracle.subset_variables(G2, k, gcs.num_markers(), int(A_DEPTH))
        red = oracle.reduce_gcs(G2, C2, _dense(k, x, y, S), P2, k, p, ML, gcs.new_to_old)
        oracle.write_reduced(red, str(out / info[b]["stem"]), with_sep=True)
        info[b]["ixs"] = [int(v) for v in red.new_to_old]
        info[b]["adj"] = np.asarray(red.G, np.int32).reshape(len(red.new_to_old), -1)
        for a in (Cd, Nd, C2d, N2d):
            a.free()
    return dict(out=out, info=info)


@pytest.fixture(scope="module")
def composed(dataset, cg, eng, oracle, tmp_path_factory):
    return {flag: compose(dataset, cg, eng, oracle, tmp_path_factory.mktemp("composed_%d" % flag), flag) for flag in (False, True)}


def _mps_cusk(ds, out, block, words):
    os.makedirs(out, exist_ok=True)
    argv = [MPS, "cusk", ds["gaps"], ds["stem"], ds["blocks"], A_ALPHA, A_L1, A_L2, A_DEPTH, str(out), str(block)] + words
    r = subprocess.run(argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _all_kept(comp):
    files = sorted(os.listdir(comp["out"]))
    assert len(files) == 15 and {os.path.splitext(f)[1] for f in files} == set(EXTS)


def test_mps_cusk_het_markers_writes_the_composed_files(dataset, composed, tmp_path):
    _all_kept(composed[True])
    for words in (["het", "markers"], ["het", "rows", "markers", "filter"]):
        out = tmp_path / "_".join(words)
        for b in range(3):
            assert "marker pairs at their own counts" in _mps_cusk(dataset, out, b, words)
        _same_files(str(composed[True]["out"]), str(out))


def test_without_the_flag_the_files_are_the_parents(dataset, composed, tmp_path):
    """`mps cusk ... het`: N between markers, as before -- and not the files of the flag"""
    _all_kept(composed[False])
    for b in range(3):
        assert "marker pairs" not in _mps_cusk(dataset, tmp_path, b, ["het"])
    _same_files(str(composed[False]["out"]), str(tmp_path))
    assert any(open(os.path.join(composed[False]["out"], f), "rb").read() != open(os.path.join(composed[True]["out"], f), "rb").read()
               for f in os.listdir(composed[False]["out"]))


@pytest.mark.parametrize("stage", [False, True])
def test_blockset_het_markers_writes_the_composed_files(dataset, composed, tmp_path, cg, stage):
    from cigwas_amd import run_blocks as rb

    bs = rb.BlockSet(dataset["gaps"], dataset["stem"], dataset["blocks"], float(A_ALPHA), int(A_L1), int(A_L2), int(A_DEPTH))
    with pytest.raises(RuntimeError, match="per-pair sample sizes"):
        bs.set_het_markers(True)  # not a het set yet
    bs.set_het(True)
    bs.set_het_markers(True)
    e = cg.Engine(0)
    if stage:
        assert bs.stage(e)
    out = tmp_path / "bs"
    out.mkdir()
    for b in range(3):
        res, st = bs.run_block(e, b, next_block=b + 1 if stage and b < 2 else -1)  # (no build left in flight for the batch below)
        assert res is not None and st.num_sig == composed[True]["info"][b]["num_sig"]
        res.write(str(out))
    _same_files(str(composed[True]["out"]), str(out))
    if stage:  # the batch form, one block named twice
        res, st = bs.run_batch_het(e, [0, 1, 2, 1])
        out2 = tmp_path / "batch"
        out2.mkdir()
        res.write(str(out2))
        _same_files(str(composed[True]["out"]), str(out2))
    import cigwas_amd._lib as L

    L.lib().cusk_blockset_release_engine(bs.h, e.h)
    e.close()
    bs.close()


@pytest.mark.parametrize("mode", [["--het"], ["--het-batch-vars", "256"]])
def test_run_blocks_het_markers_writes_the_composed_files(dataset, composed, tmp_path, mode):
    cmd = [sys.executable, os.path.join(ROOT, "ci-gwas_amd", "run_blocks.py"), dataset["gaps"], dataset["stem"], dataset["blocks"],
           A_ALPHA, A_L1, A_L2, A_DEPTH, str(tmp_path)] + mode + ["--het-markers", "--writer", "local"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _same_files(str(composed[True]["out"]), str(tmp_path))


def test_cuskss_merged_het_markers_ess_square_is_the_counts(dataset, composed, tmp_path):
    """`cuskss-merged --bfiles --phen --het --het-markers` on a selection of markers: the marker x marker part of
    cuskss_merged.ess holds the counts of the retained markers, the rest is what the run without the flag writes"""
    from cigwas_amd import cli

    sel = np.array(sorted({f + i for b, (f, l) in enumerate(dataset["bounds"]) for i in composed[True]["info"][b]["ixs"] if i < l - f + 1}
                          | {1, 2, 10}), np.int32)
    sel.tofile(str(tmp_path / "sel.ixs"))
    outs = {}
    for flag in (False, True):
        out = tmp_path / ("on" if flag else "off")
        out.mkdir()
        args = cli.build_parser().parse_args(["cuskss-merged", "--alpha", A_ALPHA, "--marker-indices", str(tmp_path / "sel.ixs"),
                                              "--bfiles", dataset["stem"], "--phen", dataset["gaps"], "--max-level-one", A_L1,
                                              "--max-level-two", A_L2, "--outdir", str(out), "--het"] + (["--het-markers"] if flag else []))
        r = subprocess.run(cli.cuskss_argv(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        mdim = [int(v) for v in open(out / "cuskss_merged.mdim").read().split()]
        nv, npn = mdim[0], mdim[1]
        ixs = np.fromfile(str(out / "cuskss_merged.ixs"), np.int32)
        ess = np.fromfile(str(out / "cuskss_merged.ess"), np.float32).reshape(nv, nv)
        outs[flag] = (nv, npn, ixs, ess)
    nv, npn, ixs, ess = outs[True]
    k = nv - npn
    assert npn == A_P and k >= 2
    rows = sel[ixs[:k]]
    assert np.array_equal(ess[:k, :k], marker_pair_counts(dataset["bed"][rows], A_N).astype(np.float32))
    nv0, _, ixs0, ess0 = outs[False]
    k0 = nv0 - A_P
    assert np.all(ess0[:k0, :k0] == np.float32(A_N))
    common = np.intersect1d(ixs[:k], ixs0[:k0])
    a, b = np.searchsorted(ixs[:k], common), np.searchsorted(ixs0[:k0], common)
    assert len(common) >= 2 and np.array_equal(ess[np.ix_(a, np.arange(k, nv))].view(np.uint32),
                                               ess0[np.ix_(b, np.arange(k0, nv0))].view(np.uint32))


def test_the_flag_matters(dataset, composed, cg, tmp_path):
    """the planted pair of small-array markers: its correlation passes level 0 at N and fails at the 600 individuals both
    were genotyped on; both markers stay in the block's result (trait 0), the edge between them is in the .adj without
    `markers` and absent with it"""
    import scipy.stats

    q = float(scipy.stats.norm.ppf(1.0 - float(A_ALPHA) / 2.0))
    info = composed[True]["info"][0]
    at_N, at_own = pair_premise(info["C"], info["counts"], A_N, q, PLANT_A, PLANT_B)
    print(f"planted pair: r {info['C'][PLANT_A, PLANT_B]:.4f} on {info['counts'][PLANT_A, PLANT_B]} individuals; |z| sqrt(n - 3) / q = "
          f"{at_N:.3f} at N, {at_own:.3f} at its own count")
    assert info["counts"][PLANT_A, PLANT_B] == 600
    assert at_N > 1.1 and at_own < 0.9  # the premise, with room on either side
    for flag in (False, True):
        ix = composed[flag]["info"][0]["ixs"]
        assert PLANT_A in ix and PLANT_B in ix
        a, b = ix.index(PLANT_A), ix.index(PLANT_B)
        assert composed[flag]["info"][0]["adj"][a, b] == (0 if flag else 1)  # the oracle-composed pipeline agrees
    stem = "1_%d_%d" % dataset["bounds"][0]

    def edge(outdir):
        ix = list(np.fromfile(os.path.join(str(outdir), stem + ".ixs"), np.int32))
        adj = np.fromfile(os.path.join(str(outdir), stem + ".adj"), np.int32).reshape(len(ix), len(ix))
        return int(adj[ix.index(PLANT_A), ix.index(PLANT_B)])

    _mps_cusk(dataset, tmp_path / "het", 0, ["het"])
    _mps_cusk(dataset, tmp_path / "markers", 0, ["het", "markers"])
    assert edge(tmp_path / "het") == 1 and edge(tmp_path / "markers") == 0
