"""CPU: the oracle's host-side restatement vs the REFERENCE's own host C++, through what that code computed for seeded
inputs: tests/golden/ref_host_kat.npz holds the inputs and the reference's outputs, written by
tests/golden/make_ref_host_golden.py from oracle/_ref/libref_host.so (the reference's host sources compiled where they
lie, in the build container).  Nothing outside the repository is read."""
import hashlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "ref_host_kat.npz")

SUBSET_SEEDS, SUBSET_DEPTHS = range(6), range(0, 4)
GCS_SEEDS = range(4)
EXTS = ("ixs", "adj", "corr")
BLOCKING_CASES = [(0, 3000, 300), (1, 5000, 800), (2, 1200, 150), (3, 800, 2000)]
BLOCKING_WINDOWS = (5, 101, 333)
PREP_SUFFIXES = (".dim", ".means", ".stds", ".modes")


# ---- seeded inputs (the generator stores what these return; the tests read the stored copies) ----------------------
def _rand_graph(rng, n, dens):
    G = (rng.random((n, n)) < dens).astype(np.int32)
    G = np.triu(G, 1)
    return np.ascontiguousarray(G + G.T)


def subset_case(seed):
    rng = np.random.default_rng(seed)
    n, p = 40, 4
    return _rand_graph(rng, n, 0.06), n, p


def gcs_case(seed, use_map):
    rng = np.random.default_rng(100 + seed)
    n, p, ml = 18, 3, 3
    G = _rand_graph(rng, n, 0.2)
    Cm = rng.standard_normal((n, n)).astype(np.float32)
    S = np.full((n, n, 14), -1, np.int32)
    for i in range(n):
        for j in range(n):
            k = rng.integers(0, ml + 1)
            S[i, j, :k] = rng.choice(n, size=k, replace=False)
    P = np.sort(rng.choice(n, size=9, replace=False)).astype(np.int32)
    imap = (np.arange(n, dtype=np.int32) * 3 + 1) if use_map else None
    return G, Cm, S, P, imap, n, p, ml


def gc_case(use_map):
    rng = np.random.default_rng(5)
    n, p = 15, 2
    G = _rand_graph(rng, n, 0.2)
    Cm = rng.standard_normal((n, n)).astype(np.float32)
    N = rng.uniform(1e3, 1e5, (n, n)).astype(np.float32)
    P = np.sort(rng.choice(n, size=7, replace=False)).astype(np.int32)
    imap = (np.arange(n, dtype=np.int32) + 100) if use_map else None
    return G, Cm, N, P, imap, n, p


def het_case():
    """hetcor inputs: correlation + standard-error files, with NA entries."""
    rng = np.random.default_rng(11)
    p, m = 4, 6
    c = np.triu(rng.uniform(-0.4, 0.4, (p, p)), 1)
    np.fill_diagonal(c, 1.0)
    se = rng.uniform(0.001, 0.01, (p, p))
    mc = rng.uniform(-0.05, 0.05, (m, p))
    ms = rng.uniform(0.001, 0.005, (m, p))
    return c, se, mc, ms


def write_het_files(d, c, se, mc, ms):
    p, m = c.shape[0], mc.shape[0]
    names = [f"T{i}" for i in range(p)]
    paths = {k: os.path.join(str(d), k + ".txt") for k in ("pxp", "pxp_se", "mxp", "mxp_se")}
    with open(paths["pxp"], "w") as f, open(paths["pxp_se"], "w") as g:
        f.write(" ".join(names) + "\n")
        g.write(" ".join(names) + "\n")
        for i in range(p):
            vals = [("NaN" if (i, j) == (0, 2) else repr(float(c[i, j]))) for j in range(p)]
            f.write(names[i] + " " + " ".join(vals) + "\n")
            g.write(names[i] + " " + " ".join(repr(float(se[i, j])) for j in range(p)) + "\n")
    with open(paths["mxp"], "w") as f, open(paths["mxp_se"], "w") as g:
        f.write("chr snp ref " + " ".join(names) + "\n")
        g.write("chr snp ref " + " ".join(names) + "\n")
        for i in range(m):
            vals = [("NaN" if (i, j) == (2, 1) else repr(float(mc[i, j]))) for j in range(p)]
            f.write(f"1 rs{i} A " + " ".join(vals) + "\n")
            g.write(f"1 rs{i} A " + " ".join(repr(float(ms[i, j])) for j in range(p)) + "\n")
    return paths


def blocking_case(seed, n):
    """forward |r| row sums look like a noisy positive curve with dips at block boundaries"""
    rng = np.random.default_rng(100 + seed)
    base = 20.0 + 10.0 * np.sin(np.arange(n) / 37.0) + 5.0 * np.sin(np.arange(n) / 211.0 + seed)
    dips = np.ones(n)
    for c in rng.integers(50, n - 50, size=max(3, n // 250)):
        dips[max(0, c - 15): c + 15] *= rng.uniform(0.2, 0.6)
    return (base * dips + rng.normal(0.0, 0.8, n)).astype(np.float32)


def synthetic_prep_inputs(stem, synth):
    """bfiles for `mps prep` with missing genotypes; N not a multiple of four: the last byte of every marker is partly
    padding"""
    N = 1003
    G = synth.make_genotypes(300, N, np.random.default_rng(5), miss=0.02)
    mu, sd = synth.bed_stats(G)
    synth.write_bfiles(stem, synth.pack_bed(G), N, mu, sd)
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)


# ---- tests ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    with np.load(KAT) as z:
        return {k: z[k] for k in z.files}


def _read_outputs(base, exts):
    return {ext: open(base + "." + ext, "rb").read() for ext in ("mdim",) + exts}


@pytest.mark.parametrize("seed", SUBSET_SEEDS)
def test_subset_variables_random(oracle, ref, seed):
    G = ref[f"subset/{seed}/G"]
    n, p = G.shape[0], 4
    for depth in SUBSET_DEPTHS:
        assert list(ref[f"subset/{seed}/d{depth}"]) == list(oracle.subset_variables(G, n, n - p, depth))


@pytest.mark.parametrize("seed", GCS_SEEDS)
@pytest.mark.parametrize("use_map", [False, True])
def test_reduce_gcs_files(oracle, ref, tmp_path, seed, use_map):
    k = f"gcs/{seed}/{int(use_map)}"
    G, Cm, S, P = (ref[f"{k}/{x}"] for x in ("G", "C", "S", "P"))
    n, p, ml = G.shape[0], 3, 3
    imap = ref[f"{k}/imap"] if use_map else None
    b = str(tmp_path / "orc")
    oracle.write_reduced(oracle.reduce_gcs(G, Cm, S, P, n, p, ml, imap), b, with_sep=True)
    got = _read_outputs(b, EXTS + ("sep",))
    for ext, data in got.items():
        assert data == ref[f"{k}/{ext}"].tobytes(), ext


@pytest.mark.parametrize("use_map", [False, True])
def test_reduce_gc_files(oracle, ref, tmp_path, use_map):
    k = f"gc/{int(use_map)}"
    G, Cm, N, P = (ref[f"{k}/{x}"] for x in ("G", "C", "N", "P"))
    n, p = G.shape[0], 2
    imap = ref[f"{k}/imap"] if use_map else None
    b = str(tmp_path / "orc")
    oracle.write_reduced(oracle.reduce_gc(G, Cm, N, P, n, p, 14, imap), b, with_sep=False)
    got = _read_outputs(b, EXTS)
    for ext, data in got.items():
        assert data == ref[f"{k}/{ext}"].tobytes(), ext


def test_loaders_on_reference_fixtures(oracle, ref, golden_dir):
    g = lambda f: os.path.join(golden_dir, f)  # noqa: E731
    assert np.array_equal(ref["load/mxm"], oracle.load_mxm(g("small_mxm.bin")))
    # pxp with fixed sample size
    _, c2, e2 = oracle.load_pxp(g("trait_summary_stats.txt"), sample_size=500000.0)
    assert ref["load/pxp_p"][0] == 3 and np.array_equal(ref["load/pxp_corr"], c2) and np.array_equal(ref["load/pxp_ess"], e2)
    # mxp by block and by marker indices
    c2, _ = oracle.load_mxp(g("marker_trait_summary_stats.txt"), range(0, 3))
    assert list(ref["load/mxp_block_counts"]) == [3, 3] and np.array_equal(ref["load/mxp_block_corr"], c2)
    ix = np.fromfile(g("marker_indices.bin"), np.int32)
    c2, _ = oracle.load_mxp(g("marker_trait_summary_stats.txt"), ix)
    assert ref["load/mxp_ix_count"][0] == len(ix) and np.array_equal(ref["load/mxp_ix_corr"], c2)
    # blocks
    bl = oracle.read_blocks(g("test.blocks"))
    assert [(b[1], b[2], b[3]) for b in bl] == [tuple(r) for r in ref["load/blocks"]]
    # phen with NaN
    n2, p2, d2 = oracle.load_phen(g("with_nan.phen"))
    assert (n2, p2) == tuple(ref["load/phen_shape"]) and np.array_equal(ref["load/phen"], d2, equal_nan=True)


def test_het_loaders_with_se(oracle, ref, tmp_path):
    """hetcor inputs: correlation + standard-error files, with NA entries."""
    paths = write_het_files(tmp_path, ref["het/c"], ref["het/se"], ref["het/mc"], ref["het/ms"])
    _, c2, e2 = oracle.load_pxp(paths["pxp"], se_path=paths["pxp_se"])
    assert np.array_equal(ref["het/pxp_corr"], c2)
    assert np.array_equal(ref["het/pxp_ess"], e2, equal_nan=True)
    c2, e2 = oracle.load_mxp(paths["mxp"], range(1, 5), se_path=paths["mxp_se"])
    assert ref["het/mxp_count"][0] == 4 and np.array_equal(ref["het/mxp_corr"], c2)
    assert np.array_equal(ref["het/mxp_ess"], e2, equal_nan=True)


@pytest.mark.parametrize("seed,n,maxb", BLOCKING_CASES)
def test_blocking_matches_reference_code(oracle, ref, seed, n, maxb):
    """the oracle's restatement of blocking.cpp against what the reference's own blocking.cpp computed: smoothed curve
    bit-equal, identical blocks, on random LD-like row-sum profiles"""
    v = ref[f"blocking/{seed}/v"]
    assert v.shape == (n,)
    for ws in BLOCKING_WINDOWS:
        assert np.array_equal(oracle.hanning_smoothing(v, ws), ref[f"blocking/{seed}/smooth{ws}"])
    blocks = ref[f"blocking/{seed}/blocks"]
    assert len(blocks) > 0
    assert oracle.block_chr(v, maxb) == [(int(a), int(b)) for a, b in blocks]


@pytest.mark.parametrize("which", ["small", "synthetic"])
def test_mps_prep_writes_the_reference_files(ref, kat, golden_dir, tmp_path, which):
    """`mps prep` of this build (host code, runs without a GPU) against what the reference's prep.cpp wrote for the
    same files: .dim/.means/.stds/.modes byte for byte; on small.* also the values the reference's prep_tests.cpp
    expects"""
    import shutil
    import subprocess

    from cigwas_amd.cli import MPS_PATH

    assert os.path.exists(MPS_PATH), "mps not built: run build()"
    stem = str(tmp_path / "x")
    for sfx in (".bed", ".bim", ".fam"):
        if which == "small":
            shutil.copy(os.path.join(golden_dir, "small" + sfx), stem + sfx)
        else:
            ref[f"prep/{which}/in{sfx}"].tofile(stem + sfx)
    subprocess.run([MPS_PATH, "prep", stem], check=True, capture_output=True)
    for sfx in PREP_SUFFIXES:
        assert open(stem + sfx, "rb").read() == ref[f"prep/{which}/out{sfx}"].tobytes(), sfx
    if which == "small":
        k = kat["prep_small"]
        assert np.allclose(np.loadtxt(stem + ".means"), k["exp_means"], atol=k["tol"], rtol=0)
        assert np.allclose(np.loadtxt(stem + ".stds"), k["exp_stds"], atol=k["tol"], rtol=0)
        assert open(stem + ".dim").read().split() == [str(v) for v in k["exp_dims"]]


def test_stored_inputs_are_the_seeded_ones(ref, synth, tmp_path):
    """the stored inputs are what the seeded generators above produce on this numpy (so make_ref_host_golden.py
    regenerates the same cases)"""
    for seed in SUBSET_SEEDS:
        assert np.array_equal(subset_case(seed)[0], ref[f"subset/{seed}/G"])
    for seed, n, _ in BLOCKING_CASES:
        assert np.array_equal(blocking_case(seed, n), ref[f"blocking/{seed}/v"])
    stem = str(tmp_path / "x")
    synthetic_prep_inputs(stem, synth)
    for sfx in (".bed", ".bim", ".fam"):
        assert hashlib.sha256(open(stem + sfx, "rb").read()).digest() == hashlib.sha256(ref[f"prep/synthetic/in{sfx}"].tobytes()).digest()
