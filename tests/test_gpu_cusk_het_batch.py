"""GPU: batched block runs at per-pair sample sizes -- the block-diagonal sample-size matrix (cusk_ess_square_batch), the
batched engine run (cusk_run_skeleton_batch_het), the batch pipeline above them (cusk_blockset_run_batch_het,
run_blocks.py --het-batch-vars).

References: a numpy restatement for the size matrix (bitwise); per block the single-block run cusk_run_skeleton_het on
that block alone (identical adjacency and records required) and, so that this does not rest on that run alone, the
oracle's `hetcor_skeleton` and `Skeleton`; for the pipeline the files of cusk_blockset_run_block on a het block set (byte
for byte)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cusk_het_batch_formats import SENTINEL, ess_square_batch_expected
from test_cusk_het_formats import ess_square_inputs
from test_gpu_cusk_het import (ALPHA, B_ALPHA, B_DEPTH, B_L1, B_L2, B_N, B_P, B_SIZES, HET_LEVELS, NS, PLANT, _dense,
                               _star, het_case, make_dataset, plant_premise, uniform_thresholds)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML = 14


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
# 1. cusk_ess_square_batch
# ---------------------------------------------------------------------------------------------------------------------
E_BLOCKS = [(5, 3), (61, 3), (130, 3)]
E_BASE = [0, 64, 128]


def _ess_inputs():
    tabs = [ess_square_inputs(m, p, seed=10 + m) for m, p in E_BLOCKS]
    return [t[0] for t in tabs], [t[1] for t in tabs], [m for m, _ in E_BLOCKS]


# 320: every block row starts on a 16-byte boundary (16-byte stores and a tail of single floats); 263: rows start at every
# residue (single floats throughout), and the last block ends two columns short of the allocation
@pytest.mark.parametrize("n", [320, 263])
def test_ess_square_batch_is_the_numpy_restatement_bitwise(cg, eng, n):
    mxp, pxp, m = _ess_inputs()
    want = ess_square_batch_expected(mxp, pxp, m, E_BASE, 3, NS, n)
    buf = cg.DeviceArray(np.full((n, n), SENTINEL, np.uint32))
    eng.ess_square_batch(np.concatenate([t.reshape(-1) for t in mxp]), np.concatenate([t.reshape(-1) for t in pxp]), m, E_BASE, 3,
                         NS, n, buf.ptr)
    got = buf.download(np.uint32, (n, n))
    buf.free()
    for (mb, p), b0 in zip(E_BLOCKS, E_BASE):
        assert np.array_equal(got[b0:b0 + mb + p, b0:b0 + mb + p], want[b0:b0 + mb + p, b0:b0 + mb + p]), (mb, b0)
    assert np.array_equal(got, want)  # every other cell still holds the sentinel
    assert np.count_nonzero(got == SENTINEL) == n * n - sum((mb + p) ** 2 for mb, p in E_BLOCKS)


def test_ess_square_batch_argument_errors_and_the_engine_goes_on(cg, eng):
    n = 320
    mxp, pxp, m = _ess_inputs()
    mx, px = np.concatenate([t.reshape(-1) for t in mxp]), np.concatenate([t.reshape(-1) for t in pxp])
    buf = cg.DeviceArray(np.full((n + 1, n), SENTINEL, np.uint32))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        eng.ess_square_batch(mx, px, m, [0, 72, 128], 3, NS, n, buf.ptr)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        eng.ess_square_batch(mx, px, m, [0, 128, 64], 3, NS, n, buf.ptr)  # not ascending
    with pytest.raises(RuntimeError, match="beyond"):
        eng.ess_square_batch(mx, px, m, E_BASE, 3, NS, 256, buf.ptr)  # the last block ends at 261
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        eng.ess_square_batch(mx, px, m, E_BASE, 3, NS, n, buf.ptr + 4)
    assert np.all(buf.download(np.uint32, (n + 1, n)) == SENTINEL)  # none of them wrote anything
    eng.ess_square_batch(mx, px, m, E_BASE, 3, NS, n, buf.ptr)
    got = buf.download(np.uint32, (n + 1, n))
    buf.free()
    assert np.array_equal(got[:n], ess_square_batch_expected(mxp, pxp, m, E_BASE, 3, NS, n)) and np.all(got[n] == SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------
# 2. cusk_run_skeleton_batch_het against the single-block run and the oracle
# ---------------------------------------------------------------------------------------------------------------------
def het_sizes(n, p, seed, lo=0.25):
    """het_case's size matrix for any block: NS between the first n - p variables, every pair with one of the last p
    ("traits") at a size of its own, NaN on the trait diagonal and for one trait against two markers"""
    m = n - p
    rng = np.random.default_rng(seed)
    Nsz = np.full((n, n), NS, np.float32)
    U = np.floor(rng.uniform(lo, 1.0, (n, p)) * NS).astype(np.float32)
    Nsz[:, m:] = U
    Nsz[m:, :] = U.T
    Nsz[m:, m:] = np.minimum(Nsz[m:, m:], Nsz[m:, m:].T)
    Nsz[np.arange(m, n), np.arange(m, n)] = np.nan
    for mk in (3, m // 2):
        Nsz[mk, m + 1] = Nsz[m + 1, mk] = np.nan
    return Nsz


def _blocks(synth):
    """name -> (C, N): het_case; exactly one bitmap word; a second word that is partly used; a hub with 130 neighbours
    (rows of the unstaged degree class); one block at a single size (the oracle's Skeleton applies)"""
    Chet, Nhet, _m, _p = het_case(synth)
    C64 = synth.synth_corr_block(58, 6, N=16384, block_index=801)
    C75 = synth.synth_corr_block(69, 6, N=16384, block_index=802)
    Cst = _star(130, seed=5)
    Cun = synth.synth_corr_block(43, 5, N=16384, block_index=1)
    assert C64.shape[0] == 64 and C75.shape[0] == 75 and Cst.shape[0] == 131
    return {
        "het_case": (Chet, Nhet),
        "one_word64": (C64, het_sizes(64, 6, seed=64)),
        "partial_word75": (C75, het_sizes(75, 6, seed=75)),
        "star130_unstaged": (Cst, het_sizes(131, 6, seed=131, lo=0.5)),
        "uniform48": (Cun, np.full((48, 48), NS, np.float32)),
    }


# the batch of the issue at maxlevel 2 (the hub's row has C(130, l) sets per neighbour), and the blocks without the star down
# to het_case's own four levels beside the block at one size
BATCHES = {
    "with_star_l2": (["het_case", "one_word64", "partial_word75", "star130_unstaged"], 2),
    "deep_l4": (["het_case", "one_word64", "uniform48", "partial_word75"], HET_LEVELS),
}


@pytest.fixture(scope="module")
def blocks(synth):
    return _blocks(synth)


@pytest.fixture(scope="module")
def single_runs(cg, eng, blocks):
    """(name, maxlevel) -> the single-block het run of that block alone, computed once"""
    th = cg.hetcor_threshold(ALPHA)
    out = {}
    for names, maxlevel in BATCHES.values():
        for name in names:
            if (name, maxlevel) in out:
                continue
            Cm, Nsz = blocks[name]
            n = Cm.shape[0]
            Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nsz)
            st = eng.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, maxlevel)
            out[(name, maxlevel)] = dict(st=st, G=eng.adjacency(), rec=eng.sepsets())
            Cd.free()
            Nd.free()
    return out


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_batch_het_is_the_single_block_het_run_per_block(cg, eng, oracle, blocks, single_runs, batch):
    names, maxlevel = BATCHES[batch]
    th = cg.hetcor_threshold(ALPHA)
    sizes = [blocks[k][0].shape[0] for k in names]
    lo, pos = [], 0
    for k in sizes:
        lo.append(pos)
        pos += (k + 63) // 64 * 64
    hi = [a + k for a, k in zip(lo, sizes)]
    n = pos + 64  # a word of padding rows behind the last block
    # cells outside the diagonal blocks: NaN correlations and a size below 3 -- a kernel that read them would differ
    big = np.full((n, n), np.nan, np.float32)
    bigN = np.full((n, n), 2.0, np.float32)
    for name, a, b in zip(names, lo, hi):
        big[a:b, a:b], bigN[a:b, a:b] = blocks[name]
    Cd, Nd = cg.DeviceArray(big), cg.DeviceArray(bigN)
    st = eng.run_skeleton_batch_het(Cd.ptr, Nd.ptr, n, lo, hi, th, maxlevel)
    Gs = eng.adjacency_blocks()
    Gfull = eng.adjacency()
    x, y, lv, z, S = eng.sepsets()
    Cd.free()
    Nd.free()
    inside = np.zeros((n, n), bool)
    for a, b in zip(lo, hi):
        inside[a:b, a:b] = True
    assert not np.any(Gfull[~inside])  # padding rows have degree 0, no row meets a column outside its block
    assert st.tests[0] == sum(k * (k - 1) // 2 for k in sizes)
    assert sum(st.rechecks) == 0 and st.exact_fallbacks == 0  # exact path only: nothing is queued
    for name, a, b, G in zip(names, lo, hi, Gs):
        one = single_runs[(name, maxlevel)]
        assert np.array_equal(G, one["G"]), name
        assert np.array_equal(Gfull[a:b, a:b], one["G"]), name
        sel = (x >= a) & (x < b)
        x1, y1, lv1, _z1, S1 = one["rec"]
        assert np.all((y[sel] >= a) & (y[sel] < b)), name
        assert np.array_equal(x[sel] - a, x1) and np.array_equal(y[sel] - a, y1) and np.array_equal(lv[sel], lv1), name
        assert np.array_equal(np.where(S[sel] >= 0, S[sel] - a, -1), S1), name
        assert len(x1) > 0, name
    assert st.level == max(single_runs[(name, maxlevel)]["st"].level for name in names)
    if "star130_unstaged" in names:  # the case reaches the class it is named after
        assert single_runs[("star130_unstaged", maxlevel)]["st"].max_degree[1] >= 128
    # not only the single-block run: the oracle's hetcor_skeleton for het_case ...
    k = names.index("het_case")
    Cm, Nsz = blocks["het_case"]
    nb = Cm.shape[0]
    ref = oracle.hetcor_skeleton(Cm, np.ones((nb, nb), np.int32), Nsz, th, maxlevel, np.zeros(nb, np.int32))
    assert np.array_equal(Gs[k], ref.G)
    # ... and its Skeleton, at the thresholds the rule yields at one size, for the block at one size
    if "uniform48" in names:
        k = names.index("uniform48")
        Cm = blocks["uniform48"][0]
        ref = oracle.skeleton(Cm, uniform_thresholds(th, NS), maxlevel)
        sel = (x >= lo[k]) & (x < hi[k])
        assert np.array_equal(Gs[k], ref.G)
        assert np.array_equal(_dense(48, x[sel] - lo[k], y[sel] - lo[k], np.where(S[sel] >= 0, S[sel] - lo[k], -1)), ref.sepset)


def test_batch_het_unsupported_combinations_are_errors_and_the_engine_goes_on(cg, blocks, single_runs):
    Cm, Nsz = blocks["one_word64"]
    th = cg.hetcor_threshold(ALPHA)
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nsz)
    e.set_row_shard(0, 2, exchange=lambda *a: 0)
    with pytest.raises(RuntimeError, match="row-sharded"):
        e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, 64, [0], [64], th, 2)
    e.set_row_shard(0, 1)
    e.set_option("validate", 1)
    with pytest.raises(RuntimeError, match="validate"):
        e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, 64, [0], [64], th, 2)
    e.set_option("validate", 0)
    with pytest.raises(RuntimeError, match="sample-size matrix"):
        e.run_skeleton_batch_het(Cd.ptr, None, 64, [0], [64], th, 2)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, 64, [8], [64], th, 2)
    e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, 64, [0], [64], th, 2)
    assert np.array_equal(e.adjacency_blocks()[0], single_runs[("one_word64", 2)]["G"])
    Cd.free()
    Nd.free()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. the batch pipeline
# ---------------------------------------------------------------------------------------------------------------------
NULL_M = 40        # markers of the fourth block: independent draws, in LD with nothing, no effect on any trait
NULL_SEED = 1


def make_dataset4(synth):
    """make_dataset (test_gpu_cusk_het.py: three blocks, five traits, gaps in traits 1 and 3) and a fourth block of NULL_M
    markers drawn on their own after everything else -- the first three blocks and the traits are bit for bit those of
    make_dataset"""
    G, Y, Yg = make_dataset(synth)
    rng = np.random.default_rng(77000 + NULL_SEED)
    G4 = rng.binomial(2, rng.uniform(0.2, 0.5, (NULL_M, 1)), (NULL_M, B_N)).astype(np.int8)
    return np.concatenate([G, G4]), Y, Yg


def null_block_premise(G, Yg):
    """float64: the largest |z| sqrt(n - 3) over the fourth block's markers x traits, each pair on the individuals it is
    observed on (the premise of "the het prefilter keeps nothing of the fourth block")"""
    worst = 0.0
    for g in G[sum(B_SIZES):].astype(np.float64):
        for y in Yg.astype(np.float64):
            ok = (g >= 0) & ~np.isnan(y)
            r = np.corrcoef(g[ok], y[ok])[0, 1]
            worst = max(worst, abs(np.arctanh(r)) * np.sqrt(ok.sum() - 3.0))
    return worst


@pytest.fixture(scope="module")
def dataset4(tmp_path_factory, synth):
    d = tmp_path_factory.mktemp("cusk_het_batch")
    G, Y, Yg = make_dataset4(synth)
    means, stds = synth.bed_stats(G)
    stem = str(d / "geno")
    synth.write_bfiles(stem, synth.pack_bed(G), B_N, means, stds)
    synth.write_phen(str(d / "gaps.phen"), Yg.reshape(-1), B_N, B_P)
    bounds, first = [], 0
    with open(d / "b.blocks", "w") as f:
        for s in B_SIZES + [NULL_M]:
            f.write(f"1\t{first}\t{first + s - 1}\n")
            bounds.append((first, first + s - 1))
            first += s
    return dict(dir=d, stem=stem, gaps=str(d / "gaps.phen"), blocks=str(d / "b.blocks"), bounds=bounds, G=G, Y=Y, Yg=Yg)


def _blockset(ds):
    from cigwas_amd import run_blocks as rb

    return rb.BlockSet(ds["gaps"], ds["stem"], ds["blocks"], float(B_ALPHA), int(B_L1), int(B_L2), int(B_DEPTH))


@pytest.fixture(scope="module")
def per_block(dataset4, cg, tmp_path_factory):
    """the reference of the pipeline tests: every block through run_block on a het block set, files per block"""
    import cigwas_amd._lib as L

    root = tmp_path_factory.mktemp("per_block")
    bs = _blockset(dataset4)
    bs.set_het(True)
    e = cg.Engine(0)
    dirs, skipped = [], []
    for b in range(len(dataset4["bounds"])):
        d = root / f"b{b}"
        d.mkdir()
        res, st = bs.run_block(e, b)
        skipped.append(bool(st.skipped))
        if res is not None:
            res.write(str(d))
        dirs.append(d)
    L.lib().cusk_blockset_release_engine(bs.h, e.h)
    e.close()
    bs.close()
    return dict(dirs=dirs, skipped=skipped)


def _expect(per_block, out, blocks):
    """`out` holds exactly the per-block files of `blocks`, byte for byte"""
    want = {}
    for b in blocks:
        for f in os.listdir(per_block["dirs"][b]):
            want[f] = open(os.path.join(per_block["dirs"][b], f), "rb").read()
    assert sorted(os.listdir(out)) == sorted(want)
    for f, data in want.items():
        assert open(os.path.join(str(out), f), "rb").read() == data, f


def test_the_fourth_block_has_nothing_for_the_prefilter(dataset4, per_block):
    """NULL_SEED = 1 was taken on the CPU as the first seed of 1, 2, ... whose fourth block stays below 0.85 q = 3.307 in
    float64 (the room test_the_flag_matters leaves its premise): its largest |z| sqrt(n - 3) over 40 markers x 5 traits is
    2.807, before any GPU run"""
    import scipy.stats

    q = float(scipy.stats.norm.ppf(1.0 - float(B_ALPHA) / 2.0))
    worst = null_block_premise(dataset4["G"], dataset4["Yg"])
    print(f"fourth block: largest |z| sqrt(n - 3) = {worst:.4f}, q = {q:.4f}")
    assert worst < 0.85 * q
    assert per_block["skipped"][3] and not os.listdir(per_block["dirs"][3])
    assert not any(per_block["skipped"][:3]) and all(len(os.listdir(d)) == 5 for d in per_block["dirs"][:3])


def test_run_batch_het_writes_the_per_block_het_files(dataset4, per_block, cg, tmp_path):
    import cigwas_amd._lib as L

    bs = _blockset(dataset4)  # no set_het: the entry point does not ask
    e = cg.Engine(0)
    for tag, order in (("asc", [0, 1, 2, 3]), ("mixed", [2, 0, 3, 1])):
        out = tmp_path / tag
        out.mkdir()
        res, st = bs.run_batch_het(e, order)
        assert st.blocks == 4 and st.skipped == 1 and sorted(res.block_indices) == [0, 1, 2]
        assert res.block_indices == [b for b in order if b != 3]
        res.write(str(out))
        res.free()
        _expect(per_block, out, [0, 1, 2])  # the fourth block writes nothing
    # a batch the prefilter empties, then a further batch on the same engine
    res, st = bs.run_batch_het(e, [3])
    assert res.count == 0 and st.blocks == 1 and st.skipped == 1
    res.free()
    out = tmp_path / "after"
    out.mkdir()
    res, st = bs.run_batch_het(e, [1, 0])
    res.write(str(out))
    res.free()
    _expect(per_block, out, [0, 1])
    # on a het set the plain batch still refuses, the het batch runs as before
    bs.set_het(True)
    with pytest.raises(RuntimeError, match="per-pair sample sizes"):
        bs.run_batch(e, [0, 1])
    out = tmp_path / "hetset"
    out.mkdir()
    res, st = bs.run_batch_het(e, [2])
    res.write(str(out))
    res.free()
    _expect(per_block, out, [2])
    L.lib().cusk_blockset_release_engine(bs.h, e.h)
    e.close()
    bs.close()


def test_run_blocks_het_batch_vars_local_writer_writes_the_same_directory(dataset4, per_block, tmp_path):
    out = tmp_path / "rb"
    out.mkdir()
    cmd = [sys.executable, os.path.join(ROOT, "ci-gwas_amd", "run_blocks.py"), dataset4["gaps"], dataset4["stem"], dataset4["blocks"],
           B_ALPHA, B_L1, B_L2, B_DEPTH, str(out), "--het-batch-vars", "256", "--writer", "local"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "4 blocks (1 skipped)" in r.stdout, r.stdout
    _expect(per_block, out, [0, 1, 2])


def test_the_mode_is_really_on(dataset4, per_block, cg, tmp_path):
    """the premise of test_the_flag_matters (same genotypes, same traits): the planted marker's effect on the 25 % trait is
    significant at N and not on the observed quarter -- the plain batch keeps the marker, the het batch drops it"""
    import scipy.stats

    import cigwas_amd._lib as L

    q = float(scipy.stats.norm.ppf(1.0 - float(B_ALPHA) / 2.0))
    (z_full, n_full), (z_sub, n_sub) = plant_premise(dataset4["G"], dataset4["Y"], dataset4["Yg"])
    assert abs(z_full) * np.sqrt(n_full - 3) > 1.2 * q and abs(z_sub) * np.sqrt(B_N - 3) > 1.2 * q
    assert abs(z_sub) * np.sqrt(n_sub - 3) < 0.85 * q
    f, l = dataset4["bounds"][1]
    stem, local = f"1_{f}_{l}", PLANT - f
    bs = _blockset(dataset4)
    e = cg.Engine(0)
    outs = {}
    for tag, run in (("plain", bs.run_batch), ("het", bs.run_batch_het)):
        outs[tag] = tmp_path / tag
        outs[tag].mkdir()
        res, _st = run(e, [0, 1, 2, 3])
        res.write(str(outs[tag]))
        res.free()
    L.lib().cusk_blockset_release_engine(bs.h, e.h)
    e.close()
    bs.close()
    kept = lambda d: local in list(np.fromfile(os.path.join(str(d), stem + ".ixs"), np.int32))
    assert kept(outs["plain"]) and not kept(outs["het"])
    assert any(open(os.path.join(str(outs["plain"]), stem + x), "rb").read() != open(os.path.join(str(outs["het"]), stem + x), "rb").read()
               for x in (".ixs", ".adj", ".corr"))
    _expect(per_block, outs["het"], [0, 1, 2])
