"""GPU: the inputs of `cuskss-merged` from genotypes -- the correlation build over a marker index list
(cusk_corr_build_indexed + cusk_pack_lower_tri), `sumstats` (the three files `cuskss` reads) and
`cuskss-merged --bfiles --phen` (the same step without the files).

Bounds: SNP x SNP correlations are bit-exact against the oracle (integer contingency counts, the reference's fp32
epilogue), SNP x trait and trait x trait within 1e-5 absolute, the tolerance of the reference's own correlation tests
(tests/test_gpu_workflow_chain.py uses the same two).  Everything that compares the product with itself -- the indexed
build against the build on rows the host made contiguous, the files against the matrix in HBM, the two routes of
`cuskss-merged` against each other -- is bit for bit / byte for byte.
"""
import os
import pathlib
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M1, M2, N, P = 900, 700, 4001, 6  # N is not a multiple of 4: a .bed row ends inside a byte and starts at any alignment
K_SEL = 150
ALPHA, L1, L2, DEPTH = 1e-4, 3, 14, 1
MAX_BLOCK, WIDTH = 400, 200


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


def _write_inputs(d, synth, m, chr_ids, seed):
    """PLINK set + .phen with 8 planted marker effects per trait and a trait DAG (the recipe of the workflow chain test),
    then `prep-bed` for .dim / .means / .stds"""
    from cigwas_amd import cli

    d = pathlib.Path(d)
    rng = synth.rng_for(seed)
    G = synth.make_genotypes(m, N, rng, miss=0.002)
    g = G.astype(np.float64)
    g[G < 0] = np.nan
    gs = np.nan_to_num((g - np.nanmean(g, 1, keepdims=True)) / np.nanstd(g, 1, keepdims=True))
    Y = np.zeros((P, N))
    for k in range(P):
        idx = rng.choice(m, size=8, replace=False)
        y = (rng.uniform(0.12, 0.25, 8) * rng.choice([-1.0, 1.0], 8)) @ gs[idx]
        for k2 in range(k):
            if rng.random() < 0.5:
                y = y + rng.uniform(0.15, 0.3) * rng.choice([-1.0, 1.0]) * Y[k2]
        y = y + rng.standard_normal(N)
        Y[k] = (y - y.mean()) / y.std()
    stem = str(d / "geno")
    bed = synth.pack_bed(G)
    synth.write_bfiles(stem, bed, N, np.zeros(m), np.zeros(m), chr_ids)
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    synth.write_phen(str(d / "y.phen"), np.ascontiguousarray(Y.astype(np.float32)).reshape(-1), N, P)
    cli.main(["prep-bed", stem])
    return dict(dir=d, stem=stem, phen_path=str(d / "y.phen"), bed=bed, chr_ids=chr_ids, m=m,
                means=np.loadtxt(stem + ".means", dtype=np.float32), stds=np.loadtxt(stem + ".stds", dtype=np.float32))


@pytest.fixture(scope="module")
def data(tmp_path_factory, synth, oracle):
    m = M1 + M2
    dat = _write_inputs(tmp_path_factory.mktemp("sumstats"), synth, m, ["1"] * M1 + ["2"] * M2, 5151)
    dat["phen"] = oracle.load_phen(dat["phen_path"])[2]
    rng = np.random.Generator(np.random.PCG64(77))
    inner = rng.choice(np.arange(1, m - 1), size=K_SEL - 2, replace=False)
    ixs = np.sort(np.concatenate([[0, m - 1], inner])).astype(np.int32)
    assert (ixs < M1).sum() > 20 and (ixs >= M1).sum() > 20
    dat["ixs"] = ixs
    ixs.tofile(str(dat["dir"] / "selected.ixs"))
    return dat


def _oracle_square(oracle, dat, ixs):
    k = len(ixs)
    mxm, mxp, pxp = oracle.corr_pearson_npn(dat["bed"][ixs], dat["phen"], k, N, P, dat["means"][ixs], dat["stds"][ixs])
    sq = oracle.square_from_cusk_corrs(mxm, mxp, pxp, k, P)
    assert not np.isnan(sq).any()
    return sq


def _indexed(eng, dat, ixs, bed, means, stds):
    import cigwas_amd as cg

    k, n = len(ixs), len(ixs) + P
    Cd = cg.DeviceArray(nbytes=4 * n * n)
    mxp = eng.corr_build_indexed(bed, dat["phen"], ixs, dat["m"], N, P, means, stds, Cd.ptr, want_mxp=True)
    sq = Cd.download(np.float32, (n, n))
    tri = eng.pack_lower_tri(Cd.ptr, n, k)
    Cd.free()
    return sq, mxp.reshape(k, P), tri


def test_indexed_build_against_oracle_and_contiguous_build(data, oracle):
    import cigwas_amd as cg

    ixs, k = data["ixs"], len(data["ixs"])
    n = k + P
    ref = _oracle_square(oracle, data, ixs)
    eng = cg.Engine(0)
    sq, mxp, tri = _indexed(eng, data, ixs, data["bed"], data["means"], data["stds"])
    err_mxp = float(np.abs(sq[:k, k:] - ref[:k, k:]).max())
    err_pxp = float(np.abs(sq[k:, k:] - ref[k:, k:]).max())
    print(f"indexed build: max |mxp - oracle| = {err_mxp:.3g}, max |pxp - oracle| = {err_pxp:.3g}")
    assert np.array_equal(_bits(sq[:k, :k]), _bits(ref[:k, :k]))  # SNP x SNP bit-exact
    assert err_mxp <= 1e-5 and err_pxp <= 1e-5
    assert np.array_equal(_bits(sq), _bits(sq.T)) and np.array_equal(_bits(mxp), _bits(sq[:k, k:]))
    assert tri.shape == (k * (k + 1) // 2,) and np.array_equal(_bits(tri), _bits(ref[:k, :k][np.tril_indices(k)]))
    # the same bits from device-resident inputs (the row-gather kernel) ...
    bed_d, means_d, stds_d = cg.DeviceArray(data["bed"]), cg.DeviceArray(data["means"]), cg.DeviceArray(data["stds"])
    sq_d, mxp_d, tri_d = _indexed(eng, data, ixs, bed_d, means_d, stds_d)
    assert np.array_equal(_bits(sq_d), _bits(sq)) and np.array_equal(_bits(mxp_d), _bits(mxp)) and np.array_equal(_bits(tri_d), _bits(tri))
    # ... and from cusk_corr_build on the rows made contiguous on the host
    Cd = cg.DeviceArray(nbytes=4 * n * n)
    mxp_c = eng.corr_build(data["bed"][ixs], data["phen"], k, N, P, data["means"][ixs], data["stds"][ixs], Cd.ptr, want_mxp=True)
    assert np.array_equal(_bits(Cd.download(np.float32, (n, n))), _bits(sq)) and np.array_equal(_bits(mxp_c.reshape(k, P)), _bits(mxp))
    # a NaN in the square matrix is 0 in the packed triangle and after nan_to_zero
    hole = sq.copy()
    hole[3, 1] = hole[1, 3] = hole[k - 1, k - 1] = hole[k, 0] = np.nan
    Hd = cg.DeviceArray(hole)
    want = np.where(np.isnan(hole), np.float32(0), hole)
    assert np.array_equal(_bits(eng.pack_lower_tri(Hd.ptr, n, k)), _bits(want[:k, :k][np.tril_indices(k)]))
    eng.nan_to_zero(Hd.ptr, n * n)
    assert np.array_equal(_bits(eng.download(Hd.ptr, np.float32, (n, n))), _bits(want))  # ordered after the engine's stream
    # index lists the build must refuse
    for bad in ([5, 5, 9], [9, 5], [0, data["m"]], [-1, 4]):
        with pytest.raises(RuntimeError, match="ascending"):
            eng.corr_build_indexed(data["bed"], data["phen"], bad, data["m"], N, P, data["means"], data["stds"], Cd.ptr)
    for a in (bed_d, means_d, stds_d, Cd, Hd):
        a.free()
    eng.close()


def test_indexed_build_with_16_byte_rows(synth, oracle):
    """N = 4096: rows of 1024 bytes, the aligned forms of the gather and of the build kernels"""
    import cigwas_amd as cg

    m, n_ind, p, k = 300, 4096, 3, 41
    bed, phen, means, stds, _ = synth.synth_bed_block(m, n_ind, p, block_index=9, miss=0.002)
    ixs = np.sort(np.random.Generator(np.random.PCG64(5)).choice(m, size=k, replace=False)).astype(np.int32)
    ixs[0], ixs[-1] = 0, m - 1
    n = k + p
    eng = cg.Engine(0)
    bed_d, Cd, Cc = cg.DeviceArray(bed), cg.DeviceArray(nbytes=4 * n * n), cg.DeviceArray(nbytes=4 * n * n)
    eng.corr_build_indexed(bed_d, phen, ixs, m, n_ind, p, means, stds, Cd.ptr)
    eng.corr_build(bed[ixs], phen, k, n_ind, p, means[ixs], stds[ixs], Cc.ptr)
    sq = Cd.download(np.float32, (n, n))
    assert np.array_equal(_bits(sq), _bits(Cc.download(np.float32, (n, n))))
    mxm, _, _ = oracle.corr_pearson_npn(bed[ixs], phen, k, n_ind, p, means[ixs], stds[ixs])
    assert np.array_equal(_bits(sq[:k, :k][np.triu_indices(k, 1)]), _bits(mxm))
    for a in (bed_d, Cd, Cc):
        a.free()
    eng.close()


def _check_text_columns(path, dat, names):
    lines = open(path).read().split("\n")
    assert lines[0].split() == ["chr", "snp", "ref"] + names and lines[-1] == "" and len(lines) == dat["m"] + 2
    bim = [ln.split() for ln in open(dat["stem"] + ".bim").read().splitlines()]
    assert [ln.split()[:3] for ln in lines[1:-1]] == [[b[0], b[1], b[4]] for b in bim]


def test_sumstats_files(data, oracle, tmp_path):
    import cigwas_amd as cg
    from cigwas_amd import cli

    ixs, k, m = data["ixs"], len(data["ixs"]), data["m"]
    cli.main(["sumstats", data["stem"], data["phen_path"], str(tmp_path), "--marker-indices", str(data["dir"] / "selected.ixs")])
    ref = _oracle_square(oracle, data, ixs)
    eng = cg.Engine(0)
    sq, mxp_ix, tri = _indexed(eng, data, ixs, data["bed"], data["means"], data["stds"])
    eng.close()
    # mxm.bin: the oracle's triangle, bit for bit
    assert os.path.getsize(tmp_path / "mxm.bin") == 4 * k * (k + 1) // 2
    assert np.array_equal(_bits(np.fromfile(tmp_path / "mxm.bin", np.float32)), _bits(ref[:k, :k][np.tril_indices(k)]))
    assert np.array_equal(_bits(oracle.load_mxm(str(tmp_path / "mxm.bin"))), _bits(ref[:k, :k]))
    # mxp.txt: every marker of the .bim
    names = [f"T{t}" for t in range(P)]
    _check_text_columns(str(tmp_path / "mxp.txt"), data, names)
    mxp_all, _ = oracle.load_mxp(str(tmp_path / "mxp.txt"), list(range(m)))
    mxp_all = np.asarray(mxp_all, np.float32).reshape(m, P)
    want = oracle.marker_phen_corr_pearson(data["bed"], data["phen"], m, N, P, data["means"], data["stds"]).reshape(m, P)
    err = float(np.abs(mxp_all - want).max())
    print(f"sumstats: max |mxp.txt - oracle| over all {m} markers = {err:.3g}")
    assert err <= 1e-5
    assert np.array_equal(_bits(mxp_all[ixs]), _bits(mxp_ix))  # the rows --marker-indices picks = the indexed build's
    mxp_sel, _ = oracle.load_mxp(str(tmp_path / "mxp.txt"), [int(v) for v in ixs])
    assert np.array_equal(_bits(np.asarray(mxp_sel, np.float32).reshape(k, P)), _bits(mxp_ix))
    # pxp.txt
    got_names, pxp, _ = oracle.load_pxp(str(tmp_path / "pxp.txt"), sample_size=float(N))
    assert list(got_names) == names
    err = float(np.abs(pxp - ref[k:, k:]).max())
    print(f"sumstats: max |pxp.txt - oracle| = {err:.3g}")
    assert err <= 1e-5
    assert np.array_equal(_bits(pxp), _bits(sq[k:, k:])) and np.array_equal(_bits(pxp), _bits(pxp.T))
    assert np.array_equal(np.diag(pxp), np.ones(P, np.float32))


def test_sumstats_all_markers_of_one_chromosome(data, oracle, synth, tmp_path):
    """--marker-indices absent: mxm.bin holds the LD of every marker of the file set"""
    from cigwas_amd import cli

    d = tmp_path / "chr2"
    d.mkdir()
    stem = str(d / "geno")
    bed = data["bed"][M1:]
    synth.write_bfiles(stem, bed, N, np.zeros(M2), np.zeros(M2), ["2"] * M2)
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    cli.main(["prep-bed", stem])
    means, stds = np.loadtxt(stem + ".means", dtype=np.float32), np.loadtxt(stem + ".stds", dtype=np.float32)
    out = tmp_path / "out"
    out.mkdir()
    cli.main(["sumstats", stem, data["phen_path"], str(out)])
    mxm, _, _ = oracle.corr_pearson_npn(bed, data["phen"], M2, N, P, means, stds)
    full = np.ones((M2, M2), np.float32)
    iu = np.triu_indices(M2, 1)
    full[iu] = mxm
    full.T[iu] = mxm
    assert not np.isnan(full).any()
    assert os.path.getsize(out / "mxm.bin") == 4 * M2 * (M2 + 1) // 2
    assert np.array_equal(_bits(np.fromfile(out / "mxm.bin", np.float32)), _bits(full[np.tril_indices(M2)]))
    assert len(open(out / "mxp.txt").read().split("\n")) == M2 + 2


@pytest.mark.timeout(1500)
def test_cuskss_merged_from_genotypes_equals_the_file_route(data, oracle, tmp_path):
    from cigwas_amd import cli

    stem, phen_path = data["stem"], data["phen_path"]
    # a real merged_blocks.ixs: block, cusk on every block (one `mps cusk` each), merge-block-outputs
    cli.main(["block", stem, str(MAX_BLOCK), "1", str(WIDTH)])
    blocks = f"{stem}_m{MAX_BLOCK}.blocks"
    nblocks = len(open(blocks).read().splitlines())
    assert nblocks >= 4
    out = tmp_path / "cusk"
    out.mkdir()
    for b in range(nblocks):
        cli.main(["cusk", str(b), blocks, stem, phen_path, str(ALPHA), str(L1), str(L2), str(DEPTH), str(out)])
    cli.main(["merge-block-outputs", str(out), blocks])
    ixs_path = str(out / "merged_blocks.ixs")
    ixs = np.fromfile(ixs_path, np.int32)
    k = len(ixs)
    assert k >= 6 and np.all(np.diff(ixs) > 0) and ixs[-1] < data["m"] and (ixs < M1).any() and (ixs >= M1).any()

    # route one: straight from the genotypes
    direct = tmp_path / "direct"
    direct.mkdir()
    shutil.copy(ixs_path, direct)
    cli.main(["cuskss-merged", "--bfiles", stem, "--phen", phen_path, "--marker-indices", str(direct / "merged_blocks.ixs"),
              "--alpha", str(ALPHA), "--max-level-one", "3", "--max-level-two", "3", "--max-depth", "1", "--outdir", str(direct)])

    # route two: the three files, then cuskss-merged on them
    ss = tmp_path / "sumstats"
    ss.mkdir()
    cli.main(["sumstats", stem, phen_path, str(ss), "--marker-indices", ixs_path])
    files = tmp_path / "files"
    files.mkdir()
    shutil.copy(ixs_path, files)
    cli.main(["cuskss-merged", "--mxm", str(ss / "mxm.bin"), "--mxp", str(ss / "mxp.txt"), "--pxp", str(ss / "pxp.txt"),
              "--marker-indices", str(files / "merged_blocks.ixs"), "--alpha", str(ALPHA), "--max-level-one", "3", "--max-level-two", "3",
              "--max-depth", "1", "--num-samples", str(N), "--outdir", str(files)])
    for f in ("cuskss_merged.mdim", "cuskss_merged.ixs", "cuskss_merged.adj", "cuskss_merged.corr", "cuskss_merged_sam.mtx",
              "cuskss_merged_scm.mtx"):
        _same(str(direct / f), str(files / f))

    # ... and the oracle's hetcor pipeline on the files `sumstats` wrote (the CLI's post-step leaves .mdim / .adj / .corr as
    # `mps` wrote them and replaces .ixs by global marker indices)
    mxm_l = oracle.load_mxm(str(ss / "mxm.bin"))
    _, pxp_l, _ = oracle.load_pxp(str(ss / "pxp.txt"), sample_size=float(N))
    mxp_l, _ = oracle.load_mxp(str(ss / "mxp.txt"), [int(v) for v in ixs])
    sq, es = oracle.make_square_cuskss_inputs(mxm_l, mxp_l, pxp_l, float(N))
    red = oracle.cuskss_from_square(sq, es, P, ALPHA, 3, 3, 1)
    expc = tmp_path / "cuskss_oracle"
    expc.mkdir()
    oracle.write_reduced(red, str(expc / "cuskss_merged"), with_sep=False)
    for ext in (".mdim", ".adj", ".corr"):
        _same(str(direct / "cuskss_merged") + ext, str(expc / "cuskss_merged") + ext)
    assert red.num_var > P + 5  # a graph with markers in it: an empty result would pass every comparison above
