"""GPU: polychoric / polyserial correlations of ordinal traits (csrc/ordinal.hip) -- the table kernel by equality with a
numpy decode, the fit kernels against the float64 oracle of ordinal_ref64.py, and `sumstats --ordinal` /
`cuskss-merged --bfiles --het --ordinal` end to end.

Tolerances.  Largest deviations from the oracle measured over the cases of this file on an MI355X (printed by the tests):
see MEASURED below; the bounds are ten times those, and neither may exceed 1e-6 (the results leave as float32).
"""
import os
import pathlib
import shutil

import numpy as np
import pytest

import ordinal_cases as cases_mod
import ordinal_ref64 as R
from ordinal_cases import fit_cases

pytestmark = pytest.mark.gpu

# measured on the first run: max |rho - oracle| and max |se / oracle - 1| over the polychoric tables and polyserial pairs
MEASURED = dict(rho=9.85e-11, se=6.04e-9)  # both at the polychoric tables; polyserial: 1.3e-15 and 5.2e-13
RHO_TOL, SE_TOL = 10 * MEASURED["rho"], 10 * MEASURED["se"]
assert RHO_TOL <= 1e-6 and SE_TOL <= 1e-6


# ------------------------------------------------------------------------------------------------ tables
def _decode(bed_rows, n):
    return np.stack([R.bed_class_codes(row, n) for row in bed_rows])


def _tables_numpy(bed_rows, phen, n, ord_ix, levels, nlev):
    cls = _decode(bed_rows, n)
    q = len(ord_ix)
    codes = []
    for t, ix in enumerate(ord_ix):
        c, _ = R.codes_of(phen[ix], levels[t, :nlev[t]])
        codes.append(c)
    mxo = np.zeros((len(bed_rows), q, 3, 8), np.int32)
    for i in range(len(bed_rows)):
        for t in range(q):
            mxo[i, t] = R.pair_table(cls[i], codes[t], 3, 8)
    oxo = np.zeros((q, q, 8, 8), np.int32)
    for a in range(q):
        for b in range(q):
            oxo[a, b] = R.pair_table(codes[a], codes[b], 8, 8)
    return mxo, oxo


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4099])
def test_tables_equal_a_numpy_decode(n):
    import cigwas_amd as cg

    class _View(cg.DeviceArray):
        """rows inside another allocation, which stays the owner"""

        def __init__(self, base, off, nbytes):
            self.ptr, self.nbytes = base.ptr + off, nbytes

        def free(self):
            self.ptr = None

    rng = np.random.Generator(np.random.PCG64(500 + n))
    clb, m = (n + 3) // 4, 23
    rows = rng.integers(0, 256, (m, clb), dtype=np.uint8)  # all four codes, random bits in the padding of the last byte
    rows[3] = 0xFF  # a single class (and garbage in the padding)
    rows[4] = 0x55  # every call missing
    p, ks = 5, (2, 3, 8)
    phen = rng.standard_normal((p, n)).astype(np.float32)
    ord_ix = np.array([4, 0, 2], np.int32)
    for t, K in zip(ord_ix, ks):
        phen[t] = rng.integers(0, K, n).astype(np.float32) * 1.5 - 1.0
        phen[t, rng.random(n) < 0.2] = np.nan
    # a level of the second trait that never occurs together with the upper level of the first
    phen[0, phen[4] == 0.5] = np.where(phen[0, phen[4] == 0.5] == 2.0, 0.5, phen[0, phen[4] == 0.5])
    levels, nlev = np.zeros((3, 8), np.float32), np.zeros(3, np.int32)
    for t, (ix, K) in enumerate(zip(ord_ix, ks)):
        levels[t, :K], nlev[t] = np.arange(K, dtype=np.float32) * 1.5 - 1.0, K  # all K levels, seen or not
    want_mxo, want_oxo = _tables_numpy(rows, phen, n, ord_ix, levels, nlev)
    eng = cg.Engine(0)
    got_mxo, got_oxo = eng.ordinal_tables(rows, phen, n, p, ord_ix, levels, nlev)
    assert np.array_equal(got_mxo, want_mxo) and np.array_equal(got_oxo, want_oxo)
    assert not got_mxo[4].any() and not got_mxo[3, :, 1:].any()
    assert np.array_equal(got_oxo, got_oxo.transpose(1, 0, 3, 2))
    # rows at byte offsets 0, 1 and 15 of a poisoned device buffer, garbage behind them; device-resident phenotypes
    phen_d = cg.DeviceArray(phen)
    for off in (0, 1, 15):
        buf = np.full(off + m * clb + 64, 0xA7, np.uint8)
        buf[off:off + m * clb] = rows.reshape(-1)
        buf_d = cg.DeviceArray(buf)
        view = _View(buf_d, off, m * clb)
        dev_mxo, dev_oxo = eng.ordinal_tables(view, phen_d, n, p, ord_ix, levels, nlev)
        assert np.array_equal(dev_mxo, want_mxo) and np.array_equal(dev_oxo, want_oxo), off
        # a scattered index list from the resident rows
        ix = np.array([0, 3, 4, 9, 22], np.int32)
        ix_mxo, _ = eng.ordinal_tables(view, phen_d, n, p, ord_ix, levels, nlev, marker_ix=ix, m_total=m)
        assert np.array_equal(ix_mxo, want_mxo[ix]), off
        buf_d.free()
    ix_mxo, _ = eng.ordinal_tables(rows, phen, n, p, ord_ix, levels, nlev, marker_ix=ix, m_total=m)
    assert np.array_equal(ix_mxo, want_mxo[ix])
    _, only_oxo = eng.ordinal_tables(None, phen, n, p, ord_ix, levels, nlev, want_mxo=False)
    assert np.array_equal(only_oxo, want_oxo)
    phen_d.free()
    eng.close()


# ------------------------------------------------------------------------------------------------ fits
@pytest.fixture(scope="module")
def fit_oracle():
    cases = fit_cases()
    return cases, [R.polychoric(t) for _, t, _ in cases]


def test_polychoric_fits_match_the_oracle(fit_oracle):
    import cigwas_amd as cg

    cases, want = fit_oracle
    assert 280 <= len(cases) <= 320
    eng = cg.Engine(0)
    got = [None] * len(cases)
    for shape in sorted({s for s, _, _ in cases}):
        idx = [i for i, (s, _, _) in enumerate(cases) if s == shape]
        r, se, st = eng.polychoric_fit(np.stack([cases[i][1] for i in idx]).astype(np.int32))
        for j, i in enumerate(idx):
            got[i] = (r[j], se[j], st[j])
    # the same tables padded to 3 x 8 / 8 x 8 with empty levels, as cusk_ordinal_tables hands them over: the same bits
    idx = [i for i, (s, _, _) in enumerate(cases) if s[0] <= 3]
    padded = np.zeros((len(idx), 3, 8), np.int32)
    for j, i in enumerate(idx):
        t = cases[i][1]
        padded[j, :t.shape[0], :t.shape[1]] = t
    tab_d = cg.DeviceArray(padded)
    r, se, st = eng.polychoric_fit(tab_d, ka=3, kb=8, ntab=len(idx))
    tab_d.free()
    eng.close()
    for j, i in enumerate(idx):
        assert st[j] == got[i][2] and np.array_equal([r[j], se[j]], [got[i][0], got[i][1]], equal_nan=True), i

    left_out, random_total, d_rho, d_se = 0, 0, 0.0, 0.0
    for (shape, t, is_random), (wr, wse, wst), (gr, gse, gst) in zip(cases, want, got):
        assert gst == wst, (t, wst, gst)  # statuses by equality
        random_total += is_random
        if wst == R.DEGENERATE:
            assert np.isnan(gr) and np.isnan(gse)
            left_out += is_random
        elif wst == R.BOUNDARY:
            assert np.isnan(gse) and (gr == wr if abs(wr) == R.RHO_MAX else abs(gr - wr) <= RHO_TOL)
            left_out += is_random
        else:
            d_rho, d_se = max(d_rho, abs(gr - wr)), max(d_se, abs(gse / wse - 1.0))
    print(f"polychoric: {len(cases)} tables, max |rho - oracle| = {d_rho:.3g}, max |se / oracle - 1| = {d_se:.3g}, "
          f"{left_out} of {random_total} random tables boundary or degenerate")
    assert left_out <= 0.02 * random_total
    assert d_rho <= RHO_TOL and d_se <= SE_TOL


@pytest.mark.parametrize("n, K", [(65, 2), (65, 5), (4099, 2), (4099, 5)])
def test_polyserial_matches_the_oracle(n, K):
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(77 + n + K))
    p = 4
    phen = rng.standard_normal((p, n)).astype(np.float32)
    latent = 0.6 * phen[0] - 0.4 * phen[2] + rng.standard_normal(n)
    cuts = np.quantile(latent, np.linspace(0, 1, K + 1)[1:-1])
    phen[3] = np.searchsorted(cuts, latent).astype(np.float32)
    for t, rate in ((0, 0.1), (1, 0.0), (2, 0.3), (3, 0.15)):
        phen[t, rng.random(n) < rate] = np.nan
    phen[1, :] = 2.5  # a constant partner: degenerate
    ord_ix, cont_ix = [3], [0, 1, 2]
    levels, nlev = cg.ordinal_levels(phen, ord_ix)
    eng = cg.Engine(0)
    r, se, st = eng.polyserial_fit(phen, n, p, cont_ix, ord_ix, levels, nlev)
    phen_d = cg.DeviceArray(phen)
    r2, se2, st2 = eng.polyserial_fit(phen_d, n, p, cont_ix, ord_ix, levels, nlev)
    phen_d.free()
    eng.close()
    assert np.array_equal(r, r2, equal_nan=True) and np.array_equal(se, se2, equal_nan=True) and np.array_equal(st, st2)
    codes, _ = R.codes_of(phen[3])
    d_rho = d_se = 0.0
    for j, c in enumerate(cont_ix):
        wr, wse, wst = R.polyserial(phen[c], codes)
        assert st[j, 0] == wst, (c, wst, st[j, 0])
        if wst == R.OK:
            d_rho, d_se = max(d_rho, abs(r[j, 0] - wr)), max(d_se, abs(se[j, 0] / wse - 1.0))
        else:
            assert np.isnan(se[j, 0])
    print(f"polyserial n={n} K={K}: max |rho - oracle| = {d_rho:.3g}, max |se / oracle - 1| = {d_se:.3g}")
    assert st[0, 0] == R.OK and st[1, 0] == R.DEGENERATE and st[2, 0] == R.OK
    assert d_rho <= RHO_TOL and d_se <= SE_TOL


# ------------------------------------------------------------------------------------------------ routes
M, N, P, K_SEL = 300, 1000, 6, 60
ORD = (1, 4)  # 0-based: a binary trait at 10 % prevalence and a four-grade trait
ALPHA, L1, L2, DEPTH = 1e-3, 2, 2, 1
FILES = ("cuskss_merged.mdim", "cuskss_merged.ixs", "cuskss_merged.adj", "cuskss_merged.corr", "cuskss_merged_sam.mtx",
         "cuskss_merged_scm.mtx")


@pytest.fixture(scope="module")
def data(tmp_path_factory, synth):
    from cigwas_amd import cli

    d = pathlib.Path(tmp_path_factory.mktemp("ordinal"))
    rng = synth.rng_for(4242)
    G = synth.make_genotypes(M, N, rng, miss=0.02)
    g = G.astype(np.float64)
    g[G < 0] = np.nan
    gs = np.nan_to_num((g - np.nanmean(g, 1, keepdims=True)) / np.nanstd(g, 1, keepdims=True))
    Y = np.zeros((P, N))
    for t in range(P):
        idx = rng.choice(M, size=5, replace=False)
        y = (rng.uniform(0.15, 0.3, 5) * rng.choice([-1.0, 1.0], 5)) @ gs[idx] + rng.standard_normal(N)
        if t:
            y = y + 0.4 * Y[t - 1]
        Y[t] = (y - y.mean()) / y.std()
    Y[ORD[0]] = (Y[ORD[0]] > np.quantile(Y[ORD[0]], 0.9)).astype(np.float64)
    Y[ORD[1]] = np.searchsorted(np.quantile(Y[ORD[1]], [0.3, 0.6, 0.85]), Y[ORD[1]]).astype(np.float64)
    Y = Y.astype(np.float32)
    for t, rate in enumerate((0.0, 0.05, 0.2, 0.0, 0.1, 0.3)):
        Y[t, rng.random(N) < rate] = np.nan
    ixs = np.sort(rng.choice(M, size=K_SEL, replace=False)).astype(np.int32)
    stem = str(d / "geno")
    bed = synth.pack_bed(G)
    synth.write_bfiles(stem, bed, N, np.zeros(M), np.zeros(M), ["1"] * 170 + ["2"] * (M - 170))
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    synth.write_phen(str(d / "y.phen"), np.ascontiguousarray(Y).reshape(-1), N, P)
    cli.main(["prep-bed", stem])
    ixs.tofile(str(d / "merged_blocks.ixs"))
    names = open(d / "y.phen").readline().split()[2:]
    se, ordinal = d / "se", d / "ordinal"
    se.mkdir()
    ordinal.mkdir()
    common = ["sumstats", stem, str(d / "y.phen")]
    cli.main(common + [str(se), "--marker-indices", str(d / "merged_blocks.ixs"), "--se"])
    cli.main(common + [str(ordinal), "--marker-indices", str(d / "merged_blocks.ixs"), "--ordinal", f"{names[ORD[0]]},{ORD[1] + 1}"])
    return dict(dir=d, stem=stem, phen_path=str(d / "y.phen"), ixs_path=str(d / "merged_blocks.ixs"), se=se, ordinal=ordinal,
                bed=bed, Y=Y, names=names)


def _mxp_columns(path):
    lines = open(path).read().splitlines()
    return lines[0].split(), [ln.split() for ln in lines[1:]]


def _f32(tok):
    return np.float32(np.nan) if tok in ("NA", "nan") else np.float32(tok)


def test_sumstats_ordinal_files(data):
    se, od = data["se"], data["ordinal"]
    assert sorted(os.listdir(od)) == ["mxm.bin", "mxp.txt", "mxp_se.txt", "pxp.txt", "pxp_se.txt"]
    assert open(se / "mxm.bin", "rb").read() == open(od / "mxm.bin", "rb").read()
    cont = [t for t in range(P) if t not in ORD]
    Y, bed = data["Y"], data["bed"]
    codes = {t: R.codes_of(Y[t])[0] for t in ORD}
    d_rho = d_se = 0.0

    def check(tok_r, tok_se, want):
        nonlocal d_rho, d_se
        wr, wse, wst = want
        gr, gse = _f32(tok_r), _f32(tok_se)
        assert np.isnan(gr) == np.isnan(wr) and np.isnan(gse) == np.isnan(wse), (tok_r, tok_se, want)
        if wst == R.OK:
            # float32 rounding of a value within the bound of the oracle's
            assert abs(float(gr) - wr) <= RHO_TOL + 6e-8 * abs(wr) and abs(float(gse) / wse - 1.0) <= SE_TOL + 6e-8
            d_rho, d_se = max(d_rho, abs(float(gr) - wr)), max(d_se, abs(float(gse) / wse - 1.0))

    for f in ("mxp.txt", "mxp_se.txt"):
        h0, r0 = _mxp_columns(se / f)
        h1, r1 = _mxp_columns(od / f)
        assert h0 == h1 and len(r0) == len(r1) == M
        for a, b in zip(r0, r1):
            assert a[:3] == b[:3] and [a[3 + t] for t in cont] == [b[3 + t] for t in cont]  # the same text
    _, rr = _mxp_columns(od / "mxp.txt")
    _, rs = _mxp_columns(od / "mxp_se.txt")
    for i in range(M):  # every marker against the oracle
        cls = R.bed_class_codes(bed[i], N)
        for t in ORD:
            check(rr[i][3 + t], rs[i][3 + t], R.polychoric(R.pair_table(cls, codes[t], 3, 8)))
    for f in ("pxp.txt", "pxp_se.txt"):
        a = [ln.split() for ln in open(se / f).read().splitlines()]
        b = [ln.split() for ln in open(od / f).read().splitlines()]
        assert a[0] == b[0]
        for x in cont:
            assert [a[1 + x][1 + y] for y in cont] == [b[1 + x][1 + y] for y in cont]
        for x in range(P):
            assert a[1 + x][0] == b[1 + x][0] and a[1 + x][1 + x] == b[1 + x][1 + x]  # labels and diagonal
    pr = [ln.split()[1:] for ln in open(od / "pxp.txt").read().splitlines()[1:]]
    ps = [ln.split()[1:] for ln in open(od / "pxp_se.txt").read().splitlines()[1:]]
    for o in ORD:
        for x in range(P):
            if x == o:
                continue
            assert pr[x][o] == pr[o][x] and ps[x][o] == ps[o][x]
            if x in ORD:
                a, b = min(x, o), max(x, o)
                want = R.polychoric(R.pair_table(codes[a], codes[b], 8, 8))
            else:
                want = R.polyserial(Y[x], codes[o])
            check(pr[x][o], ps[x][o], want)
    print(f"sumstats --ordinal: max |r - oracle| = {d_rho:.3g}, max |se / oracle - 1| = {d_se:.3g} after float32 rounding")


def _merged(cli, data, outdir, extra):
    outdir.mkdir()
    shutil.copy(data["ixs_path"], outdir)
    cli.main(["cuskss-merged", "--marker-indices", str(outdir / "merged_blocks.ixs"), "--alpha", str(ALPHA), "--max-level-one", str(L1),
              "--max-level-two", str(L2), "--max-depth", str(DEPTH), "--outdir", str(outdir)] + extra)


def test_cuskss_merged_ordinal_equals_the_file_route(data, tmp_path):
    from cigwas_amd import cli

    od = data["ordinal"]
    spec = f"{ORD[0] + 1},{data['names'][ORD[1]]}"
    _merged(cli, data, tmp_path / "direct", ["--bfiles", data["stem"], "--phen", data["phen_path"], "--het", "--ordinal", spec])
    _merged(cli, data, tmp_path / "files", ["--mxm", str(od / "mxm.bin"), "--mxp", str(od / "mxp.txt"), "--pxp", str(od / "pxp.txt"),
                                            "--mxp-se", str(od / "mxp_se.txt"), "--pxp-se", str(od / "pxp_se.txt"),
                                            "--num-samples", str(N)])
    outdir = tmp_path / "files"
    produced = sorted(f for f in os.listdir(outdir) if f.startswith("cuskss_merged"))
    assert produced == sorted(f for f in os.listdir(tmp_path / "direct") if f.startswith("cuskss_merged"))
    for f in produced:
        assert open(tmp_path / "direct" / f, "rb").read() == open(outdir / f, "rb").read(), f
    assert set(FILES) <= set(produced)

def _edge_in(outdir, marker, trait):
    """is selected marker `marker` adjacent to trait `trait` in the result files?  Retained markers come first (their
    positions in the selection are in .ixs), then all traits"""
    nv, npn = (int(v) for v in open(outdir / "cuskss_merged.mdim").read().split()[:2])
    kept = [int(v) for v in np.fromfile(str(outdir / "cuskss_merged.ixs"), np.int32)][:nv - npn]
    adj = np.fromfile(str(outdir / "cuskss_merged.adj"), np.int32).reshape(nv, nv)
    return marker in kept and bool(adj[kept.index(marker), nv - npn + trait])


def test_planted_edge_survives_with_ordinal_only(tmp_path, synth):
    """the planted marker-disease edge (ordinal_cases.planted_set) through `sumstats --ordinal` + the file route, through
    `cuskss-merged --bfiles --het --ordinal`, and through plain `--het`, at the alpha chosen on the CPU with the oracle
    (test_ordinal_formats.py checks that choice): kept by both ordinal routes, removed without the option"""
    from cigwas_amd import cli

    G, phen = cases_mod.planted_set()
    k, n, p = cases_mod.PLANTED_K, cases_mod.PLANTED_N, cases_mod.PLANTED_TRAITS
    stem, phen_path, ixs_path = str(tmp_path / "geno"), str(tmp_path / "y.phen"), str(tmp_path / "merged_blocks.ixs")
    synth.write_bfiles(stem, synth.pack_bed(G.astype(np.int8)), n, np.zeros(k), np.zeros(k), ["1"] * k)
    for sfx in (".dim", ".means", ".stds"):
        os.remove(stem + sfx)
    synth.write_phen(phen_path, np.ascontiguousarray(phen).reshape(-1), n, p)
    cli.main(["prep-bed", stem])
    np.arange(k, dtype=np.int32).tofile(ixs_path)
    files = tmp_path / "sumstats"
    files.mkdir()
    spec = str(cases_mod.PLANTED_DISEASE + 1)
    cli.main(["sumstats", stem, phen_path, str(files), "--marker-indices", ixs_path, "--ordinal", spec])

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        shutil.copy(ixs_path, out)
        cli.main(["cuskss-merged", "--marker-indices", str(out / "merged_blocks.ixs"), "--alpha", repr(cases_mod.PLANTED_ALPHA),
                  "--max-level-one", str(cases_mod.PLANTED_L1), "--max-level-two", str(cases_mod.PLANTED_L2), "--outdir", str(out)] + extra)
        return _edge_in(out, cases_mod.PLANTED_MARKER, cases_mod.PLANTED_DISEASE)

    geno = ["--bfiles", stem, "--phen", phen_path, "--het"]
    assert run("direct", geno + ["--ordinal", spec])
    assert run("files", ["--mxm", str(files / "mxm.bin"), "--mxp", str(files / "mxp.txt"), "--pxp", str(files / "pxp.txt"),
                         "--mxp-se", str(files / "mxp_se.txt"), "--pxp-se", str(files / "pxp_se.txt"), "--num-samples", str(n)])
    assert not run("plain", geno)
    for f in FILES:
        assert open(tmp_path / "direct" / f, "rb").read() == open(tmp_path / "files" / f, "rb").read(), f
