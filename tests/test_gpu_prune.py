"""GPU: `prune-bed` -- the genotype count kernel, the scan kernel alone on the bitmaps of tests/test_prune_cases.py, the
composed cusk_ld_prune against the restated rule applied to the engine's own banded correlations, and `mps prune` through
the CLI.  No tolerance anywhere: statuses and counts are compared by equality, and the correlations the composed step
thresholds are held to the bits `Engine.corr_banded` returns."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_prune_cases import (CONSTANT, KEEP, LD, case_names, check_pruned_fileset, check_properties, constant_restated,
                              counts_restated, expected, pack_bed, planted_genotypes, scan_cases, scan_restated, threshold_bits,
                              write_fileset)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
COUNT_NS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027)
COMPOSED_MS = (1, 2, 64, 65, 600)
COMPOSED_NS = (5, 64, 301)
R_MAXES = (1.0, 0.9, 0.5)


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def count_genotypes(m, N, seed):
    """markers of every kind: random with missing calls, all missing, one genotype (each of the three), two genotypes"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-1, 3, (m, N))
    special = [np.full(N, -1), np.full(N, 0), np.full(N, 1), np.full(N, 2), np.arange(N) % 2, np.arange(N) % 2 + 1,
               np.where(rng.random(N) < 0.5, -1, 2)]
    for k, row in enumerate(special):
        if m > 1:
            g[(1 + 9 * k) % m] = row
    if m == 1:
        g[0] = special[seed % len(special)]
    return g


@pytest.mark.parametrize("m", (1, 65))
@pytest.mark.parametrize("N", COUNT_NS)
def test_counts_equal_numpy_decode(eng, m, N):
    """rows of ceil(N / 4) bytes start at every alignment (the row length is odd for most N); the padding codes of the
    last byte are 00 as PLINK writes them and, in a second run, 11, 10 and 01: they are nobody's genotype either way"""
    for pad in (0, 3, 2, 1):
        g = count_genotypes(m, N, 100 * N + m + pad)
        bed = pack_bed(g, pad_code=pad)
        want = counts_restated(bed, m, N)
        assert np.array_equal(want, np.stack([(g == 2).sum(1), (g == -1).sum(1), (g == 1).sum(1), (g == 0).sum(1)], axis=1))
        assert np.all(want.sum(axis=1) == N)
        out = np.full(4 * m + GUARD, -12345, np.int32)
        got = eng.genotype_counts(bed, m, N, out=out)
        assert np.all(out[4 * m:] == -12345)  # nothing written past the m rows
        assert np.array_equal(got, want), (m, N, pad)
        if m > 1:
            const = constant_restated(want)
            assert np.all(const[[(1 + 9 * k) % m for k in (0, 1, 2, 3, 6)]] == 1)  # all missing, one genotype, one beside missing
            assert N == 1 or np.all(const[[(1 + 9 * k) % m for k in (4, 5)]] == 0)  # two genotypes (one individual has one)


@pytest.mark.parametrize("name", case_names())
def test_scan_equals_the_restated_rule(eng, name):
    bits, const, m, W, _kind = scan_cases()[name]
    out = np.full(m + GUARD, 0xAB, np.uint8)
    got = eng.ld_prune_scan(bits, const, m, W, out=out)
    assert np.all(out[m:] == 0xAB)
    assert np.array_equal(got, expected(name)), name


def composed_expected(eng, bed, m, N, W, r_max):
    _sums, band = eng.corr_banded(bed, m, N, W, want_band=True)
    counts = counts_restated(bed, m, N)
    const = constant_restated(counts)
    bits = threshold_bits(band, m, W, r_max)
    st = scan_restated(bits, const, m, W)
    check_properties(bits, const, m, W, st)
    return st, counts, band


def windows_of(m):
    return sorted({1, 2, 63, 64, 65, 130, m + 5})


@pytest.mark.parametrize("N", COMPOSED_NS)
@pytest.mark.parametrize("m", COMPOSED_MS)
def test_composed_equals_rule_on_the_engines_own_band(eng, m, N):
    for W in windows_of(m):
        g = planted_genotypes(m, N, W, 31 * m + N)
        bed = pack_bed(g)
        for r_max in R_MAXES:
            want, counts, band = composed_expected(eng, bed, m, N, W, r_max)
            got, got_counts = eng.ld_prune(bed, m, N, W, r_max, want_counts=True)
            assert np.array_equal(got_counts, counts), (m, N, W)
            assert np.array_equal(got, want), (m, N, W, r_max, np.flatnonzero(got != want)[:10])
            if m == 600 and N == 301 and W in (65, 130):
                assert {KEEP, CONSTANT, LD} == set(want.tolist()), (W, r_max)
                if W == 65:
                    # the planted duplicates at distance W and W + 1: inside and outside the window
                    assert band[30, W - 1] == 1.0 and want[30] == KEEP and want[30 + W] == LD
                    a = 31 + W + 40
                    assert want[a] == KEEP and want[a + W + 1] == KEEP
        # without counts
        assert np.array_equal(eng.ld_prune(bed, m, N, W, R_MAXES[-1]), want)


def test_two_chromosomes_no_window_crosses_the_boundary(eng):
    """the last marker of the first chromosome and the first of the second are duplicates: run per chromosome, as `mps
    prune` does, both stay; run as one chromosome the second goes"""
    m1, m2, N, W = 70, 50, 101, 20
    g = planted_genotypes(m1 + m2, N, W, 9)
    g[m1] = g[m1 - 1]
    bed = pack_bed(g)
    whole = eng.ld_prune(bed, m1 + m2, N, W, 1.0)
    assert whole[m1 - 1] == KEEP and whole[m1] == LD
    first, second = eng.ld_prune(bed[:m1], m1, N, W, 1.0), eng.ld_prune(bed[m1:], m2, N, W, 1.0)
    assert first[m1 - 1] == KEEP and second[0] == KEEP
    assert np.array_equal(first, composed_expected(eng, bed[:m1], m1, N, W, 1.0)[0])
    assert np.array_equal(second, composed_expected(eng, bed[m1:], m2, N, W, 1.0)[0])


def _cli(*argv):
    return subprocess.run([sys.executable, "-c", "import sys, cigwas_amd.cli as c; c.main(sys.argv[1:])", *argv], cwd=ROOT,
                          capture_output=True, text=True)


def test_mps_prune_files_then_prep_and_band(eng, tmp_path):
    import cigwas_amd as cg

    m1, m2, N, W = 70, 50, 101, 20
    g = planted_genotypes(m1 + m2, N, W, 9)
    g[m1] = g[m1 - 1]
    bed = pack_bed(g)
    chr_ids = ["1"] * m1 + ["2"] * m2
    src = str(tmp_path / "in")
    write_fileset(src, bed, N, chr_ids)
    for r_max in (1.0, 0.5):
        out, want_stem = str(tmp_path / f"out{r_max}"), str(tmp_path / f"want{r_max}")
        r = _cli("prune-bed", src, out, "--r-max", str(r_max), "--window", str(W))
        assert r.returncode == 0, r.stdout + r.stderr
        status = np.concatenate([eng.ld_prune(bed[:m1], m1, N, W, r_max), eng.ld_prune(bed[m1:], m2, N, W, r_max)])
        assert {KEEP, CONSTANT, LD} == set(status.tolist())
        assert status[m1 - 1] == KEEP and status[m1] == KEEP
        for cid, st in (("1", status[:m1]), ("2", status[m1:])):
            line = (f"[Chr {cid}]: {len(st)} markers: {(st == KEEP).sum()} kept, {(st == CONSTANT).sum()} constant, "
                    f"{(st == LD).sum()} dropped for LD.")
            assert line in r.stdout, r.stdout
        cg.prune_write(src, want_stem, status)
        check_pruned_fileset(src, want_stem, bed, status)
        for sfx in (".bed", ".bim", ".fam", ".prune.in", ".prune.out"):
            assert open(out + sfx, "rb").read() == open(want_stem + sfx, "rb").read(), sfx
        # prep-bed on the result: no marker without variation is left
        r = _cli("prep-bed", out)
        assert r.returncode == 0, r.stdout + r.stderr
        stds = np.array([float(x) for x in open(out + ".stds").read().split()])
        kept = np.flatnonzero(status == KEEP)
        assert len(stds) == len(kept) and np.all(stds > 0)
        if r_max == 1.0:
            # and no pair within the window is collinear
            for lo, hi in ((0, (status[:m1] == KEEP).sum()), ((status[:m1] == KEEP).sum(), len(kept))):
                rows = bed[kept[lo:hi]]
                _sums, band = eng.corr_banded(rows, len(rows), N, W, want_band=True)
                with np.errstate(invalid="ignore"):
                    assert not np.any(np.abs(band) >= np.float32(1.0))


def test_argument_errors_launch_nothing_and_leave_the_engine_usable(eng):
    from cigwas_amd._lib import lib

    L = lib()
    m, N, W = 10, 9, 4
    bed = pack_bed(planted_genotypes(m, N, W, 3))
    status = np.full(m + GUARD, 0xAB, np.uint8)
    counts = np.full(4 * m + GUARD, -5, np.int32)
    bits = np.zeros((m, 1), np.uint64)
    flags = np.zeros(m, np.uint8)
    ARG = 2
    bad_prune = [(None, m, N, W, 0.5, _ptr(status), None), (_ptr(bed), m, N, W, 0.5, None, None), (_ptr(bed), 0, N, W, 0.5, _ptr(status), None),
                 (_ptr(bed), m, 0, W, 0.5, _ptr(status), None), (_ptr(bed), m, N, 0, 0.5, _ptr(status), None),
                 (_ptr(bed), m, N, 4097, 0.5, _ptr(status), None), (_ptr(bed), m, N, W, 0.0, _ptr(status), _ptr(counts)),
                 (_ptr(bed), m, N, W, -0.5, _ptr(status), None), (_ptr(bed), m, N, W, 1.0001, _ptr(status), None),
                 (_ptr(bed), m, N, W, float("nan"), _ptr(status), _ptr(counts))]
    for args in bad_prune:
        assert L.cusk_ld_prune(eng.h, *args) == ARG, args[1:5]
    assert L.cusk_ld_prune(None, _ptr(bed), m, N, W, 0.5, _ptr(status), None) == ARG
    bad_counts = [(None, m, N, _ptr(counts)), (_ptr(bed), 0, N, _ptr(counts)), (_ptr(bed), m, 0, _ptr(counts)), (_ptr(bed), m, N, None)]
    for args in bad_counts:
        assert L.cusk_genotype_counts(eng.h, *args) == ARG
    bad_scan = [(None, _ptr(flags), m, W, _ptr(status)), (_ptr(bits), None, m, W, _ptr(status)), (_ptr(bits), _ptr(flags), 0, W, _ptr(status)),
                (_ptr(bits), _ptr(flags), m, 0, _ptr(status)), (_ptr(bits), _ptr(flags), m, 4097, _ptr(status)),
                (_ptr(bits), _ptr(flags), m, W, None)]
    for args in bad_scan:
        assert L.cusk_ld_prune_scan(eng.h, *args) == ARG
    assert np.all(status == 0xAB) and np.all(counts == -5)
    with pytest.raises(RuntimeError):
        eng.ld_prune(bed, m, N, W, 0.0)
    # the engine is usable afterwards, and the largest window is accepted
    want = composed_expected(eng, bed, m, N, W, 0.5)[0]
    assert np.array_equal(eng.ld_prune(bed, m, N, W, 0.5), want)
    assert np.array_equal(eng.ld_prune(bed, m, N, 4096, 0.5), composed_expected(eng, bed, m, N, 4096, 0.5)[0])
