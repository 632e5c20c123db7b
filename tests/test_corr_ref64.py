"""CPU: the float64 reference of the correlation build (oracle/ref64.py), pinned against textbook implementations, and the
oracle's C restatement (oracle.corr_pearson_npn, oracle.marker_corr_banded) against it on the data edges, up to 70k
individuals.  ref64 starts from the dosages, not from .bed bytes, so it shares no decoding and no arithmetic with the
oracle or the kernels."""
import numpy as np
import pytest

from oracle import ref64


def _pairwise(G, x, y):
    ok = (G[x] >= 0) & (G[y] >= 0)
    return G[x][ok].astype(np.float64), G[y][ok].astype(np.float64)


@pytest.mark.parametrize("m,N,miss,seed", [(6, 40, 0.0, 0), (7, 301, 0.1, 1), (9, 1000, 0.3, 2), (8, 17, 0.5, 3)])
def test_ref64_tau_b_against_scipy(m, N, miss, seed):
    from scipy.stats import kendalltau

    G, _ = ref64.make_case(m, N, 1, seed, miss=miss, edges=False)
    G[0, : N // 2] = 1  # a marker with many ties
    R = ref64.mxm(G)
    for x in range(m):
        for y in range(x + 1, m):
            a, b = _pairwise(G, x, y)
            if a.size < 2 or np.all(a == a[0]) or np.all(b == b[0]):
                assert np.isnan(R[x, y]), (x, y)
                continue
            tau = kendalltau(a, b, variant="b").statistic
            assert abs(R[x, y] - np.sin(np.pi / 2 * tau)) <= 1e-12, (x, y)
            assert R[x, y] == R[y, x]


def test_ref64_pearson_forms_against_a_loop():
    G, Y = ref64.make_case(8, 211, 5, 4, miss=0.2)
    mean, sd = ref64.stats(G)
    r, s_abs = ref64.mxp(G, Y, mean, sd)
    for x in range(8):
        for t in range(5):
            sgy = sy = sa = n = 0.0
            for i in range(211):
                g, y = int(G[x, i]), float(Y[t, i])
                if g < 0 or np.isnan(y):
                    continue
                sgy += g * y
                sy += y
                sa += abs(g * y) + abs(float(mean[x])) * abs(y)
                n += 1
            den = n * float(sd[x])
            want = (sgy - float(mean[x]) * sy) / den if den else np.nan
            if not np.isfinite(want):
                assert not np.isfinite(r[x, t])
            else:
                assert abs(r[x, t] - want) <= 1e-12 * max(1.0, abs(want)), (x, t)
                assert abs(s_abs[x, t] - sa / den) <= 1e-12 * s_abs[x, t]
    q, q_abs = ref64.pxp(Y)
    for a in range(5):
        for b in range(5):
            ok = ~np.isnan(Y[a]) & ~np.isnan(Y[b])
            want = np.sum(Y[a][ok].astype(np.float64) * Y[b][ok]) / ok.sum() if ok.any() else np.nan
            assert (np.isnan(want) and np.isnan(q[a, b])) or abs(q[a, b] - want) <= 1e-12 * max(1.0, abs(want))


def test_ref64_banded_form():
    G, _ = ref64.make_case(300, 150, 1, 5, miss=0.05)
    band, sums = ref64.banded(G, 40)
    full = ref64.mxm(G)
    for row in (0, 1, 255, 256, 259, 299):
        k = min(40, 299 - row)
        assert np.array_equal(band[row, :k], full[row, row + 1: row + 1 + k], equal_nan=True)
        assert np.all(band[row, k:] == 0)
    assert np.allclose(sums, np.abs(band).sum(axis=1), equal_nan=True)


# oracle.corr_pearson_npn's summation: 512 threads, each a chain of N / 512 additions, then a 9-level scan
def _oracle_chain(N):
    return N / 512 + 9


# (m, N, p, miss): the boundary each case hits
ORACLE_CASES = [
    (1, 5, 1, 0.0),          # one marker, one trait: no SNP x SNP pair, N % 4 = 1
    (2, 3, 2, 0.0),          # N < 4: one partial .bed byte per row
    (9, 64, 4, 0.01),        # the edges (all-missing, monomorphic 0 / 2, heterozygous-only) at a byte-aligned N
    (12, 1027, 6, 0.60),     # 60 % missing genotypes; N % 4 = 3
    (10, 16388, 5, 0.01),    # N above 2^14, traits scaled by 1e-3 / 1e3
    (7, 70001, 4, 0.01),     # N ~ 70k: the largest the oracle comparisons keep to 1e-5
]


@pytest.mark.parametrize("m,N,p,miss", ORACLE_CASES)
def test_oracle_corr_against_ref64(oracle, synth, m, N, p, miss):
    G, Y = ref64.make_case(m, N, p, seed=m * 7 + N, miss=miss)
    mean, sd = ref64.stats(G)
    bed = synth.pack_bed(G)
    o_mxm, o_mxp, o_pxp = oracle.corr_pearson_npn(bed, Y.reshape(-1), m, N, p, mean, sd)
    iu, ip = np.triu_indices(m, 1), np.triu_indices(p, 1)
    R = ref64.mxm(G)
    ref64.check_mxm_nan("oracle mxm", o_mxm, R[iu])
    r, s_abs = ref64.mxp(G, Y, mean, sd)
    cap = ref64.cap_1e5(sd, Y, N)
    bar = ref64.sum_bar(s_abs, _oracle_chain(N), cap)
    ref64.check_close("oracle mxp", np.asarray(o_mxp).reshape(m, p), r, bar)
    q, q_abs = ref64.pxp(Y)
    qbar = ref64.sum_bar(q_abs, _oracle_chain(N))
    ref64.check_close("oracle pxp", o_pxp, q[ip], qbar[ip])
    # the zero-padded and the randomly padded .bed give the same answers
    if N % 4:
        bed2 = ref64.random_padding(bed, N, seed=N)
        assert not np.array_equal(bed2, bed) or m == 1
        o2 = oracle.corr_pearson_npn(bed2, Y.reshape(-1), m, N, p, mean, sd)
        for a, b in zip(o2, (o_mxm, o_mxp, o_pxp)):
            assert np.array_equal(a, b, equal_nan=True)
    # sensitivity: without the last individual some element moves by more than 4x its bar
    r1, _ = ref64.mxp(G[:, :-1], Y[:, :-1], mean, sd)
    q1, _ = ref64.pxp(Y[:, :-1])
    R1 = ref64.mxm(G[:, :-1])
    mv = max(ref64.moved(r, r1, bar), ref64.moved(q[ip], q1[ip], qbar[ip]), ref64.moved(R[iu], R1[iu], ref64.MXM_BAR))
    assert mv > 4, f"the bars cannot see a lost individual (largest move {mv:.3g} bars)"


@pytest.mark.parametrize("m,N,width", [(70, 777, 16), (300, 259, 64), (40, 20001, 50)])
def test_oracle_banded_against_ref64(oracle, synth, m, N, width):
    G, _ = ref64.make_case(m, N, 1, seed=N, miss=0.02)
    band, sums = ref64.banded(G, width)
    o_band = oracle.marker_corr_banded(synth.pack_bed(G), m, N, width)
    ref64.check_mxm_nan("oracle band", o_band, band)
    o_sums = oracle.banded_row_abs_sums(o_band)
    # float sums of <= width terms of size <= 1, in column order: width roundings of at most 2^-24 * sum each
    ref64.check_close("oracle band row sums", o_sums, sums, width * ref64.U * sums + width * ref64.MXM_BAR)
