"""Float64 reference of the correlation build (TEST INFRASTRUCTURE ONLY).

Independent of oracle/cusk_oracle.c and of the kernels: it starts from the dosage matrix G (int8, 0 / 1 / 2, -1 = missing,
as cigwas_amd.synth.make_genotypes returns it) and the traits, never from .bed bytes, and computes the definitions in
float64:

  mxm  Kendall tau-b of every marker pair over the individuals valid in both, from the 3 x 3 contingency counts (nine
       indicator matmuls, exact in float64), returned as sin(pi/2 tau).  NaN where the pair has no concordant and no
       discordant pair of individuals (then one of the two tie terms is zero too, so tau-b is 0 / 0).
  mxp  r = (sum g y - mean_g sum y) / (n sd_g) over the individuals with g valid and y not NaN, n their count; mean_g and
       sd_g are the inputs (synth.bed_stats, as `prep` writes them).  Also S_abs = (sum |g y| + |mean_g| sum |y|) / (n sd_g),
       the scale of the rounding error of any summation of those terms.
  pxp  sum a b / n over the individuals where both traits are non-NaN; S_abs = sum |a b| / n.
"""
from __future__ import annotations

import numpy as np

_CHUNK = 1 << 16  # individuals per matmul: keeps the float64 indicator planes of a 500k-individual block small


def _chunks(N: int):
    for i0 in range(0, N, _CHUNK):
        yield slice(i0, min(N, i0 + _CHUNK))


def contingency(G: np.ndarray) -> np.ndarray:
    """m x m x 3 x 3 float64 counts: cnt[x, y, a, b] = #individuals with G[x] = a and G[y] = b (both valid)"""
    G = np.asarray(G)
    m, N = G.shape
    cnt = np.zeros((3, 3, m, m), np.float64)
    for sl in _chunks(N):
        ind = [(G[:, sl] == a).astype(np.float64) for a in range(3)]
        for a in range(3):
            for b in range(3):
                cnt[a, b] += ind[a] @ ind[b].T
    return np.ascontiguousarray(cnt.transpose(2, 3, 0, 1))


def npn_from_counts(cnt: np.ndarray) -> np.ndarray:
    """sin(pi/2 tau_b) from [..., 3, 3] counts (float64, exact for counts below 2^26)"""
    c = np.asarray(cnt, np.float64)
    P = np.zeros(c.shape[:-2])
    Q = np.zeros_like(P)
    Ta = np.zeros_like(P)
    Tb = np.zeros_like(P)
    for a1 in range(3):
        for b1 in range(3):
            x = c[..., a1, b1]
            for a2 in range(3):
                for b2 in range(3):
                    if (a2, b2) <= (a1, b1):
                        continue
                    y = c[..., a2, b2]
                    if a2 != a1 and b2 != b1:
                        if (a2 > a1) == (b2 > b1):
                            P += x * y
                        else:
                            Q += x * y
                    elif a2 == a1:
                        Ta += x * y  # tied in the first marker only
                    else:
                        Tb += x * y  # tied in the second marker only
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = (P - Q) / np.sqrt((P + Q + Ta) * (P + Q + Tb))
    return np.sin(np.pi / 2 * tau)


def mxm(G: np.ndarray) -> np.ndarray:
    """m x m float64 Kendall-npn correlations (the diagonal is not meaningful)"""
    return npn_from_counts(contingency(G))


def mxp(G: np.ndarray, Y: np.ndarray, mean, sd):
    """(r, S_abs), both m x p float64; Y is p x N"""
    G = np.asarray(G)
    Y = np.asarray(Y, np.float32)
    Y = Y.reshape(-1, G.shape[1]) if Y.ndim == 1 else Y
    m, p = G.shape[0], Y.shape[0]
    sgy, sy, n, sagy, say = (np.zeros((m, p)) for _ in range(5))
    for sl in _chunks(G.shape[1]):
        g = G[:, sl].astype(np.float64)
        gv = (g >= 0).astype(np.float64)
        g = np.where(g >= 0, g, 0.0)
        y = Y[:, sl].astype(np.float64)
        yv = (~np.isnan(y)).astype(np.float64)
        y = np.nan_to_num(y, nan=0.0)
        sgy += g @ y.T
        sy += gv @ y.T
        n += gv @ yv.T
        sagy += g @ np.abs(y).T
        say += gv @ np.abs(y).T
    mu = np.asarray(mean, np.float32).astype(np.float64)[:, None]
    sg = np.asarray(sd, np.float32).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (sgy - mu * sy) / (n * sg)
        s_abs = (sagy + np.abs(mu) * say) / (n * sg)
    return r, s_abs


def pxp(Y: np.ndarray):
    """(r, S_abs), both p x p float64"""
    Y = np.asarray(Y, np.float32)
    p, N = Y.shape
    s, sa, n = (np.zeros((p, p)) for _ in range(3))
    for sl in _chunks(N):
        y = Y[:, sl].astype(np.float64)
        v = (~np.isnan(y)).astype(np.float64)
        y = np.nan_to_num(y, nan=0.0)
        s += y @ y.T
        sa += np.abs(y) @ np.abs(y).T
        n += v @ v.T
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / n, sa / n


def banded(G: np.ndarray, width: int):
    """(band m x width, forward row sums of |band|): band[row, col] = mxm(row, row + 1 + col), 0 past the last marker"""
    G = np.asarray(G)
    m = G.shape[0]
    band = np.zeros((m, width), np.float64)
    for r0 in range(0, m, 256):  # rows r0.. need the markers up to r0 + 256 + width
        r1 = min(m, r0 + 256)
        c1 = min(m, r1 + width)
        full = mxm(G[r0:c1])
        for row in range(r0, r1):
            k = min(width, m - row - 1)
            band[row, :k] = full[row - r0, row - r0 + 1: row - r0 + 1 + k]
    return band, np.abs(band).sum(axis=1)


# ---- inputs with the data edges of the correlation tests ----------------------------------------------------------
def make_case(m: int, N: int, p: int, seed: int, miss: float = 0.01, edges: bool = True):
    """(G m x N int8, Y p x N float32) from cigwas_amd.synth with the edges the kernels must survive, where m and p leave
    room for them: an all-missing marker, markers monomorphic at 0 and at 2, a heterozygous-only marker; an all-NaN
    trait, a trait whose last individual is NaN, traits scaled by 1e-3 and by 1e3."""
    from cigwas_amd import synth

    rng = synth.rng_for(1000 + seed)
    G = synth.make_genotypes(m, N, rng, window=min(100, max(m, 1)), miss=miss)
    Y = synth.make_traits(G, p, rng) if p else np.zeros((0, N), np.float32)
    if miss > 0 and p:
        Y[rng.random(Y.shape) < miss] = np.nan
    if N >= 2:  # tiny N: keep every marker polymorphic (the edges below add the monomorphic ones)
        G[:, 0], G[:, -1] = 0, 2
    if edges and m >= 6:
        G[1] = -1
        G[2] = 0
        G[m // 2] = 2
        G[m - 2] = np.where(G[m - 2] < 0, -1, 1)
    if edges and p >= 2:
        Y[p - 1, -1] = np.nan
    if edges and p >= 4:
        Y[0] = np.nan
        Y[1] *= np.float32(1e-3)
        Y[p // 2] *= np.float32(1e3)
    return G, np.ascontiguousarray(Y, np.float32)


def stats(G):
    """per-marker mean and population sd over the valid individuals (synth.bed_stats), NaN for an all-missing marker"""
    from cigwas_amd import synth

    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return synth.bed_stats(G)


def random_padding(bed: np.ndarray, N: int, seed: int) -> np.ndarray:
    """the .bed rows with random bits where the last byte holds no individual (N % 4 != 0): PLINK writes zeros there,
    a reader must ignore whatever is there"""
    bed = np.array(bed, np.uint8, copy=True)
    r = N % 4
    if r:
        rng = np.random.default_rng(seed)
        keep = np.uint8((1 << (2 * r)) - 1)
        bed[:, -1] = (bed[:, -1] & keep) | (rng.integers(0, 256, bed.shape[0]).astype(np.uint8) & ~keep)
    return bed


# ---- bars ---------------------------------------------------------------------------------------------------------
U = 2.0 ** -24  # unit roundoff of float32
MXM_BAR = 1e-6  # exact counts; the float epilogue (products, P - Q, sqrt, divide, sin) costs <= ~5e-7


def sum_bar(s_abs, chain: float, cap=None):
    """|computed - exact| bar of a float32 summation whose longest chain of dependent additions is `chain` long: every
    addition rounds by at most U times a partial sum, which is at most the sum of |terms| (S_abs after the epilogue's
    scaling).  The roundings of a chain are independent and zero-mean, so their sum grows like sqrt(chain):
    c = 3 sqrt(chain) is more than five standard deviations of a chain of uniform roundings; + 8 for the epilogue
    (products mean_g sum y and n sd_g, the difference, the quotient, the three bf16 pieces).  `cap` bounds the bar where
    the caller says so (the 1e-5 of the existing oracle comparisons)."""
    c = 3.0 * np.sqrt(chain) + 8.0
    bar = c * U * np.asarray(s_abs, np.float64) + 1e-7
    if cap is not None:
        bar = np.where(cap[0], np.minimum(bar, cap[1]), bar)
    return bar


def cap_1e5(sd, Y, N: int):
    """where a bar may be no looser than 1e-5 (the tolerance of the existing oracle comparisons): markers with sd >= 0.1
    against traits of unit scale (rms <= 1.5; a trait scaled by 1e3 scales its correlations and their roundings), N <= 70k"""
    import warnings

    with warnings.catch_warnings():  # an all-NaN trait has no rms (and no finite correlation either)
        warnings.simplefilter("ignore", RuntimeWarning)
        rms = np.sqrt(np.nanmean(np.asarray(Y, np.float64) ** 2, axis=1)) if np.asarray(Y).size else np.zeros(0)
    return (np.asarray(sd) >= 0.1)[:, None] & (rms <= 1.5)[None, :] & (N <= 70_000), 1e-5


def check_close(name: str, got, want, bar) -> None:
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    fin_g, fin_w = np.isfinite(got), np.isfinite(want)
    bad = np.flatnonzero((fin_g != fin_w).ravel())
    assert bad.size == 0, f"{name}: finite/non-finite differ at {bad[:6].tolist()} (got {got.ravel()[bad[:6]]}, ref {want.ravel()[bad[:6]]})"
    bar = np.broadcast_to(bar, want.shape)
    err = np.where(fin_w, np.abs(got - want), 0.0)
    over = np.where(fin_w, err - bar, -np.inf)
    worst = np.unravel_index(np.argmax(over), err.shape) if err.size else None
    assert err.size == 0 or not np.any(over > 0), (f"{name}: |got - ref64| = {err[worst]:.3g} > bar {bar[worst]:.3g} at "
                                                 f"{tuple(int(i) for i in worst)} (got {got[worst]!r}, ref {want[worst]!r})")


def check_mxm_nan(name: str, got, want) -> None:
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN positions differ from ref64"
    check_close(name, got, want, MXM_BAR)


def moved(full, cut, bar) -> float:
    """largest |full - cut| / bar; a change of finiteness counts as infinite"""
    full, cut = np.asarray(full, np.float64), np.asarray(cut, np.float64)
    if full.size == 0:
        return 0.0
    if np.any(np.isfinite(full) != np.isfinite(cut)):
        return np.inf
    bar = np.broadcast_to(bar, full.shape)
    ok = np.isfinite(full) & np.isfinite(bar)
    return float(np.max(np.where(ok, np.abs(full - cut) / np.where(ok, bar, 1.0), 0.0)))
