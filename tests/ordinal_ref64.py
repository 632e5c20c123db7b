"""Float64 oracle of the polychoric / polyserial two-step estimators (a plain module, shared by test_ordinal_formats.py
and test_gpu_ordinal.py; written from the definitions, not from the device code):

  Phi2(h, k; rho) = Phi(h) Phi(k) + int_0^rho phi2(h, k; t) dt   by scipy.integrate.quad at epsabs = epsrel = 1e-13
  rho-hat         by scipy.optimize.brentq on the closed-form score over [-0.9999, 0.9999]
  se              1 / sqrt(-l''), l'' from a central difference of the analytic score

Status: 0 fitted, 1 boundary (rho-hat at +-0.9999, or no positive information; se NaN), 2 degenerate (fewer than two
levels with observations on a side; r and se NaN).  A cell or observation with observations whose probability is below
1e-14 (rounding noise of the distribution values it is a difference of) stands for a likelihood of -infinity, and the
score is then taken as pointing to rho = 0 (at rho = 0 every probability is a product of positive shares).
"""
import numpy as np
from scipy import integrate, optimize, special

RHO_MAX = 0.9999
OK, BOUNDARY, DEGENERATE = 0, 1, 2
TINY = 1e-14  # below this a rectangle probability is rounding noise of four distribution values


def phi2(h, k, t):
    s = 1.0 - t * t
    return np.exp(-0.5 * (h * h - 2.0 * t * h * k + k * k) / s) / (2.0 * np.pi * np.sqrt(s))


def Phi2(h, k, rho):
    if h == -np.inf or k == -np.inf:
        return 0.0
    if h == np.inf:
        return 1.0 if k == np.inf else float(special.ndtr(k))
    if k == np.inf:
        return float(special.ndtr(h))
    base = float(special.ndtr(h) * special.ndtr(k))
    if rho == 0.0:
        return base
    # t = sin(theta): the integrand stays smooth up to |rho| = 1, where phi2 itself peaks ever more sharply
    hs, hk = 0.5 * (h * h + k * k), h * k
    val, _ = integrate.quad(lambda th: np.exp((np.sin(th) * hk - hs) / np.cos(th) ** 2), 0.0, np.arcsin(rho), epsabs=1e-13, epsrel=1e-13,
                            limit=200)
    return base + val / (2.0 * np.pi)


def thresholds(margin):
    """upper thresholds of the levels of a margin (counts): Phi^-1 of the cumulative shares, +inf for the last"""
    margin = np.asarray(margin, np.int64)
    cum, n = np.cumsum(margin), int(margin.sum())
    out = np.empty(len(margin))
    for i, c in enumerate(cum):
        out[i] = -np.inf if c <= 0 else np.inf if c >= n else special.ndtri(c / n)
    return out


def _solve(score):
    """rho-hat and status from a score function that returns +-inf where the likelihood is -inf"""
    if score(RHO_MAX) >= 0.0:
        return RHO_MAX, BOUNDARY
    if score(-RHO_MAX) <= 0.0:
        return -RHO_MAX, BOUNDARY
    return optimize.brentq(score, -RHO_MAX, RHO_MAX, xtol=1e-14, rtol=8.9e-16, maxiter=500), OK


def _se(score, rho):
    """from the five-point central difference of the score; the step follows 1 - rho^2, the scale on which it varies"""
    h = 1e-4 * (1.0 - rho * rho)
    d2 = (-score(rho + 2 * h) + 8.0 * score(rho + h) - 8.0 * score(rho - h) + score(rho - 2 * h)) / (12.0 * h)
    return (1.0 / np.sqrt(-d2), OK) if np.isfinite(d2) and -d2 > 0.0 else (np.nan, BOUNDARY)


def polychoric(table):
    """table: integer counts (ka x kb) -> (rho-hat, se, status)"""
    t = np.asarray(table, np.int64)
    t = t[t.sum(1) > 0][:, t.sum(0) > 0]
    if t.shape[0] < 2 or t.shape[1] < 2:
        return np.nan, np.nan, DEGENERATE
    al = np.concatenate([[-np.inf], thresholds(t.sum(1))])
    be = np.concatenate([[-np.inf], thresholds(t.sum(0))])

    def score(rho):
        F = np.array([[Phi2(a, b, rho) for b in be] for a in al])
        f = np.array([[phi2(a, b, rho) if np.isfinite(a) and np.isfinite(b) else 0.0 for b in be] for a in al])
        pi = F[1:, 1:] - F[:-1, 1:] - F[1:, :-1] + F[:-1, :-1]
        dpi = f[1:, 1:] - f[:-1, 1:] - f[1:, :-1] + f[:-1, :-1]
        seen = t > 0
        if np.any(pi[seen] < TINY):
            return -np.inf if rho > 0 else np.inf
        return float(np.sum(t[seen] * dpi[seen] / pi[seen]))

    rho, status = _solve(score)
    if status != OK:
        return rho, np.nan, status
    se, status = _se(score, rho)
    return rho, se, status


def pair_table(x_codes, y_codes, ka, kb):
    """contingency table of two integer-coded variables; a negative code is a missing value"""
    x_codes, y_codes = np.asarray(x_codes), np.asarray(y_codes)
    ok = (x_codes >= 0) & (y_codes >= 0)
    t = np.zeros((ka, kb), np.int64)
    np.add.at(t, (x_codes[ok], y_codes[ok]), 1)
    return t


def polyserial(x, y_codes):
    """x: continuous values (NaN = missing), y_codes: integer level codes (negative = missing) -> (rho-hat, se, status)"""
    x, y = np.asarray(x, np.float64), np.asarray(y_codes)
    ok = ~np.isnan(x) & (y >= 0)
    x, y = x[ok], y[ok]
    levels = np.unique(y)
    if len(levels) < 2 or len(x) < 2 or not x.std() > 0:
        return np.nan, np.nan, DEGENERATE
    y = np.searchsorted(levels, y)
    z = (x - x.mean()) / x.std(ddof=1)
    tau = np.concatenate([[-np.inf], thresholds(np.bincount(y))])
    t_lo, t_hi = tau[y], tau[y + 1]
    fin_lo, fin_hi = np.isfinite(t_lo), np.isfinite(t_hi)

    def score(rho):
        s = 1.0 - rho * rho
        with np.errstate(invalid="ignore"):
            A_hi = np.where(fin_hi, (t_hi - rho * z) / np.sqrt(s), np.inf)
            A_lo = np.where(fin_lo, (t_lo - rho * z) / np.sqrt(s), -np.inf)
            d_hi = np.where(fin_hi, (rho * t_hi - z) / s ** 1.5, 0.0)
            d_lo = np.where(fin_lo, (rho * t_lo - z) / s ** 1.5, 0.0)
        up = A_lo > 0
        P = np.where(up, special.ndtr(-A_lo) - special.ndtr(-A_hi), special.ndtr(A_hi) - special.ndtr(A_lo))
        if np.any(P < 1e-290):  # formed in the tail, so small values are not noise: only an underflow is -infinity
            return -np.inf if rho > 0 else np.inf
        f_hi = np.where(fin_hi, np.exp(-0.5 * np.where(fin_hi, A_hi, 0.0) ** 2), 0.0) / np.sqrt(2 * np.pi)
        f_lo = np.where(fin_lo, np.exp(-0.5 * np.where(fin_lo, A_lo, 0.0) ** 2), 0.0) / np.sqrt(2 * np.pi)
        return float(np.sum((f_hi * d_hi - f_lo * d_lo) / P))

    rho, status = _solve(score)
    if status != OK:
        return rho, np.nan, status
    se, status = _se(score, rho)
    return rho, se, status


def codes_of(values, levels=None):
    """integer level codes of an ordinal trait (sorted distinct non-NaN values), -1 for NaN -> (codes, levels)"""
    values = np.asarray(values, np.float32)
    if levels is None:
        levels = np.unique(values[~np.isnan(values)])
    codes = np.searchsorted(levels, values).astype(np.int64)
    codes[np.isnan(values)] = -1
    return codes, levels


def bed_class_codes(bed_row, n):
    """genotype classes of a .bed row in the order of the dosage: code 11 -> 0, 10 -> 1, 00 -> 2, 01 (missing) -> -1"""
    b = np.asarray(bed_row, np.uint8)
    two = ((b[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n]
    return np.array([2, -1, 1, 0], np.int64)[two]
