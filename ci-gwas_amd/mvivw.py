"""`ci-gwas mvivw`: multivariable inverse-variance-weighted causal effects between the traits of a merged skeleton.

Counterpart of the reference's mvivw/cig_mvivw.R and cig_mvivw_filtered.R, written from their semantics: for every outcome
trait one weighted regression through the origin of the outcome's marker correlations on those of its exposures, over the
outcome's instruments.

NOT the reference's estimator.  The reference calls `mr_mvivw(..., robust = TRUE)` of the R package MendelianRandomization,
which uses `robustbase::lmrob`: an MM-estimator with random subsampling.  Neither R nor that package is on our machines and
its program text is not in the reference tree; it can be neither run nor restated, so nothing here claims to equal it.
This module computes the plain IVW estimator with multiplicative random effects: weighted least squares through the
origin with a standard-error inflation.  To our knowledge that is what the package computes with `robust = FALSE`; nobody
has checked this against R.  The rule is stated in include/cusk_hip.h above `cusk_mvivw` (csrc/mvivw.hip on the device,
`HostEngine` below in float64 numpy with the same chunked sums, used when no engine is given).

Inputs as for `check-ivs` (`ivcheck.load`): `<stem>_sam.mtx`, `<stem>_scm.mtx`, `<stem>.mdim`; traits are variables
0 .. p-1, marker row r is variable p + r, beta = corr[p:, :p], weight = 1 / byse^2 with byse = (1 - beta^2) / sqrt(N - 2)
(the reference's `SE`).  With `het` N is the size of marker and outcome in `<stem>_ssz.mtx`; a size <= 2 makes the weight
non-positive or non-finite and gives the outcome status 3.  Adjacency means `!= 0`, as in ivcheck.py.

Selections of the instruments I and exposures E of outcome o:
  all       E = every trait != o; I = markers not adjacent to o (the reference's default)
  skeleton  E = traits adjacent to o; I = markers adjacent neither to o nor to any trait that is not adjacent to o
  prior     E = traits t != o with prior[o, t] != 1 (p x p int32, row-major); I = markers not adjacent to o
  ivs       E and I = the distinct exposures and IVs a table `Exposure,Outcome,IV` (as `check-ivs` writes it: 1-based, IV
            counted from the first marker) lists for o
Deliberate deviations from the reference's scripts:
  * skeleton: the reference's `B[-rm_rows, ]` with an empty `rm_rows` selects ZERO rows in R; here an empty removal
    removes nothing.
  * prior: the reference also drops the marker rows whose row numbers happen to equal the removed trait numbers (it mixes
    the two index spaces); we do not.
  * `num_snps` is the outcome's own m; the reference's column carries one recycled value (the `num_snp` / `num_snps` slip
    of its script).
"""
from __future__ import annotations

import sys

import numpy as np

from . import ivcheck

CHUNK = 256          # CUSK_MVIVW_CHUNK
MAX_EXPOSURES = 127  # CUSK_MVIVW_MAX_EXPOSURES
PIVOT_MIN = 1e-8     # CUSK_PHEN_PIVOT_MIN
MODELS = {"default": 0, "random": 1, "fixed": 2}


def weights(beta, n):
    """1 / byse^2, byse = (1 - beta^2) / sqrt(n - 2); n a number or an array in the layout of beta"""
    with np.errstate(all="ignore"):
        byse = (1.0 - beta * beta) / np.sqrt(np.asarray(n, np.float64) - 2.0)
        return np.array(np.broadcast_to(1.0 / (byse * byse), beta.shape), dtype=np.float64, order="C")


def read_prior(path: str, p: int):
    prior = np.fromfile(path, dtype=np.int32)
    if prior.size != p * p:
        raise ValueError(f"{path}: expected {p} x {p} 32-bit integers, found {prior.size}")
    return prior.reshape(p, p)


def read_ivs(path: str):
    """the rows (Exposure, Outcome, IV) of a table written by ivcheck.write_csv"""
    with open(path) as f:
        header = f.readline().strip()
        if header != "Exposure,Outcome,IV":
            raise ValueError(f"{path}: the header is not Exposure,Outcome,IV")
        rows = [tuple(int(v) for v in line.split(",")) for line in f if line.strip()]
    if any(len(r) != 3 for r in rows):
        raise ValueError(f"{path}: a row does not have three fields")
    return rows


def read_group_labels(path: str, M: int):
    """`--jackknife-groups FILE`: M lines, one non-decreasing integer label per marker row"""
    with open(path) as f:
        words = f.read().split()
    try:
        labels = np.array([int(v) for v in words], np.int64)
    except ValueError:
        raise ValueError(f"{path}: a label is not an integer") from None
    if labels.shape[0] != M:
        raise ValueError(f"{path}: expected {M} labels, one per marker row, found {labels.shape[0]}")
    if np.any(np.diff(labels) < 0):
        raise ValueError(f"{path}: the labels are not non-decreasing")
    return labels


def select(adj, p: int, mode: str = "all", prior=None, iv_rows=None):
    """[(I, E)] per outcome: ascending int arrays of marker rows and exposure traits"""
    adj = np.asarray(adj)
    M = adj.shape[0] - p
    mxp = adj[:p, p:].T != 0  # M x p
    pxp = adj[:p, :p] != 0
    traits = np.arange(p)
    out = []
    if mode == "ivs":
        rows = np.asarray(iv_rows, np.int64).reshape(-1, 3)
        if rows.size and (rows[:, :2].min() < 1 or rows[:, :2].max() > p or rows[:, 2].min() < 1 or rows[:, 2].max() > M):
            raise ValueError("mvivw: the instrument table names a trait or a marker the skeleton does not have")
        if np.any(rows[:, 0] == rows[:, 1]):
            raise ValueError("mvivw: the instrument table lists a trait as its own exposure")
        for o in range(p):
            mine = rows[rows[:, 1] == o + 1]
            out.append((np.unique(mine[:, 2]) - 1, np.unique(mine[:, 0]) - 1))
        return out
    for o in range(p):
        keep = ~mxp[:, o]
        if mode == "all":
            E = traits[traits != o]
        elif mode == "skeleton":
            near = pxp[:, o].copy()
            near[o] = False
            E = traits[near]
            keep &= ~mxp[:, ~near].any(axis=1)  # ~near holds o itself
        elif mode == "prior":
            E = traits[(np.asarray(prior)[o, :] != 1) & (traits != o)]
        else:
            raise ValueError(f"mvivw: unknown selection {mode!r}")
        out.append((np.flatnonzero(keep), E))
    return out


def pack(selection):
    """the list arguments of the engine call"""
    nout = len(selection)
    iv_off, ex_off = np.zeros(nout + 1, np.int64), np.zeros(nout + 1, np.int32)
    iv_off[1:] = np.cumsum([len(I) for I, _ in selection])
    ex_off[1:] = np.cumsum([len(E) for _, E in selection])
    iv = np.concatenate([np.asarray(I, np.int32) for I, _ in selection]) if nout else np.zeros(0, np.int32)
    ex = np.concatenate([np.asarray(E, np.int32) for _, E in selection]) if nout else np.zeros(0, np.int32)
    return iv_off, iv.astype(np.int32), ex_off, ex.astype(np.int32)


def check_arguments(M, p, outcome, iv_off, iv, ex_off, ex, model):
    """the argument errors of cusk_mvivw (csrc/host/mvivw_plan.h), as a ValueError"""
    if model not in (0, 1, 2):
        raise ValueError(f"mvivw: model {model} is not 0 (default), 1 (random) or 2 (fixed)")
    if np.any(np.diff(iv_off) < 0) or np.any(np.diff(ex_off) < 0) or (len(iv_off) and (iv_off[0] < 0 or ex_off[0] < 0)):
        raise ValueError("mvivw: offsets are not monotone")
    for a, o in enumerate(outcome):
        I, E = iv[iv_off[a]:iv_off[a + 1]], ex[ex_off[a]:ex_off[a + 1]]
        if not 0 <= o < p:
            raise ValueError(f"mvivw: outcome {a}: {o} is not a trait index")
        if len(E) > MAX_EXPOSURES:
            raise ValueError(f"mvivw: outcome {a}: more than {MAX_EXPOSURES} exposures")
        if len(I) and (I.min() < 0 or I.max() >= M or np.any(np.diff(I) <= 0)):
            raise ValueError(f"mvivw: outcome {a}: the instrument list is not strictly ascending inside [0, M)")
        if len(E) and (E.min() < 0 or E.max() >= p or np.any(np.diff(E) <= 0) or np.any(E == o)):
            raise ValueError(f"mvivw: outcome {a}: the exposure list is not strictly ascending inside [0, p) without the outcome")


def _gram_sums(Z, w):
    """Step 1 of the rule: Z'WZ for Z = (X, y), chunk partials added in chunk order"""
    m, k = Z.shape[0], Z.shape[1] - 1
    S = np.zeros((k + 1, k + 1), Z.dtype)
    for c0 in range(0, m, CHUNK):
        Zc = Z[c0:c0 + CHUNK]
        S += (Zc * w[c0:c0 + CHUNK, None]).T @ Zc
    return S


def _tri_solve(L, b, trans: bool):
    """L x = b (trans: L' x = b) for a lower triangular L, in the type of L"""
    if L.dtype == np.float64:
        from scipy.linalg import solve_triangular

        return solve_triangular(L, b, lower=True, trans=1 if trans else 0)
    k = L.shape[0]
    x = b.copy()  # scipy has no solver of the extended type: by columns
    for j in (range(k - 1, -1, -1) if trans else range(k)):
        x[j] = x[j] / L[j, j]
        if trans:
            x[:j] -= L[j, :j] * x[j]
        else:
            x[j + 1:] -= L[j + 1:, j] * x[j]
    return x


def _solve_sums(S, want_v: bool = True):
    """Steps 2 - 3 of the rule for the sums S = Z'WZ -> (status 0 | 2, theta, v, d, pivot): the smallest squared pivot, or
    the one that failed (0 for a G_jj that is not positive).  want_v False: v is None, theta by two substitutions"""
    from scipy.linalg import solve_triangular

    k = S.shape[0] - 1
    G, b = S[:k, :k], S[k, :k]
    dg = np.diag(G)
    if not (dg > 0).all():
        return 2, None, None, None, 0.0
    d = np.sqrt(dg)
    L = np.tril(G / np.outer(d, d))
    np.fill_diagonal(L, 1.0)
    minpiv = np.inf
    for j in range(k):  # right-looking Cholesky with the pivot test
        piv = L[j, j]
        minpiv = min(minpiv, piv)
        if not piv >= PIVOT_MIN:
            return 2, None, None, None, float(piv)
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(L[j + 1:, j], L[j + 1:, j]))
    if not want_v:
        return 0, _tri_solve(L, _tri_solve(L, b / d, False), True) / d, None, d, float(minpiv)
    if S.dtype == np.float64:
        Linv = solve_triangular(L, np.eye(k), lower=True)
    else:  # the extended-precision restatement of the tests: scipy has no such solver
        Linv = np.zeros((k, k), S.dtype)
        for j in range(k):
            Linv[j, j] = 1 / L[j, j]
            for i in range(j + 1, k):
                Linv[i, j] = -(L[i, j:i] @ Linv[j:i, j]) / L[i, i]
    theta = (Linv.T @ (Linv @ (b / d))) / d
    v = (Linv * Linv).sum(axis=0) / (d * d)
    return 0, theta, v, d, float(minpiv)


def _gram_solve(Z, w):
    """Steps 1 - 3 of the rule for Z = (X, y) with the row weights w -> (status 0 | 2, theta, v, d, pivot): the smallest
    squared pivot, or the one that failed (0 for a G_jj that is not positive)"""
    return _solve_sums(_gram_sums(Z, w))


def solve_one(X, y, w, model: int):
    """One problem by the rule of include/cusk_hip.h -> (status, theta, se, (rss, sigma, smallest squared pivot))"""
    m, k = X.shape
    nan3 = (np.nan, np.nan, np.nan)
    if k == 0 or m <= k:
        return 1, None, None, nan3
    if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(w).all() and (w > 0).all()):
        return 3, None, None, nan3
    st, theta, v, _, minpiv = _gram_solve(np.concatenate([X, y[:, None]], axis=1), w)
    if st != 0:
        return st, None, None, (np.nan, np.nan, minpiv)
    r = y - X @ theta
    t = w * (r * r)
    rss = 0.0
    for c0 in range(0, m, CHUNK):  # the second pass, same chunks
        rss += float(t[c0:c0 + CHUNK].sum())
    sigma = float(np.sqrt(rss / (m - k)))
    random = model == 1 or (model == 0 and m >= 4)
    se = np.sqrt(v) * (sigma if random and sigma > 1.0 else 1.0)
    return 0, theta, se, (rss, sigma, float(minpiv))


PSI = {"huber": 1, "bisquare": 2}
MAX_UPDATES = 100                  # per stage
MAD, HUBER_C, BISQUARE_C, ROBUST_TOL = 1.4826, 1.345, 4.685, 1e-10


def abs_median(e):
    """The exact median of |e|: the middle value of the sorted absolute values, or (a + b) * 0.5 of the two middle ones"""
    a = np.sort(np.abs(e))
    n = a.shape[0]
    return a[n // 2] if n & 1 else (a[n // 2 - 1] + a[n // 2]) * 0.5


def robust_rho(e, s, stage: int):
    """(rho, psi') of the residuals e at the scale s: stage 0 Huber, 1 bisquare"""
    one, zero = e.dtype.type(1), e.dtype.type(0)
    if stage == 0:
        a, c = np.abs(e), e.dtype.type(HUBER_C) * s
        inside = a <= c
        with np.errstate(all="ignore"):
            return np.where(inside, one, c / a), np.where(inside, one, zero)
    u = e / (e.dtype.type(BISQUARE_C) * s)
    u2 = u * u
    inside = np.abs(u) < 1
    return np.where(inside, (1 - u2) * (1 - u2), zero), np.where(inside, (1 - u2) * (1 - 5 * u2), zero)


def _chunk_sum(t):
    tot = t.dtype.type(0)
    for c0 in range(0, t.shape[0], CHUNK):
        tot += t[c0:c0 + CHUNK].sum()
    return tot


def solve_one_robust(X, y, w, model: int, psi: int, max_updates: int = MAX_UPDATES):
    """One problem of `cusk_mvivw_robust` by the rule of include/cusk_hip.h, in the floating-point type of X (float64; the
    tests restate it in np.longdouble by passing such arrays).  `max_updates`: the cap per stage, 100 in the rule.
    -> (status, theta, se, (rss, s, tau, smallest squared pivot of the last weighted Gram, updates, sum rho), rho)"""
    m, k = X.shape
    ft = X.dtype.type
    nan6 = (np.nan,) * 6
    if psi not in (1, 2):
        raise ValueError(f"mvivw: psi {psi} is not 1 (Huber) or 2 (bisquare)")
    if k == 0 or m <= k:
        return 1, None, None, nan6, None
    if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(w).all() and (w > 0).all()):
        return 3, None, None, nan6, None
    Z = np.concatenate([X, y[:, None]], axis=1)
    sw = np.sqrt(w)

    def failed(st, piv=np.nan):
        return st, None, None, (np.nan, np.nan, np.nan, piv, np.nan, np.nan), None

    st, theta, v, d, piv = _gram_solve(Z, w)
    if st != 0:
        return failed(st, piv)
    e = sw * (y - X @ theta)
    s = ft(MAD) * abs_median(e)
    if not s > 0:
        return failed(6)
    updates = 0
    for stage in range(psi):
        for t in range(max_updates):
            rho, _ = robust_rho(e, s, stage)
            st, new, _, _, piv = _gram_solve(Z, w * rho)
            if st != 0:
                return failed(st, piv)
            e = sw * (y - X @ new)
            if stage == 0:
                s = ft(MAD) * abs_median(e)
                if not s > 0:
                    return failed(6)
            updates += 1
            step = np.max(d * np.abs(new - theta))
            theta = new
            if step <= ft(ROBUST_TOL) * s * np.sqrt(ft(m)):
                break
        else:
            return failed(5)
    rho, dpsi = robust_rho(e, s, psi - 1)
    ps = e * rho
    A, B = _chunk_sum(ps * ps) / ft(m - k), _chunk_sum(dpsi) / ft(m)
    if not B > 0:
        return failed(5)
    tau = np.sqrt(A) / B
    random = model == 1 or (model == 0 and m >= 4)
    g = tau if random else tau / s
    se = np.sqrt(v) * (g if g > 1 else ft(1))
    return 0, theta, se, (_chunk_sum(e * e), s, tau, piv, updates, _chunk_sum(rho)), rho


JK_CHUNK = 256  # kMvJkChunk of csrc/host/mvivw_jk_plan.h: groups per chunk of the sums over groups


def groups(I, spec, labels=None):
    """The group boundaries of an instrument list I (ascending marker rows) for `cusk_mvivw_jackknife`: list positions,
    strictly ascending from 0 to m = len(I).  spec "loo": one group per instrument; an integer B >= 2: boundary
    g = floor(g m / B), B capped at m; "labels": `labels` holds a non-decreasing integer per marker row and the boundaries
    fall where the label changes along I.  An empty list gives the single boundary 0."""
    m = len(I)
    if spec == "loo":
        return np.arange(m + 1, dtype=np.int32)
    if spec == "labels":
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.dtype.kind not in "iu":
            raise ValueError("mvivw: the group labels are not a list of integers")
        if np.any(np.diff(lab) < 0):
            raise ValueError("mvivw: the group labels are not non-decreasing")
        if m and (int(np.min(I)) < 0 or int(np.max(I)) >= lab.shape[0]):
            raise ValueError("mvivw: an instrument has no group label")
        li = lab[np.asarray(I, np.int64)]
        return np.concatenate([[0], np.flatnonzero(np.diff(li) != 0) + 1, [m]] if m else [[0]]).astype(np.int32)
    if isinstance(spec, (bool, np.bool_)) or not isinstance(spec, (int, np.integer)) or spec < 2:
        raise ValueError(f"mvivw: jackknife {spec!r} is not loo, labels or a number of groups >= 2")
    B = min(int(spec), m)
    return np.array([g * m // B for g in range(B + 1)] if m else [0], dtype=np.int32)


def check_groups(iv_off, ex_off, grp_off, grp):
    """the argument errors `cusk_mvivw_jackknife` adds to those of cusk_mvivw (csrc/host/mvivw_jk_plan.h), as a ValueError"""
    if grp_off is None:
        raise ValueError("mvivw: no group offsets")
    if len(grp_off) != len(iv_off) or np.any(np.diff(grp_off) < 0) or (len(grp_off) and grp_off[0] < 0):
        raise ValueError("mvivw: group offsets are not monotone")
    for a in range(len(iv_off) - 1):
        m, b = int(iv_off[a + 1] - iv_off[a]), grp[grp_off[a]:grp_off[a + 1]]
        if m > 0 and len(b) < 2:
            raise ValueError(f"mvivw: outcome {a}: instruments and no groups")
        if len(b) and (b[0] != 0 or b[-1] != m or np.any(np.diff(b) <= 0)):
            raise ValueError(f"mvivw: outcome {a}: the group boundaries are not strictly ascending from 0 to m")


def _group_sum(t):
    """a sum over groups: chunks of JK_CHUNK groups, inside a chunk in ascending order, the chunk sums in chunk order"""
    tot = np.zeros(t.shape[1:], t.dtype)
    for c0 in range(0, t.shape[0], JK_CHUNK):
        s = np.zeros(t.shape[1:], t.dtype)
        for row in t[c0:c0 + JK_CHUNK]:
            s = s + row
        tot = tot + s
    return tot


def solve_one_jackknife(X, y, w, bounds, model: int):
    """One problem of `cusk_mvivw_jackknife` by the rule of include/cusk_hip.h, in the floating-point type of X (float64;
    the tests restate it in np.longdouble by passing such arrays).  bounds: the ng + 1 group boundaries.
    -> (status, theta, se, (rss, sigma, pivot), jk_status, jk (k x 4: theta_J, se_J, min, max) | None, jk_arg | None,
    (press, pivot), pres | None, refit (ng x k) | None)"""
    m, k = X.shape
    ft = X.dtype.type
    bounds = np.asarray(bounds, np.int64)
    none = (None, None, (np.nan, np.nan), None, None)
    nan3 = (np.nan, np.nan, np.nan)
    if k == 0 or m <= k:
        return (1, None, None, nan3, 1) + none
    if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(w).all() and (w > 0).all()):
        return (3, None, None, nan3, 3) + none
    Z = np.concatenate([X, y[:, None]], axis=1)
    S = _gram_sums(Z, w)
    st, theta, v, _, minpiv = _solve_sums(S)
    if st != 0:
        return (st, None, None, (np.nan, np.nan, minpiv), st) + none
    r = y - X @ theta
    rss = _chunk_sum(w * (r * r))
    sigma = np.sqrt(rss / ft(m - k))
    random = model == 1 or (model == 0 and m >= 4)
    se = np.sqrt(v) * (sigma if random and sigma > 1 else ft(1))
    plain = (0, theta, se, (rss, sigma, minpiv))
    ng = len(bounds) - 1
    mg = np.diff(bounds)
    if ng < 2 or np.any(m - mg <= k):
        return plain + (1,) + none
    sw = np.sqrt(w)
    refit, pres, gpress = np.zeros((ng, k), X.dtype), np.zeros(m, X.dtype), np.zeros(ng, X.dtype)
    jpiv = np.inf
    for g in range(ng):
        r0, r1 = bounds[g], bounds[g + 1]
        Zg = Z[r0:r1]
        st, th, _, _, piv = _solve_sums(S - (Zg * w[r0:r1, None]).T @ Zg, want_v=False)
        if st != 0:
            return plain + (2, None, None, (np.nan, piv), None, None)
        jpiv = min(jpiv, piv)
        refit[g] = th
        pres[r0:r1] = sw[r0:r1] * (y[r0:r1] - X[r0:r1] @ th)
        gpress[g] = _chunk_sum(pres[r0:r1] * pres[r0:r1])
    fm = ft(m)
    mgf = mg.astype(X.dtype)
    diff = theta[None, :] - refit
    thj = theta + _group_sum((1 - mgf / fm)[:, None] * diff)
    h1 = fm / mgf - 1
    dev = h1[:, None] * diff - (thj - theta)[None, :]
    var = _group_sum(dev * dev / h1[:, None]) / ft(ng)
    jk = np.stack([thj, np.sqrt(var), refit.min(axis=0), refit.max(axis=0)], axis=1)
    arg = np.argmax(np.abs(refit - theta[None, :]), axis=0).astype(np.int32)  # the first group on ties
    return plain + (0, jk, arg, (_group_sum(gpress), jpiv), pres, refit)


LD_PANEL = 64  # kLdPanel of csrc/host/mvivw_ld_plan.h


def cholesky_ld(R):
    """Right-looking Cholesky of the lower triangle of R (unit diagonal included) with the pivot rule, in panels of
    LD_PANEL columns as on the device -> (status 0 | 4, C or None, smallest squared pivot | the pivot that failed)"""
    from scipy.linalg import solve_triangular

    A = np.tril(R)
    m = A.shape[0]
    minpiv = np.inf
    for j0 in range(0, m, LD_PANEL):
        j1 = min(j0 + LD_PANEL, m)
        D = A[j0:j1, j0:j1]
        for j in range(j1 - j0):
            piv = D[j, j]
            minpiv = min(minpiv, piv)
            if not piv >= PIVOT_MIN:
                return 4, None, float(piv)
            D[j, j] = np.sqrt(piv)
            D[j + 1:, j] /= D[j, j]
            D[j + 1:, j + 1:] -= np.tril(np.outer(D[j + 1:, j], D[j + 1:, j]))
        if j1 < m:
            A[j1:, j0:j1] = solve_triangular(D, A[j1:, j0:j1].T, lower=True).T
            A[j1:, j1:] -= np.tril(A[j1:, j0:j1] @ A[j1:, j0:j1].T)
    return 0, A, float(minpiv)


def solve_one_ld(X, y, w, R, model: int, ridge: float = 0.0):
    """One problem of `cusk_mvivw_ld` by the rule of include/cusk_hip.h.  R: m x m, the LD of the instruments in list
    order; its strict lower triangle is read.  -> (status, theta, se, (rss, sigma, pivot of R))"""
    from scipy.linalg import solve_triangular

    m, k = X.shape
    nan3 = (np.nan, np.nan, np.nan)
    if k == 0 or m <= k:
        return 1, None, None, nan3
    low = np.tril(np.asarray(R, np.float64), -1)
    if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(w).all() and (w > 0).all() and np.isfinite(low).all()):
        return 3, None, None, nan3
    st, C, rpiv = cholesky_ld(low * (1.0 - ridge) + np.eye(m))
    if st != 0:
        return st, None, None, (np.nan, np.nan, rpiv)
    Zw = solve_triangular(C, np.concatenate([X, y[:, None]], axis=1) * np.sqrt(w)[:, None], lower=True)
    st, theta, se, stat = solve_one(Zw[:, :k], Zw[:, k], np.ones(m), model)
    return st, theta, se, ((stat[0], stat[1], rpiv) if st == 0 else stat)


class HostEngine:
    """`Engine.mvivw` and `Engine.mvivw_ld` in float64 numpy: what `mvivw(engine=None)` runs on, and the comparison form of
    the tests"""

    @staticmethod
    def _run(beta, weight, outcome, iv_off, iv, ex_off, ex, model, solve, ncol=3, dtype=np.float64):
        """The batch every method walks; `solve(I, E, o, a)` -> (status, theta, se, stats) of outcome a (solve_one's)"""
        M, p = beta.shape
        outcome = np.asarray(outcome, np.int64).reshape(-1)
        iv_off, ex_off = np.asarray(iv_off, np.int64).reshape(-1), np.asarray(ex_off, np.int64).reshape(-1)
        iv, ex = np.asarray(iv, np.int64).reshape(-1), np.asarray(ex, np.int64).reshape(-1)
        check_arguments(M, p, outcome, iv_off, iv, ex_off, ex, model)
        nout = outcome.shape[0]
        nex = int(ex_off.max()) if nout else 0
        theta, se = np.full(max(nex, 1), np.nan, dtype), np.full(max(nex, 1), np.nan, dtype)
        stats, status = np.full((nout, ncol), np.nan, dtype), np.zeros(nout, np.int32)
        for a, o in enumerate(outcome):
            st, th, s, stat = solve(iv[iv_off[a]:iv_off[a + 1]], ex[ex_off[a]:ex_off[a + 1]], o, a)
            status[a], stats[a] = st, stat
            if st == 0:
                theta[ex_off[a]:ex_off[a + 1]] = th
                se[ex_off[a]:ex_off[a + 1]] = s
        return theta, se, stats, status, 0.0

    def mvivw_ld(self, beta, weight, ld, outcome, iv_off, iv, ex_off, ex, model=0, ridge=0.0):
        beta, weight, ld = np.asarray(beta, np.float64), np.asarray(weight, np.float64), np.asarray(ld, np.float64)
        M = beta.shape[0]
        if ld.shape != (M, M):
            raise ValueError(f"mvivw: ld is not {M} x {M}")
        if not 0.0 <= ridge < 1.0:
            raise ValueError("mvivw: ridge is not in [0, 1)")
        return self._run(beta, weight, outcome, iv_off, iv, ex_off, ex, model, lambda I, E, o, a: solve_one_ld(
            beta[np.ix_(I, E)], beta[I, o], weight[I, o], ld[np.ix_(I, I)], model, ridge))

    def mvivw(self, beta, weight, outcome, iv_off, iv, ex_off, ex, model=0):
        beta, weight = np.asarray(beta, np.float64), np.asarray(weight, np.float64)
        return self._run(beta, weight, outcome, iv_off, iv, ex_off, ex, model, lambda I, E, o, a: solve_one(
            beta[np.ix_(I, E)], beta[I, o], weight[I, o], model))

    def mvivw_robust(self, beta, weight, outcome, iv_off, iv, ex_off, ex, model=0, psi=2, want_rho=True, dtype=np.float64,
                     max_updates=MAX_UPDATES):
        """`Engine.mvivw_robust`; `dtype` np.longdouble gives the extended-precision restatement of the tests"""
        beta, weight = np.asarray(beta, dtype), np.asarray(weight, dtype)
        if psi not in (1, 2):
            raise ValueError(f"mvivw: psi {psi} is not 1 (Huber) or 2 (bisquare)")
        iv_off = np.asarray(iv_off, np.int64).reshape(-1)
        rho = np.full(max(int(iv_off.max()) if len(iv_off) else 0, 1), np.nan, dtype)

        def solve(I, E, o, a):
            st, th, se, stat, r = solve_one_robust(beta[np.ix_(I, E)], beta[I, o], weight[I, o], model, psi, max_updates)
            if st == 0:
                rho[iv_off[a]:iv_off[a + 1]] = r
            return st, th, se, stat

        theta, se, stats, status, ms = self._run(beta, weight, outcome, iv_off, iv, ex_off, ex, model, solve, ncol=6, dtype=dtype)
        return theta, se, stats, status, (rho if want_rho else None), ms


    def mvivw_jackknife(self, beta, weight, outcome, iv_off, iv, ex_off, ex, grp_off, grp, model=0, want_pres=True,
                        want_refit=True, dtype=np.float64):
        """`Engine.mvivw_jackknife`; `dtype` np.longdouble gives the extended-precision form of the tests"""
        beta, weight = np.asarray(beta, dtype), np.asarray(weight, dtype)
        iv_off = np.asarray(iv_off, np.int64).reshape(-1)
        ex_off = np.asarray(ex_off, np.int64).reshape(-1)
        check_arguments(beta.shape[0], beta.shape[1], np.asarray(outcome, np.int64).reshape(-1), iv_off,
                        np.asarray(iv, np.int64).reshape(-1), ex_off, np.asarray(ex, np.int64).reshape(-1), model)
        if grp_off is None:
            raise ValueError("mvivw: no group offsets")
        grp_off, grp = np.asarray(grp_off, np.int64).reshape(-1), np.asarray(grp, np.int64).reshape(-1)
        check_groups(iv_off, ex_off, grp_off, grp)
        nout = len(iv_off) - 1
        nex, niv = (int(ex_off.max()), int(iv_off.max())) if nout else (0, 0)
        ngs = np.maximum(np.diff(grp_off) - 1, 0)
        refit_off = np.concatenate([[0], np.cumsum(ngs * np.diff(ex_off))]).astype(np.int64)
        jk, jk_arg = np.full((max(nex, 1), 4), np.nan, dtype), np.full(max(nex, 1), -1, np.int32)
        jk_stats, jk_status = np.full((nout, 2), np.nan, dtype), np.zeros(nout, np.int32)
        pres, refit = np.full(max(niv, 1), np.nan, dtype), np.full(max(int(refit_off[-1]), 1), np.nan, dtype)

        def solve(I, E, o, a):
            r = solve_one_jackknife(beta[np.ix_(I, E)], beta[I, o], weight[I, o], grp[grp_off[a]:grp_off[a + 1]], model)
            jk_status[a], jk_stats[a] = r[4], r[7]
            if r[4] == 0:
                jk[ex_off[a]:ex_off[a + 1]], jk_arg[ex_off[a]:ex_off[a + 1]] = r[5], r[6]
                pres[iv_off[a]:iv_off[a + 1]] = r[8]
                refit[refit_off[a]:refit_off[a + 1]] = r[9].reshape(-1)
            return r[:4]

        theta, se, stats, status, ms = self._run(beta, weight, outcome, iv_off, iv, ex_off, ex, model, solve, dtype=dtype)
        return (theta, se, stats, status, jk[:nex], jk_arg[:nex], jk_stats, jk_status, pres if want_pres else None,
                refit if want_refit else None, ms)


def run(stem: str, num_samples: int, mode: str = "all", prior_path: str | None = None, ivs_path: str | None = None,
        het: bool = False, model: int = 0, engine=None, data=None, ld: bool = False, ld_ridge: float = 0.0,
        robust: str | None = None, jackknife=None):
    """The estimates of every outcome of a merged skeleton.  `engine`: a device Engine (skeleton.Engine), or None for the
    numpy form.  `data`: what `ivcheck.load(stem, het)` returned.  Returns a dict: p, selection [(I, E)], theta, se (lists
    per outcome, None unless status 0), stats, status, sk_adj (p x p bool), kernel_ms, ld.  `ld`: the instruments are taken as
    correlated with the marker block corr[p:, p:] of the skeleton as their LD (`mvivw_ld`, ridge `ld_ridge`); stats[:, 2] is
    then the pivot of the LD matrix and status may be 4.  `robust`: None, "huber" or "bisquare" (`mvivw_robust`): stats is
    then nout x 6 (rss, scale, tau, pivot, updates, sum of rho), status may be 5 or 6, and the dict has robust (the name) and
    rho (per outcome the final rho of its instruments in the order of I, None unless status 0).  `jackknife`: None, "loo",
    a number of groups B >= 2, or a non-decreasing integer label per marker row (`groups`; `mvivw_jackknife`): the dict then
    has jackknife (True), bounds (per outcome the group boundaries), jk_status, jk_stats (nout x 2: PRESS, pivot) and, per
    outcome and None unless jk_status 0, jk (k x 4: theta_J, se_J, min, max), jk_arg, pres and refit (ng x k)."""
    if jackknife is not None and (ld or robust is not None):
        raise ValueError("mvivw: jackknife with ld or robust: whitening mixes the rows, and a reweighted refit per deletion "
                         "is another estimator")
    if robust is not None and robust not in PSI:
        raise ValueError(f"mvivw: robust {robust!r} is not huber or bisquare")
    if robust is not None and ld:
        raise ValueError("mvivw: robust with ld: whitening mixes the rows, a weight per instrument has no meaning there")
    adj, corr, p, ssz = ivcheck.load(stem, het=het) if data is None else data
    beta = np.ascontiguousarray(corr[p:, :p])
    weight = weights(beta, ssz[p:, :p] if het else num_samples)
    prior = read_prior(prior_path, p) if mode == "prior" else None
    iv_rows = read_ivs(ivs_path) if mode == "ivs" else None
    selection = select(adj, p, mode, prior=prior, iv_rows=iv_rows)
    for o, (_, E) in enumerate(selection):
        if len(E) > MAX_EXPOSURES:
            raise ValueError(f"mvivw: outcome trait {o + 1} (1-based) has {len(E)} exposures; at most {MAX_EXPOSURES} are supported")
    iv_off, iv, ex_off, ex = pack(selection)
    eng = engine if engine is not None else HostEngine()
    if ld_ridge != 0.0 and not ld:
        raise ValueError("mvivw: ld_ridge without ld")
    extra = {}
    if jackknife is not None:
        if isinstance(jackknife, str) or np.ndim(jackknife) == 0:
            if jackknife != "loo" and not (isinstance(jackknife, (int, np.integer)) and not isinstance(jackknife, bool)):
                raise ValueError(f"mvivw: jackknife {jackknife!r} is not loo, a number of groups or a list of labels")
            bounds = [groups(I, jackknife) for I, _ in selection]
        else:
            labels = np.asarray(jackknife)
            if labels.shape != (beta.shape[0],):
                raise ValueError(f"mvivw: {labels.size} group labels for {beta.shape[0]} marker rows")
            bounds = [groups(I, "labels", labels) for I, _ in selection]
        grp_off = np.zeros(p + 1, np.int64)
        grp_off[1:] = np.cumsum([len(b) for b in bounds])
        theta, se, stats, status, jk, jk_arg, jk_stats, jk_status, pres, refit, ms = eng.mvivw_jackknife(
            beta, weight, np.arange(p, dtype=np.int32), iv_off, iv, ex_off, ex, grp_off, np.concatenate(bounds).astype(np.int32), model)
        rf_off = np.concatenate([[0], np.cumsum([(len(b) - 1) * len(E) for b, (_, E) in zip(bounds, selection)])])
        jok = [int(jk_status[o]) == 0 for o in range(p)]
        extra = {"jackknife": True, "bounds": bounds, "jk_status": np.asarray(jk_status[:p]).copy(),
                 "jk_stats": np.asarray(jk_stats[:p]).copy(),
                 "jk": [np.array(jk[ex_off[o]:ex_off[o + 1]]) if jok[o] else None for o in range(p)],
                 "jk_arg": [np.array(jk_arg[ex_off[o]:ex_off[o + 1]]) if jok[o] else None for o in range(p)],
                 "pres": [np.array(pres[iv_off[o]:iv_off[o + 1]]) if jok[o] else None for o in range(p)],
                 "refit": [np.array(refit[rf_off[o]:rf_off[o + 1]]).reshape(len(bounds[o]) - 1, -1) if jok[o] else None
                           for o in range(p)]}
    elif ld:
        theta, se, stats, status, ms = eng.mvivw_ld(beta, weight, np.ascontiguousarray(corr[p:, p:], dtype=np.float64),
                                                    np.arange(p, dtype=np.int32), iv_off, iv, ex_off, ex, model, ridge=ld_ridge)
    elif robust is not None:
        theta, se, stats, status, rho, ms = eng.mvivw_robust(beta, weight, np.arange(p, dtype=np.int32), iv_off, iv, ex_off, ex,
                                                             model, psi=PSI[robust])
    else:
        theta, se, stats, status, ms = eng.mvivw(beta, weight, np.arange(p, dtype=np.int32), iv_off, iv, ex_off, ex, model)
    ok = [int(status[o]) == 0 for o in range(p)]
    if robust is not None:
        extra = {"robust": robust, "rho": [np.array(rho[iv_off[o]:iv_off[o + 1]]) if ok[o] else None for o in range(p)]}
    return {**extra, "p": p, "selection": selection, "status": np.asarray(status[:p]).copy(), "stats": np.asarray(stats[:p]).copy(),
            "theta": [np.array(theta[ex_off[o]:ex_off[o + 1]]) if ok[o] else None for o in range(p)],
            "se": [np.array(se[ex_off[o]:ex_off[o + 1]]) if ok[o] else None for o in range(p)],
            "sk_adj": np.asarray(adj)[:p, :p] != 0, "kernel_ms": ms, "ld": bool(ld)}


def _g(v) -> str:
    return "%.15g" % v


def write_results(path: str, res) -> None:
    """`<stem>_mvivw_results.tsv`: one row per ordered pair, outcome outer, exposure inner, both 1-based"""
    from scipy.special import ndtr

    p = res["p"]
    with_jk = bool(res.get("jackknife"))
    with open(path, "w") as f:
        f.write("source\tsink\teffect\tp\tsk_adj\tnum_snps\tse" + ("\tjk_effect\tjk_se\tjk_p\tjk_min\tjk_max\tjk_marker" if with_jk else "")
                + "\n")
        for o in range(p):
            I, E = res["selection"][o]
            st = int(res["status"][o])
            pos = {int(t): j for j, t in enumerate(E)}
            if st in (2, 3, 5, 6):
                print(f"mvivw: outcome trait {o + 1} (1-based): status {st}, no estimates", file=sys.stderr)
            elif st == 4:
                print(f"mvivw: outcome trait {o + 1} (1-based): status 4, the LD matrix of its instruments is not positive "
                      "definite to eight digits, no estimates; try --ld-ridge, or prune-bed at a smaller r", file=sys.stderr)
            jst = int(res["jk_status"][o]) if with_jk else 0
            if with_jk and st == 0 and jst in (1, 2):
                print(f"mvivw: outcome trait {o + 1} (1-based): jackknife status {jst}, no jackknife estimates", file=sys.stderr)
            for e in range(p):
                if e == o:
                    continue
                tail = ""
                if with_jk and e in pos and jst == 0:
                    tj, sj, lo, hi = (float(v) for v in res["jk"][o][pos[e]])
                    first = int(I[int(res["bounds"][o][int(res["jk_arg"][o][pos[e]])])]) + 1
                    with np.errstate(all="ignore"):
                        pj = 2.0 * ndtr(-abs(np.float64(tj) / np.float64(sj)))
                    tail = "\t" + "\t".join((_g(tj), _g(sj), _g(pj), _g(lo), _g(hi), str(first)))
                elif with_jk:
                    tail = "\tNA" * 6
                if e not in pos or st == 1:
                    eff, pv, se = "0", "1", "NA"  # the reference's fill
                elif st != 0:
                    eff, pv, se = "NA", "NA", "NA"
                else:
                    th, s = float(res["theta"][o][pos[e]]), float(res["se"][o][pos[e]])
                    with np.errstate(all="ignore"):
                        eff, pv, se = _g(th), _g(2.0 * ndtr(-abs(np.float64(th) / np.float64(s)))), _g(s)
                adjacent = "TRUE" if res["sk_adj"][e, o] else "FALSE"
                f.write(f"{e + 1}\t{o + 1}\t{eff}\t{pv}\t{adjacent}\t{len(I)}\t{se}{tail}\n")


def write_outcomes(path: str, res) -> None:
    """`<stem>_mvivw_outcomes.tsv`: per outcome the heterogeneity statistic q = rss and its upper chi-square tail; with
    `--ld` a last column ld_pivot, the smallest squared pivot of the LD matrix (status 4: the pivot that failed); with
    `--robust` the last columns scale, tau, iterations, rho_sum of the robust fit, q = the plain rss at the robust estimate
    and sigma = sqrt(q / (m - k))"""
    from scipy.stats import chi2

    with_ld, robust, with_jk = bool(res.get("ld")), res.get("robust") is not None, bool(res.get("jackknife"))
    with open(path, "w") as f:
        f.write("sink\tn_exposures\tnum_snps\tsigma\tq\tq_p\tstatus" + ("\tld_pivot" if with_ld else "")
                + ("\tscale\ttau\titerations\trho_sum" if robust else "")
                + ("\tjk_groups\tpress\tjk_pivot\tjk_status" if with_jk else "") + "\n")
        for o in range(res["p"]):
            I, E = res["selection"][o]
            st = int(res["status"][o])
            if st == 0 and robust:
                rss = float(res["stats"][o][0])
                sigma = float(np.sqrt(rss / (len(I) - len(E))))
                cols = (_g(sigma), _g(rss), _g(float(chi2.sf(rss, len(I) - len(E)))))
            elif st == 0:
                rss, sigma = float(res["stats"][o][0]), float(res["stats"][o][1])
                cols = (_g(sigma), _g(rss), _g(float(chi2.sf(rss, len(I) - len(E)))))
            else:
                cols = ("NA", "NA", "NA")
            piv = float(res["stats"][o][2])
            tail = ("\t" + (_g(piv) if st in (0, 4) and np.isfinite(piv) else "NA")) if with_ld else ""
            if robust:
                r = res["stats"][o]
                tail += "\t" + ("\t".join((_g(float(r[1])), _g(float(r[2])), str(int(r[4])), _g(float(r[5])))) if st == 0
                                else "NA\tNA\tNA\tNA")
            if with_jk:
                jst, (press, jpiv) = int(res["jk_status"][o]), (float(v) for v in res["jk_stats"][o])
                tail += (f"\t{len(res['bounds'][o]) - 1}\t" + (_g(press) if jst == 0 else "NA") + "\t"
                         + (_g(jpiv) if np.isfinite(jpiv) else "NA") + f"\t{jst}")
            f.write(f"{o + 1}\t{len(E)}\t{len(I)}\t" + "\t".join(cols) + f"\t{st}{tail}\n")


def write_weights(path: str, res) -> None:
    """`--robust-weights`: `sink marker rho` for every instrument of an estimated outcome whose final rho is below 1; sink
    1-based, marker counted from the first marker as in the `Exposure,Outcome,IV` tables"""
    with open(path, "w") as f:
        f.write("sink\tmarker\trho\n")
        for o in range(res["p"]):
            rho = res["rho"][o]
            if rho is None:
                continue
            I = res["selection"][o][0]
            for j in np.flatnonzero(np.asarray(rho) < 1.0):
                f.write(f"{o + 1}\t{int(I[j]) + 1}\t{_g(float(rho[j]))}\n")


def write_jackknife_residuals(path: str, res) -> None:
    """`--jackknife-residuals`: `sink marker group press_residual` for every instrument of an outcome of jk_status 0; sink,
    marker (counted from the first marker) and group 1-based"""
    with open(path, "w") as f:
        f.write("sink\tmarker\tgroup\tpress_residual\n")
        for o in range(res["p"]):
            if res["pres"][o] is None:
                continue
            I, b = res["selection"][o][0], res["bounds"][o]
            grp = np.repeat(np.arange(len(b) - 1), np.diff(b))
            for j in range(len(I)):
                f.write(f"{o + 1}\t{int(I[j]) + 1}\t{int(grp[j]) + 1}\t{_g(float(res['pres'][o][j]))}\n")


def write_jackknife_table(path: str, res) -> None:
    """`--jackknife-table`: `sink group first_marker last_marker n source effect`, the estimate of every exposure without
    each group, for the outcomes of jk_status 0; all numbers 1-based, markers counted from the first marker"""
    with open(path, "w") as f:
        f.write("sink\tgroup\tfirst_marker\tlast_marker\tn\tsource\teffect\n")
        for o in range(res["p"]):
            if res["refit"][o] is None:
                continue
            (I, E), b = res["selection"][o], res["bounds"][o]
            for g in range(len(b) - 1):
                head = f"{o + 1}\t{g + 1}\t{int(I[b[g]]) + 1}\t{int(I[b[g + 1] - 1]) + 1}\t{int(b[g + 1] - b[g])}"
                for j, t in enumerate(E):
                    f.write(f"{head}\t{int(t) + 1}\t{_g(float(res['refit'][o][g][j]))}\n")
