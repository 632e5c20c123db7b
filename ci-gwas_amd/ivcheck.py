"""`ci-gwas iv-candidates` / `check-ivs`: the instrument table of a merged skeleton under the MR assumptions.

Counterpart of the reference's cusk_postprocessing/check_mr_assumptions.py (`get_iv_candidates`, `check_ivs`), written
from its semantics; the table `Exposure,Outcome,IV` is what the reference's Mendelian-randomisation back-ends read.

Inputs: `<stem>_sam.mtx` (dense), `<stem>_scm.mtx` (dense, diagonal set to 1), `<stem>.mdim` (three tab-separated
integers, the second is the number of traits p; traits are variables 0 .. p-1).  No collinear markers are removed.

Kept on purpose, because the reference's tables depend on it:
  * the instrument candidates of trait t are {v : adj[t, v] != 0 and v > p} -- STRICTLY greater, so the first marker
    (variable p) is never a candidate.
Deliberate deviations: rows of one (exposure, outcome) pair come out by ascending IV (the reference's order there is the
iteration order of a Python set and is not promised); a result without rows still writes the header line (the
reference's empty frame has no columns and writes an empty line).

One test of (x, y | S) at level alpha: z = |0.5 log|(1 + rho)/(1 - rho)|| with rho the partial correlation of x and y
given S, "independent" iff z < norm.ppf(1 - alpha/2) / sqrt(N - |S| - 3), all in IEEE double; a NaN on either side makes
the comparison false ("dependent").  The reference inverts the sub-matrix over [x, y] + S once per test; per outcome the
set is the same for every SNP, so here W = C[S,S]^-1 is formed once per set and a test costs the 2 x 2 Schur complement
(csrc/iv_check.hip on the device, `host_z` / `HostEngine` below in numpy -- the same formula, used when no engine is given).

Not in the reference: `het=True` decides every test at the sample sizes of the variables it is about, read from
`<stem>_ssz.mtx`: the threshold of a test over V = {x, y} + S, |S| = l, is q / sqrt(mean - l - 3) with mean the integer
sum of the sizes of all unordered pairs of V over their count (the rule of `sepselect --het`); `num_samples` is not used.
"""
from __future__ import annotations

import os

import numpy as np


class SingularSetError(RuntimeError):
    pass


def load(stem: str, het: bool = False):
    """(adj dense, corr dense float64 with unit diagonal, p, ssz or None)"""
    from scipy.io import mmread

    if het and not os.path.exists(f"{stem}_ssz.mtx"):
        raise FileNotFoundError(f"{stem}_ssz.mtx is missing: --het needs the per-pair sample sizes that "
                                "`cuskss-merged --het` (or cuskss with --mxp-se/--pxp-se) writes beside the skeleton")
    with open(f"{stem}.mdim") as fin:
        _, p, _ = (int(f) for f in fin.readline().strip().split("\t"))
    adj = np.asarray(mmread(f"{stem}_sam.mtx").toarray())
    corr = np.array(mmread(f"{stem}_scm.mtx").toarray(), dtype=np.float64)
    np.fill_diagonal(corr, 1.0)
    ssz = None
    if het:
        ssz = np.nan_to_num(np.asarray(mmread(f"{stem}_ssz.mtx").toarray(), dtype=np.float64), nan=0.0)
        if ssz.shape != corr.shape:
            raise ValueError(f"{stem}_ssz.mtx and {stem}_scm.mtx differ in shape")
    return adj, corr, p, ssz


def _candidates(adj, p: int):
    """per trait: the ascending marker neighbours; `v > p` leaves the first marker (variable p) out, as the reference does"""
    out = []
    for t in range(p):
        nb = np.flatnonzero(adj[t, :])
        out.append(nb[nb > p])
    return out


def _rows(per_pair, p: int):
    """(e, o) pairs e outer, o inner; ascending IV inside a pair; 1-based traits, IV counted from the first marker"""
    rows = []
    for e in range(p):
        for o in range(p):
            if e != o:
                rows.extend((e + 1, o + 1, int(v) + 1 - p) for v in sorted(per_pair.get((e, o), ())))
    return rows


def iv_candidates(stem: str, data=None):
    """get_iv_candidates: every candidate of the exposure, for every (exposure, outcome) pair.  `data`: what `load(stem)`
    returned, to spare reading the files again."""
    adj, _, p, _ = load(stem) if data is None else data
    cands = _candidates(adj, p)
    return _rows({(e, o): cands[e].tolist() for e in range(p) for o in range(p) if e != o}, p)


def write_csv(path: str, rows) -> None:
    """pandas' to_csv(index=False) of the three integer columns; an empty table keeps its header"""
    with open(path, "w") as f:
        f.write("Exposure,Outcome,IV\n")
        for e, o, v in rows:
            f.write(f"{int(e)},{int(o)},{int(v)}\n")


def thresholds(alpha: float, num_samples: int, p: int):
    """thr[l] = norm.ppf(1 - alpha/2) / sqrt(N - l - 3), l = 0 .. p-1 (NaN where the radicand is negative)"""
    from scipy.stats import norm

    with np.errstate(invalid="ignore", divide="ignore"):
        return norm.ppf(1 - (alpha / 2)) / np.sqrt(num_samples - np.arange(p, dtype=np.int64) - 3)


def _fisher_z(r):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(0.5 * np.log(np.abs((1 + r) / (1 - r))))


def exactly_singular(A) -> bool:
    """The device's rule for status 2 (csrc/iv_check.hip, iv_setup_kernel), restated: Gauss-Jordan with partial pivoting
    in double without fused multiply-add meets a pivot column that is exactly zero.  Two identical traits cancel to exact
    zeros under it, which LAPACK's factorisation behind np.linalg.inv need not notice."""
    A = np.array(A, dtype=np.float64)
    s = A.shape[0]
    with np.errstate(all="ignore"):
        for k in range(s):
            col = np.abs(A[k:, k])
            best = np.nanmax(col) if not np.all(np.isnan(col)) else -1.0
            if best == 0.0:
                return True
            r = k + int(np.nanargmax(col)) if best > 0 else k
            A[[k, r]] = A[[r, k]]
            f = A[:, k] / A[k, k]
            f[k] = 0.0
            A = A - np.outer(f, A[k])
    return False


def host_z(trait_corr, set_off, sets, item_x, item_y, item_set):
    """z of every item by the Schur formula in float64 numpy: one np.linalg.inv per set, vectorised over the items of a
    (set, y) group.  Returns (z, status); status 2 marks the items of a set that is singular by the device's rule
    (`exactly_singular`) or that np.linalg.inv refuses."""
    tc = np.asarray(trait_corr, np.float64)
    p = tc.shape[1]
    item_x, item_y, item_set = (np.asarray(a, np.int64).reshape(-1) for a in (item_x, item_y, item_set))
    z = np.full(item_x.shape[0], np.nan)
    status = np.zeros(item_x.shape[0], np.int32)
    if item_x.shape[0] == 0:
        return z, status
    key = item_set * (int(tc.shape[0]) + 1) + item_y
    order = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    inv = {}
    for grp in np.split(order, cuts):
        s, y = int(item_set[grp[0]]), int(item_y[grp[0]])
        xs = item_x[grp]
        cxy = tc[xs, y] if y < p else tc[y, xs]
        if s < 0 or set_off[s + 1] == set_off[s]:
            z[grp] = _fisher_z(cxy)
            continue
        ids = np.asarray(sets[set_off[s]:set_off[s + 1]], np.int64)
        if s not in inv:
            try:
                inv[s] = None if exactly_singular(tc[np.ix_(ids, ids)]) else np.linalg.inv(tc[np.ix_(ids, ids)])
            except np.linalg.LinAlgError:
                inv[s] = None
        W = inv[s]
        if W is None:
            status[grp] = 2
            continue
        cy = tc[y, ids]
        wy = W @ cy
        dyy = 1.0 - cy @ wy
        X = tc[np.ix_(xs, ids)]
        dxy = cxy - X @ wy
        dxx = 1.0 - np.einsum("ij,ij->i", X @ W, X)
        with np.errstate(invalid="ignore", divide="ignore"):
            z[grp] = _fisher_z(dxy / np.sqrt(np.abs(dxx * dyy)))
    return z, status


def het_thresholds(trait_n, set_off, sets, item_x, item_y, item_set, q: float):
    """q / sqrt(mean - l - 3) per item, mean = integer sum of the sizes of all unordered pairs of {x, y} + S / their count"""
    tn = np.asarray(trait_n, np.int64)
    n, p = tn.shape
    item_x, item_y, item_set = (np.asarray(a, np.int64).reshape(-1) for a in (item_x, item_y, item_set))
    thr = np.empty(item_x.shape[0])
    if item_x.shape[0] == 0:
        return thr
    key = item_set * (n + 1) + item_y
    order = np.argsort(key, kind="stable")
    for grp in np.split(order, np.flatnonzero(np.diff(key[order])) + 1):
        s, y = int(item_set[grp[0]]), int(item_y[grp[0]])
        xs = item_x[grp]
        ids = np.asarray(sets[set_off[s]:set_off[s + 1]], np.int64) if s >= 0 else np.zeros(0, np.int64)
        l = ids.shape[0]
        base = int(np.triu(tn[np.ix_(ids, ids)], 1).sum()) + int(tn[y, ids].sum())  # the pairs inside S + {y}
        nsum = base + tn[np.ix_(xs, ids)].sum(axis=1) + (tn[xs, y] if y < p else tn[y, xs])
        mean = nsum.astype(np.float64) / np.float64((l + 2) * (l + 1) // 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            thr[grp] = q / np.sqrt(mean - np.float64(l) - 3.0)
    return thr


class HostEngine:
    """The engine's two calls in numpy: what `check_ivs(engine=None)` runs on"""

    def iv_check(self, trait_corr, set_off, sets, item_x, item_y, item_set, thr):
        z, status = host_z(trait_corr, set_off, sets, item_x, item_y, item_set)
        lens = np.diff(np.asarray(set_off, np.int64)) if len(set_off) > 1 else np.zeros(0, np.int64)
        iset = np.asarray(item_set, np.int64).reshape(-1)
        l = np.where(iset >= 0, lens[np.maximum(iset, 0)] if lens.shape[0] else 0, 0)
        with np.errstate(invalid="ignore"):
            indep = z < np.asarray(thr, np.float64)[l]
        return z, indep.astype(np.int32) * (status == 0) | (status << 8), 0.0

    def iv_check_het(self, trait_corr, set_off, sets, item_x, item_y, item_set, trait_n, q):
        z, status = host_z(trait_corr, set_off, sets, item_x, item_y, item_set)
        thr = het_thresholds(trait_n, set_off, sets, item_x, item_y, item_set, q)
        with np.errstate(invalid="ignore"):
            indep = z < thr
        return z, indep.astype(np.int32) * (status == 0) | (status << 8), 0.0


class _Tester:
    """One alpha-specific call per batch; verdicts as bool arrays"""

    def __init__(self, engine, corr, p, num_samples, ssz):
        self.engine = engine
        self.tc = np.ascontiguousarray(corr[:, :p])
        self.p = p
        self.N = num_samples
        self.tn = None if ssz is None else np.ascontiguousarray(ssz[:, :p]).astype(np.int32)
        self.kernel_ms = 0.0
        self.calls = 0

    def run(self, alpha, set_lists, xs, ys, iset, outcome_of_set):
        """independent? for every item; `set_lists` = list of trait-id lists"""
        if len(xs) == 0:
            return np.zeros(0, bool)
        set_off = np.zeros(len(set_lists) + 1, np.int32)
        set_off[1:] = np.cumsum([len(s) for s in set_lists])
        sets = np.array([t for s in set_lists for t in s], np.int32)
        if self.tn is not None:
            from scipy.stats import norm

            _, flags, ms = self.engine.iv_check_het(self.tc, set_off, sets, xs, ys, iset, self.tn, norm.ppf(1 - (alpha / 2)))
        else:
            _, flags, ms = self.engine.iv_check(self.tc, set_off, sets, xs, ys, iset, thresholds(alpha, self.N, self.p))
        self.kernel_ms += ms
        self.calls += 1
        bad = np.flatnonzero((flags >> 8) == 2)
        if bad.size:
            o = outcome_of_set[int(np.asarray(iset)[bad[0]])]
            raise SingularSetError(f"check-ivs: the correlation matrix of the conditioning traits of outcome trait {o + 1} "
                                   "(1-based) is singular")
        return (flags & 1).astype(bool)


def check_ivs(stem: str, num_samples: int, accept_alpha: float, reject_alpha: float, relaxed_local_faithfulness: bool = False,
              check_reverse_causality: bool = False, het: bool = False, engine=None, stats: dict | None = None, data=None):
    """The rows (Exposure, Outcome, IV) of the instruments that pass.  `engine`: a device Engine (skeleton.Engine), or None
    for the numpy form.  `stats`, if given, receives kernel_ms and the number of engine calls (at most four).  `data`: what
    `load(stem, het)` returned, to spare reading the files again."""
    # a missing _ssz.mtx is reported before anything else happens
    adj, corr, p, ssz = load(stem, het=het) if data is None else data
    n = corr.shape[0]
    if not np.array_equal(corr[:, :p], corr[:p, :].T, equal_nan=True):
        raise ValueError("check-ivs: the correlation matrix is not symmetric on its trait rows / columns")
    if het and not np.array_equal(ssz[:, :p], ssz[:p, :].T):
        raise ValueError("check-ivs: the sample sizes are not symmetric on their trait rows / columns")
    tester = _Tester(engine if engine is not None else HostEngine(), corr, p, num_samples, ssz)
    cands = _candidates(adj, p)
    traits = np.arange(p)
    # marginal tests (snp, trait | {}) at accept_alpha, shared by both passes: 0 unknown, 1 dependent, 2 independent
    marg = np.zeros((n, p), np.int8)

    def marginal(xs, ys):
        xs, ys = np.asarray(xs, np.int32), np.asarray(ys, np.int32)
        todo = np.flatnonzero(marg[xs, ys] == 0)
        if todo.size:
            pair = np.unique(np.stack([xs[todo], ys[todo]], axis=1), axis=0)
            ind = tester.run(accept_alpha, [], pair[:, 0], pair[:, 1], np.full(pair.shape[0], -1, np.int32), {})
            marg[pair[:, 0], pair[:, 1]] = np.where(ind, 2, 1)
        return marg[xs, ys] == 1  # dependent

    rev_cause = [set() for _ in range(p)]
    if check_reverse_causality:
        xs, ys, os_ = [], [], []
        for o in range(p):
            if cands[o].size == 0:
                continue
            for e in range(p):
                if e != o:
                    xs.append(cands[o])
                    ys.append(np.full(cands[o].size, e))
                    os_.append(np.full(cands[o].size, o))
        if xs:
            xs, ys, os_ = (np.concatenate(a).astype(np.int32) for a in (xs, ys, os_))
            dep = marginal(xs, ys)
            ind = tester.run(reject_alpha, [[o] for o in range(p)], xs, ys, os_, {o: o for o in range(p)})
            for k in np.flatnonzero(dep & ind):
                rev_cause[int(os_[k])].add(int(ys[k]))
    valid = [sorted(set(traits.tolist()) - rev_cause[o] - {o}) for o in range(p)]

    # main pass: the conditional test of (snp, o | valid[o]) does not depend on the exposure
    xs, os_ = [], []
    for o in range(p):
        pool = [cands[e] for e in valid[o] if cands[e].size]
        if pool:
            u = np.unique(np.concatenate(pool))
            xs.append(u)
            os_.append(np.full(u.size, o))
    kept = {}
    if xs:
        xs, os_ = (np.concatenate(a).astype(np.int32) for a in (xs, os_))
        ok = np.ones(xs.size, bool) if relaxed_local_faithfulness else marginal(xs, os_)
        iset = np.where([len(valid[int(o)]) > 0 for o in os_], os_, -1).astype(np.int32)
        ok &= tester.run(reject_alpha, valid, xs, os_, iset, {o: o for o in range(p)})
        passed = np.zeros((n, p), bool)
        passed[xs[ok], os_[ok]] = True
        for o in range(p):
            for e in valid[o]:
                kept[(e, o)] = cands[e][passed[cands[e], o]].tolist()
    if stats is not None:
        stats["kernel_ms"] = tester.kernel_ms
        stats["calls"] = tester.calls
    return _rows(kept, p)
