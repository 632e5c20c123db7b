"""Deterministic synthetic inputs for tests and bench.py.

Mirrors the parameters of the reference's simulator
(/root/reference/simulation/simulate_dag.R:106-115: SNP -> trait effects,
trait -> trait DAG, unit noise) on genotypes with realistic block LD so that
level-0 degrees look like an LD-pruned block: windows of `window` SNPs, latent
AR(1) Gaussian (rho) inside a window, two latent copies thresholded at the
MAF and summed to {0,1,2}.  Seeds: numpy Generator(PCG64(20251003 + block_index)).
"""
from __future__ import annotations

import numpy as np

BASE_SEED = 20251003


def rng_for(block_index: int = 0) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(BASE_SEED + int(block_index)))


def make_genotypes(m: int, N: int, rng, window: int = 100, rho: float = 0.85, miss: float = 0.001) -> np.ndarray:
    """m x N int8 dosages in {0,1,2}, -1 = missing."""
    from scipy.stats import norm

    G = np.empty((m, N), np.int8)
    maf = rng.uniform(0.05, 0.5, size=m)
    thr = norm.ppf(1.0 - maf).astype(np.float32)
    s = np.float32(np.sqrt(1.0 - rho * rho))
    for w0 in range(0, m, window):
        w1 = min(m, w0 + window)
        acc = np.zeros((w1 - w0, N), np.int8)
        for _copy in range(2):
            z = rng.standard_normal((w1 - w0, N), dtype=np.float32)
            for j in range(1, w1 - w0):
                z[j] = np.float32(rho) * z[j - 1] + s * z[j]
            acc += (z > thr[w0:w1, None]).astype(np.int8)
        G[w0:w1] = acc
    if miss > 0:
        mask = rng.random((m, N), dtype=np.float32) < miss
        G[mask] = -1
    return G


def make_traits(G: np.ndarray, p: int, rng, causal_per_1000: float = 5.0) -> np.ndarray:
    """p x N float32 standardised traits: sparse SNP effects + lower-triangular trait DAG."""
    m, N = G.shape
    Y = np.zeros((p, N), np.float64)
    ncausal = max(1, int(round(causal_per_1000 * m / 1000.0)))
    for k in range(p):
        idx = rng.choice(m, size=min(ncausal, m), replace=False)
        beta = rng.uniform(0.02, 0.08, size=idx.size) * rng.choice([-1.0, 1.0], size=idx.size)
        g = G[idx].astype(np.float64)
        g[g < 0] = np.nan
        mu = np.nanmean(g, axis=1, keepdims=True)
        sd = np.nanstd(g, axis=1, keepdims=True)
        sd[sd == 0] = 1.0
        gs = np.nan_to_num((g - mu) / sd)
        y = beta @ gs
        for k2 in range(k):
            if rng.random() < 3.0 / p:
                y = y + rng.uniform(0.05, 0.2) * rng.choice([-1.0, 1.0]) * Y[k2]
        y = y + rng.standard_normal(N)
        Y[k] = (y - y.mean()) / y.std()
    return Y.astype(np.float32)


_CODE = np.array([3, 2, 0, 1], np.uint8)  # dosage 0,1,2,missing(-1) -> 2-bit code 11,10,00,01


def pack_bed(G: np.ndarray) -> np.ndarray:
    """m x ceil(N/4) uint8, PLINK SNP-major 2-bit codes, low bits first (no magic bytes).
    Padding samples get code 0 like PLINK's writers."""
    m, N = G.shape
    codes = _CODE[G.astype(np.int64)]  # -1 indexes the last entry (missing)
    pad = (-N) % 4
    if pad:
        codes = np.concatenate([codes, np.zeros((m, pad), np.uint8)], axis=1)
    c = codes.reshape(m, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def bed_stats(G: np.ndarray):
    """per-marker mean and population std over non-missing samples (reference prep.cpp:56-73)."""
    m = G.shape[0]
    mean = np.empty(m, np.float32)
    std = np.empty(m, np.float32)
    for r0 in range(0, m, 512):
        g = G[r0:r0 + 512].astype(np.float64)
        g[g < 0] = np.nan
        mean[r0:r0 + 512] = np.nanmean(g, axis=1)
        std[r0:r0 + 512] = np.nanstd(g, axis=1)
    return mean, std


def synth_bed_block(m: int, N: int, p: int, block_index: int = 0, **kw):
    """(bed bytes m x ceil(N/4), phen column-major p*N float32, means, stds, G)."""
    rng = rng_for(block_index)
    G = make_genotypes(m, N, rng, **kw)
    Y = make_traits(G, p, rng)
    means, stds = bed_stats(G)
    return pack_bed(G), np.ascontiguousarray(Y).reshape(-1), means, stds, G


def corr_from_samples(G: np.ndarray, Y: np.ndarray, device: str | None = None) -> np.ndarray:
    """(m+p) x (m+p) float32 Pearson correlation of mean-imputed dosages and traits."""
    m, N = G.shape
    X = np.concatenate([G.astype(np.float32), Y.astype(np.float32)], axis=0)
    X[:m][G < 0] = np.nan
    mu = np.nanmean(X, axis=1, keepdims=True)
    X = np.nan_to_num(X - mu)
    X /= np.maximum(np.sqrt((X * X).sum(axis=1, keepdims=True)), 1e-30)
    if device is not None:
        import torch

        t = torch.from_numpy(X).to(device)
        Cm = (t @ t.T).float().cpu().numpy()
    else:
        Cm = X @ X.T
    Cm = np.clip(Cm, -1.0, 1.0).astype(np.float32)
    Cm = np.maximum(Cm, Cm.T) * (np.abs(Cm) >= np.abs(Cm.T)) + np.minimum(Cm, Cm.T) * (np.abs(Cm) < np.abs(Cm.T))
    np.fill_diagonal(Cm, 1.0)
    return np.ascontiguousarray(Cm, np.float32)


def synth_corr_block(m: int, p: int, N: int = 16384, block_index: int = 0, device: str | None = None, **kw):
    """Summary-statistics style input for cuskss: symmetric n x n fp32 correlation matrix."""
    rng = rng_for(block_index)
    G = make_genotypes(m, N, rng, **kw)
    Y = make_traits(G, p, rng)
    return corr_from_samples(G, Y, device)


def random_corr(n: int, seed: int, k: int | None = None, strength: float = 1.0) -> np.ndarray:
    """Small dense test matrix: sample correlation of a random sparse linear SEM
    (recipe of /root/reference/cusk/scripts/skeleton_gen.py:19-90, own code)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = k or 4 * n
    B = np.tril(rng.random((n, n)) < min(1.0, 2.5 / n), -1) * rng.uniform(0.3, 0.9, (n, n)) * strength
    B *= rng.choice([-1.0, 1.0], size=(n, n))
    X = np.zeros((n, k))
    E = rng.standard_normal((n, k))
    for i in range(n):
        X[i] = B[i] @ X + E[i]
    Cm = np.corrcoef(X).astype(np.float32)
    Cm = np.triu(Cm, 1)
    Cm = Cm + Cm.T
    np.fill_diagonal(Cm, 1.0)
    return np.ascontiguousarray(Cm, np.float32)


def write_bfiles(stem: str, bed: np.ndarray, N: int, means, stds, chr_ids=None) -> None:
    """<stem>.bed/.bim/.fam/.dim/.means/.stds as the reference's `mps prep` leaves them
    (reference io.h:30-64, prep.cpp:157-201, bfiles_base.h:8-9)."""
    m = bed.shape[0]
    chr_ids = chr_ids if chr_ids is not None else ["1"] * m
    with open(stem + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.ascontiguousarray(bed, np.uint8).tobytes())
    with open(stem + ".bim", "w") as f:
        for i in range(m):
            f.write(f"{chr_ids[i]}\trs{i}\t0\t{1000 + i}\tA\tG\n")
    with open(stem + ".fam", "w") as f:
        for i in range(N):
            f.write(f"f{i} i{i} 0 0 0 -9\n")
    with open(stem + ".dim", "w") as f:
        f.write(f"{N}\t{m}\n")
    for sfx, arr in ((".means", means), (".stds", stds)):
        with open(stem + sfx, "w") as f:
            for v in np.asarray(arr, np.float32):
                f.write(repr(float(v)) + "\n")


def write_phen(path: str, phen_colmajor: np.ndarray, N: int, p: int) -> None:
    """header + `FID IID v1..vp` rows, NaN written as NA (reference phen.cpp:9-74)."""
    Y = np.asarray(phen_colmajor, np.float32).reshape(p, N)
    with open(path, "w") as f:
        f.write("FID IID " + " ".join(f"T{k}" for k in range(p)) + "\n")
        for i in range(N):
            f.write(f"f{i} i{i} " + " ".join("NA" if np.isnan(Y[k, i]) else repr(float(Y[k, i])) for k in range(p)) + "\n")


def synth_corr_block_torch(m: int, p: int, N: int = 16384, block_index: int = 0, device: str = "cuda",
                           window: int = 100, rho: float = 0.85):
    """Full-size variant of synth_corr_block generated on the GPU with torch (plumbing only): same
    generative model (LD windows with latent AR(1), MAF ~ U(0.05, 0.5), sparse SNP effects + trait DAG),
    torch's generator instead of numpy's.  Returns a CUDA float32 tensor (m+p) x (m+p), symmetric, unit diagonal."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(BASE_SEED + int(block_index))
    n = m + p
    X = torch.empty((n, N), dtype=torch.float32, device=device)
    s = (1.0 - rho * rho) ** 0.5
    nrm = torch.distributions.Normal(0.0, 1.0)
    for w0 in range(0, m, window):
        w1 = min(m, w0 + window)
        maf = torch.rand(w1 - w0, generator=g, device=device) * 0.45 + 0.05
        thr = nrm.icdf(1.0 - maf).unsqueeze(1)
        acc = torch.zeros((w1 - w0, N), dtype=torch.float32, device=device)
        for _copy in range(2):
            z = torch.randn((w1 - w0, N), generator=g, device=device)
            for j in range(1, w1 - w0):
                z[j] = rho * z[j - 1] + s * z[j]
            acc += (z > thr).float()
        X[w0:w1] = acc
    Xs = X[:m] - X[:m].mean(1, keepdim=True)
    Xs = Xs / Xs.std(1, keepdim=True).clamp_min(1e-6)
    ncausal = max(1, int(round(5.0 * m / 1000.0)))
    for k in range(p):
        idx = torch.randint(0, m, (ncausal,), generator=g, device=device)
        beta = (torch.rand(ncausal, generator=g, device=device) * 0.06 + 0.02) * (
            torch.randint(0, 2, (ncausal,), generator=g, device=device).float() * 2 - 1)
        y = beta @ Xs[idx]
        for k2 in range(k):
            if float(torch.rand(1, generator=g, device=device)) < 3.0 / p:
                y = y + (0.05 + 0.15 * float(torch.rand(1, generator=g, device=device))) * X[m + k2]
        y = y + torch.randn(N, generator=g, device=device)
        X[m + k] = (y - y.mean()) / y.std()
    del Xs
    X -= X.mean(1, keepdim=True)
    X /= X.norm(dim=1, keepdim=True).clamp_min(1e-30)
    Cm = X @ X.T
    del X
    Cm.clamp_(-1.0, 1.0)
    Cm = torch.triu(Cm, 1)
    Cm = Cm + Cm.T
    Cm.fill_diagonal_(1.0)
    return Cm


def hub_corr(nleaf: int, nhub: int, seed: int, noise: float = 1.0) -> np.ndarray:
    """Population correlation matrix of `nleaf` nearly independent variables and `nhub` hubs, each a random signed
    combination of ALL leaves plus noise.  A hub stays adjacent to every leaf whatever is conditioned on (the edges are
    real), so the skeleton keeps a degree of nleaf + nhub - 1 to the deepest level: the matrix that drives the sweep
    through levels 9..14 in the tests (level l of a hub row enumerates C(nleaf + nhub - 1, l) conditioning sets)."""
    rng = np.random.default_rng(seed)
    n = nleaf + nhub
    A = np.eye(nleaf) + 0.02 * rng.normal(size=(nleaf, nleaf))
    SL = A @ A.T
    W = rng.uniform(0.5, 1.0, size=(nhub, nleaf)) * rng.choice([-1.0, 1.0], size=(nhub, nleaf))
    S = np.zeros((n, n))
    S[:nleaf, :nleaf] = SL
    S[nleaf:, :nleaf] = W @ SL
    S[:nleaf, nleaf:] = S[nleaf:, :nleaf].T
    S[nleaf:, nleaf:] = W @ SL @ W.T + noise * np.eye(nhub)
    d = np.sqrt(np.diag(S))
    C = (S / d[:, None] / d[None, :]).astype(np.float32)
    C = np.minimum(C, C.T)
    np.fill_diagonal(C, 1.0)
    return np.ascontiguousarray(C)


def merged_skeleton(seed: int, p: int, m: int, duplicates: int = 0, with_prior: bool = False, block: int = 5,
                    trait_edge_prob: float = 0.35, noise: float = 0.0):
    """A merged cusk skeleton in the layout `merge-block-outputs` writes (traits 0..p-1, then m selected markers):
    the population correlation matrix of a linear model -- markers in LD blocks of `block`, each trait driven by
    a few markers, a random lower-triangular trait DAG -- and an adjacency read off it.  Marker-marker entries
    outside a block are dropped (zero), as in a merged `_scm.mtx`; the trait rows and columns are complete, so
    every sub-matrix the separation-set search inverts is positive definite.  `duplicates` markers are exact
    copies of their predecessor (what `rm_collinear_markers` is there for).  `noise` > 0 adds symmetric Gaussian
    estimation noise of that scale to the stored off-diagonal entries (population values carry structural exact
    zeros and with them exact ties between candidates, which sample correlations do not have).
    Returns (adj bool n x n, corr f64 n x n with unit diagonal, ixs i32 m, prior i32 p x p or None)."""
    rng = np.random.default_rng(seed)
    n = p + m
    blk = np.arange(m) // block
    Sm = np.where(blk[:, None] == blk[None, :], 0.6 ** np.abs(np.arange(m)[:, None] - np.arange(m)[None, :]), 0.0)
    B = np.zeros((p, m))
    for t in range(p):
        k = rng.integers(2, 5)
        cols = rng.choice(m, size=min(k, m), replace=False)
        B[t, cols] = rng.uniform(0.12, 0.35, size=cols.size) * rng.choice([-1.0, 1.0], size=cols.size)
    A = np.tril(rng.uniform(0.15, 0.45, size=(p, p)) * rng.choice([-1.0, 1.0], size=(p, p)), -1)
    A *= np.tril(rng.random((p, p)) < trait_edge_prob, -1)
    T = np.linalg.inv(np.eye(p) - A)
    # variables [traits, markers]:  y = T (B x + e),  x ~ (0, Sm),  e ~ (0, I)
    cov = np.zeros((n, n))
    cov[p:, p:] = Sm
    cov[:p, p:] = T @ B @ Sm
    cov[p:, :p] = cov[:p, p:].T
    cov[:p, :p] = T @ (B @ Sm @ B.T + np.eye(p)) @ T.T
    sd = np.sqrt(np.diag(cov))
    corr = cov / np.outer(sd, sd)
    corr = 0.5 * (corr + corr.T)
    dup = rng.choice(np.arange(1, m), size=duplicates, replace=False) if duplicates else []
    for b in dup:  # marker b becomes an exact copy of marker b - 1
        a = p + b - 1
        b = p + b
        corr[b, :] = corr[a, :]
        corr[:, b] = corr[:, a]
        corr[a, b] = corr[b, a] = 1.0
    np.fill_diagonal(corr, 1.0)
    same_block = np.zeros((n, n), dtype=bool)
    same_block[p:, p:] = blk[:, None] == blk[None, :]
    adj = np.abs(corr) > 0.08
    adj[p:, p:] &= same_block[p:, p:] & (np.abs(corr[p:, p:]) > 0.2)
    np.fill_diagonal(adj, False)
    keep = np.ones((n, n), dtype=bool)
    keep[p:, p:] = same_block[p:, p:]
    corr = np.where(keep, corr, 0.0)
    if noise > 0.0:
        g = np.random.default_rng(seed + 7919).normal(scale=noise, size=(n, p))
        e = np.zeros((n, n))
        e[:, :p] = g
        e[:p, :] = g.T
        e[:p, :p] = 0.5 * (g[:p] + g[:p].T)
        np.fill_diagonal(e, 0.0)
        corr = corr + e
    ixs = np.sort(rng.choice(50 * m, size=m, replace=False)).astype(np.int32)
    prior = None
    if with_prior:
        prior = np.zeros((p, p), dtype=np.int32)
        ii, jj = np.nonzero(np.triu(adj[:p, :p], 1))
        for k in rng.choice(ii.size, size=min(3, ii.size), replace=False) if ii.size else []:
            prior[jj[k], ii[k]] = 1
    return adj, corr, ixs, prior


# ---------------------------------------------------------------------------
# whole-chromosome file sets (BASELINE.json config 4: ~200 LD blocks x ~500 SNPs x 20 traits)
# ---------------------------------------------------------------------------
def chromosome_block_sizes(nblocks: int, seed: int = 0, mean: int = 500, lo: int = 100, hi: int = 2000, quantum: int = 100):
    """Unequal LD-block sizes (multiples of the LD window): log-normal around `mean`, clipped to [lo, hi].  Block b's
    size depends on (seed, b) only, so a job with more ranks extends the same chromosome."""
    out = []
    for b in range(nblocks):
        r = np.random.Generator(np.random.PCG64(BASE_SEED + 7919 * (seed + 1) + b))
        s = mean * float(np.exp(r.normal(-0.1, 0.6)))
        out.append(int(min(hi, max(lo, quantum * round(s / quantum)))))
    return out


def chromosome_segment(sizes, seg_first: int, seg_last: int, N: int, p: int, seed: int = 0, **kw):
    """Genotypes of blocks seg_first..seg_last-1 of the chromosome `sizes` (own RNG stream per block) and their
    genetic contribution to the p traits: (G int8 [m_seg, N], contrib float64 [p, N]).  Each trait gets
    5 causal SNPs per 1,000 with |beta| ~ U(0.02, 0.08) as in make_traits."""
    Gs, contrib = [], np.zeros((p, N), np.float64)
    for b in range(seg_first, seg_last):
        rng = np.random.Generator(np.random.PCG64(BASE_SEED + 104729 * (seed + 1) + b))
        G = make_genotypes(sizes[b], N, rng, **kw)
        g = G.astype(np.float32)
        g[G < 0] = np.nan
        mu = np.nanmean(g, axis=1, keepdims=True)
        sd = np.nanstd(g, axis=1, keepdims=True)
        sd[sd == 0] = 1.0
        ncausal_f = 5.0 * sizes[b] / 1000.0
        for k in range(p):
            nc = int(ncausal_f) + (1 if rng.random() < ncausal_f - int(ncausal_f) else 0)
            if nc == 0:
                continue
            idx = rng.choice(sizes[b], size=nc, replace=False)
            beta = rng.uniform(0.02, 0.08, size=nc) * rng.choice([-1.0, 1.0], size=nc)
            contrib[k] += beta @ np.nan_to_num((g[idx] - mu[idx]) / sd[idx]).astype(np.float64)
        Gs.append(G)
    return np.concatenate(Gs, axis=0), contrib


def chromosome_traits(contrib: np.ndarray, seed: int = 0) -> np.ndarray:
    """p x N float32 standardised traits from the summed genetic contributions: lower-triangular trait DAG
    (edge probability 3/p, |b| ~ U(0.05, 0.2)) + unit noise, as make_traits."""
    p, N = contrib.shape
    rng = np.random.Generator(np.random.PCG64(BASE_SEED + 15485863 * (seed + 1)))
    Y = np.zeros((p, N), np.float64)
    for k in range(p):
        y = contrib[k].copy()
        for k2 in range(k):
            if rng.random() < 3.0 / p:
                y = y + rng.uniform(0.05, 0.2) * rng.choice([-1.0, 1.0]) * Y[k2]
        y = y + rng.standard_normal(N)
        Y[k] = (y - y.mean()) / y.std()
    return Y.astype(np.float32)


def write_blocks_file(path: str, sizes, chr_id: str = "1") -> None:
    first = 0
    with open(path, "w") as f:
        for s in sizes:
            f.write(f"{chr_id}\t{first}\t{first + s - 1}\n")
            first += s


def write_phen_fast(path: str, Y: np.ndarray) -> None:
    """same format as write_phen (header + `FID IID v1..vp` rows), %.9g values, written in one go"""
    p, N = Y.shape
    cols = Y.T.astype(np.float64)
    with open(path, "w") as f:
        f.write("FID IID " + " ".join(f"T{k}" for k in range(p)) + "\n")
        f.write("".join(f"f{i} i{i} " + " ".join("NA" if np.isnan(v) else "%.9g" % v for v in cols[i]) + "\n" for i in range(N)))


def rand_dag_corr(snp: int = 500, tr: int = 5, nl: int = 2, n: int = 16000, deg: float = 3.0, prob_pleio: float = 0.2,
                  lo_mp: float = 0.001, hi_mp: float = 0.05, lo_pp: float = 0.001, hi_pp: float = 0.2, seed: int = 1,
                  return_dag: bool = False):
    """BASELINE config 1: the simulated correlation matrix of the reference's random-DAG simulator, restated in NumPy
    (/root/reference/simulation/simulate_dag.R:3-98 `gen_rand_dag`, parameters :106-115 with SNP = 500, Tr = 5; own RNG
    stream -- PCG64(BASE_SEED + seed) -- so not draw-for-draw identical to R's).

    Variables in generation order: `snp` markers, `nl` latent confounders, `tr` traits (pq = snp + nl + tr).  Edges
    only point forward in that order (:22-28 marker -> any later variable with probability deg / snp; :42-48 latent or
    trait -> any later variable with probability min(deg / tr, 1)); a marker with exactly one trait child gets
    pleiotropic edges to the other traits with probability prob_pleio each (:30-40: the whole draw replaces the other
    entries, and only when it is not all zero).  Effects (:54-78): marker -> marker and latent / trait -> anything
    U(lo_pp, hi_pp), marker -> latent / trait U(lo_mp, hi_mp), random sign.  Data (:80-91): a root is N(0, 1), a child
    is its parents' linear combination g plus N(0, 1 - var(g)) noise (sample variance, n - 1 denominator as R's var).
    Returns the (snp + tr) x (snp + tr) fp32 sample correlation of markers and traits (latents dropped, :120-127:
    `cor(dag_data_mat)`), markers first -- the variable order of every n x n object on the path; with return_dag also
    the 0/1 DAG and the effect matrix over all pq variables."""
    rng = np.random.Generator(np.random.PCG64(BASE_SEED + 7919 * int(seed)))
    pq = snp + nl + tr
    t0 = snp + nl  # first trait
    prob1 = deg / snp
    prob2 = min(deg / tr, 1.0)
    G = np.zeros((pq, pq), np.int8)
    for i in range(snp):
        G[i, i + 1:] = rng.random(pq - i - 1) < prob1
    for i in range(snp):
        iv = np.flatnonzero(G[i, t0:] == 1)
        if iv.size == 1 and tr > 1:
            draw = (rng.random(tr - 1) < prob_pleio).astype(np.int8)
            if draw.any():
                others = np.delete(np.arange(tr), iv[0])
                G[i, t0 + others] = draw
    for j in range(snp, pq):
        G[j, j + 1:] = rng.random(pq - j - 1) < prob2

    def effects(k, lo, hi):
        return rng.uniform(lo, hi, k) * np.where(rng.standard_normal(k) < 0, -1.0, 1.0)

    A = np.zeros((pq, pq), np.float64)
    for i in range(snp):
        d = np.flatnonzero(G[i, :snp])
        A[i, d] = effects(d.size, lo_pp, hi_pp)
        d = snp + np.flatnonzero(G[i, snp:])
        A[i, d] = effects(d.size, lo_mp, hi_mp)
    for i in range(snp, pq):
        d = np.flatnonzero(G[i])
        A[i, d] = effects(d.size, lo_pp, hi_pp)
    X = np.empty((pq, n), np.float64)
    for i in range(pq):
        anc = np.flatnonzero(G[:, i])
        if anc.size == 0:
            X[i] = rng.standard_normal(n)
        else:
            g = A[anc, i] @ X[anc]
            X[i] = g + rng.standard_normal(n) * np.sqrt(max(1.0 - g.var(ddof=1), 0.0))
    keep = np.concatenate([np.arange(snp), np.arange(t0, pq)])
    Cm = np.corrcoef(X[keep]).astype(np.float32)
    Cm = np.triu(Cm, 1)
    Cm = Cm + Cm.T
    np.fill_diagonal(Cm, 1.0)
    Cm = np.ascontiguousarray(Cm, np.float32)
    if return_dag:
        return Cm, G, A
    return Cm


# ---------------------------------------------------------------- inputs that steer the level sweep's dispatch
# Ranks of conditioning sets at the work-item boundaries of the sweep kernels: k * 64 - 1, k * 64, k * 64 + 1 for the
# small items (chunk0 = chunk0_low = 64), and the same around 256, 512 and 2048 (chunk = 256 and the default items).
DISPATCH_RANKS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049)


def comb_rank(pos, d: int) -> int:
    """0-based lexicographic rank of the ascending positions `pos` among the l-subsets of range(d): the order in which
    the level sweep enumerates the conditioning sets of a row with d neighbours (rank r is the reference's r + 1)."""
    from math import comb

    l, r, prev = len(pos), 0, -1
    for i, p in enumerate(pos):
        for v in range(prev + 1, p):
            r += comb(d - 1 - v, l - 1 - i)
        prev = p
    return r


def comb_unrank(r: int, d: int, l: int) -> list:
    """inverse of comb_rank"""
    from math import comb

    out, v = [], 0
    for i in range(l):
        while r >= comb(d - 1 - v, l - 1 - i):
            r -= comb(d - 1 - v, l - 1 - i)
            v += 1
        out.append(v)
        v += 1
    return out


def _partial_z(A: np.ndarray, x: int, y: int, S) -> float:
    """|atanh| of the partial correlation of x and y given S, in float64, for variables that are rows of A over
    independent unit innovations (covariance A A^T)"""
    idx = [x, y] + list(S)
    M = A[idx] @ A[idx].T
    P = np.linalg.inv(M)
    return abs(float(np.arctanh(-P[0, 1] / np.sqrt(P[0, 0] * P[1, 1]))))


def _bisect(f, lo: float, hi: float, target: float, it: int = 60) -> float:
    """f increasing on [lo, hi]: the argument where f crosses target"""
    for _ in range(it):
        mid = 0.5 * (lo + hi)
        if f(mid) < target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def dispatch_case(degrees, level: int, seed: int, N: int = 2_000_000, alpha: float = 1e-4, ranks=DISPATCH_RANKS,
                  max_twins: int = 2):
    """Population correlation matrix (float32) of independent hub blocks that reach level `level` with one hub row of
    each degree in `degrees`, and what the sweep of that level must find.

    A hub H is a signed combination of its "sources" (independent variables) plus noise; its neighbour list at level l
    is positions 0..d-1 in variable order.  "Hangers" V = sum_{t in T} sign(w_t) X_t + 5 e sit at free positions of that
    list: V stays adjacent to H below level |T| = l and is separated from it by T exactly, which sits at rank r of H's
    list.  Every target rank in `ranks` below C(d, l) gets one hanger.  Up to `max_twins` of them get a second passing
    set in a later work item: one member t of T gets a near copy X_p = X_t + sigma e at a free position p whose set
    T - t + p has a rank in a later 64-set item; sigma is tuned so that set's z is about th / 2.  Two more hangers per
    hub carry a weak extra path gamma X_c whose z given T is tuned to th (1 -+ 2.5e-4): inside the guard band of the
    fast filters (+-1e-3 relative on |rho|), one just passing and one just failing.  One hanger per level below l
    (random sources) thins the hub's list on the way.

    Returns (Cm, info): info["hubs"] is a list with, per hub, its index "h", degree "d", the variable index of every
    list position "pos" (ascending), "targets" (variable index of V, rank, T as variable indices), "twins" (V, rank of
    the second set, that set), "near" (V, T, passes), and info["th"] is the level's Fisher-z threshold."""
    from math import comb
    from statistics import NormalDist

    rng = np.random.default_rng(seed)
    th = NormalDist().inv_cdf(1.0 - alpha / 2.0) / np.sqrt(N - level - 3.0)
    l = level
    blocks = []  # per hub: the roles of its list positions
    for d in degrees:
        targets = [(r, comb_unrank(r, d, l)) for r in ranks if r < comb(d, l)]
        while True:  # small rows: as many targets as leave room for their hangers (and the near copies)
            used = set()
            for _, T in targets:
                used.update(T)
            if len(used) + len(targets) + max_twins + 2 * (l + 2) <= d:
                break
            targets.pop()
        # near copies: replace the largest member of T whose replacement whose replacement by a free position lands in a later 64-set item
        twins = []
        for r, T in targets:
            if len(twins) >= max_twins:
                break
            best = None
            for t in sorted(T, reverse=True):
                for p in range(t + 1, d):
                    if p in used or any(p == q for _, _, q in twins):
                        continue
                    T2 = sorted([v for v in T if v != t] + [p])
                    r2 = comb_rank(T2, d)
                    if r2 // 64 > r // 64:
                        best = (r, t, p)
                        break
                if best:
                    break
            if best:
                twins.append(best)
                used.add(best[2])
        free = [p for p in range(d) if p not in used]
        rng.shuffle(free)
        near = []
        for passes in (True, False):
            if len(free) < l + 1 + len(targets) + 3:
                break
            T = sorted(free[:l])
            c = free[l]
            free = free[l + 1:]
            near.append((T, c, passes))
        nhang = len(targets) + len(near)
        if len(free) < nhang:
            raise ValueError(f"degree {d} at level {l}: {nhang} hangers but {len(free)} free positions")
        hang_pos = sorted(free[:nhang])
        sources = [p for p in range(d) if p not in set(hang_pos)]
        lower = []
        plain = [p for p in sources if p not in used and p not in {q for T, c, _ in near for q in T + [c]}]
        for l2 in range(1, l if len(plain) >= l else 1):
            lower.append(sorted(rng.choice(plain, l2, replace=False).tolist()))
        blocks.append(dict(d=d, targets=targets, twins=twins, near=near, hang_pos=hang_pos, sources=sources, lower=lower))

    n = sum(b["d"] + len(b["lower"]) + 1 for b in blocks)
    A = np.zeros((n, n))
    hubs = []
    base = 0
    for b in blocks:
        d = b["d"]
        H = base + d + len(b["lower"])
        idx = lambda p: base + p  # noqa: E731
        twin_of = {p: t for _, t, p in b["twins"]}
        for p in b["sources"]:
            A[idx(p), idx(p)] = 1.0
        for p, t in twin_of.items():
            A[idx(p), idx(t)] = 1.0
            A[idx(p), idx(p)] = 0.1  # sigma, tuned below
        w = rng.uniform(0.8, 1.2, d) * rng.choice([-1.0, 1.0], d)
        for p, t in twin_of.items():  # H - X_t | X_p ~ w_t sigma / sd(H) keeps both copies in H's list
            w[p] = w[t]

        def set_hub():
            A[H] = 0.0
            for p in b["sources"]:
                A[H] += w[p] * A[idx(p)]
            A[H, H] += 1.0

        set_hub()
        hang = iter(b["hang_pos"])
        info = dict(h=H, d=d, pos=[idx(p) for p in range(d)], targets=[], twins=[], near=[])

        def add_hanger(v, T):
            A[v] = 0.0
            for t in T:
                A[v] += np.sign(w[t]) * A[idx(t)]  # (signs of H's: no path cancels another)
            A[v, v] += 5.0  # a noisy proxy of its sources: conditioning on hangers attenuates H - X_t, never cancels it

        vt = {}
        for r, T in b["targets"]:
            v = idx(next(hang))
            add_hanger(v, T)
            vt[r] = v
            info["targets"].append((v, r, [idx(t) for t in T]))
        near_pos = [idx(next(hang)) for _ in b["near"]]  # (the hub's row is final once the near copies are tuned)
        for r, t, p in b["twins"]:
            v = vt[r]
            T2 = sorted([q for q in comb_unrank(r, d, l) if q != t] + [p])

            def z_of(sigma):
                A[idx(p), idx(p)] = sigma
                set_hub()
                return _partial_z(A, H, v, [idx(q) for q in T2])

            z_of(_bisect(z_of, 1e-3, 1.0, 0.5 * th))
            info["twins"].append((v, comb_rank(T2, d), [idx(q) for q in T2]))
        for T, c, passes in b["near"]:
            v = near_pos.pop(0)
            add_hanger(v, T)
            row = A[v].copy()
            g = np.sign(w[c])

            def z_of(gamma):
                A[v] = row + gamma * g * A[idx(c)]
                return _partial_z(A, H, v, [idx(t) for t in T])

            gamma = _bisect(z_of, 0.0, 4.0, th * (1.0 - 2.5e-4 if passes else 1.0 + 2.5e-4))
            z_of(gamma)
            info["near"].append((v, [idx(t) for t in T], passes))
        for k, T in enumerate(b["lower"]):
            add_hanger(base + d + k, T)
        hubs.append(info)
        base = H + 1
    S = A @ A.T
    s = np.sqrt(np.diag(S))
    Cm = S / np.outer(s, s)
    Cm = (Cm + Cm.T) / 2
    np.fill_diagonal(Cm, 1.0)
    return np.ascontiguousarray(Cm, np.float32), dict(hubs=hubs, th=float(th), level=l, N=N, alpha=alpha)


# (level, hub degrees at the start of that level): every degree class, each class boundary (39/40, 63/64, 127/128,
# 191/192) at level 2, class 3 at level 3, class 2 at level 4, class 1 at level 5; the oracle's cost per hub row is
# about C(d, l) (d - l) tests
DISPATCH_CASES = {
    "l2": (2, (39, 40, 63, 64, 127, 128, 191, 192)),
    "l3": (3, (39, 40, 63, 64, 127, 128)),
    "l4": (4, (39, 40, 63, 64)),
    "l5": (5, (39, 40, 41)),
}


def level1_star_case(n: int = 1301, hub: int = 3, seed: int = 1, N: int = 4096, alpha: float = 1e-4, pairs: int = 256):
    """Population correlation matrix (float32) of a star for the level-1 row kernel: one hub row with n - 1 neighbours
    at the start of level 1 (more than two staging rounds of a 512-thread workgroup), child rows of every degree up to
    about 0.6 n, and a level 1 that removes most of what level 0 left.

    One factor: C[hub, c_k] = rho_k and C[c_j, c_k] = rho_j rho_k, so the hub separates every pair of children exactly.
    rho_k runs from 0.5 down to 0.08 (denser at the low end, shuffled over the indices), so rho_j rho_k straddles
    tanh(Th[0]) and level 0 keeps the child-child edges with the larger products.  `pairs` disjoint pairs of children
    with rho >= 0.2 get a partial correlation e in [0.15, 0.3] given the hub on top (C += e sqrt((1 - rho_j^2)
    (1 - rho_k^2))): those edges survive level 1.  n is not a multiple of 4 (the 16-byte row staging clamps its last
    piece).  Returns (Cm, info) with info["hub"], "N", "alpha", "rho" and the perturbed "pairs"."""
    rng = np.random.default_rng(seed)
    kids = np.array([v for v in range(n) if v != hub])
    rho = np.zeros(n)
    rho[kids] = rng.permutation(0.08 + 0.42 * np.linspace(0.0, 1.0, n - 1) ** 2.5)
    rho[hub] = 1.0
    Cm = np.outer(rho, rho)
    strong = rng.permutation(kids[rho[kids] >= 0.2])[: 2 * pairs].reshape(-1, 2)
    e = rng.uniform(0.15, 0.3, len(strong))
    for (j, k), ee in zip(strong, e):
        Cm[j, k] = Cm[k, j] = rho[j] * rho[k] + ee * np.sqrt((1 - rho[j] ** 2) * (1 - rho[k] ** 2))
    np.fill_diagonal(Cm, 1.0)
    info = {"hub": hub, "N": N, "alpha": alpha, "rho": rho, "pairs": [(int(j), int(k)) for j, k in strong]}
    return np.ascontiguousarray(Cm.astype(np.float32)), info


# ---------------------------------------------------------------- per-pair sample sizes and removals at depth
def het_sizes(n: int, seed: int, N0: float, lo: float = 0.5, symmetric: bool = True) -> np.ndarray:
    """n x n float32 sample sizes floor(U(lo, 1) N0), one draw per ORDERED pair (default_rng(seed)).  symmetric: the
    element-wise minimum with the transpose (a pair is observed on the individuals both orders share); otherwise the raw
    draw, N[i, j] != N[j, i] almost everywhere -- no estimator produces that, it pins which of the two elements a kernel
    reads.  The diagonal is part of the draw and is never read by a sweep."""
    rng = np.random.default_rng(seed)
    Nm = np.floor(rng.uniform(lo, 1.0, (n, n)) * float(N0))
    if symmetric:
        Nm = np.minimum(Nm, Nm.T)
    return np.ascontiguousarray(Nm, np.float32)


def deep_removal_case(levels=range(5, 15), seed: int = 0, N: int = 20000, extras: int = 2, extra_weight: float = 0.3,
                      weak: float = 2.77, return_info: bool = False):
    """Float32 sample correlation matrix (N individuals) with removals at every level in `levels`: for each k one group
    of independent variables [w_1..w_extras, p_1..p_k] and three children

        x  = s + extra_weight (w_1 + .. + w_extras) + e_x        s = (p_1 + .. + p_k) / sqrt(k)
        y  = s + e_y
        y' = s + g e_x + e_y'

    Groups share nothing.  x, y and y' are pairwise dependent given any proper subset of the parents (one parent left out
    keeps a partial correlation of about 1 / (k + 1), z sqrt(N) of 9 and more at N = 20000), so the edges x - y, x - y',
    y - y' survive to level k and only the set of all k parents separates them there.  The children's noise is as large
    as the parents' sum: y and y' are then weak proxies of it, and a parent stays dependent on x given both (with unit
    noise against a sum of variance 14 the two proxies explain a single parent away at level 2).  The w's stay neighbours of x (real edges) and come before the parents in
    x's list, so the parents are not the first set of x's row: the winning rank is above 0.  g is chosen so that the
    population z of (x, y' | parents) is weak / sqrt(N): with weak = 2.77 between the cut-off of alpha = 0.01 at N
    (2.58 / sqrt(N)) and at the 0.75 N that `het_sizes` averages to over the pairs of a deep test (2.97 / sqrt(N));
    sampling noise (sd 1 / sqrt(N)) decides per seed and level on which side the estimate falls.  The largest row,
    x of k = 14, has 14 + 2 + extras neighbours.
    Returns Cm, with return_info also {k: dict(x, y, y2, parents, extras)} (variable indices)."""
    rng = np.random.default_rng(seed)
    levels = [int(k) for k in levels]
    n = sum(k + extras + 3 for k in levels)
    X = np.empty((n, N), np.float64)
    info, base = {}, 0
    vx = 1.0 + extras * extra_weight ** 2  # variance of x given its parents
    rho = weak / np.sqrt(N)
    g = rho * np.sqrt(vx) / np.sqrt(max(1.0 - rho * rho * vx, 1e-12))  # g / sqrt(vx (g^2 + 1)) = rho
    for k in levels:
        w = np.arange(base, base + extras)
        p = np.arange(base + extras, base + extras + k)
        x, y, y2 = base + extras + k, base + extras + k + 1, base + extras + k + 2
        X[base:x] = rng.standard_normal((extras + k, N))
        s = X[p].sum(0) / np.sqrt(k)
        ex = rng.standard_normal(N)
        X[x] = s + extra_weight * X[w].sum(0) + ex
        X[y] = s + rng.standard_normal(N)
        X[y2] = s + g * ex + rng.standard_normal(N)
        info[k] = dict(x=int(x), y=int(y), y2=int(y2), parents=[int(v) for v in p], extras=[int(v) for v in w])
        base = y2 + 1
    Cm = np.corrcoef(X).astype(np.float32)
    Cm = np.triu(Cm, 1)
    Cm = Cm + Cm.T
    np.fill_diagonal(Cm, 1.0)
    Cm = np.ascontiguousarray(Cm, np.float32)
    return (Cm, info) if return_info else Cm


# ---------------------------------------------------------------- level-1 tests placed at the decision boundary
# (name, N, alpha) of level1_band_thresholds(); the two sizes around kThMinFilter are derived, not written down
LEVEL1_BAND_GRID = (0.05, 0.3, 0.5, 0.9, 0.999)
LEVEL1_BAND_ULPS = (-4096, -256, -16, -2, -1, 0, 1, 2, 16, 256, 4096)
LEVEL1_BAND_BETAS = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
LEVEL1_BAND_SETS = 40
# planted triples that need no flip: name -> (a = C[X,S], b = C[Y,S], c = C[X,Y], private leaf on X in the hub layout).
# "1+" is the float behind 1 (a correlation that rounding pushed past 1: 1 - v v < 0); "ab" / "cb" is the float product
# of the two other entries, which makes h01 exactly 0: the squared form then sees lhs = 0 > t2 (h00 hc) (1 + beta) with
# h00 < 0 ("certainly dependent") where the exact form gets rho = 0 and removes the edge.
LEVEL1_BAND_DEGENERATE = {
    "a=+1": (1.0, 0.5, 0.45, False), "a=-1": (-1.0, 0.5, 0.45, False),
    "a=b=+1": (1.0, 1.0, 0.5, False), "a=b=-1": (-1.0, -1.0, 0.5, False),
    "hc<0": (0.6, 0.5, "1+", False),
    "nan:a": (np.nan, 0.5, 0.45, False), "nan:b": (0.6, np.nan, 0.45, False), "nan:c": (0.6, 0.5, np.nan, False),
    "c=+1": (0.6, 0.5, 1.0, False), "c=-1": (0.6, 0.5, -1.0, False),
    "h00<0:a": ("1+", 0.5, "ab", False), "h00<0:a,leaf": ("1+", 0.5, "ab", True),
    "h00<0:c": ("cb", 0.5, "1+", False), "h00<0:c,leaf": ("cb", 0.5, "1+", True),
}


def _csrc_constant(header: str, name: str) -> float:
    """a `constexpr float name = <expression of float literals>;` of csrc/<header>"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", header)).read()
    expr = re.search(r"constexpr\s+float\s+" + name + r"\s*=\s*([^;]+);", src).group(1)
    return float(eval(re.sub(r"(?<=[0-9.])f\b", "", expr), {"__builtins__": {}}, {}))


def _f32_ord(x) -> int:
    """float32 -> integer whose order is the order of the floats (adjacent floats differ by 1)"""
    i = int(np.float32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _f32_from_ord(k: int) -> np.float32:
    return np.int32(k).view(np.float32) if k >= 0 else np.float32(-(np.int32(-k).view(np.float32)))


def level1_beta(t2) -> float:
    """level1_beta of csrc/level1.hip for t2 = (float) tanh(th)^2, capped at kBeta of ci_fast.h.  It only places
    inputs here."""
    t = np.sqrt(max(float(np.float32(t2)), 1e-30))
    return float(np.float32(min(_csrc_constant("ci_fast.h", "kBeta"), 16.0 * (2.0 * (2.4e-7 + 5.6e-8 / t) + 3.0e-7))))


def level1_band_thresholds(alpha: float = 1e-4) -> dict:
    """name -> (N, alpha) of the level-1 band cases.  `above_min` / `below_min`: the largest N whose Th[1] is still
    >= kThMinFilter (the filter runs) and the next one (everything on the exact form), found on oracle.threshold_array."""
    from oracle import oracle as O

    th_min = np.float32(_csrc_constant("sweep_common.h", "kThMinFilter"))
    lo, hi = 1000, 1 << 30  # Th[1] >= th_min at lo, < th_min at hi
    assert O.threshold_array(lo, alpha)[1] >= th_min > O.threshold_array(hi, alpha)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if O.threshold_array(mid, alpha)[1] >= th_min:
            lo = mid
        else:
            hi = mid
    return {"n60": (60, 1e-2), "headline": (16384, alpha), "biobank": (500000, alpha), "above_min": (lo, alpha),
            "below_min": (hi, alpha)}


def _het_lth(th, sizes):
    """ess_threshold_exact<1>: float sum of the int-truncated sizes (NaN -> 0) in the order (N[Y,X] + N[S,X]) + N[S,Y],
    float division by 3, double square root and division, rounded to float"""
    s = np.float32(0.0)
    for v in sizes:
        s = np.float32(s + np.float32(0.0 if np.isnan(v) else int(v)))
    me = np.float32(s / np.float32(3.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(np.float32(th)) / np.sqrt(np.float64(me) - 4.0))


def _het_size_classes(th, N0):
    """[(name, (N[X,Y], N[X,S], N[Y,S]))]: sums of three sizes on both sides of kHetUMin, kHetUMax (u = th^2 / (me - 4))
    and kHetDMin (me - 4), two adjacent sums on each side, in the float32 steps of the row kernel; N0 everywhere; one
    class each with a NaN, a zero and a negative size"""
    F = np.float32
    th2 = F(np.float64(F(th)) ** 2)
    umin, umax, dmin = (F(_csrc_constant("level1.hip", k)) for k in ("kHetUMin", "kHetUMax", "kHetDMin"))

    def dm_u(s):
        dm = F(F(F(s) * F(0.33333334)) - F(4.0))
        return dm, F(th2 * F(F(1.0) / dm))

    def first(pred, guess):
        """smallest integer sum at which pred holds (pred is monotone around guess)"""
        s = int(guess) - 64
        assert not pred(s)
        while not pred(s):
            s += 1
        return s

    s_umin = first(lambda s: not dm_u(s)[1] >= umin, 3.0 * (float(th2) / float(umin) + 4.0))
    s_umax = first(lambda s: dm_u(s)[1] <= umax, 3.0 * (float(th2) / float(umax) + 4.0))
    s_dmin = first(lambda s: dm_u(s)[0] >= dmin, 3.0 * (float(dmin) + 4.0))
    out = []
    for name, s0 in (("umin", s_umin), ("umax", s_umax), ("dmin", s_dmin)):
        for j in (-2, -1, 0, 1):
            s = s0 + j
            n1 = s // 3
            n2 = (s - n1) // 2
            out.append((f"{name}{j:+d}", (float(n1), float(n2), float(s - n1 - n2))))
    out.append(("N0", (float(N0),) * 3))
    out += [("nan", (np.nan, float(N0), float(N0))), ("zero", (float(N0), 0.0, float(N0))), ("negative", (float(N0), float(N0), -5.0))]
    return out


def level1_band_case(layout: str, N: int, alpha: float, mode: str = "skeleton", seed: int = 0):
    """Symmetric float32 matrix (not positive definite: engine and oracle take any) of triples (X, Y, S) whose level-1 test
    (X; Y | S) sits at the decision boundary, and what was placed where.

    A parameter set is (a = C[X,S], b = C[Y,S], sign of rho): |a|, |b| from LEVEL1_BAND_GRID with a != b, every sign
    pattern in turn, topped up with seeded random draws to LEVEL1_BAND_SETS sets.  A set is used only where the premises
    can hold at the case's threshold t = tanh(Th[1]): |a|, |b|, |c| clear of the level-0 cut, the other tests of the triple
    ((X; S | Y), (Y; S | X)) and, with a shared S, the tests of S given another triple's variable (rho = v / sqrt(1 - w^2))
    at least 5 % off t^2 and 1 / t^2 in rho^2 (a |rho| > 1 of this indefinite matrix reads as 1 / |rho|).  The flip point c
    of C[X,Y] is found by bisection over float32 bit patterns on the ORACLE's verdict for the 3 x 3 matrix (`mode`:
    oracle.skeleton, oracle.hetcor_skeleton at one size, or at the triple's own three sizes for "het"): the edge X - Y
    is removed at the float next to c on the side of a b and kept at c (for rho > 0 the smallest float at which it is kept,
    for rho < 0 the largest).  Every set is instantiated, as triples of their own, at c + j ulp (LEVEL1_BAND_ULPS) and at
    the values that move rho^2 by LEVEL1_BAND_BETAS x beta relative to c, beta = level1_beta at the set's threshold.
    LEVEL1_BAND_DEGENERATE lists the planted triples that need no flip.

    layout "cliques": disjoint 3-cliques on the diagonal (roles permuted over the three indices), everything else 0.
    layout "hub": one S for all triples (degree 2 per triple plus fillers: more than two staging rounds of 512), a few
    fillers before S, then the triples in seeded order with X / Y in either order, fillers (adjacent to S only, |f| in
    [0.4, 0.7]) strewn between, and for every third triple a private leaf (adjacent to the first of X / Y only, +-0.5)
    between the two, so that the triple's second variable is the SECOND position of a lane's pair in the row kernel.
    n is not a multiple of 4.

    mode "het": per-pair sample sizes.  The sets are dealt over _het_size_classes (two per class, the rest at N0); the
    returned size matrix is bitwise symmetric with N0 outside the triples.

    Returns (Cm, info) or, for "het", (Cm, Nm, info).  info: "Th" (skeleton) / "th", "N", "alpha", "t", "beta", "sets"
    (a, b, s, c, sizes, cls, t, beta), "entries" (set or None, label, degenerate or None, X, Y, S, a, b, c, sizes, leaf),
    "hub", "fillers", "leaves"."""
    from oracle import oracle as O

    assert layout in ("cliques", "hub") and mode in ("skeleton", "hetcor", "het")
    F = np.float32
    rng = np.random.default_rng(BASE_SEED + 977 * seed + (0 if mode != "het" else 1))
    Th = O.threshold_array(N, alpha)
    th = O.hetcor_threshold(alpha)
    ones3, ti3 = np.ones((3, 3), np.int32), np.zeros(3, np.int32)

    def kept(a, b, c, sizes):
        C3 = np.array([[1, c, a], [c, 1, b], [a, b, 1]], F)
        if mode == "skeleton":
            return O.skeleton(C3, Th, 1).G[0, 1] == 1
        nxy, nxs, nys = sizes
        N3 = np.array([[np.nan, nxy, nxs], [nxy, np.nan, nys], [nxs, nys, np.nan]], F)
        return O.hetcor_skeleton(C3, ones3, N3, th, 1, ti3).G[0, 1] == 1

    def cuts(sizes):
        """(t of the level-1 tests of the triple, level-0 cuts of X-Y, X-S, Y-S) in float64"""
        if mode == "skeleton":
            return float(np.tanh(np.float64(Th[1]))), (float(np.tanh(np.float64(Th[0]))),) * 3
        with np.errstate(invalid="ignore", divide="ignore"):
            t0 = np.tanh(np.float64(F(th)) / np.sqrt(np.array(sizes, np.float64) - 3.0))
        return float(np.tanh(np.float64(_het_lth(th, sizes)))), tuple(0.0 if np.isnan(v) else float(v) for v in t0)

    M = 0.05

    def feasible(a, b, s, sizes):
        t, (t0xy, t0xs, t0ys) = cuts(sizes)
        a, b = float(F(a)), float(F(b))
        vmax = 1.0 / np.sqrt(1.0 + t * t * (1.0 + M))
        if mode == "het":  # a test of S given another triple's variable mixes the sizes of two classes: t up to 0.052
            vmax = min(vmax, 0.95)
        if not (t0xs * 1.02 <= abs(a) <= vmax and t0ys * 1.02 <= abs(b) <= vmax):
            return False
        c = a * b + s * t * np.sqrt((1 - a * a) * (1 - b * b))
        if not (max(t0xy, t * 0.9) * 1.02 <= abs(c) <= 0.98):
            return False
        for v, w in ((a, b), (b, a)):  # (X; S | Y) and (Y; S | X)
            r2 = (v - c * w) ** 2 / ((1 - c * c) * (1 - w * w))
            if not (t * t * (1 + M) <= r2 <= 1.0 / (t * t * (1 + M))):
                return False
        return True

    classes = _het_size_classes(th, N) if mode == "het" else [("N", (float(N),) * 3)]
    combos = [(sa, sb, s) for sa in (1, -1) for sb in (1, -1) for s in (1, -1)]
    cand = []
    for i, (va, vb) in enumerate((va, vb) for va in LEVEL1_BAND_GRID for vb in LEVEL1_BAND_GRID if va != vb):
        for j in range(8):
            sa, sb, s = combos[(3 * i + j) % 8]
            cand.append((sa * va, sb * vb, s))
    cand = [cand[k] for i in range(8) for k in range(i, len(cand), 8)]  # every magnitude pair before its next sign pattern
    # how many sets each class gets
    if mode == "het":
        quota = [2 if name != "N0" else 0 for name, _ in classes]
        quota[[name for name, _ in classes].index("N0")] = LEVEL1_BAND_SETS - sum(quota)
    else:
        quota = [LEVEL1_BAND_SETS]
    sets, used = [], set()
    for ci, ((cname, sizes), q) in enumerate(zip(classes, quota)):
        got = 0
        grid_share = q if mode == "het" else (3 * q) // 4  # the rest are random draws
        for k in range(len(cand)):
            kk = (k + 7 * ci) % len(cand)
            if got >= grid_share:
                break
            if kk in used or not feasible(*cand[kk], sizes):
                continue
            used.add(kk)
            sets.append(dict(a=F(cand[kk][0]), b=F(cand[kk][1]), s=cand[kk][2], sizes=sizes, cls=cname))
            got += 1
        t, t0 = cuts(sizes)
        tries = 0
        while got < q:
            tries += 1
            if tries > 20000:
                raise ValueError(f"level1_band_case: no feasible parameter set for size class {cname}")
            lo = max(1.1 * max(t0[1], t0[2], t), 0.02)
            a, b = (rng.uniform(min(lo, 0.95), 0.95, 2) * rng.choice([-1.0, 1.0], 2)).tolist()
            s = int(rng.choice([-1, 1]))
            if F(a) != F(b) and feasible(a, b, s, sizes):
                sets.append(dict(a=F(a), b=F(b), s=s, sizes=sizes, cls=cname))
                got += 1

    entries = []
    for si, p in enumerate(sets):
        a, b, s, sizes = p["a"], p["b"], p["s"], p["sizes"]
        t, _ = cuts(sizes)
        beta = level1_beta(F(t * t))
        ab = float(a) * float(b)
        D = np.sqrt((1 - float(a) ** 2) * (1 - float(b) ** 2))
        # (a far end just past the flip: farther out C[X,Y] can fall below the level-0 cut when a b and rho differ in sign)
        lo, hi = s * _f32_ord(F(ab)), s * _f32_ord(F(ab + s * 1.005 * t * D))
        f = lambda k: kept(a, b, _f32_from_ord(s * k), sizes)  # noqa: E731
        if not (lo < hi and not f(lo) and f(hi)):
            raise ValueError(f"level1_band_case: no flip for set {si} {p}")
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if f(mid):
                hi = mid
            else:
                lo = mid
        c = _f32_from_ord(s * hi)
        p.update(c=c, t=t, beta=beta)
        ladder = [(f"{j:+d}ulp", _f32_from_ord(_f32_ord(c) + j)) for j in LEVEL1_BAND_ULPS]
        ladder += [(f"{r:+g}beta", F(ab + (float(c) - ab) * np.sqrt(1.0 + r * beta))) for r in LEVEL1_BAND_BETAS]
        for label, cv in ladder:
            entries.append(dict(set=si, label=label, degenerate=None, a=a, b=b, c=F(cv), sizes=sizes, want_leaf=(len(entries) % 3 == 0)))
    onep = np.nextafter(F(1.0), F(2.0))
    for name, (a, b, c, leaf) in LEVEL1_BAND_DEGENERATE.items():
        b = F(b)
        a = onep if isinstance(a, str) and a == "1+" else a
        c = onep if isinstance(c, str) and c == "1+" else c
        if isinstance(c, str):  # "ab"
            c = F(F(a) * b)
        if isinstance(a, str):  # "cb"
            a = F(F(c) * b)
        entries.append(dict(set=None, label=name, degenerate=name, a=F(a), b=b, c=F(c), sizes=(float(N),) * 3, want_leaf=leaf))

    E = len(entries)
    fillers, leaves, hub = [], [], None
    if layout == "cliques":
        n = 3 * E
        n += 1 if n % 4 == 0 else 0
        perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
        for k, e in enumerate(entries):
            pm = perms[k % 6]
            e.update(X=3 * k + pm[0], Y=3 * k + pm[1], S=3 * k + pm[2], leaf=None)
        leaf_val = {}
    else:
        seq = [("F", -1)] * 6 + [("S", -1)]
        for k in rng.permutation(E):
            e = entries[k]
            if (e["degenerate"] or "").startswith("h00<0:a"):
                continue  # |C[X,S]| > 1 would separate everything from a shared S: these get an S of their own, below
            if rng.random() < 0.22:
                seq.append(("F", -1))
            first, second = ("X", "Y") if (rng.random() < 0.5 or e["degenerate"]) else ("Y", "X")
            seq.append((first, k))
            if e["want_leaf"]:
                seq.append(("L", k))
            if rng.random() < 0.10:
                seq.append(("F", -1))
            seq.append((second, k))
        for k, e in enumerate(entries):
            if (e["degenerate"] or "").startswith("h00<0:a"):
                seq += [("P", k), ("X", k)] + ([("L", k)] if e["want_leaf"] else []) + [("Y", k)]
        while len(seq) % 4 == 0 or len(seq) % 4 == 1:  # n = 2 or 3 mod 4
            seq.append(("F", -1))
        n = len(seq)
        for e in entries:
            e["leaf"] = None
        leaf_val = {}
        for idx, (kind, k) in enumerate(seq):
            if kind == "S":
                hub = idx
            elif kind == "F":
                fillers.append(idx)
            elif kind == "P":
                entries[k]["S"] = idx
            elif kind == "L":
                entries[k]["leaf"] = idx
                leaves.append(idx)
                leaf_val[idx] = F(0.5 * rng.choice([-1.0, 1.0]))
            else:
                entries[k][kind] = idx
        for e in entries:
            e.setdefault("S", hub)
            e["leaf_of"] = None if e["leaf"] is None else ("X" if e["X"] < e["Y"] else "Y")
    Cm = np.zeros((n, n), F)
    np.fill_diagonal(Cm, 1.0)
    Nm = np.full((n, n), F(N), F) if mode == "het" else None

    def put(M_, i, j, v):
        M_[i, j] = M_[j, i] = v

    for e in entries:
        X, Y, S = e["X"], e["Y"], e["S"]
        put(Cm, X, S, e["a"])
        put(Cm, Y, S, e["b"])
        put(Cm, X, Y, e["c"])
        if Nm is not None:
            put(Nm, X, Y, F(e["sizes"][0]))
            put(Nm, X, S, F(e["sizes"][1]))
            put(Nm, Y, S, F(e["sizes"][2]))
        if e.get("leaf") is not None:
            put(Cm, e["leaf"], e[e["leaf_of"]], leaf_val[e["leaf"]])
        e.pop("want_leaf")
    for f_ in fillers:
        put(Cm, f_, hub, F(rng.uniform(0.4, 0.7) * rng.choice([-1.0, 1.0])))
    t_all, _ = cuts((float(N),) * 3)
    info = dict(layout=layout, mode=mode, N=N, alpha=alpha, Th=Th, th=th, t=t_all, beta=level1_beta(F(t_all * t_all)), sets=sets,
                entries=entries, hub=hub, fillers=fillers, leaves=leaves, size_classes=classes)
    Cm = np.ascontiguousarray(Cm)
    return (Cm, np.ascontiguousarray(Nm), info) if mode == "het" else (Cm, info)
