"""Cases shared by test_ordinal_formats.py (CPU) and test_gpu_ordinal.py: the tables the polychoric fit is compared on, and
the planted-effect data set on which `--ordinal` decides an edge differently from plain `--het`."""
import numpy as np

import ordinal_ref64 as R


def _sampled_table(rng, ka, kb, n, rho, spread=1.2):
    """a table of n draws of a bivariate normal at rho, cut at random thresholds"""
    x = rng.standard_normal(n)
    y = rho * x + np.sqrt(1.0 - rho * rho) * rng.standard_normal(n)
    ca = np.sort(rng.uniform(-spread, spread, ka - 1))
    cb = np.sort(rng.uniform(-spread, spread, kb - 1))
    return R.pair_table(np.searchsorted(ca, x), np.searchsorted(cb, y), ka, kb)


def fit_cases():
    """(shape, table, random?) -- about 300 tables"""
    rng = np.random.Generator(np.random.PCG64(20261))
    cases = []
    for n in (50, 1000, 500000):
        for (ka, kb), count in (((3, 2), 20), ((3, 3), 20), ((3, 8), 20), ((2, 2), 20), ((8, 8), 8)):
            for _ in range(count):
                # fifty observations seldom fill the corners of a table at a strong correlation or a far threshold: those
                # tables are boundary cases, which have their own entries below
                lim, spread = (0.5, 0.6) if n == 50 else (0.9, 1.2)
                cases.append(((ka, kb), _sampled_table(rng, ka, kb, n, rng.uniform(-lim, lim), spread), True))
    for rho in (0.0, 1e-3, -1e-3, 0.99, -0.99, 0.985, -0.995):  # near 0 and near +-0.99
        cases.append(((3, 3), _sampled_table(rng, 3, 3, 200000, rho), False))
        cases.append(((2, 2), _sampled_table(rng, 2, 2, 200000, rho), False))
    cases.append(((3, 3), np.array([[40, 0, 3], [0, 25, 0], [2, 0, 30]]), False))  # zero cells
    cases.append(((3, 8), np.array([[5, 0, 0, 9, 0, 0, 0, 1], [0, 7, 0, 0, 0, 4, 0, 0], [1, 0, 0, 2, 0, 0, 0, 8]]), False))
    cases.append(((2, 2), np.array([[10, 20], [30, 0]]), False))
    cases.append(((3, 3), np.array([[10, 5, 1], [0, 0, 0], [2, 6, 9]]), False))  # an empty row in the middle: removed
    cases.append(((3, 3), np.array([[0, 0, 0], [10, 5, 1], [2, 6, 9]]), False))  # an empty first row
    for t in ([[5, 9, 2], [0, 0, 0], [0, 0, 0]], [[5, 0, 0], [7, 0, 0], [1, 0, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 0]]):
        cases.append(((3, 3), np.array(t), False))  # a zero margin that leaves one level: degenerate
    for t in ([[9, 0, 0], [0, 7, 0], [0, 0, 4]], [[0, 0, 4], [0, 7, 0], [9, 0, 0]], [[9, 3, 0], [0, 7, 0], [0, 2, 4]]):
        cases.append(((3, 3), np.array(t), False))  # perfectly monotone: boundary
    cases.append(((2, 2), np.array([[50, 0], [0, 50]]), False))
    cases.append(((2, 2), np.array([[0, 50], [50, 0]]), False))
    return cases


# ------------------------------------------------------------------------------------------------ planted effect
# A marker acts on a liability (latent correlation 0.5) of which the disease is the upper 5 %; the continuous trait Y is
# a noisy reading of the same liability (0.8), Z is noise.  Marker, Y and disease are all dependent, and the marker stays
# dependent on the disease given Y.  On Pearson values the marker-disease and Y-disease correlations are attenuated by
# the same factor while marker-Y is not, and every pair counts N observations: given Y the marker-disease edge falls
# below the threshold.  On polychoric / polyserial values with their own sample sizes it stays.
PLANTED_N, PLANTED_K, PLANTED_MARKER, PLANTED_TRAITS, PLANTED_DISEASE = 2000, 24, 5, 3, 1
PLANTED_ALPHA, PLANTED_L1, PLANTED_L2 = 1e-8, 1, 0  # the oracle drops the edge on Pearson values from 1e-6 to 1e-13 at least


def planted_set():
    """-> (G k x N dosages 0/1/2, phen 3 x N float32, standardised: Y, disease (two values), Z)"""
    rng = np.random.Generator(np.random.PCG64(1))
    N, k = PLANTED_N, PLANTED_K
    x = rng.standard_normal(N)
    liab = 0.5 * x + np.sqrt(0.75) * rng.standard_normal(N)
    case = (liab > np.quantile(liab, 0.95)).astype(np.float32)
    Y = 0.8 * liab + 0.6 * rng.standard_normal(N)
    Z = rng.standard_normal(N)
    G = np.zeros((k, N), np.int64)
    for i in range(k):
        maf = rng.uniform(0.1, 0.5)
        G[i] = (rng.random(N) < maf).astype(np.int64) + (rng.random(N) < maf).astype(np.int64)
    G[PLANTED_MARKER] = np.searchsorted([-0.5, 0.8], x)
    phen = np.stack([Y, case, Z])
    # standardised, as the Pearson build expects a .phen to be: the disease keeps its two levels
    phen = (phen - phen.mean(1, keepdims=True)) / phen.std(1, keepdims=True)
    return G, phen.astype(np.float32)


def planted_squares(G, phen):
    """square correlation and sample-size matrices (markers, then traits) as plain `--het` forms them (Pearson, N) and as
    `--ordinal` does (oracle estimates through float32 and ess = ((1 - r^2) / se)^2 for the pairs of the disease)"""
    k, N = G.shape
    p, o = phen.shape[0], k + PLANTED_DISEASE
    V = np.vstack([G.astype(np.float64), phen.astype(np.float64)])
    C = np.corrcoef(V).astype(np.float32)
    E = np.full((k + p, k + p), float(N), np.float32)
    E[np.arange(k, k + p), np.arange(k, k + p)] = np.nan
    Co, Eo = C.copy(), E.copy()
    codes = (phen[PLANTED_DISEASE] > 0).astype(np.int64)
    for v in range(k + p):
        if v == o:
            continue
        r, se, _ = R.polychoric(R.pair_table(G[v], codes, 3, 2)) if v < k else R.polyserial(V[v], codes)
        r, se = np.float32(r), np.float32(se)
        Co[v, o] = Co[o, v] = r
        Eo[v, o] = Eo[o, v] = np.float32(((1.0 - float(r) ** 2) / float(se)) ** 2)
    return C, E, Co, Eo


def has_edge(num_var, new_to_old, adj, a, b):
    """is the edge between the input variables a and b in a reduced skeleton?"""
    ixs = [int(v) for v in new_to_old]
    if a not in ixs or b not in ixs:
        return False
    return bool(np.asarray(adj).reshape(num_var, num_var)[ixs.index(a), ixs.index(b)])
