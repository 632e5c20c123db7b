"""GPU: every path of the correlation build against the float64 reference of oracle/ref64.py (computed from the dosages,
not from .bed bytes), at the shapes where the kernels change branch and up to N = 500,001 individuals.

Bars (oracle/ref64.py):
  mxm  NaN where ref64 has NaN, elsewhere |gpu - ref64| <= 1e-6 (exact counts, float epilogue); and bit-equal to the
       oracle, as before.
  mxp  |gpu - ref64| <= (3 sqrt(chain) + 8) 2^-24 S_abs + 1e-7, S_abs = (sum |g y| + |mean_g| sum |y|) / (n sd_g), with
       `chain` the longest chain of dependent f32 additions of the path (CHAIN below); never looser than 1e-5 for markers
       with sd >= 0.1 against unit-scale traits at N <= 70k.  pxp the same with S_abs = sum |a b| / n.
Every case also asserts that its bars would see a lost individual (the last one; the last 64 when N > 70k): ref64
without them moves some element by more than 4 bars."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref64

pytestmark = pytest.mark.gpu

# longest chain of dependent f32 additions per SNP x trait / trait x trait element, from the kernels' summation structure
CHAIN = {
    # mxp_bf16_kernel: 4 waves split K; a wave adds one 16-individual MFMA product per step -> N / 64 steps, + 4 waves
    "bf16": lambda N: N / 64 + 4,
    # mxp_mfma_kernel (corr_mxp_f32): 8 waves split K, 2 individuals per v_mfma_f32_32x32x2 step -> N / 16, + 8 waves
    "f32": lambda N: N / 16 + 8,
    # mxp_kernel (corr_popcount): one wave per marker, 64 lanes each over N / 64 individuals, + a 6-level reduction
    "scalar": lambda N: N / 64 + 6,
    # pxp_kernel: 256 threads each over N / 256 individuals, + an 8-level tree
    "pxp": lambda N: N / 256 + 8,
}

# (m, N, p, miss): the boundary each case hits.  FAST = the .bed rows are whole 64-individual requests (N % 64 == 0);
# nfull = N / 256 full K blocks of mxm_fp4_kernel<true>, streamed two at a time (odd / even branches).
CASES = [
    (1, 1, 1, 0.0),        # N = 1: one individual, every correlation undefined; m = p = 1
    (2, 2, 2, 0.0),        # N = 2: one partial .bed byte; one SNP pair, one trait pair
    (33, 3, 1, 0.0),       # N = 3; m = 33: one marker past a 32-row tile
    (31, 5, 22, 0.0),      # N = 5: second byte partial; p = 22: one past a 21-trait bf16 launch
    (63, 63, 2, 0.01),     # N = 63: non-FAST, one short of a 64-individual request; m = 63
    (64, 64, 20, 0.01),    # N = 64: FAST, nfull = 0 (tail only); m = 64 whole tiles
    (65, 65, 21, 0.01),    # N = 65: non-FAST, one past; p = 21: exactly one bf16 launch
    (32, 255, 42, 0.01),   # N = 255: non-FAST; m = 32; p = 42: two whole bf16 launches
    (129, 256, 43, 0.01),  # N = 256: FAST, nfull = 1 (odd), no tail; m = 129; p = 43: three bf16 launches, two f32 ones
    (63, 257, 64, 0.60),   # N = 257: non-FAST, 60 % missing; p = 64: two whole 32-trait f32 launches
    (65, 768, 5, 0.01),    # N = 768: FAST, nfull = 3 (odd >= 3: the loop leaves after its first half), no tail
    (33, 1088, 3, 0.01),   # N = 1088: FAST, nfull = 4 (even) + a 64-individual tail
    (64, 1280, 7, 0.0),    # N = 1280: FAST, nfull = 5 (odd), no missing data
    (40, 16388, 6, 0.01),  # N = 16388: non-FAST for both MFMA mxp forms (N % 4 == 0, N % 64 != 0)
]
LARGE = [
    (96, 131136, 22, 0.01),  # large tier, FAST: nfull = 512 (even) + a 64-individual tail
    (64, 500001, 20, 0.01),  # large tier, non-FAST, N % 4 = 1
]
PATHS = {  # engine options of each path (compat = cu_corr_pearson_npn, an engine of its own per call)
    "default": ({}, "bf16"),
    "fp4_0": ({"corr_fp4": 0}, "bf16"),
    "popcount": ({"corr_popcount": 1}, "scalar"),
    "mxp_f32": ({"corr_mxp_f32": 1}, "f32"),
}


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


@pytest.fixture(scope="module")
def engines(cg):
    out = {}
    for name, (opts, _) in PATHS.items():
        e = cg.Engine(0)
        for k, v in opts.items():
            e.set_option(k, v)
        out[name] = e
    yield out
    for e in out.values():
        e.close()


def _square(cg, e, bed, Y, m, N, p, mean, sd):
    n = m + p
    Cd = cg.DeviceArray(nbytes=4 * n * n)
    try:
        mxp = e.corr_build(bed, Y.reshape(-1), m, N, p, mean, sd, Cd.ptr, want_mxp=True)
        sq = Cd.download(np.float32, (n, n))
    finally:
        Cd.free()
    iu, ip = np.triu_indices(m, 1), np.triu_indices(p, 1)
    assert np.array_equal(sq[:m, m:], mxp.reshape(m, p), equal_nan=True)
    assert np.array_equal(sq[m:, :m], sq[:m, m:].T, equal_nan=True)
    return sq[:m, :m][iu], sq[:m, m:], sq[m:, m:][ip]


def _reference(G, Y, mean, sd, N, cut):
    R = ref64.mxm(G)
    r, s_abs = ref64.mxp(G, Y, mean, sd)
    q, q_abs = ref64.pxp(Y)
    R1 = ref64.mxm(G[:, :-cut])
    r1, _ = ref64.mxp(G[:, :-cut], Y[:, :-cut], mean, sd)
    q1, _ = ref64.pxp(Y[:, :-cut])
    return (R, r, s_abs, q, q_abs), (R1, r1, q1)


def _check(name, got, ref, Y, sd, N, form):
    (R, r, s_abs, q, q_abs) = ref
    m, p = r.shape
    iu, ip = np.triu_indices(m, 1), np.triu_indices(p, 1)
    mxm, mxp, pxp = got
    ref64.check_mxm_nan(f"{name} mxm", mxm, R[iu])
    bar = ref64.sum_bar(s_abs, CHAIN[form](N), ref64.cap_1e5(sd, Y, N))
    ref64.check_close(f"{name} mxp", np.asarray(mxp).reshape(m, p), r, bar)
    qbar = ref64.sum_bar(q_abs, CHAIN["pxp"](N))[ip]
    ref64.check_close(f"{name} pxp", pxp, q[ip], qbar)
    return bar, qbar


def _run_case(cg, engines, oracle, synth, m, N, p, miss):
    G, Y = ref64.make_case(m, N, p, seed=3 * m + N, miss=miss)
    mean, sd = ref64.stats(G)
    bed = synth.pack_bed(G)
    cut = 1 if N <= 70_000 else 64
    ref, ref_cut = _reference(G, Y, mean, sd, N, cut)
    iu, ip = np.triu_indices(m, 1), np.triu_indices(p, 1)
    # the compat ABI (the reference's entry point, default options)
    c_mxm, c_mxp, c_pxp = cg.cu_corr_pearson_npn(bed, Y.reshape(-1), m, N, p, mean, sd)
    bar, qbar = _check("compat", (c_mxm, c_mxp, c_pxp), ref, Y, sd, N, "bf16")
    outs = {}
    for name, (_, form) in PATHS.items():
        outs[name] = _square(cg, engines[name], bed, Y, m, N, p, mean, sd)
        _check(name, outs[name], ref, Y, sd, N, form)
    for name in PATHS:  # every SNP x SNP path counts the same table
        assert np.array_equal(outs[name][0], c_mxm, equal_nan=True), name
    if N <= 131_136:  # the oracle's exact counts, same epilogue: bit-equal
        o_mxm = oracle.corr_pearson_npn(bed, Y.reshape(-1), m, N, p, mean, sd)[0] if m > 1 else np.zeros(0, np.float32)
        assert np.array_equal(c_mxm, o_mxm, equal_nan=True)
    if N % 4:  # random bits past the last individual of every row change nothing
        bed_r = ref64.random_padding(bed, N, seed=N)
        assert np.array_equal(cg.cu_corr_pearson_npn(bed_r, Y.reshape(-1), m, N, p, mean, sd)[0], c_mxm, equal_nan=True)
        again = _square(cg, engines["default"], bed_r, Y, m, N, p, mean, sd)
        for a, b in zip(again, outs["default"]):
            assert np.array_equal(a, b, equal_nan=True)
    # sensitivity: the bars see the loss of the last individual(s)
    R, r, _, q, _ = ref
    R1, r1, q1 = ref_cut
    if N == 1:  # nothing is defined with one individual (sd_g = 0, no pair of individuals): nothing can move
        assert not np.isfinite(r).any() and not np.isfinite(q[ip]).any()
        return
    mv = max(ref64.moved(R[iu], R1[iu], ref64.MXM_BAR), ref64.moved(r, r1, bar), ref64.moved(q[ip], q1[ip], qbar))
    assert mv > 4, f"the bars cannot see {cut} lost individual(s): largest move {mv:.3g} bars"


@pytest.mark.parametrize("m,N,p,miss", CASES)
def test_corr_paths_against_ref64(cg, engines, oracle, synth, m, N, p, miss):
    _run_case(cg, engines, oracle, synth, m, N, p, miss)


@pytest.mark.parametrize("m,N,p,miss", LARGE)
def test_corr_paths_against_ref64_biobank_n(cg, engines, oracle, synth, m, N, p, miss):
    _run_case(cg, engines, oracle, synth, m, N, p, miss)


@pytest.mark.parametrize("m,N,width", [(65, 768, 40), (129, 257, 64), (40, 16388, 17), (33, 131136, 32)])
def test_corr_banded_against_ref64(cg, engines, synth, m, N, width):
    """`mps block`'s banded form: the band and its forward row sums of |band|"""
    G, _ = ref64.make_case(m, N, 1, seed=N + 1, miss=0.01)
    band, sums = ref64.banded(G, width)
    bed = synth.pack_bed(G)
    g_sums, g_band = engines["default"].corr_banded(bed, m, N, width, want_band=True)
    ref64.check_mxm_nan("band", g_band, band)
    # float sums of <= width terms in column order: width roundings of at most 2^-24 x the sum, + the band's own errors
    ref64.check_close("band row sums", g_sums, sums, width * ref64.U * sums + width * ref64.MXM_BAR)
    if N % 4:
        s2, b2 = engines["default"].corr_banded(ref64.random_padding(bed, N, seed=N), m, N, width, want_band=True)
        assert np.array_equal(b2, g_band, equal_nan=True) and np.array_equal(s2, g_sums, equal_nan=True)


SENTINEL = np.float32(-7.0)  # fills the batch allocation before a build: what the build leaves alone still holds it


class _BatchCase:
    """the chromosome job's batched build: blocks of 1, 63, 65 and 200 markers whose first markers are not multiples of
    64, on the diagonal of one allocation; the inputs live on the device once per (N, p)"""

    first = np.array([5, 6, 69, 134], np.int64)
    sizes = np.array([1, 63, 65, 200], np.int32)

    def __init__(self, cg, synth, N, p):
        self.cg, self.N, self.p = cg, N, p
        self.G, self.Y = ref64.make_case(340, N, p, seed=N + p, miss=0.01)
        self.mean, self.sd = ref64.stats(self.G)
        base, b = [], 0
        for k in self.sizes:
            base.append(b)
            b = (b + int(k) + p + 63) // 64 * 64
        self.base, self.n = np.array(base, np.int32), b
        self.dev = [cg.DeviceArray(np.ascontiguousarray(a)) for a in (synth.pack_bed(self.G), self.Y.reshape(-1), self.mean, self.sd)]
        self._default = self._refs = None

    def free(self):
        for d in self.dev:
            d.free()

    def build(self, e, split, keep=None):
        """-> (the n x n allocation, mxp_host) after cusk_corr_build_batch (split: _mxp + _mxm, with the keep mask)"""
        from cigwas_amd._lib import lib

        L, n, p = lib(), self.n, self.p
        Cd = self.cg.DeviceArray(np.full((n, n), SENTINEL, np.float32))
        mxp_host = np.zeros(int(self.sizes.sum()) * p, np.float32)
        args = [e.h] + [d.ptr for d in self.dev] + [self.N, p, len(self.sizes), self.first.ctypes.data, self.sizes.ctypes.data,
                                                    self.base.ctypes.data]
        try:
            if split:
                keep_a = None if keep is None else np.ascontiguousarray(keep, np.uint8)
                assert L.cusk_corr_build_batch_mxp(*args, n, Cd.ptr, mxp_host.ctypes.data) == 0
                assert L.cusk_corr_build_batch_mxm(*args, None if keep_a is None else keep_a.ctypes.data, n, Cd.ptr) == 0
            else:
                assert keep is None
                assert L.cusk_corr_build_batch(*args, n, Cd.ptr, mxp_host.ctypes.data) == 0
            sq = np.empty((n, n), np.float32)
            assert L.cusk_engine_download(e.h, sq.ctypes.data, C.c_void_p(Cd.ptr), sq.nbytes) == 0
        finally:
            Cd.free()
        return sq, mxp_host

    def build_with(self, opts):
        """the one-call entry and the split entries, each on a fresh engine with the options set"""
        out = []
        for split in (False, True):
            e = self.cg.Engine(0)
            for k, v in opts.items():
                e.set_option(k, v)
            try:
                out.append(self.build(e, split))
            finally:
                e.close()
        return out

    def default(self):
        if self._default is None:
            self._default = self.build_with({})
        return self._default

    def refs(self):
        if self._refs is None:
            self._refs = [_reference(self.G[f:f + k], self.Y, self.mean[f:f + k], self.sd[f:f + k], self.N, 1)[0]
                          for f, k in zip(self.first, self.sizes)]
        return self._refs

    def blocks(self):
        return [(int(f), int(k), int(b0)) for f, k, b0 in zip(self.first, self.sizes, self.base)]


@pytest.fixture(scope="module")
def batch_cases(cg, synth):
    cache = {}

    def get(N, p):
        if (N, p) not in cache:
            cache[(N, p)] = _BatchCase(cg, synth, N, p)
        return cache[(N, p)]

    yield get
    for c in cache.values():
        c.free()


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("N,p", [(1088, 22), (257, 43)])
def test_corr_batch_against_ref64(batch_cases, N, p, path):
    """cusk_corr_build_batch, and _mxp + _mxm, under every engine option of the single build.  The batch takes its SNP x
    trait form from corr_mxp_f32 alone and always counts SNP x SNP on the FP4 pipe: corr_popcount and corr_fp4 = 0 must
    leave every bit of the allocation and of mxp_host as the default engine leaves them."""
    case = batch_cases(N, p)
    opts, _ = PATHS[path]
    form = "f32" if opts.get("corr_mxp_f32") else "bf16"
    results = case.default() if not opts else case.build_with(opts)
    if path in ("popcount", "fp4_0"):
        for (sq, mxp_host), (sq0, mxp0) in zip(results, case.default()):
            assert np.array_equal(sq, sq0, equal_nan=True) and np.array_equal(mxp_host, mxp0, equal_nan=True), path
    assert np.array_equal(results[0][1], results[1][1], equal_nan=True)
    sq, mxp_host = results[0]
    off = 0
    written = np.zeros(sq.shape, bool)
    for (f, k, b0), ref in zip(case.blocks(), case.refs()):
        blk = sq[b0:b0 + k + p, b0:b0 + k + p]
        written[b0:b0 + k + p, b0:b0 + k + p] = True
        iu, ip = np.triu_indices(k, 1), np.triu_indices(p, 1)
        got = (blk[:k, :k][iu], blk[:k, k:], blk[k:, k:][ip])
        _check(f"batch block {f}+{k}", got, ref, case.Y, case.sd[f:f + k], N, form)
        assert np.array_equal(mxp_host[off:off + k * p].reshape(k, p), blk[:k, k:], equal_nan=True)
        assert np.array_equal(blk[k:, :k], blk[:k, k:].T, equal_nan=True)
        assert np.array_equal(blk[:k, :k], blk[:k, :k].T, equal_nan=True) and np.array_equal(blk[k:, k:], blk[k:, k:].T, equal_nan=True)
        assert np.all(np.diag(blk) == 1)
        assert np.array_equal(results[1][0][b0:b0 + k + p, b0:b0 + k + p], blk, equal_nan=True)  # _mxp + _mxm
        off += k * p
    assert np.all(sq[~written] == SENTINEL) and np.all(results[1][0][~written] == SENTINEL)  # nothing outside the blocks


def test_corr_batch_keep_mask(cg, batch_cases):
    """cusk_corr_build_batch_mxm builds the SNP x SNP part, the trait x trait part and the diagonal of the kept blocks
    only; the SNP x trait strips of every block are phase one's (cusk_corr_build_batch_mxp), whatever is kept"""
    N, p = 257, 43
    case = batch_cases(N, p)
    sq0, mxp0 = case.default()[1]  # _mxp + _mxm, every block kept
    e = cg.Engine(0)
    try:
        for keep in ([1, 0, 1, 0], [0, 0, 0, 0]):
            sq, mxp_host = case.build(e, True, keep)
            want = np.full(sq.shape, SENTINEL, np.float32)
            for (f, k, b0), kp in zip(case.blocks(), keep):
                if kp:
                    want[b0:b0 + k + p, b0:b0 + k + p] = sq0[b0:b0 + k + p, b0:b0 + k + p]
                else:
                    want[b0:b0 + k, b0 + k:b0 + k + p] = sq0[b0:b0 + k, b0 + k:b0 + k + p]
                    want[b0 + k:b0 + k + p, b0:b0 + k] = sq0[b0 + k:b0 + k + p, b0:b0 + k]
            assert np.array_equal(sq, want, equal_nan=True), keep
            assert np.array_equal(mxp_host, mxp0, equal_nan=True), keep
    finally:
        e.close()
