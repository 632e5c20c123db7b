"""GPU: the kernels that move results between the stages -- the row gather of the .bed, the lower-triangle pack, NaN -> 0,
the row and sub-matrix gathers, the bitmap and pMax readouts -- bit for bit against numpy indexing, at the sizes where
their branches change (tests/test_layout_cases.py holds the cases, the restatements and the conditions on the inputs).

Every comparison is on bit patterns (floats as uint32: NaN payloads, -0.0 and denormals count), and every output buffer,
on the host or on the device, is followed by a guard of poison words that must come back untouched.  Entry points that
skeleton.py wraps without a guard are called through `_lib.lib()`."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref64
from test_layout_cases import (BATCH_N, GATHER_N, GATHER_P, INDEX_LISTS, M_TOTAL, OFFSETS, READOUT_CASES, READOUT_LEVEL, TAILS,
                               batch_case, bits, gather_data, gather_rows_ref, kept_and_removed, nan_to_zero_ref, pack_adj_bits,
                               pack_block_bits_ref, pack_lower_tri_ref, pair_counts_ref, readout_case, unpack_adj_bits)

pytestmark = pytest.mark.gpu
ML = 14
GUARD = 8
POISON = np.uint32(0xFFC0DEAD)  # as a float a NaN with its sign bit set and a payload, as an int -4137299
POISON64 = np.uint64(0xDEADBEEFFFC0DEAD)
# NaNs (default, negative, with payloads, signalling), -0.0, +-inf, the smallest and the largest denormal
NANS = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD54321, 0x7F800001, 0xFFBFFFFF], np.uint32)
SPECIALS = np.concatenate([NANS, np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)])


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


@pytest.fixture(scope="module")
def L():
    from cigwas_amd._lib import lib

    return lib()


@pytest.fixture(scope="module")
def eng(cg):
    e = cg.Engine(0)
    yield e
    e.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ok(L, e, rc):
    assert rc == 0, L.cusk_last_error(e.h).decode()


def _poisoned(count, dtype=np.uint32):
    return np.full(count, POISON64 if dtype == np.uint64 else POISON, dtype)


def _special_floats(rng, shape, rate):
    """float32 bit patterns: standard normal values with SPECIALS at `rate` of the places"""
    b = bits(rng.standard_normal(shape, dtype=np.float32)).copy()
    sel = rng.random(shape, dtype=np.float32) < rate
    b[sel] = rng.choice(SPECIALS, int(sel.sum()))
    return b


# ---------------------------------------------------------------------------------------------------------------------
# 1. the row gather of the .bed (gather_bed_rows_kernel, gather_f32_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _build(L, e, Cd, words, call, k, p):
    """one correlation build into the poisoned allocation Cd: -> (the (k + p)^2 matrix, mxp) as bit patterns"""
    n = k + p
    _ok(L, e, L.cusk_dev_upload(Cd.ptr, _vp(_poisoned(words)), 4 * words))
    mxp = _poisoned(k * p + GUARD)
    _ok(L, e, call(Cd.ptr, _vp(mxp)))
    got = Cd.download(np.uint32, (words,))
    assert np.all(got[n * n:] == POISON) and np.all(mxp[k * p:] == POISON)
    return got[:n * n].reshape(n, n), mxp[:k * p].copy()


def _counts(L, e, bed_ptr, phen, ix, N, p):
    k = len(ix)
    mxp_n, pxp_n = _poisoned(k * p + GUARD).view(np.int32), _poisoned(p * p + GUARD).view(np.int32)
    _ok(L, e, L.cusk_pair_counts(e.h, bed_ptr, _vp(phen), _vp(ix), k, M_TOTAL, N, p, _vp(mxp_n), _vp(pxp_n)))
    assert np.all(mxp_n.view(np.uint32)[k * p:] == POISON) and np.all(pxp_n.view(np.uint32)[p * p:] == POISON)
    return mxp_n[:k * p].reshape(k, p).copy(), pxp_n[:p * p].reshape(p, p).copy()


@pytest.mark.parametrize("N", GATHER_N)
def test_bed_row_gather(cg, L, eng, N):
    """cusk_corr_build_indexed and cusk_pair_counts on device-resident rows, for every index list and with the .bed at
    byte offsets 0 .. 3 of its allocation: the bits of cusk_corr_build on bed[ixs] packed on the host (means and sds
    gathered on the host and on the device), the counts of numpy; random bits past individual N change nothing"""
    d = gather_data(N)
    p, clb, bed, phen = GATHER_P, (N + 3) // 4, d["bed"], np.ascontiguousarray(d["phen"])
    bed_r = ref64.random_padding(bed, N, seed=N)
    assert N % 4 and not np.array_equal(bed_r, bed) and np.array_equal(bed_r[:, :-1], bed[:, :-1])
    mean, sd = np.ascontiguousarray(d["mean"]), np.ascontiguousarray(d["sd"])
    mean_d, sd_d = cg.DeviceArray(mean), cg.DeviceArray(sd)
    words = (M_TOTAL + p) ** 2 + GUARD
    Cd = cg.DeviceArray(nbytes=4 * words)
    lists = [np.array(ixs, np.int32) for ixs in INDEX_LISTS]
    want = []
    for ix in lists:  # the references: once per list, shared by the offsets
        k = len(ix)
        rows, mean_k, sd_k = np.ascontiguousarray(bed[ix]), np.ascontiguousarray(mean[ix]), np.ascontiguousarray(sd[ix])
        sq, mxp = _build(L, eng, Cd, words, lambda c, m: L.cusk_corr_build(eng.h, _vp(rows), _vp(phen), k, N, p, _vp(mean_k),
                                                                             _vp(sd_k), c, m), k, p)
        assert np.array_equal(sq[:k, k:].reshape(-1), mxp)
        want.append((sq, mxp) + pair_counts_ref(rows, phen, N, p))
    rng = np.random.default_rng(N)
    for off in OFFSETS:
        allocs = []
        for b in (bed, bed_r):  # the .bed inside a larger allocation; what surrounds it is noise
            raw = rng.integers(0, 256, bed.size + 16, dtype=np.uint8)
            raw[off:off + bed.size] = b.reshape(-1)
            allocs.append(cg.DeviceArray(raw))
        for ix, (sq, mxp, mxp_n, pxp_n) in zip(lists, want):
            k, tag = len(ix), (N, len(ix), int(ix[0]), off)
            for bed_ptr, stats in ((allocs[0].ptr + off, (_vp(mean), _vp(sd))), (allocs[0].ptr + off, (mean_d.ptr, sd_d.ptr)),
                                   (allocs[1].ptr + off, (mean_d.ptr, sd_d.ptr))):
                got, got_mxp = _build(L, eng, Cd, words, lambda c, m: L.cusk_corr_build_indexed(
                    eng.h, bed_ptr, _vp(phen), _vp(ix), k, M_TOTAL, N, p, stats[0], stats[1], c, m), k, p)
                assert np.array_equal(got, sq) and np.array_equal(got_mxp, mxp), tag
            for a in allocs:
                got_n, got_pn = _counts(L, eng, a.ptr + off, phen, ix, N, p)
                assert np.array_equal(got_n, mxp_n) and np.array_equal(got_pn, pxp_n), tag
        for a in allocs:
            a.free()
    for a in (mean_d, sd_d, Cd):
        a.free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. cusk_pack_lower_tri
# ---------------------------------------------------------------------------------------------------------------------
def _tri_matrix(n, k, seed, edges):
    """n x n bit patterns: random values with SPECIALS at one place in eight everywhere; outside the triangle of the
    leading k x k block every other element is a NaN that the pack must not pick up (it would give a zero where the
    reference has a value).  edges: NaN at (0, 0), every (i, i), every (i, 0) and the last element, and -0.0, +-inf and a
    denormal inside the triangle where it has room"""
    rng = np.random.default_rng(seed)
    b = _special_floats(rng, (n, n), 0.125)
    i = np.arange(n)
    outside = i[None, :] > i[:, None]
    outside[k:, :] = True
    outside[:, k:] = True
    b[outside & ((i[:, None] + i[None, :]) % 2 == 0)] = 0xFFC0BAD0
    if edges:
        r = np.arange(k)
        b[r, r] = NANS[r % len(NANS)]
        b[r, 0] = NANS[(r + 1) % len(NANS)]
        b[k - 1, k - 1] = 0xFFC12345
        inner = [(a, c) for a in range(2, min(k, 7)) for c in range(1, a)][:5]
        for (a, c), v in zip(inner, (0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF)):
            b[a, c] = v
    return b


def _check_pack(cg, L, e, n, k, seed, edges):
    b = _tri_matrix(n, k, seed, edges)
    want = bits(pack_lower_tri_ref(b.view(np.float32), k))
    total = k * (k + 1) // 2
    assert want.shape == (total,)
    # four poison rows follow the matrix: a walk that leaves the last row reads poison, not someone else's memory
    flat = _poisoned(n * n + 4 * n + GUARD)
    flat[:n * n] = b.reshape(-1)
    Md = cg.DeviceArray(flat)
    out = _poisoned(total + GUARD)
    _ok(L, e, L.cusk_pack_lower_tri(e.h, Md.ptr, n, k, _vp(out), 0))
    assert np.array_equal(out[:total], want) and np.all(out[total:] == POISON), (n, k, edges, "host")
    Od = cg.DeviceArray(_poisoned(total + GUARD))
    assert Od.ptr % 16 == 0
    _ok(L, e, L.cusk_pack_lower_tri(e.h, Md.ptr, n, k, Od.ptr, 1))
    got = Od.download(np.uint32, (total + GUARD,))
    assert np.array_equal(got[:total], want) and np.all(got[total:] == POISON), (n, k, edges, "device")
    Md.free()
    Od.free()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 257])
def test_pack_lower_tri(cg, L, eng, k):
    for n in (k, k + 1, k + 37):
        for edges in (True, False):
            _check_pack(cg, L, eng, n, k, 100 * k + n, edges)


def test_pack_lower_tri_4097(cg, L, eng):
    """8.4 million outputs: the row of an element comes from a square root in double precision, far from small offsets"""
    _check_pack(cg, L, eng, 4097, 4097, 4097, True)


def test_pack_lower_tri_refuses_an_unaligned_device_output(cg, L, eng):
    Md, Od = cg.DeviceArray(np.zeros((4, 4), np.float32)), cg.DeviceArray(_poisoned(16 + GUARD))
    assert L.cusk_pack_lower_tri(eng.h, Md.ptr, 4, 4, Od.ptr + 4, 1) != 0
    assert "16-byte aligned" in L.cusk_last_error(eng.h).decode()
    assert np.all(Od.download(np.uint32, (16 + GUARD,)) == POISON)
    Md.free()
    Od.free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. cusk_nan_to_zero
# ---------------------------------------------------------------------------------------------------------------------
GUARD_NANS = np.array([0x7FC00100 + i if i % 2 else 0xFFC00100 + i for i in range(GUARD)], np.uint32)


def _nan_patterns(count, seed):
    rng = np.random.default_rng(seed)
    base = bits(rng.standard_normal(count, dtype=np.float32)).copy()
    for r in range(4):  # a NaN at every position r mod 4: each component of the float4 body in turn, and of the tail
        b = base.copy()
        b[r::4] = NANS[np.arange(len(b[r::4])) % len(NANS)]
        yield f"NaN at {r} mod 4", b
    yield "all NaN", NANS[np.arange(count) % len(NANS)].copy()
    yield "no NaN", base
    sel = rng.random(count) < 0.5
    sp = base.copy()
    sp[sel] = rng.choice(SPECIALS, int(sel.sum()))
    yield "special values", sp


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2049])
def test_nan_to_zero(cg, eng, count):
    for name, b in _nan_patterns(count, count):
        assert b.shape == (count,)
        Md = cg.DeviceArray(np.concatenate([b, GUARD_NANS]))
        eng.nan_to_zero(Md.ptr, count)
        got = eng.download(Md.ptr, np.uint32, (count + GUARD,))
        assert np.array_equal(got[:count], bits(nan_to_zero_ref(b.view(np.float32)))), (count, name)
        assert np.array_equal(got[count:], GUARD_NANS), (count, name)  # still NaN, payloads and all
        Md.free()


def test_nan_to_zero_refuses_an_unaligned_pointer(cg, eng):
    Md = cg.DeviceArray(np.concatenate([NANS, NANS]))
    with pytest.raises(RuntimeError, match="bad arguments"):
        eng.nan_to_zero(Md.ptr + 4, 4)
    assert np.array_equal(eng.download(Md.ptr, np.uint32, (2 * len(NANS),)), np.concatenate([NANS, NANS]))
    Md.free()


# ---------------------------------------------------------------------------------------------------------------------
# 4. cusk_gather_rows, cusk_gather_submatrix, cusk_gather_submatrix_dev
# ---------------------------------------------------------------------------------------------------------------------
GN = 300


@pytest.fixture(scope="module")
def matrix(cg):
    M = _special_floats(np.random.default_rng(300), (GN, GN), 0.125)
    Md = cg.DeviceArray(M)
    yield M, Md
    Md.free()


def _row_tables(sizes, rows_per_list, gap, seed):
    """lists of `sizes` columns (not ascending), rows_per_list[j] rows of the matrix gathered at list j, `gap` floats left
    free after every row of the output"""
    rng = np.random.default_rng(seed)
    lists = [rng.permutation(GN)[:s] for s in sizes]
    assert all(s == 1 or not np.array_equal(l, np.sort(l)) for s, l in zip(sizes, lists))
    idx = np.concatenate(lists).astype(np.int32)
    row_src, row_k, row_first, row_out = [], [], [], []
    first = out = 0
    for l, rows in zip(lists, rows_per_list):
        for src in rng.integers(0, GN, rows):
            row_src.append(int(src))
            row_k.append(len(l))
            row_first.append(first)
            row_out.append(out)
            out += len(l) + gap
        first += len(l)
    return (idx, np.array(row_src, np.int32), np.array(row_k, np.int32), np.array(row_first, np.int64), np.array(row_out, np.int64), out)


@pytest.mark.parametrize("sizes,rows_per_list", [((1, 63, 64, 65, 200), (1, 5, 4, 6, 5)), ((65,), (1,)), ((1,), (1,))])
def test_gather_rows(cg, L, eng, matrix, sizes, rows_per_list):
    """21 = 4 * 5 + 1 rows over lists of 1 to 200 columns (a wave takes one row, 64 columns a trip), and a single row.
    Device route: rows land where row_out says and the gaps between them keep the poison.  Host route: the call copies
    out_count floats of engine scratch, so only the rows and what follows out_count are defined there"""
    M, Md = matrix
    idx, row_src, row_k, row_first, row_out, count = _row_tables(sizes, rows_per_list, 3, sum(sizes))
    assert len(row_src) % 4 == 1
    want = gather_rows_ref(M, idx, row_src, row_k, row_first, row_out, _poisoned(count + GUARD))
    args = (eng.h, Md.ptr, GN, _vp(idx), len(idx), _vp(row_src), _vp(row_k), _vp(row_first), _vp(row_out), len(row_src))
    Od = cg.DeviceArray(_poisoned(count + GUARD))
    _ok(L, eng, L.cusk_gather_rows(*args, Od.ptr, count, 1))
    assert np.array_equal(Od.download(np.uint32, (count + GUARD,)), want)
    Od.free()
    out = _poisoned(count + GUARD)
    _ok(L, eng, L.cusk_gather_rows(*args, _vp(out), count, 0))
    written = want != POISON  # no value of the matrix is the poison pattern
    assert written.sum() == int(row_k.sum()) and np.array_equal(out[written], want[written]) and np.all(out[count:] == POISON)
    # the same rows without gaps, as the block driver packs them: the host route whole
    idx, row_src, row_k, row_first, row_out, count = _row_tables(sizes, rows_per_list, 0, sum(sizes))
    out = _poisoned(count + GUARD)
    _ok(L, eng, L.cusk_gather_rows(eng.h, Md.ptr, GN, _vp(idx), len(idx), _vp(row_src), _vp(row_k), _vp(row_first), _vp(row_out),
                                   len(row_src), _vp(out), count, 0))
    assert np.array_equal(out, gather_rows_ref(M, idx, row_src, row_k, row_first, row_out, _poisoned(count + GUARD)))


@pytest.mark.parametrize("k", [1, 255, 256, 257])
def test_gather_submatrix(cg, L, eng, matrix, k):
    M, Md = matrix
    idx = np.random.default_rng(k).permutation(GN)[:k].astype(np.int32)
    want = M[np.ix_(idx, idx)].reshape(-1)
    out = _poisoned(k * k + GUARD)
    _ok(L, eng, L.cusk_gather_submatrix(eng.h, Md.ptr, GN, _vp(idx), k, _vp(out)))
    assert np.array_equal(out[:k * k], want) and np.all(out[k * k:] == POISON)
    Od = cg.DeviceArray(_poisoned(k * k + GUARD))
    _ok(L, eng, L.cusk_gather_submatrix_dev(eng.h, Md.ptr, GN, _vp(idx), k, Od.ptr))
    got = Od.download(np.uint32, (k * k + GUARD,))
    assert np.array_equal(got[:k * k], want) and np.all(got[k * k:] == POISON)
    Od.free()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the readouts of one run
# ---------------------------------------------------------------------------------------------------------------------
def _pmax(L, e, C_ptr, n):
    out = _poisoned(n * n + GUARD)
    _ok(L, e, L.cusk_result_pmax(e.h, C_ptr, _vp(out)))
    assert np.all(out[n * n:] == POISON)
    return out[:n * n].reshape(n, n).copy()


@pytest.mark.parametrize("n,seed,strength", READOUT_CASES)
def test_readouts_of_one_run(cg, L, eng, n, seed, strength):
    """adjacency(), the bitmap, cusk_result_adj_i32_dev and cusk_result_adj_rows describe one graph, the oracle's; pMax and
    the dense separating sets are the oracle's too"""
    Cm, Th, ref = readout_case(n, seed, strength)
    Cd = cg.DeviceArray(Cm)
    eng.run_skeleton(Cd.ptr, n, Th, READOUT_LEVEL)
    G = eng.adjacency()
    assert np.array_equal(G, ref.G)
    kept, removed = kept_and_removed(G)
    assert n == 2 or (kept > 0 and removed > 0)
    words = (n + 63) // 64
    adj = eng.adjacency_bits()
    assert adj.shape == (n, words) and np.array_equal(unpack_adj_bits(adj, n), G)
    assert not unpack_adj_bits(adj, 64 * words)[:, n:].any()  # no bit at a column >= n in the last word
    assert np.array_equal(adj, pack_adj_bits(G))
    Gd = cg.DeviceArray(_poisoned(n * n + GUARD))
    _ok(L, eng, L.cusk_result_adj_i32_dev(eng.h, Gd.ptr))
    got = Gd.download(np.uint32, (n * n + GUARD,))
    assert np.array_equal(got[:n * n].view(np.int32).reshape(n, n), G) and np.all(got[n * n:] == POISON)
    Gd.free()
    for row0, nrows in [(0, 1), (n - 1, 1), (0, n)] + ([(63, 2)] if n > 64 else []):
        out = _poisoned(nrows * words + GUARD, np.uint64)
        _ok(L, eng, L.cusk_result_adj_rows(eng.h, row0, nrows, _vp(out)))
        assert np.array_equal(out[:nrows * words].reshape(nrows, words), adj[row0:row0 + nrows]), (row0, nrows)
        assert np.all(out[nrows * words:] == POISON64)
    # separating sets: the dense form of the records, and the oracle's
    x, y, lv, z, S = eng.sepsets()
    dense = np.full((n, n, ML), -1, np.int32)
    dense[x, y] = S
    assert np.array_equal(dense, ref.sepset)
    sep = _poisoned(n * n * ML + GUARD).view(np.int32)
    _ok(L, eng, L.cusk_result_sepset_dense(eng.h, _vp(sep)))
    assert np.array_equal(sep[:n * n * ML].reshape(n, n, ML), dense) and np.all(sep.view(np.uint32)[n * n * ML:] == POISON)
    # pMax
    pm = _pmax(L, eng, Cd.ptr, n)
    pmf = pm.view(np.float32)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(pm, pm.T)
    assert np.all(np.diag(pm) == bits(np.float32(1.0))) and np.all(pm[(G != 0) & off] == bits(np.float32(-100000.0)))
    away = (G == 0) & off
    assert not np.isnan(pmf[away]).any() and np.all(np.abs(pmf[away].astype(np.float64) - ref.pmax[away]) <= 1e-6)
    assert np.array_equal(ref.pmax[~away], pmf[~away])
    # the level-0 z of a removed pair is read at (min, max), as the reference's level 0 reads it: a matrix whose lower
    # triangle is NaN gives the same bits (the records' z are in place by now: they are not computed again)
    upper = Cm.copy()
    upper[np.tril_indices(n, -1)] = np.nan
    Ud = cg.DeviceArray(upper)
    assert np.array_equal(_pmax(L, eng, Ud.ptr, n), pm)
    assert np.array_equal(_pmax(L, eng, Cd.ptr, n), pm)
    Ud.free()
    Cd.free()


def test_readouts_of_a_batched_run(cg, L, oracle):
    """blocks of 1, 63, 64, 65 and 130 variables, unused rows between two of them: adjacency_blocks() are the per-block
    slices of adjacency() and the oracle's graphs; the packed bitmaps, whole and by tail, are the numpy restatement"""
    big, lo, hi, Th, refs = batch_case()
    e = cg.Engine(0)
    Cd = cg.DeviceArray(big)
    e.run_skeleton_batch(Cd.ptr, BATCH_N, lo, hi, Th, READOUT_LEVEL)
    G, adj = e.adjacency(), e.adjacency_bits()
    assert G.shape == (BATCH_N, BATCH_N) and np.array_equal(adj, pack_adj_bits(G))
    Gs = e.adjacency_blocks()
    inside = np.zeros(G.shape, bool)
    for b, (l, h) in enumerate(zip(lo, hi)):
        assert np.array_equal(Gs[b], G[l:h, l:h]) and np.array_equal(Gs[b], refs[b].G), b
        inside[l:h, l:h] = True
    assert not G[~inside].any()
    want = pack_block_bits_ref(adj, lo, hi)
    out = _poisoned(len(want) + GUARD, np.uint64)
    _ok(L, e, L.cusk_result_adj_bits_blocks(e.h, _vp(out)))
    assert np.array_equal(out[:len(want)], want) and np.all(out[len(want):] == POISON64)
    for tail in TAILS:
        want = pack_block_bits_ref(adj, lo, hi, tail)
        rows = np.concatenate([pack_adj_bits(Gb)[-min(tail, len(Gb)):].reshape(-1) for Gb in Gs])  # the last rows of each block
        assert np.array_equal(want, rows)
        out = _poisoned(len(want) + GUARD, np.uint64)
        _ok(L, e, L.cusk_result_adj_bits_blocks_tail(e.h, tail, _vp(out)))
        assert np.array_equal(out[:len(want)], want) and np.all(out[len(want):] == POISON64), tail
    Cd.free()
    e.close()
