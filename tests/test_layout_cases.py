"""The inputs of tests/test_gpu_layout_kernels.py, checked without a GPU, so that no assertion there can hold vacuously.

The kernels that move results between the stages (the row gather of the .bed, the lower-triangle pack, NaN -> 0, the
row / sub-matrix gathers and the bitmap readouts) are pure data movement: their reference is numpy indexing and the bar is
bit equality.  This file holds
  - the case table of the .bed row gather and a restatement of the kernel's own branch rule (`chunk_classes`): the table
    must reach every branch, and the rows shorter than 16 bytes must reach no aligned-dword chunk at all;
  - the sensitivity of what the GPU test compares: one wrong individual in a gathered byte -- at the corners of the
    gathered image and in a chunk of every branch -- changes the numpy pair counts, and moves the float64 correlations
    by more than their bar;
  - numpy restatements of the lower-triangle pack, the block-bitmap pack (with and without tail) and the row gather,
    pinned on hand-written examples;
  - the matrices of the readout tests, checked on the oracle: kept and removed pairs exist at every size.

The cases, the data (cached per case) and the restatements are imported by the GPU file."""
import functools

import numpy as np
import pytest

from oracle import ref64
from test_gpu_het_sumstats import _reference_counts as pair_counts_ref  # the boolean-product restatement of the counts

# ---------------------------------------------------------------------------------------------------------------------
# the row gather of the .bed (gather_bed_rows_kernel of csrc/corr_index.hip)
# ---------------------------------------------------------------------------------------------------------------------
GATHER_N = (1, 13, 57, 61, 65, 77, 125, 129, 4001)  # rows of 1, 4, 15, 16, 17, 20, 32, 33, 1001 bytes
M_TOTAL = 70
GATHER_P = 3
OFFSETS = (0, 1, 2, 3)  # the byte offset of the .bed inside its device allocation
DWORD = tuple(("dword", sh) for sh in range(4))
CLASSES = DWORD + ("straddle", "bed_end", "dst_tail", "before_first_dword")


def _index_lists():
    inner = np.random.default_rng(17).choice(np.arange(1, M_TOTAL - 1), size=15, replace=False)
    return ((0,), (M_TOTAL - 1,), (0, M_TOTAL - 1), tuple(int(v) for v in np.sort(np.concatenate([[0, M_TOTAL - 1], inner]))),
            tuple(range(M_TOTAL)))


INDEX_LISTS = _index_lists()
GATHER_CASES = [(N, M_TOTAL, ixs, off) for N in GATHER_N for ixs in INDEX_LISTS for off in OFFSETS]


def chunk_classes(clb, ix, bed_bytes, base_mod4):
    """the branch of gather_bed_rows_kernel that writes each 16-byte chunk of the gathered image (len(ix) rows of clb
    bytes), by the kernel's own rule: a chunk inside one row is fetched as aligned dwords and shifted by sh = (address of
    its first source byte) mod 4, unless that fetch would start before the .bed or end past it; a chunk that holds the end
    of a row goes byte by byte ("dst_tail" when it also holds the end of the image)"""
    total = len(ix) * clb
    out = []
    for d0 in range(0, total, 16):
        r, off = divmod(d0, clb)
        if off + 16 <= clb:
            s0 = ix[r] * clb + off
            sh = (base_mod4 + s0) & 3
            if s0 < sh:
                out.append("before_first_dword")
            elif s0 - sh + 20 > bed_bytes:
                out.append("bed_end")
            else:
                out.append(("dword", sh))
        else:
            out.append("dst_tail" if d0 + 16 > total else "straddle")
    return out


_DOSAGE = np.array([2, -1, 1, 0], np.int8)  # 2-bit code 00, 01, 10, 11 -> dosage (01 = missing), inverse of synth._CODE


def decode_bed(bed, N):
    """rows of 2-bit codes, low bits first -> dosages (int8, -1 = missing) of the first N individuals"""
    codes = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(bed.shape[0], -1)[:, :N]
    return _DOSAGE[codes]


@functools.lru_cache(maxsize=None)
def gather_data(N):
    """70 markers x N individuals with all four codes in every row (N >= 4; missing rate 0.2 at N <= 129 so that short
    rows are not monomorphic), three traits (the first complete, the second with gaps), means / sds, the packed rows"""
    from cigwas_amd import synth

    rng = synth.rng_for(7000 + N)
    G = synth.make_genotypes(M_TOTAL, N, rng, window=M_TOTAL, miss=0.2 if N <= 129 else 0.01)
    if N >= 2:  # the first and the last individual are called in every marker (as ref64.make_case has them)
        G[:, 0], G[:, -1] = 0, 2
    if N >= 4:
        for row in G:
            where = 1 + rng.permutation(N - 2)[:4] if N >= 8 else rng.permutation(N)[:4]
            for v, i in zip((0, 1, 2, -1), where):
                if not (row == v).any():
                    row[i] = v
        for row in G:  # a planted value may have overwritten the only call of another
            assert all((row == v).any() for v in (0, 1, 2, -1)) or N < 8
    Y = rng.standard_normal((GATHER_P, N)).astype(np.float32)
    Y[1, rng.random(N) < 0.3] = np.nan
    mean, sd = ref64.stats(G)
    bed = synth.pack_bed(G)
    assert np.array_equal(decode_bed(bed, N), G)
    for a in (G, Y, mean, sd, bed):
        a.setflags(write=False)
    return dict(G=G, Y=Y, mean=mean, sd=sd, bed=bed, phen=Y.reshape(-1))


def test_gather_cases_reach_every_branch():
    seen = {}
    for N, m_total, ixs, off in GATHER_CASES:
        clb = (N + 3) // 4
        seen.setdefault(N, set()).update(chunk_classes(clb, ixs, m_total * clb, off))
    assert set().union(*seen.values()) == set(CLASSES)
    for N in (13, 57):  # rows shorter than a chunk: every chunk holds a row end
        assert not seen[N] & set(DWORD), N
        assert "straddle" in seen[N] and "dst_tail" in seen[N]
    assert seen[1] == {"straddle", "dst_tail"}
    for N in (61, 65, 77):  # rows of 16 to 20 bytes: at most one aligned-dword chunk per row
        assert seen[N] & set(DWORD), N
    assert "bed_end" in seen[61] and "bed_end" in seen[65]  # the only chunk of the last row ends within 4 bytes of the .bed
    assert set(DWORD) <= seen[4001] and set(DWORD) <= seen[129]


def test_chunk_classes_on_hand_examples():
    # two rows of 20 bytes out of three: chunk 0 is row 0 bytes 0-15, chunk 1 straddles, chunk 2 ends the image
    assert chunk_classes(20, (0, 2), 60, 0) == [("dword", 0), "straddle", "dst_tail"]
    assert chunk_classes(20, (0, 2), 60, 3) == ["before_first_dword", "straddle", "dst_tail"]
    assert chunk_classes(20, (1, 2), 60, 1) == [("dword", 1), "straddle", "dst_tail"]
    # one row of 16 bytes, the last of the .bed: an aligned fetch of 20 bytes would pass its end
    assert chunk_classes(16, (2,), 48, 0) == ["bed_end"]
    assert chunk_classes(16, (1,), 48, 2) == [("dword", 2)]
    assert chunk_classes(4, (0, 1, 2, 3, 4), 20, 0) == ["straddle", "dst_tail"]


def _places(N, ixs):
    """(row, byte) of the gathered image to corrupt: its four corners and one byte in a chunk of every class present at
    any offset of the .bed"""
    clb, k = (N + 3) // 4, len(ixs)
    places = {(0, 0): "first byte, first row", (k - 1, 0): "first byte, last row", (0, clb - 1): "last byte, first row",
              (k - 1, clb - 1): "last byte, last row"}
    for off in OFFSETS:
        classes = chunk_classes(clb, ixs, M_TOTAL * clb, off)
        for cls in set(classes):
            c = classes.index(cls)
            places.setdefault(divmod(16 * c, clb), f"{cls} at offset {off}")
            last = min(16 * c + 15, k * clb - 1)  # and the chunk's last byte: with short rows another row than its first
            places.setdefault(divmod(last, clb), f"{cls} at offset {off} (last byte)")
    return places


@pytest.mark.parametrize("N", GATHER_N)
def test_a_wrong_gathered_byte_is_visible(N):
    """What the GPU test compares sees one wrong individual in one gathered byte: the call of one individual of the byte
    toggled between missing and not missing (bits past individual N are never touched: no reader looks at them).  The
    pair counts change; the float64 correlations move by more than their bar wherever they are defined (N >= 5: marker x
    marker where the list has two markers, marker x trait against the suite's 1e-5 where it has one)."""
    d = gather_data(N)
    for ixs in INDEX_LISTS:
        ix = np.array(ixs)
        rows = d["bed"][ix]
        mxp_n, _ = pair_counts_ref(rows, d["phen"], N, GATHER_P)
        G = d["G"][ix]
        iu = np.triu_indices(len(ix), 1)
        R = ref64.mxm(G)[iu] if N >= 5 else None
        r = ref64.mxp(G, d["Y"], d["mean"][ix], d["sd"][ix])[0]
        for (row, byte), what in _places(N, ixs).items():
            bad = rows.copy()
            # of the byte's individuals the first that another marker of the list calls too: a marker pair is taken over
            # the individuals both call, so no correlation between markers can depend on any other
            others = np.delete(G, row, axis=0)
            inds = [i for i in range(4 * byte, min(4 * byte + 4, N)) if len(ix) < 2 or (others[:, i] >= 0).any()]
            assert inds, (ixs, what)
            s = 2 * (inds[0] - 4 * byte)
            code = (bad[row, byte] >> s) & 3
            bad[row, byte] = (bad[row, byte] & ~np.uint8(3 << s)) | np.uint8((0 if code == 1 else 1) << s)
            mxp_bad, _ = pair_counts_ref(bad, d["phen"], N, GATHER_P)
            assert abs(int(mxp_bad[row, 0]) - int(mxp_n[row, 0])) == 1, (ixs, what)  # the complete trait counts every call
            assert not np.array_equal(mxp_bad, mxp_n)
            if N >= 5:
                Gb = decode_bed(bad, N)
                if len(ix) >= 2:
                    assert ref64.moved(R, ref64.mxm(Gb)[iu], ref64.MXM_BAR) > 1, (ixs, what)
                else:
                    assert ref64.moved(r, ref64.mxp(Gb, d["Y"], d["mean"][ix], d["sd"][ix])[0], 1e-5) > 1, (ixs, what)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of the layouts
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    """float32 values as their bit patterns: NaN payloads, the sign of zero and denormals count"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nan_to_zero_ref(a):
    """NaN -> +0.0, every other bit pattern unchanged"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(0.0), a)


def pack_lower_tri_ref(Cm, k):
    """cusk_pack_lower_tri: the lower triangle with diagonal of the leading k x k block, row-major, NaN -> +0.0"""
    return nan_to_zero_ref(np.asarray(Cm)[:k, :k][np.tril_indices(k)])


def pack_adj_bits(G):
    """n x n 0/1 -> n rows of ceil(n / 64) uint64 words, bit j of row i (cusk_result_adj_bits_dev)"""
    G = np.asarray(G)
    n = G.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :n] = G != 0
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, words)


def unpack_adj_bits(rows, n):
    """rows of uint64 words -> 0/1 int32, the first n columns"""
    rows = np.ascontiguousarray(rows, np.uint64)
    return np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(np.int32)


def pack_block_bits_ref(adj_bits, lo, hi, tail=0):
    """cusk_result_adj_bits_blocks (tail = 0) / _tail: per block [lo, hi) its rows -- with tail > 0 the last
    min(tail, hi - lo) of them -- each cut to the ceil((hi - lo) / 64) words of the block's own columns, back to back"""
    out = [np.zeros(0, np.uint64)]
    for l, h in zip(lo, hi):
        l, h = int(l), int(h)
        first = max(l, h - tail) if tail > 0 else l
        out.append(adj_bits[first:h, l // 64:l // 64 + (h - l + 63) // 64].reshape(-1))
    return np.concatenate(out)


def gather_rows_ref(M, idx, row_src, row_k, row_first, row_out, out):
    """cusk_gather_rows into `out` (whatever it holds stays where no row lands)"""
    for src, k, first, o in zip(row_src, row_k, row_first, row_out):
        out[o:o + k] = M[src, idx[first:first + k]]
    return out


NAN = np.float32(np.nan)


def test_pack_lower_tri_ref_on_hand_examples():
    M3 = np.array([[1, 2, 3], [4, NAN, 6], [7, 8, -0.0]], np.float32)
    assert np.array_equal(bits(pack_lower_tri_ref(M3, 3)), bits([1, 4, 0, 7, 8, -0.0]))
    assert np.array_equal(bits(pack_lower_tri_ref(M3, 2)), bits([1, 4, 0]))
    assert bits(pack_lower_tri_ref(M3, 3))[5] == 0x80000000 and bits(pack_lower_tri_ref(M3, 3))[2] == 0
    M5 = np.arange(25, dtype=np.float32).reshape(5, 5)
    assert pack_lower_tri_ref(M5, 5).tolist() == [0, 5, 6, 10, 11, 12, 15, 16, 17, 18, 20, 21, 22, 23, 24]
    assert pack_lower_tri_ref(M5, 3).tolist() == [0, 5, 6, 10, 11, 12]
    neg = np.array([0xFFC12345], np.uint32).view(np.float32)  # a NaN with its sign bit set and a payload
    assert bits(nan_to_zero_ref(neg))[0] == 0 and bits(nan_to_zero_ref(np.float32(1e-45)))[()] == 1


def test_gather_rows_ref_on_a_hand_example():
    M5 = np.arange(25, dtype=np.float32).reshape(5, 5)
    # the 3 x 3 sub-matrix of variables (4, 0, 2) at out[0:9], then row 1 at the columns (3, 1) after a gap of two
    idx = [4, 0, 2, 3, 1]
    out = gather_rows_ref(M5, idx, [4, 0, 2, 1], [3, 3, 3, 2], [0, 0, 0, 3], [0, 3, 6, 11], np.full(14, -1, np.float32))
    assert out.tolist() == [24, 20, 22, 4, 0, 2, 14, 10, 12, -1, -1, 8, 6, -1]


def test_block_bitmap_restatements_on_hand_examples():
    G3 = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
    G5 = np.array([[0, 1, 1, 0, 0], [1, 0, 0, 0, 1], [1, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0]])
    assert pack_adj_bits(G3).tolist() == [[2], [5], [2]] and pack_adj_bits(G5).tolist() == [[6], [17], [9], [4], [2]]
    assert np.array_equal(unpack_adj_bits(pack_adj_bits(G5), 5), G5)
    # the two as blocks at 0 and 64 of one run of 69 variables: two words per row, the second block in word 1
    G = np.zeros((69, 69), np.int32)
    G[:3, :3] = G3
    G[64:, 64:] = G5
    adj = pack_adj_bits(G)
    assert adj.shape == (69, 2) and adj[1].tolist() == [5, 0] and adj[65].tolist() == [0, 17]
    lo, hi = [0, 64], [3, 69]
    assert pack_block_bits_ref(adj, lo, hi).tolist() == [2, 5, 2, 6, 17, 9, 4, 2]
    assert pack_block_bits_ref(adj, lo, hi, tail=2).tolist() == [5, 2, 4, 2]
    assert pack_block_bits_ref(adj, lo, hi, tail=4).tolist() == [2, 5, 2, 17, 9, 4, 2]
    # a block of 65 variables has two words per row
    big = pack_adj_bits(np.ones((65, 65), np.int32))
    assert pack_block_bits_ref(big, [0], [65], tail=1).tolist() == [2 ** 64 - 1, 1]


# ---------------------------------------------------------------------------------------------------------------------
# the matrices of the readout tests
# ---------------------------------------------------------------------------------------------------------------------
READOUT_LEVEL = 3
READOUT_ALPHA = 0.01
# (n, seed, strength of the SEM).  Two variables are one pair, which is kept or removed: n = 2 comes twice, once each
READOUT_CASES = [(2, 2, 1.0), (2, 2, 0.0), (63, 63, 1.0), (64, 64, 1.0), (65, 65, 1.0), (127, 127, 1.0), (128, 128, 1.0),
                 (129, 129, 1.0), (257, 257, 1.0)]
BATCH_SIZES = (1, 63, 64, 65, 130)
BATCH_LO = (0, 64, 128, 192, 384)  # the block of 65 ends at 257: rows 257 .. 383 are unused, 64 more than padding needs
BATCH_N = 576
BATCH_SAMPLES = 600
TAILS = (1, 5, 200)


def readout_samples(n):
    return max(6 * n, 400)


@functools.lru_cache(maxsize=None)
def readout_case(n, seed, strength):
    """(matrix, thresholds, the oracle's skeleton) of one readout case"""
    from cigwas_amd import synth
    from oracle import oracle as O

    O.build()
    Cm = synth.random_corr(n, seed=seed, k=readout_samples(n), strength=strength)
    Th = O.threshold_array(readout_samples(n), READOUT_ALPHA)
    return Cm, Th, O.skeleton(Cm, Th, READOUT_LEVEL)


@functools.lru_cache(maxsize=None)
def batch_case():
    """(the 576 x 576 allocation with NaN outside the blocks, lo, hi, thresholds, the oracle's skeleton per block)"""
    from cigwas_amd import synth
    from oracle import oracle as O

    O.build()
    lo, hi = np.array(BATCH_LO, np.int32), np.array(BATCH_LO, np.int32) + np.array(BATCH_SIZES, np.int32)
    Th = O.threshold_array(BATCH_SAMPLES, READOUT_ALPHA)
    big = np.full((BATCH_N, BATCH_N), np.nan, np.float32)
    refs = []
    for b, (l, k) in enumerate(zip(BATCH_LO, BATCH_SIZES)):
        Cm = synth.random_corr(k, seed=900 + b, k=BATCH_SAMPLES) if k > 1 else np.ones((1, 1), np.float32)
        big[l:l + k, l:l + k] = Cm
        refs.append(O.skeleton(Cm, Th, READOUT_LEVEL))
    return big, lo, hi, Th, refs


def kept_and_removed(G):
    iu = np.triu_indices(G.shape[0], 1)
    return int((G[iu] != 0).sum()), int((G[iu] == 0).sum())


def test_readout_cases_keep_and_remove_pairs():
    both = {}
    for n, seed, strength in READOUT_CASES:
        kept, removed = kept_and_removed(readout_case(n, seed, strength)[2].G)
        assert kept + removed == n * (n - 1) // 2
        if n > 2:
            assert kept > 0 and removed > 0, (n, kept, removed)
        a = both.setdefault(n, [0, 0])
        a[0] += kept
        a[1] += removed
    assert sorted(both) == [2, 63, 64, 65, 127, 128, 129, 257]
    assert all(k > 0 and r > 0 for k, r in both.values()), both
    # removals at level 0 and later (pMax has a level-0 z, a record's z and a zero to get right), some with a set
    for n, seed, strength in READOUT_CASES[2:]:
        ref = readout_case(n, seed, strength)[2]
        assert ref.level >= 1 and (ref.sepset[:, :, 0] >= 0).any(), n


def test_batch_case_layout():
    big, lo, hi, Th, refs = batch_case()
    assert all(l % 64 == 0 for l in lo) and hi[-1] <= BATCH_N and BATCH_N % 64 == 0
    gaps = [int(lo[b + 1]) - (int(hi[b]) + 63) // 64 * 64 for b in range(len(lo) - 1)]
    assert gaps == [0, 0, 0, 64]  # one pair of blocks with unused rows between them
    for k, ref in zip(BATCH_SIZES, refs):
        kept, removed = kept_and_removed(ref.G)
        assert k == 1 or (kept > 0 and removed > 0), k
    # tails of 1 and 5 take all rows of the block of one and a part of the others; 200 takes every row of every block
    assert TAILS == (1, 5, 200) and min(BATCH_SIZES) <= 1 < 5 < sorted(BATCH_SIZES)[1] and max(BATCH_SIZES) < 200
