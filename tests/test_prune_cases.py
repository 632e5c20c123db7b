"""`prune-bed` without a GPU: the pruning rule restated in numpy, the inputs of the GPU tests (tests/test_gpu_prune.py
imports them from here) with the conditions they must meet, the fileset writer, the CLI and the ABI.

The rule (include/cusk_hip.h): markers in order; constant(j) -> status 1; otherwise j is dropped (status 2) when an
earlier KEPT marker i with j - i <= W conflicts with it, else kept (status 0).  A conflict bitmap has one row per marker
of ceil(W / 64) uint64 words, bit b of word k of row i = pair (i, i + 1 + 64 k + b); bits of columns >= W and of pairs
that reach past the last marker mean nothing.

`scan_restated` is the plain loop.  `check_properties` states what its result must satisfy without using it:
  1. no two kept markers within W conflict;
  2. every marker with status 2 conflicts with an earlier kept marker within W;
  3. a marker has status 1 exactly when it is constant.
By induction over j these three determine the statuses, so they are a second statement of the rule.

Conditions on the inputs.  EVERY bitmap case -- random, distance, all ones, garbage, constant flags -- must, under the
restated rule, keep between 20 % and 80 % of its markers, show statuses 0 and 2, and hold a chain a < b < c: a conflicts
with b, b with c, a not with c, statuses kept, dropped, kept; the structured cases assert the pattern they were built
for on top of that.  Two shapes the issue names cannot meet it: one marker has nothing to conflict with (m = 1: kept,
100 %), and two markers hold no chain of three (m = 2: the share and both statuses are asked for, the chain is not).
An all-ones bitmap keeps one marker in W + 1, so only narrow windows are used for it."""
import argparse
import os

import numpy as np
import pytest

from cigwas_amd.cli import prune_argv  # everything below is about this step: without it the module does not load

KEEP, CONSTANT, LD = 0, 1, 2
RANDOM_SHAPES = ((1, 1), (2, 1), (64, 63), (65, 64), (66, 65), (300, 130), (5000, 2000), (10000, 4096))


def nwords(W):
    return (W + 63) // 64


def row_cols(bits, i, m, W):
    """the columns c of row i that count: bit set, c < W, i + 1 + c < m"""
    limit = min(W, m - 1 - i)
    if limit <= 0:
        return np.zeros(0, np.int64)
    unpacked = np.unpackbits(np.ascontiguousarray(bits[i]).view(np.uint8), bitorder="little")
    return np.flatnonzero(unpacked[:limit])


def scan_restated(bits, const, m, W):
    status = np.zeros(m, np.uint8)
    blocked = [False] * m
    for j in range(m):
        if const[j]:
            status[j] = CONSTANT
        elif blocked[j]:
            status[j] = LD
        else:
            status[j] = KEEP
            for c in row_cols(bits, j, m, W):
                blocked[j + 1 + int(c)] = True
    return status


def check_properties(bits, const, m, W, status):
    status = np.asarray(status)
    assert status.shape == (m,) and np.all(status <= LD)
    kept = status == KEEP
    reached = np.zeros(m, bool)  # conflicts with an earlier kept marker within W
    for i in np.flatnonzero(kept):
        later = i + 1 + row_cols(bits, i, m, W)
        assert not kept[later].any(), ("two kept markers conflict", i)
        reached[later] = True
    assert reached[status == LD].all(), "a marker was dropped without a kept marker that conflicts with it"
    assert np.array_equal(status == CONSTANT, np.asarray(const) != 0)


def conflict(bits, i, j, m, W):
    if not (0 < j - i <= W) or j >= m:
        return False
    c = int(j) - int(i) - 1
    return bool((int(bits[i, c >> 6]) >> (c & 63)) & 1)


def has_chain(bits, m, W, status):
    kept = status == KEEP
    for b in np.flatnonzero(status == LD):
        cs = [int(b + 1 + c) for c in row_cols(bits, b, m, W) if kept[b + 1 + c]]
        if not cs:
            continue
        for a in range(max(0, b - W), b):
            if kept[a] and conflict(bits, a, b, m, W):
                if any(not conflict(bits, a, c, m, W) for c in cs):
                    return True
    return False


def clean(bits, m, W):
    """the bitmap with every bit that means nothing set to 0"""
    out = np.zeros_like(bits)
    for i in range(m):
        for c in row_cols(bits, i, m, W):
            out[i, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    return out


def with_garbage(bits, m, W):
    """every bit that means nothing set to 1: columns >= W of the last word, pairs that reach past the last marker"""
    out = np.full_like(bits, ~np.uint64(0))
    valid = np.zeros_like(bits)
    for i in range(m):
        limit = min(W, m - 1 - i)
        for k in range(nwords(W)):
            n = min(64, limit - 64 * k)
            if n > 0:
                valid[i, k] = ~np.uint64(0) if n == 64 else (np.uint64(1) << np.uint64(n)) - np.uint64(1)
    return (bits & valid) | (out & ~valid)


def random_bits(m, W, seed):
    """independent bits; the density makes a marker with W / 2 kept predecessors free of conflicts half of the time"""
    p = 1.0 - 2.0 ** (-2.0 / min(W, max(m - 1, 1)))
    rng = np.random.default_rng(seed)
    dense = rng.random((m, 64 * nwords(W)), dtype=np.float32) < np.float32(p)
    return clean(np.packbits(dense, axis=1, bitorder="little").view(np.uint64).reshape(m, nwords(W)), m, W)


def meets_condition(bits, const, m, W, status):
    share = np.mean(status == KEEP)
    if m == 1:
        return True
    ok = 0.2 <= share <= 0.8 and (status == KEEP).any() and (status == LD).any()
    return ok and (m == 2 or has_chain(bits, m, W, status))


_CASES = None


def scan_cases():
    """name -> (bits, const, m, W, kind); built once, never modified (the arrays are read-only)"""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = {}

    def add(name, bits, const, m, W, kind):
        bits = np.ascontiguousarray(bits, np.uint64).reshape(m, nwords(W))
        const = np.ascontiguousarray(const, np.uint8)
        bits.setflags(write=False)
        const.setflags(write=False)
        cases[name] = (bits, const, m, W, kind)

    for m, W in RANDOM_SHAPES:
        for seed in range(50):  # the first seed whose bitmap meets the condition; the test asserts that one did
            bits = random_bits(m, W, 1000 * m + seed)
            if meets_condition(bits, np.zeros(m, np.uint8), m, W, scan_restated(bits, np.zeros(m, np.uint8), m, W)):
                break
        add(f"random_m{m}_W{W}", bits, np.zeros(m, np.uint8), m, W, "random")
    for m, W in ((3, 200), (50, 64), (100, 4096)):  # W >= m
        for seed in range(50):
            bits = random_bits(m, W, 77 * m + seed)
            if meets_condition(bits, np.zeros(m, np.uint8), m, W, scan_restated(bits, np.zeros(m, np.uint8), m, W)):
                break
        add(f"wide_m{m}_W{W}", bits, np.zeros(m, np.uint8), m, W, "random")
    # a conflict at distance exactly W drops, and the bit one column further (column W of the last word: it would be
    # distance W + 1) is outside the window and drops nothing -- both planted into a random background that meets the
    # condition: (0, W) is the only conflict of marker W with a kept marker, and the stray bit sits in the row of a kept
    # marker i whose marker i + W + 1 is kept
    for W in (1, 63, 70, 130):
        m = 3 * W + 10
        assert W % 64  # column W exists in the last word
        for seed in range(200):
            bits = random_bits(m, W, 500 * W + seed).copy()
            for a in range(1, W):
                c = W - a - 1  # pair (a, W)
                bits[a, c >> 6] &= ~(np.uint64(1) << np.uint64(c & 63))
            bits[0, (W - 1) >> 6] |= np.uint64(1) << np.uint64((W - 1) & 63)  # (0, W)
            st = scan_restated(bits, np.zeros(m, np.uint8), m, W)
            rows = [a for a in np.flatnonzero(st == KEEP) if a + W + 1 < m and st[a + W + 1] == KEEP]
            if rows and meets_condition(bits, np.zeros(m, np.uint8), m, W, st):
                break
        stray = int(rows[0])
        bits[stray, W >> 6] |= np.uint64(1) << np.uint64(W & 63)
        add(f"distance_W{W}", bits, np.zeros(m, np.uint8), m, W, f"distance:{stray}")
    # all ones: a kept marker decides the W after it, so 1 / (W + 1) of the markers are kept; only W <= 4 can meet the
    # 20 % of the condition, and wider all-ones rows come in as garbage (below) instead
    for m, W in ((200, 1), (200, 3)):
        add(f"ones_m{m}_W{W}", clean(np.full((m, nwords(W)), ~np.uint64(0)), m, W), np.zeros(m, np.uint8), m, W, "ones")
    for name in ("random_m65_W64", "random_m300_W130", "random_m5000_W2000", "wide_m50_W64", "ones_m200_W3", "distance_W70"):
        bits, const, m, W, _ = cases[name]
        add("garbage_" + name, with_garbage(bits, m, W), const, m, W, "garbage:" + name)
    # constant flags on markers that the plain run keeps and that block others
    for name in ("random_m300_W130", "random_m5000_W2000", "ones_m200_W3"):
        bits, _, m, W, _ = cases[name]
        plain = scan_restated(bits, np.zeros(m, np.uint8), m, W)
        blockers = [i for i in np.flatnonzero(plain == KEEP) if len(row_cols(bits, i, m, W))]
        const = np.zeros(m, np.uint8)
        const[blockers[::3]] = 1
        const[m // 2] = 7  # any non-zero byte is a flag
        add("constant_" + name, bits, const, m, W, "constant:" + name)
    _CASES = cases
    return cases


_EXPECTED = {}


def expected(name):
    if name not in _EXPECTED:
        bits, const, m, W, _ = scan_cases()[name]
        st = scan_restated(bits, const, m, W)
        st.setflags(write=False)
        _EXPECTED[name] = st
    return _EXPECTED[name]


def case_names():
    return sorted(scan_cases())


@pytest.mark.parametrize("name", case_names())
def test_restated_rule_satisfies_the_properties_and_the_case_conditions(name):
    bits, const, m, W, kind = scan_cases()[name]
    st = expected(name)
    check_properties(bits, const, m, W, st)
    assert meets_condition(bits, const, m, W, st), (name, float(np.mean(st == KEEP)))  # every case, whatever its kind
    if kind == "random":
        if m == 1:
            assert list(st) == [KEEP]
    elif kind.startswith("distance:"):
        stray = int(kind.split(":")[1])
        assert st[0] == KEEP and conflict(bits, 0, W, m, W) and st[W] == LD
        assert not any(st[a] == KEEP and conflict(bits, a, W, m, W) for a in range(1, W))  # distance W alone drops it
        assert (int(bits[stray, W >> 6]) >> (W & 63)) & 1 and st[stray] == KEEP and st[stray + W + 1] == KEEP
    elif kind == "ones":
        want = np.where(np.arange(m) % (W + 1) == 0, KEEP, LD)  # chains all along: a and c are W + 1 apart
        assert np.array_equal(st, want)
    elif kind.startswith("garbage:"):
        base = kind.split(":")[1]
        assert not np.array_equal(bits, scan_cases()[base][0])
        assert np.array_equal(st, expected(base))
    elif kind.startswith("constant:"):
        base = expected(kind.split(":")[1])
        assert (st == CONSTANT).sum() == np.count_nonzero(const) > 1
        assert np.any((base == LD) & (st == KEEP)), "no marker came back when its blocker became constant"


def test_the_properties_reject_wrong_results():
    bits, const, m, W, _ = scan_cases()["random_m300_W130"]
    st = expected("random_m300_W130").copy()
    j = int(np.flatnonzero(st == LD)[0])
    st[j] = KEEP
    with pytest.raises(AssertionError):
        check_properties(bits, const, m, W, st)
    st = expected("random_m300_W130").copy()
    free = [i for i in np.flatnonzero(st == KEEP) if i > 0 and not any(conflict(bits, a, i, m, W) for a in range(max(0, i - W), i))]
    st[free[0]] = LD
    with pytest.raises(AssertionError):
        check_properties(bits, const, m, W, st)


# ---------------------------------------------------------------------------------------------------------------------
# genotypes: packing, counts and the planted sets of the composed GPU tests
# ---------------------------------------------------------------------------------------------------------------------
CODE_OF = np.array([3, 2, 0, 1], np.uint8)  # dosage 0, 1, 2, missing (-1) -> .bed code 11, 10, 00, 01


def pack_bed(g, pad_code=0):
    """g: (m, N) int, dosages 0 / 1 / 2 and -1 for missing -> (m, ceil(N / 4)) bytes; padding codes = pad_code"""
    m, N = g.shape
    codes = np.full((m, (N + 3) // 4 * 4), pad_code, np.uint8)
    codes[:, :N] = CODE_OF[g]
    codes = codes.reshape(m, -1, 4)
    return (codes[:, :, 0] | (codes[:, :, 1] << 2) | (codes[:, :, 2] << 4) | (codes[:, :, 3] << 6)).astype(np.uint8)


def counts_restated(bed, m, N):
    bed = np.asarray(bed, np.uint8).reshape(m, -1)
    codes = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(m, -1)[:, :N]
    return np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.int32)


def constant_restated(counts):
    return ((counts[:, [0, 2, 3]] > 0).sum(axis=1) <= 1).astype(np.uint8)


def planted_genotypes(m, N, W, seed):
    """independent markers with planted structure where it fits: exact duplicates, complements (2 - g), near-duplicates,
    constants (one genotype, one genotype beside missing calls, all missing), chains of near-duplicates, and duplicates
    at distances W and W + 1"""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.15, 0.5, m)
    g = (rng.random((m, N, 2)) < maf[:, None, None]).sum(axis=2).astype(np.int64)
    g[rng.random((m, N)) < 0.02] = -1

    def near(src, flips):
        out = src.copy()
        at = rng.choice(N, size=min(flips, N), replace=False)
        out[at] = rng.integers(0, 3, len(at))
        return out

    def comp(src):
        return np.where(src < 0, -1, 2 - src)

    plan = [(3, 4, "dup"), (10, 12, "comp"), (20, 21, "near"), (30, 30 + W, "dup"), (31 + W + 40, 31 + 2 * W + 41, "dup"),
            (200, 203, "dup"), (203, 207, "comp"), (300, 301, "near"), (301, 302, "near"), (400, 400 + W, "comp")]
    for a, b, what in plan:
        if b < m:
            g[b] = g[a] if what == "dup" else comp(g[a]) if what == "comp" else near(g[a], max(1, N // 60))
    for j, what in ((1, 0), (7, 2), (50, 1), (64, -1), (150, "one+missing"), (m - 1, 0)):
        if 0 <= j < m and m > 2:
            if what == "one+missing":
                g[j] = np.where(rng.random(N) < 0.3, -1, 1)
            else:
                g[j] = what
    return g


def threshold_bits(band, m, W, r_max):
    """the conflict bitmap of a float32 band (m, W): |r| >= r_max in float32, NaN gives no conflict"""
    with np.errstate(invalid="ignore"):
        hit = np.abs(np.asarray(band, np.float32).reshape(m, W)) >= np.float32(r_max)
    dense = np.zeros((m, 64 * nwords(W)), bool)
    dense[:, :W] = hit
    return np.packbits(dense, axis=1, bitorder="little").view(np.uint64).reshape(m, nwords(W))


def test_counts_restated_on_a_hand_made_row():
    g = np.array([[2, -1, 1, 0, 0, 1, 1]])
    bed = pack_bed(g)
    assert bed.tolist() == [[0b11100100, 0b00101011]]
    assert counts_restated(bed, 1, 7).tolist() == [[1, 1, 3, 2]]
    assert counts_restated(pack_bed(g, pad_code=2), 1, 7).tolist() == [[1, 1, 3, 2]]  # padding is nobody
    c = counts_restated(pack_bed(np.array([[1, 1, -1], [-1, -1, -1], [0, 2, 2], [0, 1, -1]])), 4, 3)
    assert constant_restated(c).tolist() == [1, 1, 0, 0]


def test_threshold_bits_layout_and_nan():
    band = np.zeros((3, 70), np.float32)
    band[0, 0], band[0, 64], band[1, 69], band[2, 5] = 1.0, -0.95, 0.9, np.nan
    bits = threshold_bits(band, 3, 70, 0.9)
    assert bits.tolist() == [[1, 1], [0, 1 << 5], [0, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# cusk_prune_write
# ---------------------------------------------------------------------------------------------------------------------
def write_fileset(stem, bed, N, chr_ids):
    m = bed.shape[0]
    with open(stem + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]) + np.ascontiguousarray(bed, np.uint8).tobytes())
    with open(stem + ".bim", "w") as f:
        for i in range(m):
            f.write(f"{chr_ids[i]}\trs{i}_{chr_ids[i]}\t0\t{1000 + 7 * i}\tA\tG\n")
    with open(stem + ".fam", "w") as f:
        for i in range(N):
            f.write(f"f{i} i{i} 0 0 {1 + i % 2} -9\n")


def read_all(stem, suffixes=(".bed", ".bim", ".fam", ".prune.in", ".prune.out")):
    return {s: open(stem + s, "rb").read() for s in suffixes}


def check_pruned_fileset(src, out, bed, status):
    """<out>.* is what the specification says for the fileset <src> (rows `bed`) and `status`"""
    got = read_all(out)
    kept = np.flatnonzero(np.asarray(status) == KEEP)
    assert got[".bed"] == bytes([0x6C, 0x1B, 0x01]) + np.ascontiguousarray(bed[kept], np.uint8).tobytes()
    lines = open(src + ".bim", "rb").read().splitlines(keepends=True)
    assert got[".bim"] == b"".join(lines[i] for i in kept)
    assert got[".fam"] == open(src + ".fam", "rb").read()
    ids = [ln.split()[1].decode() for ln in lines]
    assert got[".prune.in"].decode() == "".join(ids[i] + "\n" for i in kept)
    word = {CONSTANT: "constant", LD: "ld"}
    assert got[".prune.out"].decode() == "".join(f"{ids[i]}\t{word[int(s)]}\n" for i, s in enumerate(status) if s != KEEP)


def test_prune_write_files(tmp_path):
    import cigwas_amd as cg

    m, N = 23, 13
    rng = np.random.default_rng(5)
    bed = rng.integers(0, 256, (m, (N + 3) // 4), dtype=np.uint8)
    chr_ids = ["1"] * 9 + ["2"] * 14
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    write_fileset(src, bed, N, chr_ids)
    status = rng.integers(0, 3, m).astype(np.uint8)
    assert set(status) == {0, 1, 2}
    cg.prune_write(src, out, status)
    check_pruned_fileset(src, out, bed, status)
    # nothing kept, everything kept
    for st in (np.full(m, LD, np.uint8), np.zeros(m, np.uint8)):
        cg.prune_write(src, out, st)
        check_pruned_fileset(src, out, bed, st)
    assert read_all(out, (".bed", ".bim", ".fam")) == read_all(src, (".bed", ".bim", ".fam"))


def test_prune_write_refusals(tmp_path):
    from cigwas_amd._lib import lib

    f = lib().cusk_prune_write
    m, N = 6, 9
    bed = np.arange(m * 3, dtype=np.uint8).reshape(m, 3)
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    write_fileset(src, bed, N, ["1"] * m)
    before = read_all(src, (".bed", ".bim", ".fam"))
    status = np.array([0, 2, 0, 1, 0, 0], np.uint8)
    ptr = status.ctypes.data

    def untouched():
        return read_all(src, (".bed", ".bim", ".fam")) == before and sorted(os.listdir(tmp_path)) == ["in.bed", "in.bim", "in.fam"]

    assert f(src.encode(), src.encode(), ptr, m) != 0 and untouched()  # out == bfiles
    assert f(src.encode(), out.encode(), ptr, m - 1) != 0 and untouched()  # not one status per line of the .bim
    assert f(src.encode(), out.encode(), ptr, 0) != 0 and untouched()
    assert f(None, out.encode(), ptr, m) != 0 and f(src.encode(), None, ptr, m) != 0 and f(src.encode(), out.encode(), None, m) != 0
    assert f((src + "_absent").encode(), out.encode(), ptr, m) != 0 and untouched()
    bad = status.copy()
    bad[2] = 3
    assert f(src.encode(), out.encode(), bad.ctypes.data, m) != 0 and untouched()
    os.mkdir(tmp_path / "dir.bed")  # a stem whose .bed cannot be opened for writing
    assert f(src.encode(), str(tmp_path / "dir").encode(), ptr, m) != 0
    assert read_all(src, (".bed", ".bim", ".fam")) == before
    assert f(src.encode(), out.encode(), ptr, m) == 0
    check_pruned_fileset(src, out, bed, status)


def test_prune_write_refuses_other_spellings_of_the_input_and_cleans_up_after_a_failure(tmp_path):
    from cigwas_amd._lib import lib

    f = lib().cusk_prune_write
    m, N = 6, 9
    bed = np.arange(m * 3, dtype=np.uint8).reshape(m, 3)
    os.mkdir(tmp_path / "d")
    src = str(tmp_path / "d" / "in")
    write_fileset(src, bed, N, ["1"] * m)
    before = read_all(src, (".bed", ".bim", ".fam"))
    status = np.array([0, 2, 0, 1, 0, 0], np.uint8)
    # the same stem spelled differently, and a stem whose .bim is a link to the input's
    other = str(tmp_path / "d" / ".." / "d" / "in")
    assert other != src and f(src.encode(), other.encode(), status.ctypes.data, m) == 2
    link = str(tmp_path / "lnk")
    os.symlink(src + ".bim", link + ".bim")
    assert f(src.encode(), link.encode(), status.ctypes.data, m) == 2
    assert read_all(src, (".bed", ".bim", ".fam")) == before
    assert sorted(os.listdir(tmp_path)) == ["d", "lnk.bim"] and sorted(os.listdir(tmp_path / "d")) == ["in.bed", "in.bim", "in.fam"]
    os.remove(link + ".bim")
    # a failure after the outputs were opened (the .prune.out cannot be created) leaves none of them behind
    out = str(tmp_path / "out")
    os.mkdir(out + ".prune.out")
    assert f(src.encode(), out.encode(), status.ctypes.data, m) != 0
    assert sorted(os.listdir(tmp_path)) == ["d", "out.prune.out"]
    os.rmdir(out + ".prune.out")
    # a last .bim line without a newline is copied as it is
    with open(src + ".bim", "rb") as fh:
        text = fh.read()
    with open(src + ".bim", "wb") as fh:
        fh.write(text[:-1])
    for st in (status, np.array([0, 2, 0, 1, 0, 2], np.uint8)):
        assert f(src.encode(), out.encode(), st.ctypes.data, m) == 0
        check_pruned_fileset(src, out, bed, st)
    assert not open(out + ".bim", "rb").read().endswith(b"G")  # the last line was dropped: every kept line has its newline
    assert f(src.encode(), out.encode(), status.ctypes.data, m) == 0
    assert open(out + ".bim", "rb").read().endswith(b"G")


# ---------------------------------------------------------------------------------------------------------------------
# CLI and ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_prune_argv_default_window_and_ranges(capsys, tmp_path):
    from cigwas_amd import cli

    parser = cli.build_parser()
    args = parser.parse_args(["prune-bed", "in/stem", "out/stem", "--r-max", "0.9"])
    assert args.window == 2000 and args.func is cli.prune_bed
    assert prune_argv is cli.prune_argv
    assert cli.prune_argv(args) == [cli.MPS_PATH, "prune", "in/stem", "out/stem", "0.9", "2000"]
    args = parser.parse_args(["prune-bed", "a", "b", "--r-max", "1", "--window", "4096"])
    assert cli.prune_argv(args) == [cli.MPS_PATH, "prune", "a", "b", "1.0", "4096"]
    block_default = parser.parse_args(["block", "a", "100", "10", "2000"]).corr_width
    assert args.window != block_default and parser.parse_args(["prune-bed", "a", "b", "--r-max", "1"]).window == block_default
    # 0 passes the range check and is refused with a message of its own
    zero = parser.parse_args(["prune-bed", "a", "b", "--r-max", "0"])
    with pytest.raises(SystemExit) as ex:
        cli.prune_argv(zero)
    assert "--r-max 0" in str(ex.value.code)
    with pytest.raises(SystemExit) as ex:
        cli.prune_argv(parser.parse_args(["prune-bed", "a", "a", "--r-max", "0.5"]))
    assert "differ" in str(ex.value.code)
    stem = str(tmp_path / "s")
    write_fileset(stem, np.zeros((1, 1), np.uint8), 2, ["1"])
    with pytest.raises(SystemExit) as ex:
        cli.prune_argv(parser.parse_args(["prune-bed", stem, os.path.join(str(tmp_path), ".", "s"), "--r-max", "0.5"]))
    assert "differ" in str(ex.value.code)
    for bad in (["--r-max", "1.01"], ["--r-max", "-0.1"], [], ["--r-max", "0.5", "--window", "0"],
                ["--r-max", "0.5", "--window", "4097"]):
        with pytest.raises(SystemExit) as ex:
            parser.parse_args(["prune-bed", "a", "b"] + bad)
        assert ex.value.code == 2
    capsys.readouterr()
    assert isinstance(args, argparse.Namespace)


def test_mps_prune_usage_and_argument_checks(tmp_path):
    import subprocess

    from cigwas_amd import cli

    r = subprocess.run([cli.MPS_PATH, "prune"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: mps prune <bfiles> <out-stem> <r-max> <window>" in r.stdout
    assert "prune" in subprocess.run([cli.MPS_PATH], capture_output=True, text=True).stdout
    stem = str(tmp_path / "x")
    write_fileset(stem, np.zeros((2, 1), np.uint8), 4, ["1", "1"])
    for argv, msg in ((["prune", stem, stem + "o", "0", "10"], "r-max"), (["prune", stem, stem + "o", "1.5", "10"], "r-max"),
                      (["prune", stem, stem + "o", "0.5", "0"], "window"), (["prune", stem, stem + "o", "0.5", "4097"], "window"),
                      (["prune", stem, stem, "0.5", "10"], "differ"), (["prune", stem, os.path.join(str(tmp_path), ".", "x"), "0.5", "10"], "differ"), (["prune", stem + "none", stem + "o", "0.5", "10"], "not found"),
                      (["prune", stem, stem + "o", "abc", "10"], "numbers")):
        r = subprocess.run([cli.MPS_PATH] + argv, capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr, (argv, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["x.bed", "x.bim", "x.fam"]


def test_abi_symbols_resolve():
    import ctypes as C

    from cigwas_amd import _lib

    L = _lib.lib()
    for name in ("cusk_genotype_counts", "cusk_ld_prune_scan", "cusk_ld_prune", "cusk_prune_write"):
        assert name in _lib.SYMBOLS and getattr(L, name).restype is C.c_int
    assert "cusk_ld_prune_timing" in _lib.SYMBOLS and L.cusk_ld_prune_timing.restype is None
    ms = np.full(5, -1.0, np.float32)
    L.cusk_ld_prune_timing(None, ms.ctypes.data)  # no engine: nothing is written
    assert np.all(ms == -1.0)
    # a call without an engine is an argument error, not a crash
    out = np.zeros(4, np.int32)
    bed = np.zeros(1, np.uint8)
    assert L.cusk_genotype_counts(None, bed.ctypes.data, 1, 4, out.ctypes.data) == 2
    assert L.cusk_ld_prune(None, bed.ctypes.data, 1, 4, 1, 0.5, out.ctypes.data, None) == 2
    assert L.cusk_ld_prune_scan(None, out.ctypes.data, bed.ctypes.data, 1, 1, out.ctypes.data) == 2
    from cigwas_amd.skeleton import Engine

    for name in ("genotype_counts", "ld_prune_scan", "ld_prune"):
        assert callable(getattr(Engine, name))
