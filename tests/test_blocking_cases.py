"""The inputs of tests/test_gpu_blocking.py and of the banded / `mps block` cases added to tests/test_gpu_mps.py, checked on
the oracle alone (no GPU): the row-sum profiles and maximum block sizes make the window bisection of block_chr leave through
both of its exits and move in both directions, every pair gives a cover of 0 .. n-1, the oracle answers each of them the
same way twice (NaN weights and NaN profiles included), and the banded shapes have entries inside and past the chromosome."""
import numpy as np
import pytest

from test_oracle_vs_ref import BLOCKING_CASES, BLOCKING_WINDOWS, blocking_case, ref  # noqa: F401  (ref: the fixture)

TOL = 100  # MAX_BLOCK_SIZE_TOL of the reference's blocking.cpp
RANDOM_NS = (1, 2, 3, 4, 5, 6, 7, 100, 101, 1000)
EDGE_NS = (8, 301)
EDGE_KINDS = ("constant", "increasing", "decreasing", "sawtooth", "nan", "zeros")

# cusk_corr_banded launches (width + 63) / 64 + 1 band tiles per 64-row tile: (m, N, width) where that count and the
# clamps at the last marker change -- width 1, m below / at / just past one and two tiles, widths around 64 and 128, a band
# that reaches past the last marker in every row (width >= m - 1)
BANDED_EDGE_CASES = [(1, 64, 1), (5, 200, 1), (5, 200, 5), (40, 256, 64), (64, 256, 63), (64, 320, 65), (128, 192, 127),
                     (129, 192, 128), (200, 100, 199)]

# `mps block` at small chromosomes: sizes and ids in .bim order (not sorted by id), N no multiple of 64
SMALL_CHROMOSOMES = [("7", 3), ("2", 64), ("11", 65), ("1", 400)]
SMALL_N, SMALL_WIDTH, SMALL_MAXB = 130, 2, 50


def small_blocking_case(seed, n):
    """test_oracle_vs_ref.blocking_case for any n >= 1.  That generator draws its dip centres from [50, n - 50) and so
    needs n > 100; up to there this one draws three centres from [0, n) and is the same otherwise."""
    if n > 100:
        return blocking_case(seed, n)
    rng = np.random.default_rng(100 + seed)
    base = 20.0 + 10.0 * np.sin(np.arange(n) / 37.0) + 5.0 * np.sin(np.arange(n) / 211.0 + seed)
    dips = np.ones(n)
    for c in rng.integers(0, n, size=3):
        dips[max(0, c - 15): c + 15] *= rng.uniform(0.2, 0.6)
    return (base * dips + rng.normal(0.0, 0.8, n)).astype(np.float32)


def edge_profile(kind, n):
    i = np.arange(n)
    if kind == "constant":  # no strict minimum: one block
        v = np.full(n, 7.5)
    elif kind == "increasing":
        v = 1.0 + 0.25 * i
    elif kind == "decreasing":
        v = 1.0 + 0.25 * i[::-1]
    elif kind == "sawtooth":  # period 2: every interior point is an extremum
        v = np.where(i % 2 == 1, 3.0, 1.0)
    elif kind == "nan":  # row sums are NaN for monomorphic markers: single ones, a run, both ends
        v = small_blocking_case(7, n).astype(np.float64)
        v[[0, n // 3, n // 2, n // 2 + 1, n - 1]] = np.nan
    elif kind == "zeros":
        v = np.zeros(n)
    else:
        raise KeyError(kind)
    return v.astype(np.float32)


def max_block_sizes(n):
    """1, a value between, n, and one more than 100 above n (never within the tolerance); at the long profiles also values
    that no window satisfies from either side at once, so that the search turns round (checked below)"""
    return sorted({1, max(2, n // 6), n, n + 101} | ({2 * n // 5, n // 2} if n == 1000 else {2 * n // 3, n - 1} if n == 301 else set()))


def profiles():
    """name -> float32 row-sum profile"""
    out = {f"random{n}": small_blocking_case(n % 13, n) for n in RANDOM_NS}
    for kind in EDGE_KINDS:
        for n in EDGE_NS:
            out[f"{kind}{n}"] = edge_profile(kind, n)
    return out


def cases():
    return [(name, v, maxb) for name, v in profiles().items() for maxb in max_block_sizes(len(v))]


def smooth_restated(v, w):
    """hanning_smoothing as cusk_hanning_smooth states it, in numpy: the window walked in order, one double multiply and
    one double add per step (numpy does not fuse them); 0 outside [margin, n - margin)"""
    n, window = len(v), len(w)
    margin = window // 2
    acc = np.zeros(n, np.float64)
    if n - 2 * margin <= 0:  # no centre; the slices below would wrap
        return acc
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(window):
            acc[margin:n - margin] += w[i] * v[i:i + n - 2 * margin].astype(np.float64)
    return acc


def is_cover(blocks, n):
    """the blocks cover 0 .. n-1 exactly once, in order"""
    return (len(blocks) > 0 and blocks[0][0] == 0 and blocks[-1][1] == n - 1 and all(a <= b for a, b in blocks)
            and all(blocks[k + 1][0] == blocks[k][1] + 1 for k in range(len(blocks) - 1)))


def exit_kind(blocks, maxb):
    """how block_chr left its loop, read from its result: it returns the blocks of the last window it tried, and it stops
    on them either because the largest is within the tolerance of (and not above) maxb, or because the window stalled"""
    largest = max(b - a + 1 for a, b in blocks)
    return "tolerance" if (abs(largest - maxb) <= TOL and largest <= maxb) else "window"


def trace_block_chr(oracle, v, maxb):
    """block_chr restated over oracle.hanning_smoothing, recording the windows tried: (blocks, windows)"""
    def cut(s):
        blocks, start, left = [], 0, 0.0
        for i in range(1, len(s) - 1):
            if left > s[i] and s[i] < s[i + 1]:
                blocks.append((start, i))
                start, left = i + 1, 0.0
            elif s[i] > left:
                left = s[i]
        return blocks + [(start, len(s) - 1)]

    def odd(w):
        return w - 1 if w % 2 == 0 else w

    hi, lo = len(v), 3
    window = odd((hi + lo) // 2)
    windows = [window]
    res = cut(oracle.hanning_smoothing(v, window))
    while True:
        largest = max(b - a + 1 for a, b in res)
        if not (abs(largest - maxb) > TOL or largest > maxb):
            break
        if largest > maxb:
            hi = min(hi, window)
        else:
            lo = max(lo, window)
        nxt = odd((hi + lo) // 2)
        if nxt == window:
            break
        window = nxt
        windows.append(window)
        res = cut(oracle.hanning_smoothing(v, window))
    return res, windows


@pytest.fixture(scope="module")
def oracle_results(oracle):
    return {(name, maxb): oracle.block_chr(v, maxb) for name, v, maxb in cases()}


def test_oracle_answers_every_case_and_covers(oracle, oracle_results):
    """every (profile, maximum) pair, n = 1 and 2 (window 1, NaN weight) and the NaN profiles included, gets the same
    answer from the oracle on a second call, and the answer is a cover"""
    for name, v, maxb in cases():
        got = oracle_results[(name, maxb)]
        assert got == oracle.block_chr(v.copy(), maxb), (name, maxb)
        assert is_cover(got, len(v)), (name, maxb, got)


def test_cases_take_both_exits_and_both_directions(oracle, oracle_results):
    """the bisection leaves through the tolerance and through the stalled window (`next == window`), each of them at the
    first window, after only lowering the upper bound, after only raising the lower one, and after turning round"""
    paths = set()
    for name, v, maxb in cases():
        blocks, windows = trace_block_chr(oracle, v, maxb)
        assert blocks == oracle_results[(name, maxb)], (name, maxb)  # the trace is the oracle's search
        d = [b - a for a, b in zip(windows, windows[1:])]
        paths.add((exit_kind(blocks, maxb), any(x < 0 for x in d), any(x > 0 for x in d)))
    # (exit, the window went down, the window went up): every combination
    assert paths == {(kind, down, up) for kind in ("tolerance", "window") for down in (False, True) for up in (False, True)}
    # a stall between the bounds, not at 3 or at n: the largest block stays more than the tolerance below the maximum
    blocks, windows = trace_block_chr(oracle, profiles()["random1000"], 500)
    assert exit_kind(blocks, 500) == "window" and 3 < windows[-1] < 999 and len(windows) > 5


def test_edge_profiles_are_what_they_claim(oracle_results):
    for n in EDGE_NS:
        for maxb in max_block_sizes(n):
            # no strict minimum anywhere: one block whatever the maximum
            assert oracle_results[(f"constant{n}", maxb)] == [(0, n - 1)]
            assert oracle_results[(f"zeros{n}", maxb)] == [(0, n - 1)]
        assert np.isnan(edge_profile("nan", n)).sum() == 5
        saw = edge_profile("sawtooth", n)
        assert all((saw[i] - saw[i - 1]) * (saw[i + 1] - saw[i]) < 0 for i in range(1, n - 1))
        assert np.all(np.diff(edge_profile("increasing", n)) > 0) and np.all(np.diff(edge_profile("decreasing", n)) < 0)
    # some profile is cut into several blocks at every n from 5 on
    for n in RANDOM_NS:
        if n >= 100:
            assert len(oracle_results[(f"random{n}", 1)]) > 1


def test_weights_accessor(ref):
    """cusk_hanning_weights (host only): its arguments, the ends of the window, the single-precision cosine; and with the
    restated loop these weights give the curves the reference's own blocking.cpp recorded, bit for bit -- which also
    shows that the restated loop is the reference's operation order"""
    import ctypes as C

    import cigwas_amd as cg
    from cigwas_amd._lib import lib

    f = lib().cusk_hanning_weights
    out = np.full(4, -777.0)
    p = out.ctypes.data_as(C.c_void_p)
    assert f(0, p) != 0 and f(-1, p) != 0 and f(3, None) != 0 and np.all(out == -777.0)
    assert f(3, p) == 0 and list(out) == [0.0, 1.0, 0.0, -777.0]  # cosf(0) = cosf((float)(2 pi)) = 1, cosf((float)pi) = -1
    assert np.isnan(cg.hanning_weights(1)).all()  # 0 / 0, as in the reference
    for window in (2, 5, 101, 333):
        w = cg.hanning_weights(window)
        assert w.shape == (window,) and w[0] == 0 and np.all((w >= 0) & (w <= 1))
        cos = (0.5 - w) * 2  # exact: every weight is 0.5 - 0.5 * (a float32)
        assert np.array_equal(cos, cos.astype(np.float32).astype(np.float64))
    for seed, n, _ in BLOCKING_CASES:
        v = ref[f"blocking/{seed}/v"]
        for ws in BLOCKING_WINDOWS:
            got = smooth_restated(v, cg.hanning_weights(ws))
            assert np.array_equal(got.view(np.int64), ref[f"blocking/{seed}/smooth{ws}"].view(np.int64)), (seed, ws)


@pytest.mark.parametrize("m,N,width", BANDED_EDGE_CASES)
def test_banded_edge_cases_have_entries_inside_and_past_the_chromosome(oracle, synth, m, N, width):
    bed = synth.synth_bed_block(m, N, 1, block_index=23, miss=0.01)[0]
    band = oracle.marker_corr_banded(bed, m, N, width)
    assert band.shape == (m, width)
    past = np.arange(m)[:, None] + 1 + np.arange(width)[None, :] >= m
    assert past[-1].all() and np.all(band[past] == 0)  # the last row has no forward neighbour
    if m > 1:
        assert (band != 0).any() and not past.all()
    if width >= m - 1:
        assert past[0, m - 1:].all()  # even the first row reaches past the last marker


def test_small_chromosomes_block_file(oracle, synth):
    """the oracle's block file for the small-chromosome run of `mps block`: every chromosome in .bim order, covered"""
    sizes = [m for _, m in SMALL_CHROMOSOMES]
    ids = [c for c, _ in SMALL_CHROMOSOMES]
    assert ids != sorted(ids) and ids != sorted(ids, key=int) and SMALL_N % 64 != 0 and ((SMALL_N + 3) // 4) % 16 != 0
    bed = synth.synth_bed_block(sum(sizes), SMALL_N, 1, block_index=37)[0]
    chr_ids = [c for c, m in SMALL_CHROMOSOMES for _ in range(m)]
    lines = oracle.make_blocks(bed, chr_ids, SMALL_N, SMALL_MAXB, SMALL_WIDTH)
    for c, m in SMALL_CHROMOSOMES:
        rows = [tuple(map(int, l.split("\t")[1:])) for l in lines if l.split("\t")[0] == c]
        assert is_cover(rows, m), (c, rows)
    order = []
    for l in lines:
        if l.split("\t")[0] not in order:
            order.append(l.split("\t")[0])
    assert order == ids and len(lines) > len(ids)
