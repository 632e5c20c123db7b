"""GPU: the arithmetic of `mps block` after the banded correlations -- the smoothing kernel (cusk_hanning_smooth), the
window weights (cusk_hanning_weights) and the minima cut and window bisection of host/blocking.h behind cusk_block_chr,
the entry point `mps block` itself calls.  No tolerance anywhere: both sides of every comparison perform the same IEEE
operations in the same order, so values are compared by their bits and block lists by equality.

a. the kernel against a plain numpy restatement at the sizes where its grid, margins and empty ranges change;
b. weights, kernel and blocks against what the reference's own blocking.cpp computed (tests/golden/ref_host_kat.npz);
c. bisection paths and edge profiles against oracle.block_chr (the inputs are checked in tests/test_blocking_cases.py).

The banded tile geometry and the small-chromosome file run are in tests/test_gpu_mps.py."""
import ctypes as C

import numpy as np
import pytest

from test_blocking_cases import is_cover, max_block_sizes, profiles, smooth_restated
from test_oracle_vs_ref import BLOCKING_CASES, BLOCKING_WINDOWS, ref  # noqa: F401  (ref: the fixture)

pytestmark = pytest.mark.gpu

POISON = -777.0
GUARD = 7
SMOOTH_NS = (1, 2, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def smooth_guarded(eng, v, w):
    out = np.full(len(v) + GUARD, POISON)
    got = eng.hanning_smooth(v, w, out=out)
    assert np.all(out[len(v):] == POISON)  # nothing written past n
    return got.copy()


def windows_of(n):
    return sorted(x for x in {1, 2, 3, 4, n - 1, n, n + 1, 2 * n + 1} if x > 0)


@pytest.mark.parametrize("n", SMOOTH_NS)
def test_smoothing_kernel_equals_the_restated_loop_bit_for_bit(eng, n):
    """arbitrary weights of both signs (the kernel takes them as input), odd and even windows, windows that cover the
    profile exactly once, and windows longer than the profile (no centre: all zeros)"""
    assert any(x % 2 == 0 for x in windows_of(n))
    for window in windows_of(n):
        rng = np.random.default_rng(1000 * n + window)
        v = rng.normal(20.0, 8.0, n).astype(np.float32)
        w = rng.normal(0.0, 1.0, window)
        got = smooth_guarded(eng, v, w)
        want = smooth_restated(v, w)
        margin = window // 2
        assert np.all(want[:margin] == 0) and np.all(want[max(n - margin, 0):] == 0)
        if window > n or 2 * margin >= n:
            assert not want.any() and np.array_equal(got.view(np.int64), np.zeros(n, np.int64)), (n, window)
        else:
            assert want[margin:n - margin].all()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n, window)


@pytest.mark.parametrize("window", [8, 9])
def test_smoothing_kernel_nan_inf_denormal(eng, window):
    """NaN lands in exactly the centres whose window covers it; +inf (positive weights: no inf - inf) and a float32
    denormal go through the double accumulation like every other value"""
    n, at_nan, at_inf, at_den = 200, 50, 120, 20
    rng = np.random.default_rng(window)
    v = rng.normal(20.0, 8.0, n).astype(np.float32)
    v[at_den - window:at_den + window + 1] = 0.0  # the denormal is the only term of the sums it enters
    v[at_nan], v[at_inf], v[at_den] = np.nan, np.inf, np.float32(1e-40)
    assert 0 < v[at_den] < np.finfo(np.float32).tiny
    w = rng.uniform(0.1, 1.0, window)
    got = smooth_guarded(eng, v, w)
    want = smooth_restated(v, w)
    margin = window // 2
    c = np.arange(n)
    centre = (c >= margin) & (c < n - margin)

    def covering(at):
        return centre & (c - margin <= at) & (at <= c - margin + window - 1)

    assert covering(at_nan).sum() == window and not (covering(at_nan) & covering(at_inf)).any()
    assert np.array_equal(np.isnan(got), covering(at_nan)) and np.array_equal(np.isnan(want), covering(at_nan))
    assert np.all(got[covering(at_inf)] == np.inf)
    assert np.all(want[covering(at_den)] > 0)  # the denormal is not flushed on the way to double
    rest = ~covering(at_nan)
    assert np.array_equal(got[rest].view(np.int64), want[rest].view(np.int64))


def test_smoothing_refuses_bad_arguments_and_launches_nothing(eng):
    from cigwas_amd._lib import lib

    f = lib().cusk_hanning_smooth
    v = np.arange(10, dtype=np.float32)
    w = np.ones(3)
    out = np.full(10 + GUARD, POISON)
    bad = [(_ptr(v), 0, _ptr(w), 3, _ptr(out)),  # n = 0
           (_ptr(v), 10, _ptr(w), 0, _ptr(out)),  # window <= 0
           (_ptr(v), 10, _ptr(w), -3, _ptr(out)),
           (None, 10, _ptr(w), 3, _ptr(out)),  # null pointers
           (_ptr(v), 10, None, 3, _ptr(out)),
           (_ptr(v), 10, _ptr(w), 3, None)]
    for args in bad:
        assert f(eng.h, *args) != 0, args[1:4:2]
        assert np.all(out == POISON)
    assert f(None, _ptr(v), 10, _ptr(w), 3, _ptr(out)) != 0 and np.all(out == POISON)
    with pytest.raises(RuntimeError):
        eng.hanning_smooth(v[:0], w)
    # the engine is usable afterwards
    assert np.array_equal(smooth_guarded(eng, v, w), smooth_restated(v, w))


@pytest.mark.parametrize("seed,n,maxb", BLOCKING_CASES)
def test_product_blocking_matches_reference_code(eng, ref, seed, n, maxb):  # noqa: F811
    """what the reference's own blocking.cpp computed for seeded LD-like profiles: the smoothed curves bit for bit with the
    library's weights (single-precision cosine) and the device loop, and the final blocks"""
    import cigwas_amd as cg

    v = ref[f"blocking/{seed}/v"]
    assert v.shape == (n,)
    for ws in BLOCKING_WINDOWS:
        got = smooth_guarded(eng, v, cg.hanning_weights(ws))
        want = ref[f"blocking/{seed}/smooth{ws}"]
        assert want.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64)), ws
    blocks = [(int(a), int(b)) for a, b in ref[f"blocking/{seed}/blocks"]]
    assert len(blocks) > 0
    assert eng.block_chr(v, maxb) == blocks
    assert is_cover(blocks, n)


@pytest.mark.parametrize("name", sorted(profiles()))
def test_block_chr_matches_oracle_on_bisection_paths_and_edge_profiles(eng, oracle, name):
    """identical block lists for every profile of tests/test_blocking_cases.py at maximum block sizes 1, n // 6, n and
    n + 101 (that file shows on the CPU that these leave the bisection through both exits, after moving both ways), and
    a cover of 0 .. n-1 each time.

    No n >= 1 was dropped: at n = 1 and n = 2 the first window is 1, its only weight is 0 / 0 = NaN (in the reference
    too), every comparison with the smoothed NaN is false and the one block 0 .. n-1 comes out the same way each time.
    n = 0 is left out: the reference forms size() - 1 of an empty profile there; cusk_block_chr refuses it (below)."""
    v = profiles()[name]
    for maxb in max_block_sizes(len(v)):
        got = eng.block_chr(v, maxb)
        assert got == oracle.block_chr(v, maxb), (name, maxb)
        assert is_cover(got, len(v)), (name, maxb, got)


def test_block_chr_arguments(eng, oracle):
    from cigwas_amd._lib import lib

    f = lib().cusk_block_chr
    v = profiles()["random1000"]
    want = oracle.block_chr(v, 1)
    assert len(want) > 2
    first, last = np.full(len(v) + GUARD, -5, np.int64), np.full(len(v) + GUARD, -5, np.int64)
    count = C.c_size_t(99)
    # a capacity that is too small: the number needed comes back, nothing is written
    for cap in (0, 1, len(want) - 1):
        assert f(eng.h, _ptr(v), len(v), 1, _ptr(first), _ptr(last), cap, C.byref(count)) != 0
        assert count.value == len(want) and np.all(first == -5) and np.all(last == -5)
    assert f(eng.h, _ptr(v), len(v), 1, None, None, 0, C.byref(count)) != 0 and count.value == len(want)
    # exactly enough
    assert f(eng.h, _ptr(v), len(v), 1, _ptr(first), _ptr(last), len(want), C.byref(count)) == 0
    assert count.value == len(want) and list(zip(first[:len(want)], last[:len(want)])) == want
    assert np.all(first[len(want):] == -5) and np.all(last[len(want):] == -5)
    # n = 0, null pointers
    assert f(eng.h, _ptr(v), 0, 1, _ptr(first), _ptr(last), 10, C.byref(count)) != 0 and count.value == 0
    assert f(eng.h, None, len(v), 1, _ptr(first), _ptr(last), 10, C.byref(count)) != 0
    assert f(None, _ptr(v), len(v), 1, _ptr(first), _ptr(last), 10, C.byref(count)) != 0
    assert f(eng.h, _ptr(v), len(v), 1, _ptr(first), _ptr(last), 10, None) != 0
    assert f(eng.h, _ptr(v), len(v), 1, None, _ptr(last), 10, C.byref(count)) != 0
    with pytest.raises(RuntimeError):
        eng.block_chr(v[:0], 10)
    assert eng.block_chr(v, 1) == want
