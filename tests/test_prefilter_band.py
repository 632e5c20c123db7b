"""CPU: the library's block pre-filter (cusk_count_significant: does a marker-trait correlation pass |atanh c| >= Th[0]?
zero passes skip the block) against the reference's expression as the oracle restates it, ELEMENT BY ELEMENT, at the
thresholds of biobank cohorts.  The library decides most elements by comparing |c| with tanh(Th[0]) and sends only a band
around it through the expression; that expression rounds 1 + c and 1 - c to float, which moves its verdict by ~2^-24
absolute -- 1e-5 of tanh(Th[0]) at N = 500k.  Every float within 5e-5 (relative) of tanh(Th[0]) is checked, both signs,
one call per element so that errors of opposite sign cannot cancel in a total."""
import ctypes as C

import numpy as np
import pytest

NS = (1_000, 10_000, 100_000, 500_000, 2_000_000)
ALPHAS = (1e-2, 1e-4, 5e-8)
SPECIAL = np.array([np.nan, -np.nan, 0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1.5, -1.5, 3.0e38, -3.0e38,
                    np.nextafter(np.float32(1), np.float32(0)), -np.nextafter(np.float32(1), np.float32(0)),
                    np.nextafter(np.float32(1), np.float32(2)), np.float32(1e-30), np.float32(1e-45)], np.float32)


def _floats_around(t: float, rel: float) -> np.ndarray:
    """every float32 in [t (1 - rel), t (1 + rel)] (t > 0)"""
    lo, hi = np.float32(t * (1 - rel)), np.float32(t * (1 + rel))
    a, b = np.array([lo, hi], np.float32).view(np.int32)
    return np.arange(a, b + 1, dtype=np.int32).view(np.float32)


def _per_element(lib, c: np.ndarray, th0: np.float32) -> np.ndarray:
    c = np.ascontiguousarray(c, np.float32)
    base = c.ctypes.data
    out = np.array([lib.cusk_count_significant(C.c_void_p(base + 4 * i), 1, th0) for i in range(c.size)], np.int32)
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N", NS)
def test_count_significant_matches_reference_expression_per_element(oracle, N, alpha):
    from cigwas_amd._lib import lib

    L = lib()
    th0 = np.float32(oracle.threshold_array(N, alpha)[0])
    t = float(np.tanh(np.float64(th0)))
    near = _floats_around(t, 5e-5)
    assert near.size > 500  # ~2,000 floats at every (N, alpha) of the grid
    c = np.concatenate([near, -near, SPECIAL])
    want = oracle.prefilter_flags(c, th0)
    got = _per_element(L, c, th0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"N={N} alpha={alpha} th0={float(th0):.6g}: {bad.size} of {c.size} verdicts differ from the "
                           f"reference's expression, first c = {c[bad[:4]].tolist()}")
    # both verdicts occur inside the band (the band straddles the cut-off), and the whole array counts the same
    assert want[: near.size].any() and not want[: near.size].all()
    assert L.cusk_count_significant(c.ctypes.data, c.size, th0) == int(want.sum())


def test_count_significant_far_from_the_cut_off(oracle, synth):
    """ordinary correlations, far from tanh(Th[0]) and from +-1: the fast comparison alone decides them"""
    from cigwas_amd._lib import lib

    rng = np.random.default_rng(11)
    c = np.concatenate([rng.uniform(-1, 1, 20_000), rng.normal(0, 0.01, 20_000)]).astype(np.float32)
    for N, alpha in ((1_000, 1e-2), (500_000, 1e-4), (10_000_000, 1e-4)):
        th0 = np.float32(oracle.threshold_array(N, alpha)[0])
        want = oracle.prefilter_flags(c, th0)
        assert np.array_equal(_per_element(lib(), c, th0), want), (N, alpha)
    assert lib().cusk_count_significant(None, 0, np.float32(0.01)) == 0
