"""The inputs of tests/test_gpu_dispatch.py, checked on the oracle alone: every case reaches the degree classes it is
built for (boundary degrees and a row of d = l + 1 included), its removals are decided at work-item boundaries of the
sweep (ranks k * chunk - 1, k * chunk, k * chunk + 1 for chunk 64 and 256), some of them have a second passing set in a
later item, and the near-threshold hangers sit inside the fast filters' guard band."""
from math import comb

import numpy as np
import pytest

CAPS = np.array([39, 63, 127, 191])


def degree_class(d):
    return np.searchsorted(CAPS, d, side="left")


@pytest.mark.parametrize("name", ["l2", "l3", "l4", "l5"])
def test_dispatch_case_reaches_its_targets(oracle, synth, name):
    level, degrees = synth.DISPATCH_CASES[name]
    Cm, info = synth.dispatch_case(degrees, level, seed=level)
    Th = oracle.threshold_array(info["N"], info["alpha"])
    assert abs(Th[level] / info["th"] - 1) < 1e-6 and Th[level] >= 2e-3  # the fast filters are certified here
    pre = oracle.skeleton(Cm, Th, level - 1)
    deg = pre.G.sum(1)
    # every hub row starts the level with exactly its degree and its planned list; the classes of `degrees` are filled
    for h in info["hubs"]:
        assert list(np.flatnonzero(pre.G[h["h"]])) == h["pos"], h["d"]
    assert sorted(deg[[h["h"] for h in info["hubs"]]]) == sorted(degrees)
    assert set(degree_class(deg)) >= set(degree_class(np.array(degrees)))
    assert (deg == level + 1).any()
    if name == "l2":
        assert {39, 40, 63, 64, 127, 128, 191, 192} <= set(deg.tolist())
    ref = oracle.skeleton(Cm, Th, level)
    hit = set()
    for h in info["hubs"]:
        H, nb = h["h"], h["pos"]
        for v, r, T in h["targets"]:
            # removed at this level from the hub's row, by its planned set: the lowest passing rank is r
            S = ref.sepset[H, v]
            S = list(S[S >= 0])
            assert ref.G[H, v] == 0 and len(S) == level and S == T, (h["d"], v, r)
            assert synth.comb_rank([nb.index(q) for q in S], len(nb)) == r
            assert oracle.ci_test(Cm, H, v, T)[1] < Th[level]
            hit.add(r)
        won = {v: r for v, r, T in h["targets"]}
        for v, r2, T2 in h["twins"]:
            # a second passing set at a higher rank, in a later 64-set work item: "lowest rank wins" decides the record
            assert r2 > won[v] and r2 // 64 > won[v] // 64
            assert synth.comb_rank([nb.index(q) for q in T2], len(nb)) == r2
            assert 0.3 < oracle.ci_test(Cm, H, v, T2)[1] / Th[level] < 0.7
        for v, T, passes in h["near"]:
            z = oracle.ci_test(Cm, H, v, T)[1]
            assert 1e-4 < abs(z / Th[level] - 1) < 5e-4 and (z < Th[level]) == passes  # inside the +-1e-3 band
            assert ref.G[H, v] == (0 if passes else 1)
    for k in (1, 4):  # items of 64 and of 256 sets
        assert {k * 64 - 1, k * 64, k * 64 + 1} <= hit, (k, sorted(hit))
    assert sum(len(h["twins"]) for h in info["hubs"]) >= 4
    assert sum(p for h in info["hubs"] for _, _, p in h["near"]) >= 2
    assert sum(1 - p for h in info["hubs"] for _, _, p in h["near"]) >= 1


def test_comb_rank_is_the_oracles_enumeration(oracle, synth):
    """comb_rank / comb_unrank against the reference's IthCombination (1-based rank, 1-based positions)"""
    for d, l in [(39, 2), (64, 3), (41, 5), (192, 2)]:
        for r in (0, 1, 63, 64, 65, 255, 256, 257, 2049, comb(d, l) - 1):
            if r >= comb(d, l):
                continue
            T = synth.comb_unrank(r, d, l)
            assert synth.comb_rank(T, d) == r
            assert list(oracle.ith_combination(d, l, r + 1) - 1) == T


def test_level1_star_case_reaches_the_staging_rounds(oracle, synth):
    """the input of tests/test_gpu_level1_forms.py: one row with more than two 512-neighbour staging rounds at the start
    of level 1, rows in both degree ranges between the workgroup sizes, and a level 1 that removes most edges and keeps
    some between non-hub rows"""
    Cm, info = synth.level1_star_case()
    n, hub = Cm.shape[0], info["hub"]
    assert n % 4 != 0 and np.array_equal(Cm, Cm.T)
    Th = oracle.threshold_array(info["N"], info["alpha"])
    G0, G1 = oracle.skeleton(Cm, Th, 0).G, oracle.skeleton(Cm, Th, 1).G
    deg = G0.sum(1)
    assert deg[hub] >= 1030
    others = np.delete(deg, hub)
    assert ((others > 256) & (others <= 512)).sum() >= 3 and ((others > 512) & (others <= 1024)).sum() >= 3
    assert (G0.sum() - G1.sum()) // 2 >= 1000
    rest = np.arange(n) != hub
    assert G1[np.ix_(rest, rest)].sum() // 2 >= 100


def _parent_rows_threads(row_lds, mode, validate):
    """the launcher's loop over the candidate sizes as it stood before level1_rows_threads (no size forced)"""
    threads = best_wgs = best_waves = 0
    for t in (256, 512):
        fixed = 16 * t + 4 * (2 * t + 1) + 4 * 2 * (t // 64) + 64
        wgs = min(160 * 1024 // (row_lds + fixed), (16 if (mode == 0 and not validate) else 12) // (t // 64))
        waves = wgs * (t // 64)
        if wgs >= 2 and (wgs > best_wgs or (wgs == best_wgs and waves > best_waves)):
            best_wgs, best_waves, threads = wgs, waves, t
    return threads


def test_level1_rows_threads_is_the_former_choice():
    """level1_rows_threads (level1.hip) through its host-only entry: with nothing forced, the size the launcher chose
    before for every n, mode and validate; forced, that size whenever one row fits a CU's LDS.  (A matrix that is not
    16-byte aligned takes the gather form before the function is asked: test_gpu_level1_forms.py.)"""
    from cigwas_amd._lib import lib

    f = lib().cusk_level1_rows_threads
    ranges = {}
    for mode in (0, 1):
        for validate in (0, 1):
            got = []
            for n in range(64, 40001, 61):
                row = 4 * (n + 8)
                got.append(f(row, mode, validate, 0))
                assert got[-1] == _parent_rows_threads(row, mode, validate), (n, mode, validate)
                for forced in (256, 512):
                    fixed = 16 * forced + 4 * (2 * forced + 1) + 4 * 2 * (forced // 64) + 64
                    assert f(row, mode, validate, forced) == (forced if row + fixed <= 160 * 1024 else 0)
            ranges[(mode, validate)] = got
    # 512 threads only for Skeleton runs that do not validate (two rows of eight waves), the gather form from n ~ 16,000
    assert 512 in ranges[(0, 0)] and all(512 not in v for k, v in ranges.items() if k != (0, 0))
    assert all(v[0] == 256 and v[-1] == 0 for v in ranges.values())
    assert f(4096, 0, 0, 384) == -1 and f(-1, 0, 0, 0) == -1
