"""The inputs of tests/test_gpu_het_classes.py, checked on the oracle alone, so that no GPU assertion there can hold
vacuously: per-pair sample sizes that differ (symmetric and asymmetric) change the graph in the rows of the degree class
a case is built for, the asymmetric sizes give another graph than their transpose, `deep_removal_case` removes edges at
every level 5..14, and unusual sizes (NaN, <= l + 3, non-integers, values beyond the int range) change a sweep's result.

The cases, the oracle runs (cached per case) and the small helpers are imported by the GPU file."""
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML = 14
N0 = 16384.0
ALPHA = 1e-4
SIZE_SEED = 11
FORMS = ("sym", "asym")

# name -> (matrix, levels, class the case is named for per size form, class of the largest degree at the start of each
# level per size form).  hub230 reaches class 4 (194 neighbours) with the raw draw only: the element-wise minimum of the
# symmetric form lowers the sizes, level 0 removes more, and the largest row starts level 1 with 188.
TABLE = {
    "dense48": (lambda S: S.random_corr(48, seed=8, k=60), 4, {"sym": 1, "asym": 1},
                {"sym": (1, 0, 0, 0), "asym": (1, 0, 0, 0)}),
    "dense96": (lambda S: S.random_corr(96, seed=9, k=150), 3, {"sym": 2, "asym": 2},
                {"sym": (2, 0, 0), "asym": (2, 0, 0)}),
    "hub96": (lambda S: S.hub_corr(94, 2, seed=4), 3, {"sym": 2, "asym": 2}, {"sym": (2, 2, 2), "asym": (2, 2, 2)}),
    "hub200": (lambda S: S.hub_corr(198, 2, seed=7), 2, {"sym": 3, "asym": 3}, {"sym": (3, 3), "asym": (3, 3)}),
    "hub230": (lambda S: S.hub_corr(228, 2, seed=7), 2, {"sym": 3, "asym": 4}, {"sym": (3, 3), "asym": (4, 3)}),
}
TABLE_NAMES = list(TABLE)

DEEP_SEED = 1
DEEP_N = 20000
DEEP_ALPHA = 0.01
DEEP_LEVELS = tuple(range(5, 15))


def _mods():
    import cigwas_amd.synth as S
    from oracle import oracle as O

    return S, O


def class_caps():
    """kClassCap without its open last class, and kLdsLimit, read from csrc/cusk_internal.h"""
    src = open(os.path.join(ROOT, "ci-gwas_amd", "csrc", "cusk_internal.h")).read()
    caps = [int(v) for v in re.search(r"kClassCap\[kNumClasses\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")[:-1]]
    limit = re.search(r"kLdsLimit\s*=\s*(\d+)\s*\*\s*(\d+)", src)
    return caps, int(limit.group(1)) * int(limit.group(2))


def lds_total(cap, het):
    """lds_layout(cap, het).total of csrc/sweep_common.h"""
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    ld = (cap + 1) | 1
    best = a16(4 * (cap + 1))
    ti = a16(best + 8 * cap)
    sub = a16(ti + 4 * (cap + 1))
    ess = a16(sub + 4 * (cap + 1) * ld)
    return a16(ess + 4 * (cap + 1) * ld) if het else ess


def degree_class(d):
    return np.searchsorted(np.array(class_caps()[0]), d, side="left")


def graphs(Cm, Nm, th, levels, first=0):
    """the oracle's hetcor graphs after levels first..levels and the level counter of the last run"""
    _, O = _mods()
    n = Cm.shape[0]
    ones, ti = np.ones((n, n), np.int32), np.zeros(n, np.int32)
    runs = [O.hetcor_skeleton(Cm, ones, Nm, th, l, ti) for l in range(first, levels + 1)]
    return {l: r.G for l, r in zip(range(first, levels + 1), runs)}, runs[-1].level


@functools.lru_cache(maxsize=None)
def table_matrix(name):
    S, _ = _mods()
    return TABLE[name][0](S)


@functools.lru_cache(maxsize=None)
def table_case(name, form):
    """form: sym / asym (het_sizes), uniform (N0 everywhere), asymT (the asymmetric draw transposed)
    -> dict(C, N, th, levels, G = {level: graph}, level)"""
    S, O = _mods()
    Cm, levels = table_matrix(name), TABLE[name][1]
    n = Cm.shape[0]
    if form == "uniform":
        Nm = np.full((n, n), N0, np.float32)
    else:
        Nm = S.het_sizes(n, SIZE_SEED, N0, symmetric=(form == "sym"))
        if form == "asymT":
            Nm = np.ascontiguousarray(Nm.T)
    th = O.hetcor_threshold(ALPHA)
    G, level = graphs(Cm, Nm, th, levels)
    return dict(C=Cm, N=Nm, n=n, th=th, levels=levels, G=G, level=level)


def decided_differently(a, b, cls):
    """per level: ordered pairs (i, j) alive in both runs at the start of the level, of a row i whose degree at the start
    of the level (run a) lies in class `cls`, that one run removes at this level and the other keeps"""
    out = []
    for l in range(1, a["levels"] + 1):
        rows = degree_class(a["G"][l - 1].sum(1)) == cls
        both = (a["G"][l - 1] == 1) & (b["G"][l - 1] == 1)
        out.append(int((both & (a["G"][l] != b["G"][l]))[rows].sum()))
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_sizes_change_the_graph_in_the_rows_of_the_class(oracle, name, form):
    """Measured (default_rng(11), N0 = 16384, alpha = 1e-4; symmetric / asymmetric): largest degree at the start of each
    level dense48 43 30 17 13 both; dense96 74 37 22 / 76 38 25; hub96 94 93 91 both; hub200 176 165 / 177 167; hub230
    188 175 / 194 175.  Entries of the final graph that differ from the run at N0 everywhere 38 / 28, 128 / 98, 360 / 282,
    2638 / 2092, 3620 / 2944; from the run on the transposed asymmetric sizes 10, 38, 38, 364, 498."""
    _, levels, named, classes = TABLE[name]
    c = table_case(name, form)
    uni = table_case(name, "uniform")
    got = tuple(int(degree_class(c["G"][l - 1].sum(1).max())) for l in range(1, levels + 1))
    assert got == classes[form], [int(c["G"][l - 1].sum(1).max()) for l in range(1, levels + 1)]
    assert named[form] in got
    per_level = decided_differently(c, uni, named[form])
    total = int((c["G"][levels] != uni["G"][levels]).sum())
    print(f"{name} {form}: classes {got}, final graph differs from uniform in {total} entries, decided differently in "
          f"rows of class {named[form]} per level {per_level}")
    assert total > 0 and sum(per_level) > 0
    assert np.array_equal(c["N"], c["N"].T) == (form == "sym")
    if form == "asym":
        tr = table_case(name, "asymT")
        per_level_t = decided_differently(c, tr, named[form])
        total_t = int((c["G"][levels] != tr["G"][levels]).sum())
        print(f"{name} asym against the transposed sizes: {total_t} entries, in rows of class {named[form]} {per_level_t}")
        assert total_t > 0 and sum(per_level_t) > 0


def test_het_stages_three_classes_and_reads_two_through_the_cache():
    """what the engine derives (level_loop.hip: staged classes while lds_layout(cap, het).total <= kLdsLimit): with the
    second copy of the sub-matrix classes 0-2 are staged and 3-4 are not; without it class 3 is staged too"""
    caps, limit = class_caps()
    assert caps == [39, 63, 127, 191]
    assert [lds_total(c, True) <= limit for c in caps] == [True, True, True, False]
    assert [lds_total(c, False) <= limit for c in caps] == [True, True, True, True]
    # every class the table names is reached by some case, staged and not
    reached = {v for _, _, named, _ in TABLE.values() for v in named.values()}
    assert reached == {1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------------------------------
# removals at levels 5..14
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_case():
    """-> dict(C, info, n, Th, th, ref (oracle.skeleton at 14), N = {form: sizes})"""
    S, O = _mods()
    Cm, info = S.deep_removal_case(DEEP_LEVELS, seed=DEEP_SEED, N=DEEP_N, return_info=True)
    n = Cm.shape[0]
    Th = O.threshold_array(DEEP_N, DEEP_ALPHA)
    sizes = {f: S.het_sizes(n, DEEP_SEED, float(DEEP_N), symmetric=(f == "sym")) for f in FORMS}
    sizes["uniform"] = np.full((n, n), float(DEEP_N), np.float32)
    return dict(C=Cm, info=info, n=n, Th=Th, th=O.hetcor_threshold(DEEP_ALPHA), ref=O.skeleton(Cm, Th, ML), N=sizes)


@functools.lru_cache(maxsize=None)
def deep_graphs(form):
    """hetcor graphs of the deep case after levels 4..14 at the sizes of `form` (sym / asym / uniform)"""
    c = deep_case()
    return graphs(c["C"], c["N"][form], c["th"], ML, first=4)


def removed_at(G, l):
    return (G[l - 1] == 1) & (G[l] == 0)


def test_deep_removal_case_removes_at_every_level(oracle, synth):
    """Seed 1 (DEEP_SEED), picked on the CPU among seeds 0-3 (every one of them removes at all of levels 5..14; seed 1
    has the most levels at which the sizes matter).  Ordered pairs removed at levels 5..14 -- Skeleton at N = 20000,
    alpha = 0.01: 4 5 4 4 4 7 4 4 4 4; hetcor with het_sizes (symmetric): 6 4 4 6 6 6 6 6 4 4; hetcor at N everywhere:
    4 6 4 4 4 8 4 4 4 4.  The removed sets of the last two differ at seven levels, 5 6 8 9 10 11 12 (2 ordered pairs
    each): four of them at level 9 and deeper."""
    c = deep_case()
    ref = c["ref"]
    assert ref.level == 15 and c["n"] < 200
    # the planted rows have up to 18 neighbours; level 0 at alpha = 0.01 adds chance edges (22 on one row), which the
    # first levels remove: from level 5 on, where the binomials grow, no row has more than 20
    assert max(len(g["parents"]) + len(g["extras"]) + 2 for g in c["info"].values()) == 18
    assert int(oracle.skeleton(c["C"], c["Th"], 4).G.sum(1).max()) <= 20
    lv = (ref.sepset >= 0).sum(2)
    sk = [int(((lv == l) & (ref.G == 0)).sum()) for l in DEEP_LEVELS]
    assert all(v > 0 for v in sk), sk
    # a winning set at level >= 9 that is not the first set of its row: the planted x rows (their extras come first)
    ranks = {}
    for k in range(9, 15):
        g = c["info"][k]
        x, y = g["x"], g["y"]
        if ref.G[x, y] == 0 and lv[x, y] == k:
            assert sorted(ref.sepset[x, y][:k]) == g["parents"]
            nb = list(np.flatnonzero(oracle.skeleton(c["C"], c["Th"], k - 1).G[x]))
            ranks[k] = synth.comb_rank([nb.index(v) for v in ref.sepset[x, y][:k]], len(nb))
            break
    assert ranks and all(r > 0 for r in ranks.values()), ranks
    Gh, level_h = deep_graphs("sym")
    Gu, level_u = deep_graphs("uniform")
    assert level_h == 15 and level_u == 15
    het = [int(removed_at(Gh, l).sum()) for l in DEEP_LEVELS]
    uni = [int(removed_at(Gu, l).sum()) for l in DEEP_LEVELS]
    differ = [l for l in DEEP_LEVELS if not np.array_equal(removed_at(Gh, l), removed_at(Gu, l))]
    print(f"removed per level 5..14: Skeleton {sk}, het {het}, uniform {uni}; the sizes change the removals at {differ}")
    assert all(v > 0 for v in het), het
    assert len(differ) >= 3 and max(differ) >= 9


def test_deep_removal_case_asymmetric_sizes_remove_at_every_level(oracle):
    Ga, level = deep_graphs("asym")
    assert level == 15
    assert all(removed_at(Ga, l).any() for l in DEEP_LEVELS)


# ---------------------------------------------------------------------------------------------------------------------
# unusual sizes inside a sweep
# ---------------------------------------------------------------------------------------------------------------------
ODD_LEVELS = 4
ODD_VALUES = np.array([np.nan, 0.0, -5.0, 2.5, 4.0, 5.99, 4.0, 5.0, 6.0, 7.0, np.inf, 3e9, 16384.75], np.float32)  # l + 3: 4..7


@functools.lru_cache(maxsize=None)
def odd_case():
    """dense48 with symmetric het_sizes, about 10 % of the pairs overwritten (both orders) by a seeded draw of ODD_VALUES
    -> dict(C, N, N_plain, th, ref, G)"""
    S, O = _mods()
    Cm = table_matrix("dense48")
    n = Cm.shape[0]
    plain = S.het_sizes(n, SIZE_SEED, N0)
    rng = np.random.default_rng(SIZE_SEED + 1)
    iu = np.triu_indices(n, 1)
    pick = rng.random(len(iu[0])) < 0.10
    Nm = plain.copy()
    v = rng.choice(ODD_VALUES, int(pick.sum()))
    Nm[iu[0][pick], iu[1][pick]] = v
    Nm[iu[1][pick], iu[0][pick]] = v
    th = O.hetcor_threshold(ALPHA)
    ones, ti = np.ones((n, n), np.int32), np.zeros(n, np.int32)
    ref = O.hetcor_skeleton(Cm, ones, Nm, th, ODD_LEVELS, ti)
    return dict(C=Cm, N=Nm, N_plain=plain, n=n, th=th, ref=ref, picked=int(pick.sum()))


def test_unusual_sizes_change_the_sweep(oracle):
    c = odd_case()
    n = c["n"]
    G = c["ref"].G
    plain = table_case("dense48", "sym")
    assert 0.08 * n * (n - 1) / 2 < c["picked"] < 0.12 * n * (n - 1) / 2
    got = c["N"][np.triu_indices(n, 1)]
    for v in ODD_VALUES:  # every kind of value is in the matrix
        assert np.isnan(got).any() if np.isnan(v) else (got == v).any(), v
    assert 0 < int(G.sum()) < n * (n - 1)
    diff = int((G != plain["G"][ODD_LEVELS]).sum())
    print(f"unusual sizes on {c['picked']} pairs: {int(G.sum())} entries left, {diff} differ from the run at the drawn sizes")
    assert diff > 0
    # ... and not at level 0 alone: the graphs that start level 1 differ, and so do the removals after it
    ones, ti = np.ones((n, n), np.int32), np.zeros(n, np.int32)
    G0 = oracle.hetcor_skeleton(c["C"], ones, c["N"], c["th"], 0, ti).G
    later = (G0 == 1) & (plain["G"][0] == 1) & (G != plain["G"][ODD_LEVELS])
    assert later.any()
