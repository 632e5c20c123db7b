"""The inputs of tests/test_gpu_level1_band.py (synth.level1_band_case), checked on the oracle alone, so that no GPU
assertion there can hold vacuously: every parameter set flips between two adjacent floats of C[X,Y], about half of the
ladder lies inside the level-1 guard band (float64 only places and counts; the oracle's fp32 verdict is the one criterion
of the GPU file), nothing but X - Y differs between the entries of a ladder, the hub layout spreads the triples over
both parities of list position and three staging rounds of the row kernel, the per-triple sizes of the het case lie on
both sides of the three constants of the HET form, and the planted degenerate triples are the named ones.

The cases and the oracle runs (cached) are imported by the GPU file."""
import functools

import numpy as np
import pytest

from test_cusk_het_rows_formats import kernel_estimate

F = np.float32
THRESHOLDS = ("n60", "headline", "biobank", "above_min", "below_min")
LAYOUTS = ("cliques", "hub")
# (layout, threshold, mode) of every case the GPU file runs
SKELETON_CASES = [(lay, name, "skeleton") for name in THRESHOLDS for lay in LAYOUTS]
HETCOR_CASES = [("hub", name, "hetcor") for name in ("headline", "biobank")]
HET_CASES = [(lay, "headline", "het") for lay in LAYOUTS]
ALL_CASES = SKELETON_CASES + HETCOR_CASES + HET_CASES


def _mods():
    import cigwas_amd.synth as S
    from oracle import oracle as O

    return S, O


def _caseid(c):
    return "-".join(c)


@functools.lru_cache(maxsize=None)
def thresholds():
    S, _ = _mods()
    return S.level1_band_thresholds()


@functools.lru_cache(maxsize=None)
def band_case(layout, name, mode):
    """-> dict(C, N (het: per-triple sizes, else None), info, n, Th, th, Nval, alpha)"""
    S, _ = _mods()
    N, alpha = thresholds()[name]
    out = S.level1_band_case(layout, N, alpha, mode)
    Cm, info = out[0], out[-1]
    return dict(C=Cm, N=out[1] if mode == "het" else None, info=info, n=Cm.shape[0], Th=info["Th"], th=info["th"], Nval=N, alpha=alpha)


def time_index(layout, name, mode):
    """a seeded quarter of the variables at index 1; S, X and Y of every triple stay at 0"""
    c = band_case(layout, name, mode)
    ti = (np.random.default_rng(7).random(c["n"]) < 0.25).astype(np.int32)
    for e in c["info"]["entries"]:
        ti[[e["X"], e["Y"], e["S"]]] = 0
    return ti


@functools.lru_cache(maxsize=None)
def band_ref(layout, name, mode, with_ti=False):
    """the oracle at max level 1 -> dict(G, level, tests, sep0 (skeleton: SepSet[:, :, 0], the other 13 slots are -1), g0 =
    the graph after level 0).  The n x n x 14 array of separating sets is not kept."""
    _, O = _mods()
    c = band_case(layout, name, mode)
    Cm, n = c["C"], c["n"]
    if mode == "skeleton":
        r = O.skeleton(Cm, c["Th"], 1)
        assert (r.sepset[:, :, 1:] == -1).all()
        return dict(G=r.G, level=r.level, tests=r.tests.copy(), sep0=r.sepset[:, :, 0].copy(), g0=O.skeleton(Cm, c["Th"], 0).G)
    Nm = c["N"] if mode == "het" else np.full((n, n), c["Nval"], F)
    ti = time_index(layout, name, mode) if with_ti else np.zeros(n, np.int32)
    ones = np.ones((n, n), np.int32)
    r = O.hetcor_skeleton(Cm, ones, Nm, c["th"], 1, ti)
    return dict(G=r.G, level=r.level, tests=r.tests.copy(), sep0=None, g0=O.hetcor_skeleton(Cm, ones, Nm, c["th"], 0, ti).G)


def _kept3(c, a, b, cv, sizes):
    """the oracle's verdict on the edge X - Y of the 3 x 3 matrix (X, Y, S) at max level 1"""
    _, O = _mods()
    C3 = np.array([[1, cv, a], [cv, 1, b], [a, b, 1]], F)
    if c["info"]["mode"] == "skeleton":
        return O.skeleton(C3, c["Th"], 1).G[0, 1] == 1
    nxy, nxs, nys = sizes
    N3 = np.array([[np.nan, nxy, nxs], [nxy, np.nan, nys], [nxs, nys, np.nan]], F)
    return O.hetcor_skeleton(C3, np.ones((3, 3), np.int32), N3, c["th"], 1, np.zeros(3, np.int32)).G[0, 1] == 1


def _rho64(a, b, cv):
    """partial correlation of (X, Y | S) in float64 from the inverse of the 3 x 3 matrix of the stored floats"""
    P = np.linalg.inv(np.array([[1, cv, a], [cv, 1, b], [a, b, 1]], np.float64))
    return -P[0, 1] / np.sqrt(P[0, 0] * P[1, 1])


def _ladder(c):
    return [e for e in c["info"]["entries"] if e["degenerate"] is None]


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] == "hub"], ids=_caseid)
def test_every_set_flips_between_adjacent_floats(oracle, synth, case):
    """the sets do not depend on the layout: checked on the hub cases.  At c the oracle keeps X - Y, at the float next to c
    on the side of a b it removes it"""
    c = band_case(*case)
    sets = c["info"]["sets"]
    assert len(sets) >= 40
    for p in sets:
        assert _kept3(c, p["a"], p["b"], p["c"], p["sizes"]), p
        below = synth._f32_from_ord(synth._f32_ord(p["c"]) - p["s"])
        assert not _kept3(c, p["a"], p["b"], below, p["sizes"]), p
        assert np.sign(_rho64(p["a"], p["b"], p["c"])) == p["s"] and p["a"] != p["b"]
    grid = {float(F(v)) for v in synth.LEVEL1_BAND_GRID}
    mags = {abs(float(p[k])) for p in sets for k in ("a", "b")}
    signs = {(np.sign(p["a"]), np.sign(p["b"]), p["s"], np.sign(p["c"])) for p in sets}
    print(f"{_caseid(case)}: {len(sets)} sets, grid magnitudes used {sorted(mags & grid)}, {len(signs)} sign patterns of (a, b, rho, c)")
    # at t = 0.33 (n60) no pair of grid values leaves room for the premises below (0.05 and 0.3 go at level 0, 0.999 puts the
    # tests of S given such a variable past 1 / t, and (0.5, 0.9) has (X; S | Y) at rho = 0.05): all 40 sets are seeded draws
    assert len(mags & grid) >= (0 if case[1] == "n60" else 4) and len(signs) >= 8
    assert {np.sign(p["c"]) for p in sets} == {-1.0, 1.0}
    # the ladder of every set: 11 ulp offsets and 6 band offsets, each its own triple
    per_set = {}
    for e in _ladder(c):
        per_set.setdefault(e["set"], []).append(e["label"])
    assert len(per_set) == len(sets) and all(len(v) == 17 and len(set(v)) == 17 for v in per_set.values())


@pytest.mark.parametrize("case", [("hub", name, "skeleton") for name in THRESHOLDS] + [("hub", "headline", "het")], ids=_caseid)
def test_half_of_the_ladder_lies_inside_the_band(oracle, case):
    """Measured share of the non-degenerate entries with |rho^2 / t^2 - 1| < beta in float64 (t, beta of the entry's set):
    n60 0.554, headline 0.488, biobank 0.528, above_min 0.522, below_min 0.522, het at headline 0.572."""
    c = band_case(*case)
    sets = c["info"]["sets"]
    inside = total = 0
    for e in _ladder(c):
        p = sets[e["set"]]
        r = _rho64(e["a"], e["b"], e["c"])
        inside += abs(r * r / (p["t"] * p["t"]) - 1.0) < p["beta"]
        total += 1
    share = inside / total
    print(f"{_caseid(case)}: t {c['info']['t']:.6f} beta {c['info']['beta']:.3e}: {inside} of {total} ladder entries inside the band ({share:.3f})")
    assert total >= 40 * 17 and 0.25 <= share <= 0.75


@pytest.mark.parametrize("case", ALL_CASES, ids=_caseid)
def test_only_the_edge_x_y_differs_between_ladder_entries(oracle, case):
    c, ref = band_case(*case), band_ref(*case)
    info, Cm, n = c["info"], c["C"], c["n"]
    assert np.array_equal(Cm.view(np.uint32), Cm.T.view(np.uint32))
    sets = info["sets"]
    # every zero entry goes at level 0, every other entry stays
    g0 = ref["g0"]
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(g0 == 1, (Cm != 0) & off)
    # after level 1: the level-0 graph with nothing changed but X - Y (pairs that touch a degenerate triple's own
    # variables aside: those triples are there for what their operands do to the arithmetic)
    special = np.zeros(n, bool)
    for e in info["entries"]:
        if e["degenerate"] is not None:
            special[[v for v in (e["X"], e["Y"], e.get("leaf"), e["S"]) if v is not None and v != info["hub"]]] = True
    expect = g0.copy()
    kept = removed = 0
    for e in _ladder(c):
        expect[e["X"], e["Y"]] = expect[e["Y"], e["X"]] = ref["G"][e["X"], e["Y"]]
        kept += int(ref["G"][e["X"], e["Y"]] == 1)
        removed += int(ref["G"][e["X"], e["Y"]] == 0)
        if e["label"] == "+0ulp":
            assert ref["G"][e["X"], e["Y"]] == 1, e
        if e["label"] == f"{-sets[e['set']]['s']:+d}ulp":
            assert ref["G"][e["X"], e["Y"]] == 0, e
    plain = ~(special[:, None] | special[None, :])
    assert np.array_equal(ref["G"][plain], expect[plain])
    assert np.array_equal(ref["G"], ref["G"].T)
    print(f"{_caseid(case)}: n {n}, {kept} ladder edges kept and {removed} removed at level 1")
    assert kept >= 200 and removed >= 200
    # ... and by a margin of at least 10 beta in rho^2 (float64; |rho| > 1 of an indefinite matrix reads as 1 / |rho|)
    worst = np.inf

    def margin(r, t, beta):
        r2 = r * r
        m = min(r2 / (t * t), 1.0 / (r2 * t * t)) - 1.0
        assert m >= 10.0 * beta, (r, t, beta)
        return m / beta

    hub = info["hub"]
    w_all = np.array([Cm[hub, v] for v in np.flatnonzero(g0[hub]) if not special[v]], np.float64) if hub is not None else None
    for e in _ladder(c):
        p = sets[e["set"]]
        a, b, cv = float(e["a"]), float(e["b"]), float(e["c"])
        for v, w in ((a, b), (b, a)):  # (X; S | Y), (Y; S | X) and their mirror images
            worst = min(worst, margin((v - cv * w) / np.sqrt((1 - cv * cv) * (1 - w * w)), p["t"], p["beta"]))
        if e.get("leaf") is not None:
            first = e[e["leaf_of"]]
            l_, v = float(Cm[e["leaf"], first]), float(Cm[first, hub])
            for r in (l_ / np.sqrt(1 - v * v), l_ / np.sqrt(1 - cv * cv), v / np.sqrt(1 - l_ * l_), cv / np.sqrt(1 - l_ * l_)):
                worst = min(worst, margin(r, p["t"], p["beta"]))
    if hub is not None and case[2] != "het":
        # tests of S with another triple's variable (or a filler) as the conditioning variable: rho = v / sqrt(1 - w^2)
        t, beta = info["t"], info["beta"]
        worst = min(worst, margin(np.abs(w_all).min(), t, beta), margin(np.abs(w_all).max() / np.sqrt(1 - np.abs(w_all).max() ** 2), t, beta))
    print(f"{_caseid(case)}: the other tests of the triples clear the threshold by at least {worst:.0f} beta")


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] == "hub"], ids=_caseid)
def test_hub_layout_spreads_the_triples_over_the_row_kernel(oracle, case):
    """from the oracle's level-0 adjacency: S has more than two staging rounds of 512 neighbours, the triples' variables sit at
    both parities of its list and in three rounds, n is no multiple of 4, and a triple with a leaf has its second variable
    two positions behind S in the first one's list (the second position of a lane's pair)"""
    c, ref = band_case(*case), band_ref(*case)
    info, g0 = c["info"], ref["g0"]
    hub = info["hub"]
    nb = list(np.flatnonzero(g0[hub]))
    assert len(nb) >= 1100 and c["n"] % 4 != 0
    pos = {v: k for k, v in enumerate(nb)}
    px = np.array([pos[e[k]] for e in _ladder(c) for k in ("X", "Y")])
    rounds = sorted(set((px // 512).tolist()))
    second = first = 0
    for e in _ladder(c):
        for u, v in ((e["X"], e["Y"]), (e["Y"], e["X"])):
            lst = list(np.flatnonzero(g0[u]))
            if hub < v:
                d = lst.index(v) - lst.index(hub)
                first += d == 1
                second += d == 2
    print(f"{_caseid(case)}: n {c['n']}, S has {len(nb)} neighbours, triples in rounds {rounds}, at even / odd positions "
          f"{int((px % 2 == 0).sum())} / {int((px % 2 == 1).sum())}, tests of interest at the first / second position of a lane's pair {first} / {second}")
    assert len(rounds) >= 3 and (px % 2 == 0).sum() >= 100 and (px % 2 == 1).sum() >= 100
    assert first >= 100 and second >= 100
    # segments of odd and of even length in S's row and in the rows of the triples
    seg = np.array([len(nb) - 1 - pos[e[k]] for e in _ladder(c) for k in ("X", "Y")])
    assert (seg % 2 == 0).sum() >= 100 and (seg % 2 == 1).sum() >= 100
    assert len(info["fillers"]) >= 50 and all(g0[f].sum() == 1 and g0[f, hub] == 1 for f in info["fillers"])


def test_het_sizes_lie_on_both_sides_of_the_three_constants(oracle):
    """kernel_estimate (tests/test_cusk_het_rows_formats.py) certifies only where me - 4 >= kHetDMin and kHetUMin <= u <=
    kHetUMax: two adjacent sums on each side of each constant.  At alpha = 1e-4 a mean size of 68 has u far above kHetUMax,
    so the kHetDMin classes are looked at with th = 1 as well, where u is in range and me - 4 alone decides."""
    c = band_case("hub", "headline", "het")
    th = F(c["th"])
    classes = dict(c["info"]["size_classes"])
    used = {p["cls"] for p in c["info"]["sets"]}
    assert used == set(classes)

    def ok(name, th_):
        s = F(0.0)
        for v in classes[name]:
            s = F(s + F(int(v)))
        return kernel_estimate(th_, s)[2]

    assert [ok(f"umin{j:+d}", th) for j in (-2, -1, 0, 1)] == [True, True, False, False]
    assert [ok(f"umax{j:+d}", th) for j in (-2, -1, 0, 1)] == [False, False, True, True]
    assert [ok(f"dmin{j:+d}", F(1.0)) for j in (-2, -1, 0, 1)] == [False, False, True, True]
    assert not any(ok(f"dmin{j:+d}", th) for j in (-2, -1, 0, 1)) and ok("N0", th)
    for name in ("umin", "umax", "dmin"):
        sums = [sum(classes[f"{name}{j:+d}"]) for j in (-2, -1, 0, 1)]
        assert np.diff(sums).tolist() == [1.0, 1.0, 1.0], sums
    assert np.isnan(classes["nan"]).sum() == 1 and classes["zero"].count(0.0) == 1 and sum(v < 0 for v in classes["negative"]) == 1
    for lay in LAYOUTS:
        Nm = band_case(lay, "headline", "het")["N"]
        assert np.array_equal(Nm.view(np.uint32), Nm.T.view(np.uint32))
        for name in ("nan", "zero", "negative"):
            assert sum(e["sizes"] == classes[name] for e in band_case(lay, "headline", "het")["info"]["entries"]) >= 17


@pytest.mark.parametrize("case", ALL_CASES, ids=_caseid)
def test_the_degenerate_triples_are_the_named_ones(oracle, synth, case):
    c, ref = band_case(*case), band_ref(*case)
    deg = [e for e in c["info"]["entries"] if e["degenerate"] is not None]
    assert [e["degenerate"] for e in deg] == list(synth.LEVEL1_BAND_DEGENERATE) and len(deg) == 14
    assert all(e["set"] is not None for e in _ladder(c))
    d = {e["degenerate"]: e for e in deg}
    one = F(1.0)
    with np.errstate(invalid="ignore"):
        for k in ("a=+1", "a=-1", "a=b=+1", "a=b=-1"):
            assert one - d[k]["a"] * d[k]["a"] == 0 and abs(d[k]["a"]) == 1
        assert abs(d["a=b=+1"]["b"]) == 1 and d["a=b=-1"]["b"] == -1
        assert one - d["hc<0"]["c"] * d["hc<0"]["c"] < 0
        assert np.isnan(d["nan:a"]["a"]) and np.isnan(d["nan:b"]["b"]) and np.isnan(d["nan:c"]["c"])
        assert d["c=+1"]["c"] == 1 and d["c=-1"]["c"] == -1
        for k in ("h00<0:a", "h00<0:a,leaf"):
            e = d[k]
            assert one - e["a"] * e["a"] < 0 and e["c"] - F(e["a"] * e["b"]) == 0
            # h01 = 0: the exact form removes X - Y (rho = 0) where a squared form without its h00 > 0 guard says "dependent"
            assert ref["G"][e["X"], e["Y"]] == 0 and ref["g0"][e["X"], e["Y"]] == 1
        for k in ("h00<0:c", "h00<0:c,leaf"):
            e = d[k]
            assert one - e["c"] * e["c"] < 0 and e["a"] - F(e["c"] * e["b"]) == 0
            assert ref["G"][e["X"], e["S"]] == 0 and ref["g0"][e["X"], e["S"]] == 1
    if case[0] == "hub":
        assert d["h00<0:a,leaf"]["leaf"] is not None and d["h00<0:c,leaf"]["leaf"] is not None and d["h00<0:a"]["leaf"] is None


def test_a_set_without_a_flip_is_an_error(oracle, synth, monkeypatch):
    """a grid whose values the level-0 cut removes leaves no feasible set and no silent gap: the generator raises"""
    monkeypatch.setattr(synth, "LEVEL1_BAND_GRID", (1e-4, 2e-4))
    monkeypatch.setattr(synth, "_het_size_classes", lambda th, N0: [("N0", (5.0, 5.0, 5.0))])
    with pytest.raises(ValueError, match="level1_band_case"):
        synth.level1_band_case("cliques", 16384, 1e-4, "het")
