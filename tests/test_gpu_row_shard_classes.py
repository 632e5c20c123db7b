"""GPU: row-sharded sweeps (cusk_engine_set_row_shard) by degree class and to level 14, in one process.

tests/test_gpu_row_shard.py reaches the sharded path through processes and gloo: LD blocks at alpha = 1e-4, degrees of
the first class, levels <= 5, world 2 or 3.  Here the ranks are threads (tests/shard_threads.py: one engine per thread,
a barrier and a numpy unsigned minimum as the collective), the inputs are the small cases of test_gpu_dispatch,
test_gpu_tmaj / test_gpu_parity and test_het_class_cases, and their oracle runs are the cached ones of those modules.
Every comparison is an equality, except pMax against the oracle (the suite's 1e-6 bar).

What each group reaches that the gloo tests do not:
(a) the plan kernel's row filter and the 64-bit join with work items in every degree class (39 / 63 / 127 / 191 /
    unstaged), under the option sets that select the other kernel forms; level 1 on the row kernel at 256 and 512 threads
    and in its gather form (32-bit join), on the pair kernel and on the generic sweep (64-bit join at level 1);
(b) levels 6-14 of a sharded run (set-major kernels: sharding switches the union-major sweep off, also against option
    tmaj_min_level) and ranks that own no row with work from some level on;
(c) the hetcor join (marks_from_bitmap + level1_apply) in every degree class, at per-pair sizes, with a time index and
    with a starting graph;
(d) worlds that do not divide the rows or exceed n, n = 2, and the way back to the plain path;
(e) the exchange's contract (same call sequence on every rank, one call per level that ran, element width, count,
    on_device) and the device-buffer branch with more than one participant;
(f) a recheck queue that overflows on a sharded engine: shard_join (level_loop.hip) reads the level's queue counter
    before the exchange, sweeps the engine's rows again on the exact path at once (exact_fallbacks) and then joins, so
    the redone level is joined exactly once like every other; the `if (m.sharded && !exact_only) shard_join` of
    enqueue_sweeps guards the unsharded redo (after_read_back never asks a sharded run for one);
(g) an exchange that fails: an error ("row-shard exchange failed at level 2"), not a wait, and the engines stay usable;
(h) sensitivity: with an exchange that joins nothing, rank 0 ends with another graph than the oracle.

Counters of sharded runs: include/cusk_hip.h and DESIGN.md section 7 promise the complete RESULT on every engine and say
nothing about cusk_stats.tests / canonical_tests / removed of a sharded engine, so nothing more is asserted of them than
this: max_degree and edges are those of the global graph on every rank, and the ranks' tests[l] add up to at least the
oracle's (every test of the sequential schedule is run by the owner of its row).

Wall time on an MI355X, same session, each file run alone: this file 40.3 s (89 cases, none above 2 s but the two of
test_sharded_hetcor_to_level_14 at 7.9 s, which is the oracle's deep_graphs when test_gpu_het_classes has not cached it
in the session already), tests/test_gpu_row_shard.py 43.5 s (10 cases)."""
import functools

import numpy as np
import pytest

from shard_threads import ShardGroup, run_sharded
from test_gpu_dispatch import CASES, SMALL, _case, _hetcor_case, _optid
from test_het_class_cases import deep_case, deep_graphs

pytestmark = pytest.mark.gpu
ML = 14
OPTS = [{}, {"vec": 0}, {"fast": 0}, {"rows": 0}, {"pair": 0}, {"max_staged_classes": 0}, {"l1_threads": 512},
        {"l1_lds_row": 0}, SMALL]
WORLD_OPTS = [(3, o) for o in OPTS] + [(2, {}), (5, {})]


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


def _mods():
    import cigwas_amd.synth as S
    from oracle import oracle as O

    return S, O


def _identity(join):
    return lambda rank, level, mine: mine  # every rank keeps what it found itself


# ---------------------------------------------------------------------------------------------------------------------
# runs and comparisons
# ---------------------------------------------------------------------------------------------------------------------
def _skeleton_runs(cg, Cm, Th, maxlevel, world, opts=None, **kw):
    Cd = cg.DeviceArray(Cm)
    try:
        return run_sharded(world, lambda e: (e.run_skeleton(Cd.ptr, Cm.shape[0], Th, maxlevel), Cd.ptr), opts, **kw)
    finally:
        Cd.free()


_single_cache = {}


def _single(cg, key, Cm, Th, maxlevel, opts):
    """the same run on one plain engine with the same options (once per case and option set)"""
    k = (key, maxlevel, tuple(sorted(opts.items())))
    if k not in _single_cache:
        _single_cache[k] = _skeleton_runs(cg, Cm, Th, maxlevel, 1, opts)[0]
    return _single_cache[k]


def _dense(n, rec):
    x, y, lv, z, S = rec
    d = np.full((n, n, ML), -1, np.int32)
    d[x, y] = S
    return d


def _is_oracle_skeleton(r, ref):
    """what test_skeleton_dispatch_matrix asserts of one engine"""
    n = ref.G.shape[0]
    assert r.stats.level == ref.level
    assert np.array_equal(r.adjacency, ref.G)
    assert np.array_equal(_dense(n, r.sepsets), ref.sepset)
    assert np.allclose(r.pmax, ref.pmax, rtol=0, atol=1e-6)


def _same_bytes(a, b):
    """adjacency, level counters, every record (the bits of z included) and the bits of pMax"""
    assert a.stats.level == b.stats.level and a.stats.levels_run == b.stats.levels_run
    assert np.array_equal(a.adjacency, b.adjacency)
    assert (a.sepsets is None) == (b.sepsets is None)
    if a.sepsets is not None:
        for u, v in zip(a.sepsets, b.sepsets):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
    assert (a.pmax is None) == (b.pmax is None)
    if a.pmax is not None:
        assert a.pmax.tobytes() == b.pmax.tobytes()


def _calls_hold(res, hetcor, level1_rows=True, on_device=0):
    """(e): every rank saw the same calls; levels 1, 2, .. without gaps up to the last level that ran and none after it;
    the count is the number of directed edges at the start of the level (global); element width 4 in hetcor mode, in
    Skeleton mode 8 (selection ranks) but 4 at a level 1 on the row kernel ("4 B per directed edge
    at level 1, 8 B beyond"; with option rows = 0 or pair = 0 level 1 has no row kernel and joins 64-bit ranks like the
    levels behind it, level_loop.hip shard_join: elem = (use_rows || mode == 1) ? 4 : 8)"""
    st = res[0].stats
    swept = st.levels_run - 1
    want = [(l, int(st.edges[l]), 4 if (hetcor or (l == 1 and level1_rows)) else 8, on_device) for l in range(1, swept + 1)]
    for r in res:
        assert r.calls == want, (r.rank, r.calls, want)
        assert r.stats.levels_run == st.levels_run
    return want


def _level1_rows(opts):
    return opts.get("rows", 1) != 0 and opts.get("pair", 1) != 0


@functools.lru_cache(maxsize=None)
def _start_degrees(name):
    """the oracle's largest degree at the start of levels 1 .. level of the case"""
    _, O = _mods()
    Cm, info, Th, _, dmax = _case(name)
    out = [int(O.skeleton(Cm, Th, k - 1).G.sum(1).max()) for k in range(1, info["level"])] + [dmax]
    return [Cm.shape[0] - 1] + out


# ---------------------------------------------------------------------------------------------------------------------
# (a) Skeleton by degree class
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,opts", WORLD_OPTS, ids=[f"w{w}-{_optid(o)}" for w, o in WORLD_OPTS])
@pytest.mark.parametrize("name", CASES)
def test_sharded_skeleton_by_degree_class(cg, name, world, opts):
    Cm, info, Th, ref, dmax = _case(name)
    l = info["level"]
    res = _skeleton_runs(cg, Cm, Th, l, world, opts)
    one = _single(cg, name, Cm, Th, l, opts)
    _is_oracle_skeleton(one, ref)
    for r in res:
        _is_oracle_skeleton(r, ref)
        _same_bytes(r, one)
        # the graph is global on every rank
        assert list(r.stats.max_degree[: l + 1]) == _start_degrees(name)
        assert list(r.stats.max_degree) == list(one.stats.max_degree) and list(r.stats.edges) == list(one.stats.edges)
    assert res[0].stats.levels_run == l + 1
    for k in range(1, l + 1):
        assert sum(r.stats.tests[k] for r in res) >= ref.tests[k] > 0
    _calls_hold(res, hetcor=False, level1_rows=_level1_rows(opts))


# ---------------------------------------------------------------------------------------------------------------------
# (b) deep levels
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep(name):
    """-> (C, Th, oracle run to level 14, oracle graph at the start of level 6 or None)"""
    S, O = _mods()
    if name == "deep":
        c = deep_case()
        return c["C"], c["Th"], c["ref"], None
    nleaf, seed = {"hub16": (16, 4), "hub17": (17, 5)}[name]  # test_gpu_parity / test_gpu_tmaj: N = 20000, alpha = 0.01
    Cm = S.hub_corr(nleaf, 3, seed=seed)
    Th = O.threshold_array(20000, 0.01)
    return Cm, Th, O.skeleton(Cm, Th, ML), O.skeleton(Cm, Th, 5).G


@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("name", ["hub16", "hub17", "deep"])
def test_sharded_skeleton_to_level_14(cg, name, world):
    Cm, Th, ref, G5 = _deep(name)
    assert ref.level == 15
    if G5 is not None and world == 5:
        # condition on the input: from level 6 on (degrees only shrink) only the three hubs have more than l neighbours, so
        # at least two of the five ranks own no row with work and contribute nothing but "none" to the join
        # (hub16: the hubs 16-18 and leaf 8, which shares rank 3 with hub 18; hub17: the hubs 17-19)
        busy = np.flatnonzero(G5.sum(1) > 6)
        assert 1 <= len({int(x) % world for x in busy}) <= 3 and {int(x) for x in busy} >= set(range(Cm.shape[0] - 3, Cm.shape[0]))
    res = _skeleton_runs(cg, Cm, Th, ML, world)
    one = _single(cg, name, Cm, Th, ML, {})
    for r in res:
        assert r.stats.levels_run == 15
        _is_oracle_skeleton(r, ref)
        _same_bytes(r, one)
    for k in range(1, ML + 1):
        assert sum(r.stats.tests[k] for r in res) >= ref.tests[k] > 0
    if G5 is not None and world == 5:
        assert sum(1 for r in res if sum(r.stats.tests[6:]) == 0) >= 2
    _calls_hold(res, hetcor=False)
    # sharding overrides the option: no union-major sweep, the same bytes
    tm = _skeleton_runs(cg, Cm, Th, ML, world, {"tmaj_min_level": 2})
    for r, d in zip(tm, res):
        _same_bytes(r, d)
    _calls_hold(tm, hetcor=False)


# ---------------------------------------------------------------------------------------------------------------------
# (c) hetcor
# ---------------------------------------------------------------------------------------------------------------------
def _hetcor_runs(cg, Cm, th, maxlevel, world, opts=None, Nm=None, ess=0.0, ti=None, G_init=None, **kw):
    n = Cm.shape[0]
    arrays = [cg.DeviceArray(Cm)] + [cg.DeviceArray(a) if a is not None else None for a in (Nm, G_init)]
    Cd, Nd, Gd = arrays
    try:
        return run_sharded(world, lambda e: e.run_hetcor(Cd.ptr, n, th, maxlevel, N_dev=Nd.ptr if Nd else None, ess_uniform=ess,
                                                         G_init_dev=Gd.ptr if Gd else None, time_index=ti), opts, **kw)
    finally:
        for a in arrays:
            if a is not None:
                a.free()


HETCOR = [(name, False, ti) for name in CASES for ti in (False, True)] + \
         [(name, True, ti) for name in ("l2", "l5") for ti in (False, True)]


@pytest.mark.parametrize("opts", [{}, {"fast": 0}], ids=_optid)
@pytest.mark.parametrize("name,het,with_ti", HETCOR,
                         ids=[f"{n}-{'het' if h else 'uniform'}{'-ti' if t else ''}" for n, h, t in HETCOR])
def test_sharded_hetcor_by_degree_class(cg, name, het, with_ti, opts):
    Cm, info, _, _, _ = _case(name)
    Nm, ti, th, ref, dmax = _hetcor_case(name, het, with_ti)
    l = info["level"]
    res = _hetcor_runs(cg, Cm, th, l, 3, opts, Nm=Nm if het else None, ess=float(info["N"]), ti=ti if with_ti else None)
    for r in res:
        assert r.stats.level == ref.level
        assert np.array_equal(r.adjacency, ref.G)
        assert r.stats.max_degree[l] == dmax
        _same_bytes(r, res[0])
    assert sum(r.stats.tests[l] for r in res) > 0
    _calls_hold(res, hetcor=True)


@pytest.mark.parametrize("form,world", [("uniform", 2), ("sym", 5)])
def test_sharded_hetcor_to_level_14(cg, form, world):
    """the 32-bit marks joined at every level up to 14 (removals at each of levels 5..14, test_het_class_cases): one size
    passed as a number, and the symmetric per-pair sizes as a matrix"""
    c = deep_case()
    G, level = deep_graphs(form)
    uniform = form == "uniform"
    res = _hetcor_runs(cg, c["C"], c["th"], ML, world, Nm=None if uniform else c["N"][form],
                       ess=float(c["N"]["uniform"][0, 1]) if uniform else 0.0)
    for r in res:
        assert r.stats.level == level == 15 and r.stats.levels_run == 15
        assert np.array_equal(r.adjacency, G[ML])
    _calls_hold(res, hetcor=True)


@functools.lru_cache(maxsize=None)
def _start_graph_case():
    """l3 from a starting graph: the oracle's level-1 graph (hetcor, one sample size) without a seeded 10 % of its edges"""
    _, O = _mods()
    Cm, info, _, _, _ = _case("l3")
    n = Cm.shape[0]
    Nm = np.full((n, n), float(info["N"]), np.float32)
    th = O.hetcor_threshold(info["alpha"])
    ti = np.zeros(n, np.int32)
    G1 = O.hetcor_skeleton(Cm, np.ones((n, n), np.int32), Nm, th, 1, ti).G
    iu, ju = np.nonzero(np.triu(G1, 1))
    drop = np.random.default_rng(3).random(len(iu)) < 0.10
    G_init = np.ascontiguousarray(G1, np.int32).copy()
    G_init[iu[drop], ju[drop]] = 0
    G_init[ju[drop], iu[drop]] = 0
    return Cm, info, Nm, th, G_init, int(drop.sum()), O.hetcor_skeleton(Cm, G_init, Nm, th, info["level"], ti)


def test_sharded_hetcor_from_a_starting_graph(cg):
    Cm, info, Nm, th, G_init, dropped, ref = _start_graph_case()
    edges = int(G_init.sum()) // 2
    assert dropped > 0.05 * (edges + dropped) and ref.level == info["level"] + 1
    assert np.array_equal(G_init, G_init.T) and not np.array_equal(ref.G, G_init) and not (ref.G & ~G_init).any()
    res = _hetcor_runs(cg, Cm, th, info["level"], 3, ess=float(info["N"]), G_init=G_init)
    for r in res:
        assert r.stats.level == ref.level
        assert np.array_equal(r.adjacency, ref.G)
    _calls_hold(res, hetcor=True)


# ---------------------------------------------------------------------------------------------------------------------
# (d) worlds that do not fit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sem12():
    S, O = _mods()
    # 60 samples at alpha = 0.3 (the loose threshold of test_tmaj_recheck_queue_overflow...): levels 1-4 run with
    # 219 / 86 / 28 / 5 tests and 14 edges stay; at the 72 samples and alpha = 0.01 of test_skeleton_random_sem the
    # loop ends after three tests at level 2
    Cm = S.random_corr(12, seed=1, k=60)
    Th = O.threshold_array(60, 0.3)
    return Cm, Th, O.skeleton(Cm, Th, ML)


@pytest.mark.parametrize("world", [5, 7, 13])
def test_world_that_does_not_divide_the_rows(cg, world):
    """13 engines on 12 rows: rank 12 owns none"""
    Cm, Th, ref = _sem12()
    res = _skeleton_runs(cg, Cm, Th, ML, world)
    one = _single(cg, "sem12", Cm, Th, ML, {})
    assert ref.level == 4 and ref.G.sum() == 28 and all(ref.tests[k] > 0 for k in range(1, 5))
    for r in res:
        _is_oracle_skeleton(r, ref)
        _same_bytes(r, one)
    if world == 13:
        assert sum(res[12].stats.tests[1:]) == 0 and sum(sum(r.stats.tests[1:]) for r in res) > 0
    _calls_hold(res, hetcor=False)


def test_two_variables_three_engines(cg):
    _, O = _mods()
    Th = O.threshold_array(1000, 0.01)
    for rho in (0.5, 0.0):  # one edge / none: nothing to test behind level 0
        Cm = np.array([[1.0, rho], [rho, 1.0]], np.float32)
        ref = O.skeleton(Cm, Th, ML)
        assert int(ref.G.sum()) == (2 if rho else 0)
        res = _skeleton_runs(cg, Cm, Th, ML, 3)
        for r in res:
            _is_oracle_skeleton(r, ref)
            _same_bytes(r, res[0])
        _calls_hold(res, hetcor=False)


def test_world_one_returns_to_the_plain_path(cg):
    Cm, info, Th, ref, _ = _case("l3")
    n, l = Cm.shape[0], info["level"]
    Cd = cg.DeviceArray(Cm)
    try:
        run = lambda e: (e.run_skeleton(Cd.ptr, n, Th, l), Cd.ptr)  # noqa: E731
        fresh = _single(cg, "l3", Cm, Th, l, {})
        with ShardGroup(2) as g:
            first = g.run(run)
            assert len(first[0].calls) == l
            for e in g.engines:
                e.set_row_shard(0, 1)
            again = g.run(run)
        for r in again:  # each engine on its own now: the whole block, no exchange
            assert r.calls == []
            _is_oracle_skeleton(r, ref)
            _same_bytes(r, fresh)
    finally:
        Cd.free()


# ---------------------------------------------------------------------------------------------------------------------
# (e) device buffers with more than one participant
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", [("l4", 3), ("hub17", 2)])
def test_device_buffer_exchange_joins_several_engines(cg, name, world):
    if name == "l4":
        Cm, info, Th, ref, _ = _case(name)
        maxlevel = info["level"]
    else:
        Cm, Th, ref, _ = _deep(name)
        maxlevel = ML
    host = _skeleton_runs(cg, Cm, Th, maxlevel, world)
    dev = _skeleton_runs(cg, Cm, Th, maxlevel, world, device_buffers=True)
    for h, d in zip(host, dev):
        _is_oracle_skeleton(d, ref)
        _same_bytes(d, h)
    want_host = _calls_hold(host, hetcor=False, on_device=0)
    want_dev = _calls_hold(dev, hetcor=False, on_device=1)
    assert [c[:3] for c in want_host] == [c[:3] for c in want_dev] and len(want_dev) == maxlevel


def test_device_buffer_exchange_hetcor(cg):
    Cm, info, _, _, _ = _case("l4")
    Nm, ti, th, ref, _ = _hetcor_case("l4", False, True)
    res = _hetcor_runs(cg, Cm, th, info["level"], 3, ess=float(info["N"]), ti=ti, device_buffers=True)
    for r in res:
        assert r.stats.level == ref.level and np.array_equal(r.adjacency, ref.G)
    _calls_hold(res, hetcor=True, on_device=1)


# ---------------------------------------------------------------------------------------------------------------------
# (f) queue overflow, (g) failure, (h) sensitivity
# ---------------------------------------------------------------------------------------------------------------------
def test_recheck_queue_overflow_is_settled_before_the_join(cg):
    Cm, info, Th, ref, _ = _case("l4")
    l = info["level"]
    res = _skeleton_runs(cg, Cm, Th, l, 3, {"queue_capacity": 1})
    assert any(r.stats.exact_fallbacks > 0 for r in res)
    one = _single(cg, "l4", Cm, Th, l, {})
    for r in res:
        _is_oracle_skeleton(r, ref)
        _same_bytes(r, one)
    _calls_hold(res, hetcor=False)  # one join per level, the redone ones included


def test_failing_exchange_is_an_error_and_the_engines_recover(cg):
    Cm, info, Th, ref, _ = _case("l3")
    n, l = Cm.shape[0], info["level"]
    Cd = cg.DeviceArray(Cm)
    try:
        run = lambda e: (e.run_skeleton(Cd.ptr, n, Th, l), Cd.ptr)  # noqa: E731
        fail_at_2 = lambda join: (lambda rank, level, mine: None if level == 2 else join(rank, level, mine))  # noqa: E731
        with ShardGroup(2) as g:
            bad = g.run(run, exchange_wrap=fail_at_2, return_errors=True)  # (returning at all: no thread is left alive)
            for r in bad:
                assert isinstance(r.error, RuntimeError) and "row-shard exchange failed at level 2" in str(r.error), r.error
                assert [c[0] for c in r.calls] == [1, 2]
            good = g.run(run)
        one = _single(cg, "l3", Cm, Th, l, {})
        for r in good:
            _is_oracle_skeleton(r, ref)
            _same_bytes(r, one)
        _calls_hold(good, hetcor=False)
    finally:
        Cd.free()


@pytest.mark.parametrize("name,world", [("l3", 3), ("hub17", 2)])
def test_without_the_join_rank_0_gets_another_graph(cg, name, world):
    """so that nothing above can pass with a join that is lost: every rank keeps its own buffer (no barrier either), and
    what the other ranks' rows would have removed stays in rank 0's graph"""
    if name == "l3":
        Cm, info, Th, ref, _ = _case(name)
        maxlevel = info["level"]
    else:
        Cm, Th, ref, _ = _deep(name)
        maxlevel = ML
    res = _skeleton_runs(cg, Cm, Th, maxlevel, world, exchange_wrap=_identity)
    G = res[0].adjacency
    assert not np.array_equal(G, ref.G)
    assert all(c[3] == 0 for c in res[0].calls) and len(res[0].calls) >= 1
