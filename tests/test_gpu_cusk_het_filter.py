"""GPU: engine option het_filter -- cusk_run_skeleton_het / cusk_run_skeleton_batch_het with levels >= 2 through the
filter at the per-test threshold (sweep_fast_kernel<L, 0, true, ...>) and the recheck queue (recheck_kernel<L, 0, true>).

The inputs are those of tests/test_gpu_het_classes.py (checked on the CPU in tests/test_het_class_cases.py), each with
symmetric and raw het_sizes.  With the option the adjacency, the level counter and the separating-set records must be
bit for bit those of the run without it on the same engine (the exact path, which test_gpu_het_classes.py holds to a
float64 restatement of its records), the adjacency and the level those of the oracle's hetcor_skeleton, and the filter
must decide most tests itself.  tests/test_cusk_het_filter_formats.py checks on the CPU that the inputs stay within the
recheck cap asserted here."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cusk_het import B_ALPHA, B_DEPTH, B_L1, B_L2, B_N, B_P, B_SIZES, MPS, make_dataset
from test_het_class_cases import DEEP_LEVELS, FORMS, ML, ODD_LEVELS, TABLE_NAMES, deep_case, deep_graphs, odd_case, table_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = [{}, {"tmaj_min_level": 99}, {"tmaj_min_level": 2}, {"max_staged_classes": 0}, {"validate": 1}]
CASES = TABLE_NAMES + ["deep"]
RECHECK_CAP = 0.02
# (measured: the largest share of queued tests over all cases and option sets is 4.0e-5, on hub200 with symmetric sizes;
# no hub case needs the weaker "rechecks < tests" the 1/64 conditioning guard might have forced)


def _optid(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


@pytest.fixture(scope="module")
def cg():
    import cigwas_amd

    return cigwas_amd


def _case(name, form):
    """-> C, N, th, levels, oracle graph after the last level, oracle level counter"""
    if name == "deep":
        c = deep_case()
        G, level = deep_graphs(form)
        return c["C"], c["N"][form], c["th"], ML, G[ML], level
    c = table_case(name, form)
    return c["C"], c["N"], c["th"], c["levels"], c["G"][c["levels"]], c["level"]


def _start_graph(name, form, l):
    """the oracle's graph at the start of level l (the deep case keeps them from level 5 on)"""
    if name == "deep":
        return deep_graphs(form)[0].get(l - 1)
    return table_case(name, form)["G"][l - 1]


def union_count(G, l):
    """what the union-major sweep counts in `subsets` at level l: every (l + 1)-subset of every row's neighbours, whatever
    is live.  (The set-major sweeps count conditioning sets there, at most C(d, l) per row; `tests` cannot tell the two
    apart, since (d - l) C(d, l) = (l + 1) C(d, l + 1).)"""
    return sum(math.comb(int(d), l + 1) for d in G.sum(1))


def _run(cg, e, Cd, Nd, n, th, levels):
    st = e.run_skeleton_het(Cd.ptr, Nd.ptr, n, th, levels)
    return dict(st=st, G=e.adjacency(), bits=e.adjacency_bits(), rec=e.sepsets(), pmax=e.pmax(Cd.ptr))


def _same_result(a, b):
    assert a["st"].level == b["st"].level
    assert np.array_equal(a["bits"], b["bits"])
    for u, v in zip(a["rec"][:3] + a["rec"][4:], b["rec"][:3] + b["rec"][4:]):  # x, y, level, S
        assert np.array_equal(u, v)
    assert np.allclose(a["pmax"], b["pmax"], rtol=0.0, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=_optid)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES)
def test_het_filter_is_the_exact_het_run(cg, name, form, opts):
    Cm, Nm, th, levels, want_G, want_level = _case(name, form)
    n = Cm.shape[0]
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        for k, v in opts.items():
            if k != "validate":
                e.set_option(k, v)
        base = _run(cg, e, Cd, Nd, n, th, levels)  # het_filter = 0: the exact path (validate is an error there)
        assert sum(base["st"].rechecks) == 0
        e.set_option("het_filter", 1)
        if opts.get("validate"):
            e.set_option("validate", 1)
        got = _run(cg, e, Cd, Nd, n, th, levels)
    finally:
        Cd.free()
        Nd.free()
        e.close()
    st = got["st"]
    tests, rechecks = sum(st.tests[2:]), sum(st.rechecks[2:])
    print(f"{name} {form} {_optid(opts)}: tests per level {list(st.tests[:levels + 1])}, rechecks {list(st.rechecks[:levels + 1])}, "
          f"share {rechecks / max(tests, 1):.3e}, violations {st.violations}, exact fallbacks {st.exact_fallbacks}")
    _same_result(got, base)
    assert st.level == want_level and np.array_equal(got["G"], want_G)  # the oracle (with raw sizes too)
    assert all(st.tests[l] > 0 for l in range(2, levels + 1)), list(st.tests)
    assert st.exact_fallbacks == 0
    assert st.rechecks[0] == 0 and st.rechecks[1] == 0  # levels 0 and 1 stay as they are
    if opts.get("validate"):
        assert st.violations == 0
    if name == "deep":
        assert st.levels_run == 15 and set(DEEP_LEVELS) <= set(int(v) for v in got["rec"][2])
    assert rechecks <= RECHECK_CAP * tests
    # which levels went by unions: with symmetric sizes those from tmaj_min_level on (default 6), with raw sizes none --
    # the symmetry kernel sends them through the set-major filter
    first_tmaj = opts.get("tmaj_min_level", 6)
    for l in range(2, levels + 1):
        G = _start_graph(name, form, l)
        if G is None:
            continue
        by_unions = st.subsets[l] == union_count(G, l)
        assert by_unions == (form == "sym" and l >= first_tmaj), (l, st.subsets[l], union_count(G, l))


def test_fast_0_with_het_filter_is_the_exact_path(cg):
    Cm, Nm, th, levels, want_G, want_level = _case("dense48", "sym")
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        e.set_option("het_filter", 1)
        e.set_option("fast", 0)
        got = _run(cg, e, Cd, Nd, Cm.shape[0], th, levels)
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert sum(got["st"].rechecks) == 0 and got["st"].level == want_level and np.array_equal(got["G"], want_G)


def test_queue_overflow_redoes_the_level_on_the_exact_path(cg):
    Cm, Nm, th, levels, want_G, want_level = _case("hub96", "sym")
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        base = _run(cg, e, Cd, Nd, Cm.shape[0], th, levels)
        e.set_option("het_filter", 1)
        full = _run(cg, e, Cd, Nd, Cm.shape[0], th, levels)
        assert full["st"].rechecks[2] > 1 and full["st"].exact_fallbacks == 0  # the premise: level 2 queues more than one test
        e.set_option("queue_capacity", 1)
        got = _run(cg, e, Cd, Nd, Cm.shape[0], th, levels)
    finally:
        Cd.free()
        Nd.free()
        e.close()
    assert got["st"].exact_fallbacks > 0
    _same_result(got, base)
    assert got["st"].level == want_level and np.array_equal(got["G"], want_G)


@pytest.mark.parametrize("opts", [{}, {"max_staged_classes": 0}, {"validate": 1}], ids=_optid)
def test_unusual_sizes_with_het_filter(cg, opts):
    """NaN, 0, negative, l + 3, +inf and 3e9 among the sizes: a NaN or non-positive radicand leaves the filter as kUnsure
    and the exact path keeps the edge"""
    c = odd_case()
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(c["C"]), cg.DeviceArray(c["N"])
    try:
        base = _run(cg, e, Cd, Nd, c["n"], c["th"], ODD_LEVELS)
        e.set_option("het_filter", 1)
        for k, v in opts.items():
            e.set_option(k, v)
        got = _run(cg, e, Cd, Nd, c["n"], c["th"], ODD_LEVELS)
    finally:
        Cd.free()
        Nd.free()
        e.close()
    st = got["st"]
    print(f"unusual sizes {_optid(opts)}: tests {list(st.tests[:ODD_LEVELS + 1])}, rechecks {list(st.rechecks[:ODD_LEVELS + 1])}")
    assert st.level == c["ref"].level and np.array_equal(got["G"], c["ref"].G)
    _same_result(got, base)
    assert sum(st.rechecks[2:]) > 0 and st.exact_fallbacks == 0  # the tests with a NaN threshold are queued
    if opts.get("validate"):
        assert st.violations == 0


@pytest.mark.parametrize("opts", [{}, {"tmaj_min_level": 2}], ids=_optid)
def test_batch_with_het_filter_is_the_single_block_run_per_block(cg, opts):
    """three blocks of unequal size -- 48 variables, a hub block of 96 (rows of the third degree class), the deep case --
    to level 3, symmetric sizes as the batched entry point requires inside its blocks; per block the single-block run
    WITHOUT the filter, and the oracle where the case tables hold its graph"""
    names = [("dense48", "sym"), ("hub96", "sym"), ("deep", "sym")]
    maxlevel = 3
    th = _case("dense48", "sym")[2]
    mats = []
    for name, form in names:
        Cm, Nm = _case(name, form)[:2]
        mats.append((Cm, Nm, Cm.shape[0]))
    assert len({k for _, _, k in mats}) == 3
    e = cg.Engine(0)
    singles = []
    try:
        for Cm, Nm, k in mats:
            Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
            singles.append(_run(cg, e, Cd, Nd, k, th, maxlevel))
            # the graph each level starts with, from the exact path (the case tables hold the oracle's at another alpha for the deep case)
            singles[-1]["G_start"] = {}
            for l in (2, 3):
                e.run_skeleton_het(Cd.ptr, Nd.ptr, k, th, l - 1)
                singles[-1]["G_start"][l] = e.adjacency()
            Cd.free()
            Nd.free()
        assert all(sum(one["st"].rechecks) == 0 for one in singles)
        e.set_option("het_filter", 1)
        for k, v in opts.items():
            e.set_option(k, v)
        lo, pos = [], 0
        for _, _, k in mats:
            lo.append(pos)
            pos += (k + 63) // 64 * 64
        hi = [a + k for a, (_, _, k) in zip(lo, mats)]
        n = pos + 64
        big = np.full((n, n), np.nan, np.float32)
        bigN = np.full((n, n), 2.0, np.float32)
        bigN[np.triu_indices(n, 1)] = 3.0  # asymmetric outside the blocks: the symmetry kernel must not look there
        for (Cm, Nm, _), a, b in zip(mats, lo, hi):
            big[a:b, a:b], bigN[a:b, a:b] = Cm, Nm
        Cd, Nd = cg.DeviceArray(big), cg.DeviceArray(bigN)
        st = e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, n, lo, hi, th, maxlevel)
        Gs = e.adjacency_blocks()
        x, y, lv, z, S = e.sepsets()
        Cd.free()
        Nd.free()
    finally:
        e.close()
    assert sum(st.rechecks[2:]) > 0 and st.exact_fallbacks == 0
    if opts.get("tmaj_min_level") == 2:  # levels 2 and 3 went by unions although the cells between the blocks are asymmetric
        for l in (2, 3):
            assert st.subsets[l] == sum(union_count(one["G_start"][l], l) for one in singles)
    for (name, form), a, b, G, one in zip(names, lo, hi, Gs, singles):
        assert np.array_equal(G, one["G"]), name
        if name != "deep":
            assert np.array_equal(G, table_case(name, form)["G"][maxlevel]), name  # the oracle
        sel = (x >= a) & (x < b)
        x1, y1, lv1, _z1, S1 = one["rec"]
        assert len(x1) > 0 or name == "deep"  # (at this alpha the deep case's block removes nothing after level 0)
        assert np.array_equal(x[sel] - a, x1) and np.array_equal(y[sel] - a, y1) and np.array_equal(lv[sel], lv1), name
        assert np.array_equal(np.where(S[sel] >= 0, S[sel] - a, -1), S1), name


def test_option_handling(cg):
    Cm, Nm, th, levels, want_G, want_level = _case("dense48", "sym")
    e = cg.Engine(0)
    Cd, Nd = cg.DeviceArray(Cm), cg.DeviceArray(Nm)
    try:
        e.set_option("validate", 1)
        with pytest.raises(RuntimeError, match="validate"):
            e.run_skeleton_het(Cd.ptr, Nd.ptr, Cm.shape[0], th, levels)
        with pytest.raises(RuntimeError, match="validate"):
            e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, Cm.shape[0], [0], [Cm.shape[0]], th, levels)
        e.set_option("het_filter", 1)
        st = e.run_skeleton_het(Cd.ptr, Nd.ptr, Cm.shape[0], th, levels)
        assert st.violations == 0 and np.array_equal(e.adjacency(), want_G)
        st = e.run_skeleton_batch_het(Cd.ptr, Nd.ptr, Cm.shape[0], [0], [Cm.shape[0]], th, levels)
        assert st.violations == 0 and np.array_equal(e.adjacency_blocks()[0], want_G)
        e.set_option("het_filter", 0)
        with pytest.raises(RuntimeError, match="validate"):
            e.run_skeleton_het(Cd.ptr, Nd.ptr, Cm.shape[0], th, levels)
        # a row-sharded engine is refused with the option as without it
        e.set_option("validate", 0)
        e.set_option("het_filter", 1)
        e.set_row_shard(0, 2, exchange=lambda *a: 0)
        with pytest.raises(RuntimeError, match="row-sharded"):
            e.run_skeleton_het(Cd.ptr, Nd.ptr, Cm.shape[0], th, levels)
    finally:
        Cd.free()
        Nd.free()
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory, synth):
    """the PLINK set of test_gpu_cusk_het.py (three blocks, five traits, gaps in traits 1 and 3) and the per-block files
    of the het run without the filter"""
    import cigwas_amd
    import cigwas_amd._lib as L
    from cigwas_amd import run_blocks as rb

    d = tmp_path_factory.mktemp("cusk_het_filter")
    G, _Y, Yg = make_dataset(synth)
    means, stds = synth.bed_stats(G)
    stem = str(d / "geno")
    synth.write_bfiles(stem, synth.pack_bed(G), B_N, means, stds)
    synth.write_phen(str(d / "gaps.phen"), Yg.reshape(-1), B_N, B_P)
    first = 0
    with open(d / "b.blocks", "w") as f:
        for s in B_SIZES:
            f.write(f"1\t{first}\t{first + s - 1}\n")
            first += s
    ds = dict(stem=stem, gaps=str(d / "gaps.phen"), blocks=str(d / "b.blocks"), want=d / "het")
    ds["want"].mkdir()
    stats = {}
    for tag, filt in (("het", False), ("filter", True)):
        # the filtered runs on an engine created with validate = 1: a het run refuses that option unless het_filter has
        # reached the engine, so these runs prove that the block set sets it (the files are the same either way)
        old = os.environ.get("CUSK_OPTIONS")
        if filt:
            os.environ["CUSK_OPTIONS"] = "validate=1"
        try:
            e = cigwas_amd.Engine(0)
        finally:
            if filt:
                os.environ.pop("CUSK_OPTIONS")
                if old is not None:
                    os.environ["CUSK_OPTIONS"] = old
        bs = rb.BlockSet(ds["gaps"], stem, ds["blocks"], float(B_ALPHA), int(B_L1), int(B_L2), int(B_DEPTH))
        bs.set_het(True)
        if filt:
            bs.set_het_filter(True)
            (d / "bs_filter").mkdir()
        stats[tag] = []
        for b in range(len(B_SIZES)):
            res, st = bs.run_block(e, b)
            stats[tag].append(st)
            if res is not None:
                res.write(str(ds["want"] if not filt else d / "bs_filter"))
        L.lib().cusk_blockset_release_engine(bs.h, e.h)
        bs.close()
        e.close()
    ds["stats"] = stats
    ds["bs_filter"] = d / "bs_filter"
    return ds


def _same_files(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and len(fa) >= 10 and len(fa) % 5 == 0, (fa, fb)
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


def test_blockset_set_het_filter_writes_the_het_files_and_sets_the_option(dataset):
    _same_files(str(dataset["want"]), str(dataset["bs_filter"]))
    plain = sum(sum(st.stage[k].rechecks) for st in dataset["stats"]["het"] for k in range(2))
    assert plain == 0
    # the option reached the engine for both stages: the fixture ran them with validate = 1, which is an error without it
    for a, b in zip(dataset["stats"]["het"], dataset["stats"]["filter"]):
        assert a.skipped == b.skipped and a.num_sig == b.num_sig
        for k in range(2):
            assert b.stage[k].exact_fallbacks == 0 and b.stage[k].violations == 0


def test_mps_cusk_het_filter_writes_the_het_files(dataset, tmp_path):
    out = tmp_path / "mps"
    out.mkdir()
    for b in range(len(B_SIZES)):
        argv = [MPS, "cusk", dataset["gaps"], dataset["stem"], dataset["blocks"], B_ALPHA, B_L1, B_L2, B_DEPTH, str(out), str(b),
                "het", "filter"]
        # validate = 1 is an error on a het run unless het_filter reached the engine: without `filter` the same call fails
        r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, CUSK_OPTIONS="validate=1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "levels >= 2 through the filter" in r.stdout
        if b == 0:
            r = subprocess.run(argv[:-1], capture_output=True, text=True, env=dict(os.environ, CUSK_OPTIONS="validate=1"))
            assert r.returncode != 0 and "validate" in r.stdout + r.stderr
    _same_files(str(dataset["want"]), str(out))
    argv = [MPS, "cusk", dataset["gaps"], dataset["stem"], dataset["blocks"], B_ALPHA, B_L1, B_L2, B_DEPTH, str(tmp_path), "0"]
    for extra in (["het", "filtre"], ["het", "filter", "filter"], ["filter"]):
        r = subprocess.run(argv + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "unknown trailing argument" in r.stderr, r.stdout + r.stderr


def test_run_blocks_het_batch_vars_het_filter_writes_the_het_files(dataset, tmp_path):
    out = tmp_path / "rb"
    out.mkdir()
    cmd = [sys.executable, os.path.join(ROOT, "ci-gwas_amd", "run_blocks.py"), dataset["gaps"], dataset["stem"], dataset["blocks"],
           B_ALPHA, B_L1, B_L2, B_DEPTH, str(out), "--het-batch-vars", "256", "--het-filter", "--writer", "local"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["CUSK_OPTIONS"] = "validate=1"  # an error in a het batch unless het_filter reached the engine
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _same_files(str(dataset["want"]), str(out))
