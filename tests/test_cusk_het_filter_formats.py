"""CPU: option het_filter above the engine -- the new block-set setter in the header, the ctypes table and the library,
the argument rules of `--het-filter` (run_blocks.py, cli.py) and the `mps cusk ... het filter` argv the shim builds --
and the premise of the GPU test's recheck cap (test_gpu_cusk_het_filter.py): restated in float64 on the inputs of that
test, the share of tests that verdict_z cannot certify (guard band lth kBeta / 2 + 2e-6 on z, or one of the 1/64
conditioning guards) stays below the cap the GPU test asserts."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from test_gpu_cusk_het import het_threshold_f32
from test_het_class_cases import ML, deep_case, deep_graphs, table_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out"]
CUSK_ARGS = ["cusk", "3", "b.blocks", "stem", "y.phen", "0.0001", "3", "14", "1", "out/"]
K_BETA = 1.0 / 512.0   # ci_fast.h
K_COND_MIN = 1.0 / 64.0
RECHECK_CAP = 0.02     # the GPU test: sum(rechecks[2:]) <= RECHECK_CAP * sum(tests[2:])


def _declared(name: str) -> list:
    txt = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cusk_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_setter_is_declared_resolved_and_exported():
    from cigwas_amd._lib import SYMBOLS

    assert " ".join(" ".join(_declared("cusk_blockset_set_het_filter")).split()) == "cusk_blockset *bs int on"
    assert len(SYMBOLS["cusk_blockset_set_het_filter"][1]) == 2
    so = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")
    assert os.path.exists(so), "libcusk_hip.so is not built (run __graft_entry__.build())"
    assert hasattr(ctypes.CDLL(so), "cusk_blockset_set_het_filter")


def test_header_lists_the_option():
    txt = " ".join(open(os.path.join(ROOT, "include", "cusk_hip.h")).read().split())
    assert '"het_filter" (default 0' in txt


def test_python_wrappers_take_the_switch():
    from cigwas_amd import run_blocks

    assert callable(run_blocks.BlockSet.set_het_filter)
    assert inspect.signature(run_blocks.run_job).parameters["het_filter"].default is False


def test_run_blocks_het_filter_needs_a_het_run(capsys):
    from cigwas_amd import run_blocks

    a = run_blocks.parse_args(BASE + ["--het", "--het-filter"])
    assert a.het and a.het_filter and a.batch_vars == 0
    a = run_blocks.parse_args(BASE + ["--het-batch-vars", "4096", "--het-filter"])
    assert a.het and a.het_filter and a.het_batch_vars == 4096
    assert not run_blocks.parse_args(BASE + ["--het"]).het_filter and not run_blocks.parse_args(BASE).het_filter
    for extra in ([], ["--batch-vars", "4096"], ["--het-batch-vars", "0"]):
        with pytest.raises(SystemExit) as ex:
            run_blocks.parse_args(BASE + ["--het-filter"] + extra)
        assert ex.value.code == 2 and "--het-filter" in capsys.readouterr().err


def test_run_blocks_rejects_het_filter_before_any_engine_exists(monkeypatch):
    """main() parses first: the argument error comes before the block set is opened or torch is imported"""
    from cigwas_amd import run_blocks

    def boom(*a, **k):
        raise AssertionError("a block set was opened")

    monkeypatch.setattr(run_blocks, "BlockSet", boom)
    with pytest.raises(SystemExit) as ex:
        run_blocks.main(BASE + ["--het-filter"])
    assert ex.value.code == 2


def test_cli_cusk_het_filter_appends_two_arguments():
    from cigwas_amd import cli

    p = cli.build_parser()
    plain = cli.cusk_argv(p.parse_args(CUSK_ARGS))
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het", "--het-filter"])) == plain + ["het", "filter"]
    assert cli.cusk_argv(p.parse_args(["cusk", "--het-filter", "--het"] + CUSK_ARGS[1:])) == plain + ["het", "filter"]
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het"])) == plain + ["het"]
    with pytest.raises(SystemExit) as ex:
        cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het-filter"]))
    assert "--het-filter" in str(ex.value.code)


# ---------------------------------------------------------------------------------------------------------------------
# the recheck cap's premise
# ---------------------------------------------------------------------------------------------------------------------
def uncertain_share(C32, N32, q, start, levels, max_ranks):
    """Over the rows of the graphs start[l] (the graph level l starts with) and the first max_ranks conditioning sets of
    every row: (tests, tests verdict_z would not certify), in float64.  A test (x, y | S) is uncertain when a pivot of
    the Cholesky factor of C[S, S], H00 or H11 is below 1/64, when |z - t| <= t kBeta / 2 + 2e-6 with
    t = q / sqrt(mean size - l - 3) (sizes truncated to integers, read in mean_ess's orientation), or when t is NaN."""
    C = C32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        Ni = np.nan_to_num(np.trunc(N32.astype(np.float64)), nan=0.0)
    tests = unsure = 0
    for l in levels:
        G = start[l]
        npairs = (l + 2) * (l + 1) / 2.0
        for x in range(G.shape[0]):
            nb = np.flatnonzero(G[x] == 1)
            d = len(nb)
            if d <= l:
                continue
            for idx in itertools.islice(itertools.combinations(range(d), l), max_ranks):
                S = nb[list(idx)]
                M = C[np.ix_(S, S)]
                try:
                    F = np.linalg.cholesky(M)
                    piv = float((np.diag(F) ** 2).min())
                except np.linalg.LinAlgError:
                    piv = 0.0
                keep = np.ones(d, bool)
                keep[list(idx)] = False
                cnt = int(keep.sum())
                tests += cnt
                if piv < K_COND_MIN:
                    unsure += cnt
                    continue
                a = np.linalg.solve(F, C[x, S])
                B = np.linalg.solve(F, C[np.ix_(S, nb[keep])])
                h00 = 1.0 - a @ a
                h11 = 1.0 - (B * B).sum(0)
                h01 = C[x, nb[keep]] - a @ B
                with np.errstate(invalid="ignore", divide="ignore"):
                    rho = h01 / np.sqrt(h00 * h11)
                    z = np.abs(0.5 * np.log(np.abs((1.0 + rho) / (1.0 - rho))))
                    common = Ni[S, x].sum() + sum(Ni[S[i], S[j]] for i in range(l) for j in range(i))
                    mean = (common + Ni[nb[keep], x] + Ni[np.ix_(S, nb[keep])].sum(0)) / npairs
                    t = q / np.sqrt(mean - l - 3.0)
                    band = t * (0.5 * K_BETA) + 2e-6
                    sure = (h00 >= K_COND_MIN) & (h11 >= K_COND_MIN) & ((z < t - band) | (z > t + band))
                unsure += int((~sure).sum())
    return tests, unsure


@pytest.mark.parametrize("name,form", [(n, f) for n in ("dense48", "dense96") for f in ("sym", "asym")])
def test_dense_cases_stay_below_the_recheck_cap(name, form):
    """Measured (first 150 sets per row, levels 2 .. the case's last): the printed line has the share."""
    c = table_case(name, form)
    start = {l: c["G"][l - 1] for l in range(2, c["levels"] + 1)}
    tests, unsure = uncertain_share(c["C"], c["N"], float(np.float32(c["th"])), start, range(2, c["levels"] + 1), 150)
    print(f"{name} {form}: {unsure} of {tests} restated tests are not certified ({unsure / tests:.2e})")
    assert tests > 10000 and unsure <= RECHECK_CAP * tests


@pytest.mark.parametrize("form", ("sym", "asym"))
def test_deep_case_stays_below_the_recheck_cap(form):
    """levels 5, 9 and 14 of deep_removal_case (first 25 sets per row): conditioning sets of up to 14 members drawn from
    rows of at most 20 neighbours"""
    c = deep_case()
    G, _ = deep_graphs(form)
    levels = (5, 9, ML)
    start = {l: G[l - 1] for l in levels}
    tests, unsure = uncertain_share(c["C"], c["N"][form], float(np.float32(c["th"])), start, levels, 25)
    print(f"deep {form}: {unsure} of {tests} restated tests are not certified ({unsure / tests:.2e})")
    assert tests > 2000 and unsure <= RECHECK_CAP * tests


# ---------------------------------------------------------------------------------------------------------------------
# the union identity the union-major het sweep rests on
# ---------------------------------------------------------------------------------------------------------------------
def per_test_thresholds(Nm, th, x, T):
    """float32 bit patterns of the restated per-test threshold of (x, t | T - t) for every t of the union T, each summed
    in mean_ess's own pair order over vix = [x, t, S...]: N[vix[i]][vix[j]], j < i"""
    out = []
    for t in T:
        vix = [x, t] + [v for v in T if v != t]
        sizes = [Nm[vix[i], vix[j]] for i in range(len(vix)) for j in range(i)]
        out.append(np.float32(het_threshold_f32(th, sizes, len(T) - 1)).view(np.uint32))
    return out


def unions_met(G, l, rng, first=12, drawn=12):
    """per row of the graph level l starts with: its first (l + 1)-subsets of neighbours and a seeded draw of others"""
    for x in range(G.shape[0]):
        nb = np.flatnonzero(G[x] == 1)
        if len(nb) < l + 1:
            continue
        for T in itertools.islice(itertools.combinations(nb, l + 1), first):
            yield x, [int(v) for v in T]
        for _ in range(drawn):
            yield x, sorted(int(v) for v in rng.choice(nb, l + 1, replace=False))


def test_the_tests_of_a_union_share_one_threshold_when_the_sizes_are_symmetric():
    """hub_corr(94, 2, 4) at levels 2-4: with symmetric het_sizes every union's l + 1 thresholds are one float32 bit
    pattern (what the union-major sweep rests on); with the raw sizes some union's differ (why it needs the symmetry
    check)"""
    rng = np.random.default_rng(3)
    sym, asym = table_case("hub96", "sym"), table_case("hub96", "asym")
    checked = differing = 0
    for l in (2, 3, 4):
        G = sym["G"][min(l - 1, sym["levels"])]
        for x, T in unions_met(G, l, rng):
            assert len(set(per_test_thresholds(sym["N"], sym["th"], x, T))) == 1, (l, x, T)
            differing += len(set(per_test_thresholds(asym["N"], asym["th"], x, T))) > 1
            checked += 1
    print(f"{checked} unions checked; with the raw sizes {differing} have thresholds that differ")
    assert checked > 5000 and differing > 0
