"""CPU: `cusk --het` above the engine -- the argv the CLI shim builds, the argument rules of the block driver, the new
entry points in the header and in the ctypes table, and the numpy restatement of the square sample-size matrix that the
GPU test (test_gpu_cusk_het.py) compares cusk_ess_square with."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cusk_run_skeleton_het", "cusk_ess_square", "cusk_blockset_set_het")


def ess_square_expected(mxp_ess, pxp_ess, m: int, p: int, n_uniform: float) -> np.ndarray:
    """What cusk_ess_square writes (make_square_cuskss_inputs with N between markers): n_uniform between markers, the
    marker x trait sizes in both mirror positions, the trait x trait sizes with NaN on their diagonal."""
    n = m + p
    out = np.full((n, n), np.float32(n_uniform), np.float32)
    if p:
        mp = np.asarray(mxp_ess, np.float32).reshape(m, p)
        out[:m, m:] = mp
        out[m:, :m] = mp.T
        out[m:, m:] = np.asarray(pxp_ess, np.float32).reshape(p, p)
        out[np.arange(m, n), np.arange(m, n)] = np.nan
    return out


def ess_square_inputs(m: int, p: int, seed: int, N: float = 16384.0):
    """marker x trait and trait x trait sizes with a few NaN among them (a pair without a correlation has no size)"""
    rng = np.random.default_rng(seed)
    mxp = np.floor(rng.uniform(0.25, 1.0, (m, p)) * N).astype(np.float32)
    pxp = np.floor(rng.uniform(0.25, 1.0, (p, p)) * N).astype(np.float32)
    pxp = np.minimum(pxp, pxp.T)
    if m * p > 2:
        mxp.reshape(-1)[[1, m * p - 2]] = np.nan
    return mxp, pxp


def test_square_restatement_m5_p3():
    m, p, N = 5, 3, 16384.0
    mxp, pxp = ess_square_inputs(m, p, seed=1)
    sq = ess_square_expected(mxp, pxp, m, p, N)
    assert sq.shape == (8, 8) and sq.dtype == np.float32
    assert np.all(sq[:m, :m] == np.float32(N))
    for i in range(m):
        for t in range(p):
            a, b, want = sq[i, m + t], sq[m + t, i], mxp[i, t]
            assert (np.isnan(want) and np.isnan(a) and np.isnan(b)) or (a == want and b == want)
    for a in range(p):
        for b in range(p):
            assert np.isnan(sq[m + a, m + b]) if a == b else sq[m + a, m + b] == pxp[a, b]
    assert np.array_equal(sq, sq.T, equal_nan=True)
    assert np.count_nonzero(np.isnan(sq)) == p + 2 * 2
    # no traits: one number everywhere
    assert np.all(ess_square_expected(None, None, 4, 0, 7.0) == np.float32(7.0))


CUSK_ARGS = ["cusk", "3", "b.blocks", "stem", "y.phen", "0.0001", "3", "14", "1", "out/"]


def test_cli_cusk_het_appends_one_argument():
    from cigwas_amd import cli

    plain = cli.cusk_argv(cli.build_parser().parse_args(CUSK_ARGS))
    assert plain[1:] == ["cusk", "y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out/", "3"]
    het = cli.cusk_argv(cli.build_parser().parse_args(CUSK_ARGS + ["--het"]))
    assert het == plain + ["het"]
    assert cli.cusk_argv(cli.build_parser().parse_args(["cusk", "--het"] + CUSK_ARGS[1:])) == het


def test_cli_cusk_without_the_flag_is_the_pinned_argv():
    """tests/golden/merge/argv.json holds the argv of the workflow's commands as they were before the flag existed"""
    from cigwas_amd import cli

    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "merge", "argv.json")))["cusk"]
    got = cli.cusk_argv(cli.build_parser().parse_args(pinned["cli"]))
    assert got[0] == cli.MPS_PATH and got[1:] == pinned["mps_argv"][1:]
    assert cli.cusk_argv(cli.build_parser().parse_args(pinned["cli"] + ["--het"]))[1:] == pinned["mps_argv"][1:] + ["het"]


def test_run_blocks_het_argument_rules(capsys):
    from cigwas_amd import run_blocks

    base = ["y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out"]
    with pytest.raises(SystemExit) as ex:
        run_blocks.parse_args(base + ["--het", "--batch-vars", "4096"])
    assert ex.value.code == 2 and "--het" in capsys.readouterr().err
    a = run_blocks.parse_args(base + ["--het"])
    assert a.het and a.batch_vars == 0
    a = run_blocks.parse_args(base + ["--het", "--batch-vars", "0", "--writer", "local"])
    assert a.het and a.batch_vars == 0 and a.writer == "local"
    # without the flag nothing changes: batched by default, an explicit value is taken
    a = run_blocks.parse_args(base)
    assert not a.het and a.batch_vars == 16384
    assert run_blocks.parse_args(base + ["--batch-vars", "4096"]).batch_vars == 4096


def _declared(name: str) -> list:
    txt = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cusk_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,nargs", [("cusk_run_skeleton_het", 7), ("cusk_ess_square", 7), ("cusk_blockset_set_het", 2)])
def test_new_symbols_are_declared_and_resolved_with_matching_arguments(name, nargs):
    from cigwas_amd._lib import SYMBOLS

    args = _declared(name)
    assert len(args) == nargs
    assert name in SYMBOLS and len(SYMBOLS[name][1]) == nargs


def test_declared_signatures_are_the_ones_of_the_issue():
    flat = lambda name: " ".join(" ".join(_declared(name)).split())
    assert flat("cusk_run_skeleton_het") == ("cusk_engine *e const float *C_dev const float *N_dev int n float th "
                                            "int maxlevel cusk_stats *stats")
    assert flat("cusk_ess_square") == ("cusk_engine *e const float *mxp_ess const float *pxp_ess size_t m size_t p "
                                      "float n_uniform float *N_dev")


def test_library_exports_the_new_symbols():
    import ctypes

    so = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")
    if not os.path.exists(so):
        pytest.skip("libcusk_hip.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(so)
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)


def test_engine_wrappers_exist():
    from cigwas_amd.skeleton import Engine

    assert callable(Engine.run_skeleton_het) and callable(Engine.ess_square)
