"""CPU: batched block runs at per-pair sample sizes above the engine -- the three new entry points in the header, in the
ctypes table and in the library, the argument rules of `run_blocks.py --het-batch-vars`, and the numpy restatement of
the block-diagonal sample-size matrix that the GPU test (test_gpu_cusk_het_batch.py) compares cusk_ess_square_batch with."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_cusk_het_formats import ess_square_expected, ess_square_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"cusk_run_skeleton_batch_het": 10, "cusk_ess_square_batch": 10, "cusk_blockset_run_batch_het": 6}
SENTINEL = np.uint32(0xC0DE5EED)  # bit pattern of the cells cusk_ess_square_batch must not write (no size takes it)


def ess_square_batch_expected(mxp_list, pxp_list, m, base, p: int, n_uniform: float, n: int) -> np.ndarray:
    """What cusk_ess_square_batch leaves in an n x n allocation that held SENTINEL everywhere: block b = variables
    base[b] .. base[b] + m[b] + p gets the matrix of cusk_ess_square in its diagonal block, every other cell keeps its
    pattern.  -> uint32 view (NaN payloads and the sentinel compare as bits)."""
    out = np.full((n, n), SENTINEL, np.uint32)
    for mxp, pxp, mb, b0 in zip(mxp_list, pxp_list, m, base):
        nb = mb + p
        assert b0 % 64 == 0 and b0 + nb <= n
        out[b0:b0 + nb, b0:b0 + nb] = ess_square_expected(mxp, pxp, mb, p, n_uniform).view(np.uint32)
    return out


def test_block_diagonal_restatement_on_one_block_is_ess_square_expected():
    m, p, N = 5, 3, 16384.0
    mxp, pxp = ess_square_inputs(m, p, seed=1)
    one = ess_square_expected(mxp, pxp, m, p, N)
    for base, n in ((0, 8), (64, 128), (64, 75)):
        sq = ess_square_batch_expected([mxp], [pxp], [m], [base], p, N, n)
        assert sq.shape == (n, n) and sq.dtype == np.uint32
        assert np.array_equal(sq[base:base + 8, base:base + 8], one.view(np.uint32))
        outside = np.ones((n, n), bool)
        outside[base:base + 8, base:base + 8] = False
        assert np.all(sq[outside] == SENTINEL) and not np.any(sq[~outside] == SENTINEL)
    # two blocks: each keeps its own tables, the cells between them keep the pattern
    mxp2, pxp2 = ess_square_inputs(7, p, seed=2)
    sq = ess_square_batch_expected([mxp, mxp2], [pxp, pxp2], [m, 7], [0, 64], p, N, 128)
    assert np.array_equal(sq[:8, :8], one.view(np.uint32))
    assert np.array_equal(sq[64:74, 64:74], ess_square_expected(mxp2, pxp2, 7, p, N).view(np.uint32))
    assert np.all(sq[:8, 8:] == SENTINEL) and np.all(sq[64:74, :64] == SENTINEL) and np.all(sq[74:, :] == SENTINEL)


def _declared(name: str) -> list:
    txt = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cusk_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW_SYMBOLS))
def test_batch_het_symbols_are_declared_and_resolved_with_matching_arguments(name):
    from cigwas_amd._lib import SYMBOLS

    assert len(_declared(name)) == NEW_SYMBOLS[name]
    assert name in SYMBOLS and len(SYMBOLS[name][1]) == NEW_SYMBOLS[name]


def test_declared_signatures_are_the_ones_of_the_issue():
    flat = lambda name: " ".join(" ".join(_declared(name)).split())
    assert flat("cusk_ess_square_batch") == ("cusk_engine *e const float *mxp_ess const float *pxp_ess int nblk const int *m "
                                            "const int *base size_t p float n_uniform int n float *N_dev")
    assert flat("cusk_run_skeleton_batch_het") == ("cusk_engine *e const float *C_dev const float *N_dev int n int nblk "
                                                  "const int *lo const int *hi float th int maxlevel cusk_stats *stats")
    assert flat("cusk_blockset_run_batch_het") == ("cusk_blockset *bs cusk_engine *e const int *block_indices int nblocks "
                                                  "cusk_batch_result **out cusk_batch_stats *stats")


def test_library_exports_the_batch_het_symbols():
    so = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")
    assert os.path.exists(so), "libcusk_hip.so is not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(so)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_python_wrappers_exist():
    from cigwas_amd import run_blocks
    from cigwas_amd.skeleton import Engine

    assert callable(Engine.run_skeleton_batch_het) and callable(Engine.ess_square_batch)
    assert callable(run_blocks.BlockSet.run_batch_het)
    import inspect

    assert inspect.signature(run_blocks.run_rank_batched).parameters["het"].default is False
    assert inspect.signature(run_blocks.run_job).parameters["het"].default is False


BASE = ["y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out"]


def test_het_batch_vars_implies_het_and_takes_the_batch_size():
    from cigwas_amd import run_blocks

    a = run_blocks.parse_args(BASE + ["--het-batch-vars", "4096"])
    assert a.het is True and a.het_batch_vars == 4096
    a = run_blocks.parse_args(BASE + ["--het", "--het-batch-vars", "256", "--batch-vars", "0", "--writer", "local"])
    assert a.het is True and a.het_batch_vars == 256 and a.writer == "local"
    # 0 or absent: the flag is not there
    assert run_blocks.parse_args(BASE).het_batch_vars == 0 and not run_blocks.parse_args(BASE).het
    a = run_blocks.parse_args(BASE + ["--het-batch-vars", "0"])
    assert not a.het and a.het_batch_vars == 0 and a.batch_vars == 16384


def test_het_batch_vars_beside_batch_vars_is_an_argument_error(capsys):
    from cigwas_amd import run_blocks

    with pytest.raises(SystemExit) as ex:
        run_blocks.parse_args(BASE + ["--het-batch-vars", "4096", "--batch-vars", "4096"])
    assert ex.value.code == 2 and "--het-batch-vars" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ex:
        run_blocks.parse_args(BASE + ["--het-batch-vars", "-1"])
    assert ex.value.code == 2


def test_help_states_the_memory_of_a_het_batch(capsys):
    from cigwas_amd import run_blocks

    with pytest.raises(SystemExit):
        run_blocks.parse_args(["--help"])
    txt = " ".join(capsys.readouterr().out.split())
    assert "--het-batch-vars" in txt and "2 x 4 x V^2 bytes" in txt
