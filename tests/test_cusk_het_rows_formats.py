"""CPU: option het_rows above the engine -- the two new symbols (header, ctypes table, library), the argument rules of
`mps cusk ... het [filter] [rows]`, `run_blocks.py --het-rows` and `cli.py cusk --het-rows`, the launch sizes of the HET
forms of the level-1 row kernel -- and the premise of the kernel's widened guard band: restated in numpy float32, a
verdict the filter certifies at its estimate of tanh(lth)^2 is the verdict of the exact float32 arithmetic."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_cusk_het import MPS, het_threshold_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out"]
CUSK_ARGS = ["cusk", "3", "b.blocks", "stem", "y.phen", "0.0001", "3", "14", "1", "out/"]


def _declared(name: str) -> list:
    txt = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cusk_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_new_symbols_are_declared_resolved_and_exported():
    from cigwas_amd._lib import SYMBOLS

    assert " ".join(" ".join(_declared("cusk_blockset_set_het_rows")).split()) == "cusk_blockset *bs int on"
    assert " ".join(" ".join(_declared("cusk_engine_level1_form")).split()) == "const cusk_engine *e"
    assert len(SYMBOLS["cusk_blockset_set_het_rows"][1]) == 2 and len(SYMBOLS["cusk_engine_level1_form"][1]) == 1
    so = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")
    assert os.path.exists(so), "libcusk_hip.so is not built (run __graft_entry__.build())"
    dll = ctypes.CDLL(so)
    assert hasattr(dll, "cusk_blockset_set_het_rows") and hasattr(dll, "cusk_engine_level1_form")
    assert dll.cusk_engine_level1_form(None) == -1 and dll.cusk_blockset_set_het_rows(None, 1) != 0


def test_header_lists_the_option_and_python_takes_the_switch():
    from cigwas_amd import run_blocks, skeleton

    txt = " ".join(open(os.path.join(ROOT, "include", "cusk_hip.h")).read().split())
    assert '"het_rows" (0 or 1, default 0' in txt
    assert callable(run_blocks.BlockSet.set_het_rows) and callable(skeleton.Engine.level1_form)
    assert inspect.signature(run_blocks.run_job).parameters["het_rows"].default is False


def test_run_blocks_het_rows_needs_a_het_run(capsys, monkeypatch):
    from cigwas_amd import run_blocks

    a = run_blocks.parse_args(BASE + ["--het", "--het-rows"])
    assert a.het and a.het_rows and not a.het_filter and a.batch_vars == 0
    a = run_blocks.parse_args(BASE + ["--het-batch-vars", "4096", "--het-filter", "--het-rows"])
    assert a.het and a.het_rows and a.het_filter and a.het_batch_vars == 4096
    assert not run_blocks.parse_args(BASE + ["--het"]).het_rows and not run_blocks.parse_args(BASE).het_rows
    for extra in ([], ["--batch-vars", "4096"], ["--het-batch-vars", "0"]):
        with pytest.raises(SystemExit) as ex:
            run_blocks.parse_args(BASE + ["--het-rows"] + extra)
        assert ex.value.code == 2 and "--het-rows" in capsys.readouterr().err

    def boom(*a, **k):
        raise AssertionError("a block set was opened")

    monkeypatch.setattr(run_blocks, "BlockSet", boom)  # main() parses first: no block set, no engine
    with pytest.raises(SystemExit) as ex:
        run_blocks.main(BASE + ["--het-rows"])
    assert ex.value.code == 2


def test_cli_cusk_het_rows_appends_rows():
    from cigwas_amd import cli

    p = cli.build_parser()
    plain = cli.cusk_argv(p.parse_args(CUSK_ARGS))
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het", "--het-rows"])) == plain + ["het", "rows"]
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het-rows", "--het", "--het-filter"])) == plain + ["het", "filter", "rows"]
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het", "--het-filter"])) == plain + ["het", "filter"]
    with pytest.raises(SystemExit) as ex:
        cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het-rows"]))
    assert "--het-rows" in str(ex.value.code)


@pytest.mark.parametrize("extra,ok", [(["het", "rows"], True), (["het", "filter", "rows"], True), (["het", "rows", "filter"], True),
                                      (["het", "rows", "rows"], False), (["rows"], False), (["het", "rowz"], False)])
def test_mps_cusk_trailing_words(tmp_path, extra, ok):
    """the argv is parsed before any file is opened or any device call is made: accepted words get as far as the missing
    .phen file (a different message), the others end with the trailing-argument error and status 1"""
    assert os.path.exists(MPS), "the mps host program is not built (run __graft_entry__.build())"
    argv = [MPS, "cusk", str(tmp_path / "no.phen"), str(tmp_path / "no"), str(tmp_path / "no.blocks"), "0.0001", "3", "14", "1",
            str(tmp_path), "0"] + extra
    r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0
    if ok:
        assert "unknown trailing argument" not in r.stderr and "het: per-pair sample sizes" in r.stdout
        assert "level 1 on the row kernel" in r.stdout and ("through the filter" in r.stdout) == ("filter" in extra)
    else:
        assert r.returncode == 1 and "unknown trailing argument" in r.stderr and "Got args" not in r.stdout


def _het_row_bytes(n):
    """launch_level1_rows, HET: the row of C (n + 8 floats) and behind it, on a 16-byte boundary, the row of N"""
    return 4 * (((n + 8 + 3) & ~3) + n + 8)


def test_launch_sizes_of_the_het_forms():
    """mode 2 of the query = the HET forms (12 waves per CU whatever `validate` is): three rows of 256 threads at n = 1,301;
    at n = 10,020 one doubled row per CU is all that fits, and at 20,000 not even that at 512 threads: both gather
    """
    from cigwas_amd._lib import lib

    f = lib().cusk_level1_rows_threads
    for validate in (0, 1):
        assert [f(_het_row_bytes(n), 2, validate, 0) for n in (1301, 10020, 20000)] == [256, 0, 0]
        assert f(_het_row_bytes(1301), 2, validate, 512) == 512 and f(_het_row_bytes(10020), 2, validate, 256) == 256  # forced: one row is enough
        assert f(_het_row_bytes(20000), 2, validate, 512) == 0
        # a batch of blocks of at most 5,000 variables keeps three rows of 256 threads
        assert f(_het_row_bytes(5000), 2, validate, 0) == 256
    # mode 2 is not mode 0: where two rows fit at either size, the plain form's 16 waves take two rows of 512 threads and
    # the 12 of the HET forms two rows of 256
    assert f(60000, 0, 0, 0) == 512 and f(60000, 2, 0, 0) == 256
    assert f(1000, 3, 0, 0) == -1 and f(1000, -1, 0, 0) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the band's premise
# ---------------------------------------------------------------------------------------------------------------------
F = np.float32
K_U_MIN, K_U_MAX, K_D_MIN, K_WIDEN = F(4.1e-6), F(0.0625), F(64.0), F(4.0e-6)
K_BETA0 = F(F(16.0) * F(F(F(2.0) * F(2.4e-7)) + F(3.0e-7))) + K_WIDEN
K_BETA1 = F(F(16.0) * F(2.0)) * F(5.6e-8)


def kernel_estimate(th, s):
    """level1_rows2_kernel<..., HET>: (t2 estimate, band, certifiable) from the float sum s of the three sizes"""
    with np.errstate(all="ignore"):
        dm = F(F(s * F(0.33333334)) - F(4.0))
        th2 = F(np.float64(th) * np.float64(th))
        u = F(th2 * F(F(1.0) / dm))
        pu = F(F(1.0) + F(u * F(F(-0.33333334) + F(u * F(F(0.13333334) + F(u * F(F(-0.053968254) + F(u * F(0.021869488)))))))))
        t2 = F(u * F(pu * pu))
        be = F(K_BETA0 + F(K_BETA1 * F(F(1.0) / np.sqrt(t2))))
        ok = bool(dm >= K_D_MIN and u >= K_U_MIN and u <= K_U_MAX)
    return t2, be, ok


def filter_verdict(h00, h01, hc, t2, be):
    lhs, rhs = F(h01 * h01), F(t2 * F(h00 * hc))
    p, f = lhs < F(rhs * F(F(1.0) - be)), lhs > F(rhs * F(F(1.0) + be))
    return bool(p), bool(h00 > 0 and hc > 0 and (p or f))


def exact_verdict(h00, h01, hc, lth):
    """level1_exact: rho in float32, z_below<true>'s decisive form |0.5 (log|1 + r| - log|1 - r|)| < lth with correctly
    rounded float logs"""
    with np.errstate(all="ignore"):
        rho = F(h01 / F(np.sqrt(np.abs(h00)) * np.sqrt(np.abs(hc))))
        d = F(F(np.log(np.float64(np.abs(F(F(1.0) + rho))))) - F(np.log(np.float64(np.abs(F(F(1.0) - rho))))))
        return bool(np.abs(F(F(0.5) * d)) < lth)


def test_certified_verdicts_are_the_exact_float32_verdicts():
    rng = np.random.default_rng(5)
    grid = [5, 6, 7, 1000, 16384, 500001, 8388607, 8388608, 8388609, 10000000]
    triples = [(a, a, a) for a in grid] + [tuple(int(v) for v in rng.choice(grid, 3)) for _ in range(60)]
    triples += [(8388607, 8388609, 10000000), (8388609, 8388607, 8388608), (5, 1000, 500001), (1000, 16384, 500001)]
    th = F(3.8905919)  # the alpha / 2 quantile at alpha = 1e-4
    tests = slow = 0
    for na, nb, nab in triples:
        s = F(F(F(na) + F(nb)) + F(nab))
        lth = het_threshold_f32(th, [na, nb, nab], 1)
        assert lth == het_threshold_f32(th, [nb, na, nab], 1) or (np.isnan(lth))  # both orientations: one float
        t2, be, ok = kernel_estimate(th, s)
        with np.errstate(all="ignore"):
            t = float(np.tanh(np.float64(lth)))
        for _ in range(40):
            rb, c = F(rng.uniform(-0.7, 0.7)), F(rng.uniform(-0.7, 0.7))
            # ra chosen so that rho lands at, just beside, and well off the decision point t (both signs); |rho| stays
            # below 1, as it does for every correlation matrix
            for f in (1.0, 1.0 + 1e-7, 1.0 - 1e-7, 1.0 + 3e-6, 1.0 - 3e-6, 1.0 + 1e-4, 1.0 - 1e-4, 1.5, 0.5, -1.0, 0.0):
                target = 0.0 if not np.isfinite(t) else float(np.clip(f * t, -0.999, 0.999))
                ra = F(float(rb) * float(c) + target * np.sqrt((1.0 - float(rb) ** 2) * (1.0 - float(c) ** 2)))
                hc = F(F(1.0) - F(c * c))
                h00 = F(F(1.0) - F(rb * rb))
                h01 = F(ra - F(rb * c))
                p, sure = filter_verdict(h00, h01, hc, t2, be)
                tests += 1
                if not (ok and sure):
                    slow += 1
                    continue
                assert p == exact_verdict(h00, h01, hc, lth), (na, nb, nab, float(ra), float(rb), float(c), f)
    print(f"{slow} of {tests} restated tests go to the exact form ({slow / tests:.3f})")
    assert tests > 20000 and slow < tests
