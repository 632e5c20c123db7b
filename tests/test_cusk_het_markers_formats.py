"""CPU: per-pair sample sizes between markers (`--het-markers`) above the kernels -- the two new entry points and the
block-set switch (header, ctypes table, library), the argument rules of `mps cusk ... het [filter] [rows] [markers]`, `mps
cuskss-bed ... het markers`, `run_blocks.py --het-markers` and `cli.py ... --het-markers` -- and the rule itself restated
in numpy (`marker_pair_counts`, which the GPU tests import), checked on a fixture written by hand."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPS = os.path.join(ROOT, "ci-gwas_amd", "csrc", "mps")
BASE = ["y.phen", "stem", "b.blocks", "0.0001", "3", "14", "1", "out"]
CUSK_ARGS = ["cusk", "3", "b.blocks", "stem", "y.phen", "0.0001", "3", "14", "1", "out/"]
MERGED_ARGS = ["cuskss-merged", "--alpha", "0.0001", "--marker-indices", "m.ixs", "--outdir", "out"]


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def bed_valid(bed, N):
    """rows of .bed bytes (k x ceil(N / 4) uint8) -> k x N bool: the individual's 2-bit code (low bits first) is not 01;
    what the last byte holds beyond individual N is not looked at"""
    bed = np.ascontiguousarray(bed, np.uint8)
    k = bed.shape[0]
    codes = np.stack([(bed >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(k, -1)[:, :N]
    return codes != 1


def marker_pair_counts(bed, N):
    """k x k int64: individuals 0 .. N-1 for which neither marker of the pair is missing"""
    V = bed_valid(bed, N).astype(np.int64)
    return V @ V.T


def test_the_rule_on_a_hand_written_fixture():
    """3 markers, 5 individuals, 2 bytes per row.  Codes per individual (00 = hom, 01 = MISSING, 10 = het, 11 = hom):
         marker 0:  00 10 11 00 11        nothing missing                     byte 0 = 0b00_11_10_00, byte 1 = 0b..._11
         marker 1:  01 00 01 10 00        individuals 0 and 2 missing         byte 0 = 0b10_01_00_01, byte 1 = 0b..._00
         marker 2:  00 01 01 01 01        individuals 1-4 missing             byte 0 = 0b01_01_01_00, byte 1 = 0b..._01
    The last byte of every row carries set bits beyond individual 5 -- 0b11 codes, which would count as observed, and for
    marker 1 the missing code 01 -- that must not matter."""
    bed = np.array([[0b00111000, 0b11111111],
                    [0b10010001, 0b01111100],
                    [0b01010100, 0b11011101]], np.uint8)
    V = bed_valid(bed, 5)
    assert V.astype(int).tolist() == [[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [1, 0, 0, 0, 0]]
    want = [[5, 3, 1], [3, 3, 0], [1, 0, 1]]
    got = marker_pair_counts(bed, 5)
    assert got.dtype == np.int64 and got.tolist() == want
    clean = bed.copy()
    clean[:, 1] &= 0b00000011
    assert marker_pair_counts(clean, 5).tolist() == want
    # at N = 8 the same bytes give other counts: the bits beyond individual 5 were really left out above
    assert marker_pair_counts(bed, 8).tolist() != marker_pair_counts(clean, 8).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# symbols
# ---------------------------------------------------------------------------------------------------------------------
def _declared(name: str) -> list:
    txt = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cusk_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_symbols_are_declared_resolved_and_exported():
    from cigwas_amd._lib import SYMBOLS

    assert _declared("cusk_marker_pair_sizes") == ["cusk_engine *e", "const unsigned char *bed", "const int *marker_ix", "size_t k",
                                                   "size_t m_total", "size_t N", "float *N_dev", "size_t ld"]
    assert _declared("cusk_marker_pair_sizes_batch") == ["cusk_engine *e", "const unsigned char *bed", "const int *marker_ix",
                                                         "size_t m_total", "size_t N", "int nblk", "const int *m", "const int *base",
                                                         "int n", "float *N_dev"]
    assert _declared("cusk_blockset_set_het_markers") == ["cusk_blockset *bs", "int on"]
    assert len(SYMBOLS["cusk_marker_pair_sizes"][1]) == 8 and len(SYMBOLS["cusk_marker_pair_sizes_batch"][1]) == 10
    assert len(SYMBOLS["cusk_blockset_set_het_markers"][1]) == 2
    so = os.path.join(ROOT, "ci-gwas_amd", "csrc", "libcusk_hip.so")
    assert os.path.exists(so), "libcusk_hip.so is not built (run __graft_entry__.build())"
    dll = ctypes.CDLL(so)
    for name in ("cusk_marker_pair_sizes", "cusk_marker_pair_sizes_batch", "cusk_blockset_set_het_markers"):
        assert hasattr(dll, name), name
    assert dll.cusk_blockset_set_het_markers(None, 1) != 0
    # no engine: an argument error, no device call
    assert dll.cusk_marker_pair_sizes(None, None, None, ctypes.c_size_t(1), ctypes.c_size_t(1), ctypes.c_size_t(1), None,
                                      ctypes.c_size_t(1)) != 0


def test_python_takes_the_switch():
    from cigwas_amd import run_blocks, skeleton

    assert callable(run_blocks.BlockSet.set_het_markers)
    assert callable(skeleton.Engine.marker_pair_sizes) and callable(skeleton.Engine.marker_pair_sizes_batch)
    assert inspect.signature(run_blocks.run_job).parameters["het_markers"].default is False


# ---------------------------------------------------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------------------------------------------------
def test_run_blocks_het_markers_needs_a_het_run(capsys, monkeypatch):
    from cigwas_amd import run_blocks

    a = run_blocks.parse_args(BASE + ["--het", "--het-markers"])
    assert a.het and a.het_markers and not a.het_filter and not a.het_rows and a.batch_vars == 0
    a = run_blocks.parse_args(BASE + ["--het-batch-vars", "4096", "--het-filter", "--het-rows", "--het-markers"])
    assert a.het and a.het_markers and a.het_rows and a.het_filter and a.het_batch_vars == 4096
    assert not run_blocks.parse_args(BASE + ["--het"]).het_markers and not run_blocks.parse_args(BASE).het_markers
    for extra in ([], ["--batch-vars", "4096"], ["--het-batch-vars", "0"]):
        with pytest.raises(SystemExit) as ex:
            run_blocks.parse_args(BASE + ["--het-markers"] + extra)
        assert ex.value.code == 2 and "--het-markers" in capsys.readouterr().err

    def boom(*a, **k):
        raise AssertionError("a block set was opened")

    monkeypatch.setattr(run_blocks, "BlockSet", boom)  # main() parses first: no block set, no engine
    with pytest.raises(SystemExit) as ex:
        run_blocks.main(BASE + ["--het-markers"])
    assert ex.value.code == 2


def test_cli_appends_markers():
    from cigwas_amd import cli

    p = cli.build_parser()
    plain = cli.cusk_argv(p.parse_args(CUSK_ARGS))
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het", "--het-markers"])) == plain + ["het", "markers"]
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het-markers", "--het-rows", "--het", "--het-filter"])) == \
        plain + ["het", "filter", "rows", "markers"]
    assert cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het", "--het-rows"])) == plain + ["het", "rows"]
    with pytest.raises(SystemExit) as ex:
        cli.cusk_argv(p.parse_args(CUSK_ARGS + ["--het-markers"]))
    assert "--het-markers" in str(ex.value.code)
    bed = MERGED_ARGS + ["--bfiles", "stem", "--phen", "y.phen"]
    base = cli.cuskss_argv(p.parse_args(bed))
    assert cli.cuskss_argv(p.parse_args(bed + ["--het"])) == base + ["het"]
    assert cli.cuskss_argv(p.parse_args(bed + ["--het", "--het-markers"])) == base + ["het", "markers"]
    with pytest.raises(SystemExit) as ex:
        cli.cuskss_argv(p.parse_args(bed + ["--het-markers"]))
    assert "--het-markers" in str(ex.value.code)
    with pytest.raises(SystemExit) as ex:  # the file route has no marker x marker sizes
        cli.cuskss_argv(p.parse_args(MERGED_ARGS + ["--pxp", "pxp.txt", "--num-samples", "100", "--het-markers"]))
    assert "--het-markers" in str(ex.value.code)


@pytest.mark.parametrize("extra,ok", [(["het", "markers"], True), (["het", "markers", "filter", "rows"], True),
                                      (["het", "filter", "markers", "rows"], True), (["het", "rows", "filter", "markers"], True),
                                      (["het", "markers", "markers"], False), (["markers"], False), (["het", "marker"], False),
                                      (["het", "markers", "het"], False), (["markers", "het"], False)])
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
        assert "marker pairs at their own counts" in r.stdout
        assert ("through the filter" in r.stdout) == ("filter" in extra) and ("on the row kernel" in r.stdout) == ("rows" in extra)
    else:
        assert r.returncode == 1 and "unknown trailing argument" in r.stderr and "Got args" not in r.stdout


@pytest.mark.parametrize("extra", [["markers"], ["het", "marker"], ["het", "markers", "markers"]])
def test_mps_cuskss_bed_rejects_malformed_tails(tmp_path, extra):
    argv = [MPS, "cuskss-bed", str(tmp_path / "no.phen"), str(tmp_path / "no"), str(tmp_path / "no.ixs"), "NULL", "0.0001", "3", "14",
            "1", str(tmp_path)] + extra
    r = subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "cuskss-bed: unknown trailing argument" in r.stderr
    r = subprocess.run([MPS, "cuskss-bed"], capture_output=True, text=True)
    assert r.returncode == 1 and "[het] [markers]" in r.stdout
