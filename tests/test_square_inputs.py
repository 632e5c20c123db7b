"""The sample-size chain, its expansion to the square matrix of `mps cuskss-bed`, the ordinal overlay in both layouts
(csrc/host/square_inputs.h) and the trailing-word parser of the mps commands (csrc/host/trailing_words.h), restated cell
by cell and compared by bits on the CPU by the stand-alone program tools/square_inputs_selftest.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_square_inputs_selftest(tmp_path):
    exe = str(tmp_path / "square_inputs_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "square_inputs_selftest.cpp"),
                           os.path.join(ROOT, "ci-gwas_amd", "csrc", "host", "sumstats_api.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "square_inputs_selftest: ok" in r.stdout, r.stdout + r.stderr
