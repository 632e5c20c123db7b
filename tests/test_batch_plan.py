"""The index arithmetic of a batched run and the separating-set remap (csrc/host/batch_plan.h: stage-one layout, gather
tables, adjacency slices, kept blocks, records in the retained numbering) tabulated on the CPU by the stand-alone program
tools/batch_plan_selftest.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_selftest(tmp_path):
    exe = str(tmp_path / "batch_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "batch_plan_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "batch_plan_selftest: ok" in r.stdout, r.stdout + r.stderr
