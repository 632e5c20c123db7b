"""The tables of the batched correlation build (csrc/host/corr_plan.h: refused blocks, tiles of each phase, keep mask,
offsets in the staging area) tabulated on the CPU by the stand-alone program tools/corr_plan_selftest.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_corr_plan_selftest(tmp_path):
    exe = str(tmp_path / "corr_plan_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "corr_plan_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "corr_plan_selftest: ok" in r.stdout, r.stdout + r.stderr
