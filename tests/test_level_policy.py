"""The level loop's decisions (csrc/host/level_policy.h: kernel of a level and class, classes with work, outcome of
the read-back, saturating binomial) tabulated on the CPU by the stand-alone program tools/level_policy_selftest.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_policy_selftest(tmp_path):
    exe = str(tmp_path / "level_policy_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "level_policy_selftest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "level_policy_selftest: ok" in r.stdout, r.stdout + r.stderr
