#!/usr/bin/env python3
"""What `prep-phen` costs at cohort size: N = 500,000 individuals, p = 50 traits, c = 40 covariates, 20 % gaps in ten traits.

  * the kernels of cusk_phen_adjust by HIP events (cusk_phen_timing): median of 5 runs with min and max, after one warm-up,
    inputs resident on the device; the Gram kernel's achieved bytes per second (it reads the c covariates and the trait
    once per adjusted trait: p * (c + 1) * N * 4 bytes) against the 8 TB/s quoted for HBM -- how much of that is served
    by the caches is not known without a counter run of its own;
  * numpy lstsq per trait on this machine's CPUs, for scale;
  * `mps prep-phen` end to end on files (host clock, CUSK_TIMING phases): the share that is text parsing and writing.

    python tools/phen_adjust_time.py [--n 500000] [--p 50] [--c 40] [--out out/phen_adjust_time.json] [--skip-cli]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("scaling", "gram", "solve", "moments", "standardise")


def cohort(N, p, c, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((c, N)).astype(np.float32)
    w = rng.standard_normal((p, c)) / np.sqrt(c)
    Y = (w @ X + rng.standard_normal((p, N))).astype(np.float32)
    for t in range(min(10, p)):
        Y[t, rng.random(N) < 0.2] = np.nan
    return Y, X


def write_table(path, names, M):
    N = M.shape[1]
    with open(path, "w") as f:
        f.write("FID\tIID\t" + "\t".join(names) + "\n")
        for i in range(N):
            f.write(f"f{i}\ti{i}\t" + "\t".join("NA" if v != v else repr(v) for v in M[:, i].tolist()) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--p", type=int, default=50)
    ap.add_argument("--c", type=int, default=40)
    ap.add_argument("--out", type=str, default=os.path.join("out", "phen_adjust_time.json"))
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    import cigwas_amd as cg

    N, p, c = a.n, a.p, a.c
    Y, X = cohort(N, p, c)
    eng = cg.Engine(0)
    Yd, Xd = cg.DeviceArray(Y), cg.DeviceArray(X)
    runs = []
    for k in range(6):
        t0 = time.perf_counter()
        res = eng.phen_adjust(Yd, Xd, N, p, c)
        wall = (time.perf_counter() - t0) * 1e3
        if k:
            runs.append(list(map(float, eng.phen_timing())) + [wall])
    assert np.all(res["status"] == 0)
    runs = np.array(runs)
    result = {"N": N, "p": p, "c": c, "kernels_ms": {}}
    for j, name in enumerate(PHASES + ("call_wall",)):
        col = runs[:, j]
        result["kernels_ms"][name] = {"median": float(np.median(col)), "min": float(col.min()), "max": float(col.max())}
        print(f"{name:12s} median {np.median(col):9.3f} ms  (min {col.min():.3f}, max {col.max():.3f})")
    gram_bytes = p * (c + 1) * N * 4
    gbs = gram_bytes / (result["kernels_ms"]["gram"]["median"] * 1e-3) / 1e9
    result["gram_read_GBps"], result["gram_fraction_of_8TBps"] = gbs, gbs / 8000.0
    print(f"gram kernel: {gram_bytes / 1e9:.2f} GB requested -> {gbs:.1f} GB/s = {100 * gbs / 8000.0:.2f} % of 8 TB/s "
          "(cache share not measured)")
    Yd.free()
    Xd.free()
    eng.close()

    t0 = time.perf_counter()
    A = np.all(np.isfinite(X), axis=0)
    for t in range(p):
        U = A & np.isfinite(Y[t])
        Z = np.vstack([np.ones(U.sum()), X[:, U].astype(np.float64)]).T
        y = Y[t, U].astype(np.float64)
        e = y - Z @ np.linalg.lstsq(Z, y, rcond=None)[0]
        _ = (e - e.mean()) / e.std()
    result["numpy_lstsq_s"] = time.perf_counter() - t0
    print(f"numpy lstsq per trait, {os.cpu_count()} CPUs visible: {result['numpy_lstsq_s']:.2f} s")

    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "set.fam"), "w") as f:
                f.writelines(f"f{i} i{i} 0 0 1 -9\n" for i in range(N))
            t0 = time.perf_counter()
            write_table(os.path.join(d, "traits.tsv"), [f"t{j}" for j in range(p)], Y)
            write_table(os.path.join(d, "covar.tsv"), [f"x{j}" for j in range(c)], X)
            print(f"(writing the two input tables from Python: {time.perf_counter() - t0:.1f} s, not part of the command)")
            from cigwas_amd.cli import MPS_PATH

            t0 = time.perf_counter()
            r = subprocess.run([MPS_PATH, "prep-phen", os.path.join(d, "set"), os.path.join(d, "traits.tsv"), os.path.join(d, "out.phen"),
                                os.path.join(d, "covar.tsv")], capture_output=True, text=True, env=dict(os.environ, CUSK_TIMING="1"))
            total = time.perf_counter() - t0
            assert r.returncode == 0, r.stdout + r.stderr
            phases = {m.group(1): float(m.group(2)) for m in re.finditer(r"\[t\] ([^:]+): ([0-9.e+-]+) ms", r.stdout)}
            text_ms = phases.get("read and align tables", 0.0) + phases.get("write files", 0.0)
            result["cli"] = {"total_s": total, "phases_ms": phases, "text_io_share": text_ms / (total * 1e3)}
            print(r.stdout.strip())
            print(f"mps prep-phen: {total:.2f} s in all; parsing and writing text {text_ms / 1e3:.2f} s = {100 * text_ms / (total * 1e3):.1f} %")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
