#!/usr/bin/env python3
"""What `prep-phen --rint` costs at cohort size: N = 500,000 individuals, p = 50 traits, 10 % missing.

  * the four phases of cusk_phen_rint by HIP events (cusk_phen_rint_timing: keys, sort, ranks, moments + standardise):
    median of 5 runs with min and max, after one warm-up, input resident on the device; the number of kernel launches
    of the sort, computed from N and the tile, beside its time;
  * the whole call by the host clock: with the input resident (the 100 MB of `out` still go to pageable host memory) and
    with the input in host memory (upload included);
  * scipy.stats.rankdata + scipy.special.ndtri + standardise per trait on this machine's CPUs: the yardstick.

    python tools/phen_rint_time.py [--n 500000] [--p 50] [--missing 0.1] [--out out/phen_rint_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("keys", "sort", "ranks", "moments_standardise")


def stat(col):
    return {"median": float(np.median(col)), "min": float(np.min(col)), "max": float(np.max(col))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--p", type=int, default=50)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--out", type=str, default=os.path.join("out", "phen_rint_time.json"))
    a = ap.parse_args()
    import cigwas_amd as cg
    from cigwas_amd._lib import lib

    N, p = a.n, a.p
    rng = np.random.default_rng(1)
    V = np.exp(rng.standard_normal((p, N))).astype(np.float32)
    V[rng.random((p, N)) < a.missing] = np.nan
    T = int(lib().cusk_phen_rint_tile())
    npad = T
    while npad < N:
        npad *= 2
    stages = (npad // T).bit_length() - 1
    launches = 1 + stages + stages * (stages + 1) // 2
    eng = cg.Engine(0)
    Vd = cg.DeviceArray(V)
    out = np.empty(p * N, np.float32)
    runs, wall_host = [], []
    for k in range(6):
        t0 = time.perf_counter()
        res = eng.phen_rint(Vd, N, p, out=out)
        wall = (time.perf_counter() - t0) * 1e3
        if k:
            runs.append(list(map(float, eng.phen_rint_timing())) + [wall])
    for k in range(6):
        t0 = time.perf_counter()
        eng.phen_rint(V, N, p, out=out)
        if k:
            wall_host.append((time.perf_counter() - t0) * 1e3)
    assert np.all(res["status"] == 0)
    runs = np.array(runs)
    result = {"N": N, "p": p, "missing": a.missing, "tile": T, "npad": npad, "sort_launches": launches, "ms": {}}
    for j, name in enumerate(PHASES + ("call_resident",)):
        result["ms"][name] = stat(runs[:, j])
    result["ms"]["call_from_host"] = stat(wall_host)
    for name, s in result["ms"].items():
        print(f"{name:20s} median {s['median']:9.3f} ms  (min {s['min']:.3f}, max {s['max']:.3f})")
    print(f"sort: {launches} launches ({stages} merge stages across tiles of {T} keys, rows of {npad} keys)")
    Vd.free()
    eng.close()

    from scipy.special import ndtri
    from scipy.stats import rankdata

    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for t in range(p):
            U = np.isfinite(V[t])
            q = ndtri((rankdata(V[t, U]) - 0.375) / (U.sum() + 0.25))
            z = np.full(N, np.nan, np.float32)
            z[U] = (q - q.mean()) / q.std()
        host.append(time.perf_counter() - t0)
    result["host_rankdata_ndtri_s"] = stat(host)
    print(f"rankdata + ndtri + standardise per trait on the host, {os.cpu_count()} CPUs visible: median {np.median(host):.2f} s "
          f"(min {min(host):.2f}, max {max(host):.2f})")
    print(f"last trait: max |device - host| = {np.nanmax(np.abs(out.reshape(p, N)[p - 1] - z)):.3g}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
