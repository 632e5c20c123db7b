#!/usr/bin/env python3
"""Time `mvivw --robust` (selection `all`) on merged skeletons of 40 traits x 20,000 markers and 128 traits x 20,000 markers
(synth.merged_skeleton) with 5 % planted outliers: for every outcome, 5 % of its instruments get a direct effect of 8
standardised units.

Reports per size, warm, as the median of 5 with min and max:
  kernel_ms   device time of one cusk_mvivw_robust from the first to the last kernel
  device_ms   the engine call including the plan and the transfers
  host_ms     the same call through the numpy host form (mvivw.HostEngine) on this machine: the baseline (one run)
and the largest number of updates an outcome took.  Prints one JSON line.

Usage: python tools/mvivw_robust_time.py [--sizes 40x20000,128x20000] [--psi 2] [--reps 5] [--no-device] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cigwas_amd import mvivw  # noqa: E402
from cigwas_amd.synth import merged_skeleton  # noqa: E402

N = 100000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="40x20000,128x20000")
    ap.add_argument("--psi", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    eng = None
    if not args.no_device:
        from cigwas_amd.skeleton import Engine

        eng = Engine(0)
    res = {"reps": args.reps, "psi": args.psi, "sizes": {}}
    for size in args.sizes.split(","):
        p, m = (int(v) for v in size.split("x"))
        adj, corr, _, _ = merged_skeleton(401, p, m, noise=0.002)
        beta = np.ascontiguousarray(np.asarray(corr, np.float64)[p:, :p])
        rng = np.random.default_rng(17)
        for o in range(p):
            rows = rng.choice(m, size=m // 20, replace=False)
            beta[rows, o] = np.clip(beta[rows, o] + 8.0 / np.sqrt(N - 2), -0.9, 0.9)
        weight = mvivw.weights(beta, N)
        selection = mvivw.select(adj, p, "all")
        iv_off, iv, ex_off, ex = mvivw.pack(selection)
        outcome = np.arange(p, dtype=np.int32)
        entry = {"instruments": int(iv_off[-1])}
        out = {}
        if not args.no_host:
            t0 = time.perf_counter()
            out["host"] = mvivw.HostEngine().mvivw_robust(beta, weight, outcome, iv_off, iv, ex_off, ex, psi=args.psi)
            entry["host_ms"] = 1e3 * (time.perf_counter() - t0)
        if eng is not None:
            call_ms, kern_ms = [], []
            for rep in range(args.reps + 1):  # the first run warms up
                t0 = time.perf_counter()
                out["device"] = eng.mvivw_robust(beta, weight, outcome, iv_off, iv, ex_off, ex, psi=args.psi)
                if rep:
                    call_ms.append(1e3 * (time.perf_counter() - t0))
                    kern_ms.append(out["device"][5])
            entry["device_ms"] = {"median": statistics.median(call_ms), "min": min(call_ms), "max": max(call_ms)}
            entry["kernel_ms"] = {"median": statistics.median(kern_ms), "min": min(kern_ms), "max": max(kern_ms)}
        for name, r in out.items():
            entry[name + "_estimated"] = int((r[3] == 0).sum())
            entry[name + "_max_updates"] = float(np.nanmax(r[2][:, 4])) if (r[3] == 0).any() else None
        if len(out) == 2:
            assert out["host"][3].tolist() == out["device"][3].tolist(), size
            th, thd = out["host"][0], out["device"][0]
            ok = np.isfinite(th)
            entry["worst_rel_theta"] = float(np.max(np.abs(thd[ok] - th[ok])) / np.max(np.abs(th[ok]))) if ok.any() else 0.0
        res["sizes"][size] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
