#!/usr/bin/env python3
"""Time `mvivw` (selection `all`) on merged skeletons of 40 traits x 20,000 markers and 128 traits x 20,000 markers
(synth.merged_skeleton).

Reports per size, warm, as the median of 5 with spread = max - min:
  kernel_ms   device time of the Gram, solve and residual kernels of one cusk_mvivw
  device_ms   the engine call including the plan and the transfers
  host_ms     the same call through the numpy host form (mvivw.HostEngine) on this machine: the baseline (one run)
and checks that both give the same estimates to 1e-9.  Prints one JSON line.

Usage: python tools/mvivw_time.py [--sizes 40x20000,128x20000] [--reps 5] [--no-device] [--no-host]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="40x20000,128x20000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    eng = None
    if not args.no_device:
        from cigwas_amd.skeleton import Engine

        eng = Engine(0)
    res = {"reps": args.reps, "sizes": {}}
    for size in args.sizes.split(","):
        p, m = (int(v) for v in size.split("x"))
        adj, corr, _, _ = merged_skeleton(401, p, m, noise=0.002)
        beta = np.ascontiguousarray(np.asarray(corr, np.float64)[p:, :p])
        weight = mvivw.weights(beta, 100000)
        selection = mvivw.select(adj, p, "all")
        iv_off, iv, ex_off, ex = mvivw.pack(selection)
        outcome = np.arange(p, dtype=np.int32)
        entry = {"instruments": int(iv_off[-1]), "multiply_adds": int(sum(len(I) * (len(E) + 1) * (len(E) + 2) // 2 for I, E in selection))}
        out = {}
        if not args.no_host:
            t0 = time.perf_counter()
            out["host"] = mvivw.HostEngine().mvivw(beta, weight, outcome, iv_off, iv, ex_off, ex)
            entry["host_ms"] = 1e3 * (time.perf_counter() - t0)
        if eng is not None:
            call_ms, kern_ms = [], []
            for rep in range(args.reps + 1):  # the first run warms up
                t0 = time.perf_counter()
                out["device"] = eng.mvivw(beta, weight, outcome, iv_off, iv, ex_off, ex)
                if rep:
                    call_ms.append(1e3 * (time.perf_counter() - t0))
                    kern_ms.append(out["device"][4])
            entry["device_ms"] = {"median": statistics.median(call_ms), "spread": max(call_ms) - min(call_ms)}
            entry["kernel_ms"] = {"median": statistics.median(kern_ms), "spread": max(kern_ms) - min(kern_ms)}
        if len(out) == 2:
            (th, se, st, status, _), (thd, sed, std, statusd, _) = out["host"], out["device"]
            assert status.tolist() == statusd.tolist(), size
            ok = np.isfinite(th)
            entry["estimated"] = int((status == 0).sum())
            entry["worst_rel"] = float(max(np.max(np.abs(thd[ok] - th[ok])) / np.max(np.abs(th[ok])),
                                           np.max(np.abs(sed[ok] - se[ok])) / np.max(np.abs(se[ok])))) if ok.any() else 0.0
            assert entry["worst_rel"] <= 1e-9, (size, entry["worst_rel"])
        res["sizes"][size] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
