#!/usr/bin/env python3
"""Time `mvivw --ld` (selection `all`) on merged skeletons (synth.merged_skeleton) with a block-diagonal AR(1) LD:
rho^|a-b| in blocks of 50 markers, rho = 0.6.

Reports per size, warm, as the median of --reps with spread = max - min:
  kernel_ms   device time from the first to the last kernel of one cusk_mvivw_ld
  device_ms   the engine call including the plan and the transfers (the M x M LD is copied to the device in every call)
  host_ms     the same call through the numpy host form (mvivw.HostEngine.mvivw_ld) on this machine (one run; --no-host
              skips it: at 20,000 markers it takes minutes)
  update_tflops  sum over outcomes of m^3 / 3 multiply-adds, two flops each, over kernel_ms: a LOWER bound of the trailing
              update's rate, since kernel_ms also holds the gather, the panel kernels and the regression
Prints one JSON line.

Usage: python tools/mvivw_ld_time.py [--sizes 40x2000,40x20000] [--reps 5] [--no-device] [--no-host]
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


def ar1_ld(M, block=50, rho=0.6):
    ld = np.zeros((M, M))
    for b0 in range(0, M, block):
        idx = np.arange(min(block, M - b0))
        ld[b0:b0 + len(idx), b0:b0 + len(idx)] = rho ** np.abs(idx[:, None] - idx[None, :])
    return ld


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="40x2000,40x20000")
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
        ld = ar1_ld(m)
        selection = mvivw.select(adj, p, "all")
        iv_off, iv, ex_off, ex = mvivw.pack(selection)
        outcome = np.arange(p, dtype=np.int32)
        madds = sum(len(I) ** 3 // 3 for I, _ in selection)
        entry = {"instruments": int(iv_off[-1]), "cholesky_multiply_adds": int(madds)}
        out = {}
        if not args.no_host:
            t0 = time.perf_counter()
            out["host"] = mvivw.HostEngine().mvivw_ld(beta, weight, ld, outcome, iv_off, iv, ex_off, ex)
            entry["host_ms"] = 1e3 * (time.perf_counter() - t0)
        if eng is not None:
            call_ms, kern_ms = [], []
            for rep in range(args.reps + 1):  # the first run warms up
                t0 = time.perf_counter()
                out["device"] = eng.mvivw_ld(beta, weight, ld, outcome, iv_off, iv, ex_off, ex)
                if rep:
                    call_ms.append(1e3 * (time.perf_counter() - t0))
                    kern_ms.append(out["device"][4])
            entry["device_ms"] = {"median": statistics.median(call_ms), "spread": max(call_ms) - min(call_ms)}
            entry["kernel_ms"] = {"median": statistics.median(kern_ms), "spread": max(kern_ms) - min(kern_ms)}
            entry["update_tflops"] = 2.0 * madds / (1e-3 * entry["kernel_ms"]["median"]) / 1e12
            entry["estimated"] = int((out["device"][3] == 0).sum())
        if len(out) == 2:
            (th, se, st, status, _), (thd, sed, std, statusd, _) = out["host"], out["device"]
            assert status.tolist() == statusd.tolist(), size
            ok = np.isfinite(th)
            entry["worst_rel"] = float(max(np.max(np.abs(thd[ok] - th[ok])) / np.max(np.abs(th[ok])),
                                           np.max(np.abs(sed[ok] - se[ok])) / np.max(np.abs(se[ok])))) if ok.any() else 0.0
            assert entry["worst_rel"] <= 1e-7, (size, entry["worst_rel"])
        res["sizes"][size] = entry
        print(json.dumps({size: entry}), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
