#!/usr/bin/env python3
"""Time `mvivw --jackknife` (selection `all`) on merged skeletons of 40 traits x 20,000 markers and 128 traits x 20,000
markers (synth.merged_skeleton), each with leave-one-out groups and with B = 200 blocks.

Reports per size and grouping, warm, as the median of 5 with min and max:
  kernel_ms        device time of one cusk_mvivw_jackknife from the first to the last kernel (HIP events)
  device_ms        the engine call including the plans and the transfers (host clock); pres and refit are not asked for
  plain_kernel_ms, plain_device_ms
                   the same two for cusk_mvivw on the same inputs: what the flag adds is the difference
  host_ms          the same call through the numpy host form (mvivw.HostEngine) on this machine (one run; left out for
                   groupings of more than --host-groups refits, which take hours)
and the number of refits.  Prints one JSON line.

Usage: python tools/mvivw_jackknife_time.py [--sizes 40x20000,128x20000] [--groups loo,200] [--reps 5] [--no-device]
                                            [--no-host] [--host-groups 100000]
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


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="40x20000,128x20000")
    ap.add_argument("--groups", type=str, default="loo,200")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-groups", type=int, default=100000)
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
        weight = mvivw.weights(beta, N)
        selection = mvivw.select(adj, p, "all")
        iv_off, iv, ex_off, ex = mvivw.pack(selection)
        outcome = np.arange(p, dtype=np.int32)
        plain = (beta, weight, outcome, iv_off, iv, ex_off, ex)
        entry = {"instruments": int(iv_off[-1])}
        if eng is not None:
            call_ms, kern_ms = [], []
            for rep in range(args.reps + 1):  # the first run warms up
                t0 = time.perf_counter()
                out = eng.mvivw(*plain)
                if rep:
                    call_ms.append(1e3 * (time.perf_counter() - t0))
                    kern_ms.append(out[4])
            entry["plain_device_ms"], entry["plain_kernel_ms"] = summary(call_ms), summary(kern_ms)
        for spec in args.groups.split(","):
            bounds = [mvivw.groups(I, "loo" if spec == "loo" else int(spec)) for I, _ in selection]
            grp_off = np.zeros(p + 1, np.int64)
            grp_off[1:] = np.cumsum([len(b) for b in bounds])
            grp = np.concatenate(bounds).astype(np.int32)
            sub = {"refits": int(sum(len(b) - 1 for b in bounds))}
            out = {}
            if not args.no_host and sub["refits"] <= args.host_groups:
                t0 = time.perf_counter()
                out["host"] = mvivw.HostEngine().mvivw_jackknife(*plain, grp_off, grp, want_pres=False, want_refit=False)
                sub["host_ms"] = 1e3 * (time.perf_counter() - t0)
            if eng is not None:
                call_ms, kern_ms = [], []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    out["device"] = eng.mvivw_jackknife(*plain, grp_off, grp, want_pres=False, want_refit=False)
                    if rep:
                        call_ms.append(1e3 * (time.perf_counter() - t0))
                        kern_ms.append(out["device"][10])
                sub["device_ms"], sub["kernel_ms"] = summary(call_ms), summary(kern_ms)
            for name, r in out.items():
                sub[name + "_estimated"] = int((r[7] == 0).sum())
            if len(out) == 2:
                assert out["host"][7].tolist() == out["device"][7].tolist(), (size, spec)
                a, b = out["host"][4], out["device"][4]
                ok = np.isfinite(a)
                sub["worst_rel_jk"] = float(np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(a[ok]))) if ok.any() else 0.0
            entry[spec] = sub
        res["sizes"][size] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
