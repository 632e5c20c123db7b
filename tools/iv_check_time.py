#!/usr/bin/env python3
"""Time `check_ivs` on a merged skeleton of 40 traits x 20,000 markers (synth.merged_skeleton), all four flag combinations.

Reports, warm, as the median of 5 with spread = max - min:
  kernel_ms   device time of the set-up and item kernels of one check_ivs (summed over its engine calls)
  device_ms   the engine calls of one check_ivs including the item sort and the transfers
  host_ms     the same calls through the numpy host form (ivcheck.HostEngine) on this machine: the baseline
and checks that both give the same rows.  Prints one JSON line.

Usage: python tools/iv_check_time.py [--traits 40] [--markers 20000] [--reps 5] [--no-device]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cigwas_amd import ivcheck  # noqa: E402
from cigwas_amd.synth import merged_skeleton  # noqa: E402

FLAGS = [(False, False), (True, False), (False, True), (True, True)]


class Timed:
    """an engine whose two calls are timed"""

    def __init__(self, inner):
        self.inner, self.seconds, self.items = inner, 0.0, 0

    def iv_check(self, *a):
        t0 = time.perf_counter()
        out = self.inner.iv_check(*a)
        self.seconds += time.perf_counter() - t0
        self.items += len(a[3])
        return out

    def iv_check_het(self, *a):
        t0 = time.perf_counter()
        out = self.inner.iv_check_het(*a)
        self.seconds += time.perf_counter() - t0
        self.items += len(a[3])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traits", type=int, default=40)
    ap.add_argument("--markers", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-device", action="store_true")
    args = ap.parse_args()
    from scipy.io import mmwrite
    from scipy.sparse import coo_matrix

    p, m = args.traits, args.markers
    adj, corr, _, _ = merged_skeleton(401, p, m, noise=0.002)
    N, a_acc, a_rej = 100000, 1e-4, 1e-3
    with tempfile.TemporaryDirectory() as d:
        stem = os.path.join(d, "all_merged")
        mmwrite(stem + "_sam.mtx", coo_matrix(adj.astype(np.int32)))
        mmwrite(stem + "_scm.mtx", coo_matrix(corr))
        with open(stem + ".mdim", "w") as f:
            f.write(f"{p + m}\t{p}\t3\n")
        data = ivcheck.load(stem)  # dense, as the reference reads it: once for all runs
        engines = {"host": ivcheck.HostEngine()}
        if not args.no_device:
            from cigwas_amd.skeleton import Engine

            engines["device"] = Engine(0)
        res = {"traits": p, "markers": m, "reps": args.reps, "flags": {}}
        for relaxed, rev in FLAGS:
            key = f"relaxed={int(relaxed)},reverse={int(rev)}"
            entry, rows = {}, {}
            for which, eng in engines.items():
                call_ms, kern_ms = [], []
                for rep in range(args.reps + 1):  # the first run warms up
                    timed, stats = Timed(eng), {}
                    rows[which] = ivcheck.check_ivs(stem, N, a_acc, a_rej, relaxed_local_faithfulness=relaxed,
                                                    check_reverse_causality=rev, engine=timed, stats=stats, data=data)
                    if rep:
                        call_ms.append(1e3 * timed.seconds)
                        kern_ms.append(stats["kernel_ms"])
                entry[which + "_ms"] = {"median": statistics.median(call_ms), "spread": max(call_ms) - min(call_ms)}
                if which == "device":
                    entry["kernel_ms"] = {"median": statistics.median(kern_ms), "spread": max(kern_ms) - min(kern_ms)}
                entry["items"], entry["rows"] = timed.items, len(rows[which])
            if "device" in rows:
                assert rows["device"] == rows["host"], key
            res["flags"][key] = entry
        print(json.dumps(res))


if __name__ == "__main__":
    main()
