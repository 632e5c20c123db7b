#!/usr/bin/env python3
"""Device time of the phases of one `cusk_ld_prune` call beside the existing `cusk_corr_banded` call on the same input.

    python tools/ld_prune_time.py [--markers 50000] [--samples 16384] [--window 2000] [--r-max 0.9] [--repeats 3] [--out FILE]

The input is synthetic: a pool of 4,096 markers with binomial dosages (MAF uniform in 0.05 .. 0.5, 0.1 % missing); marker j
is a pool row rotated by a random number of individuals, every 50th marker repeats its predecessor (dropped for LD) and
every 997th is monomorphic (dropped as constant).  After one warm-up call of each, the two calls alternate `--repeats`
times.  Per `cusk_ld_prune` call: the HIP-event times of upload, band build (memset + FP4 kernel), counts, bitmap and scan
(cusk_ld_prune_timing) and the host clock around the call; per `cusk_corr_banded` call (upload, the same build, row sums,
download of m floats): the host clock.  Prints the medians and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_bed(m, N, rng):
    from cigwas_amd import synth

    pool_n = min(4096, m)
    maf = rng.uniform(0.05, 0.5, pool_n)
    g = rng.binomial(2, maf[:, None], (pool_n, N)).astype(np.int8)
    g[rng.random(g.shape) < 0.001] = -1
    clb = (N + 3) // 4
    bed = np.empty((m, clb), np.uint8)
    src = rng.integers(0, pool_n, m)
    shift = rng.integers(0, N, m)
    for lo in range(0, m, pool_n):
        hi = min(lo + pool_n, m)
        rows = np.stack([np.roll(g[src[j]], shift[j]) for j in range(lo, hi)])
        bed[lo:hi] = synth.pack_bed(rows)
    bed[49::50] = bed[48::50][:len(bed[49::50])]
    bed[996::997] = 0  # all dosage 2
    return bed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=50000)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--window", type=int, default=2000)
    ap.add_argument("--r-max", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import cigwas_amd as cg

    m, N, W = a.markers, a.samples, a.window
    t0 = time.perf_counter()
    bed = make_bed(m, N, np.random.default_rng(7))
    print(f"input: {m} markers x {N} individuals, window {W} ({time.perf_counter() - t0:.1f} s to make)", flush=True)
    eng = cg.Engine(0)
    status = eng.ld_prune(bed, m, N, W, a.r_max)  # warm-up
    eng.corr_banded(bed, m, N, W)
    phases, prune_wall, banded_wall = {}, [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        again = eng.ld_prune(bed, m, N, W, a.r_max)
        prune_wall.append((time.perf_counter() - t) * 1e3)
        assert np.array_equal(again, status)
        for k, v in eng.ld_prune_timing().items():
            phases.setdefault(k, []).append(v)
        t = time.perf_counter()
        eng.corr_banded(bed, m, N, W)
        banded_wall.append((time.perf_counter() - t) * 1e3)
    res = {"markers": m, "samples": N, "window": W, "r_max": a.r_max, "repeats": a.repeats,
           "kept": int((status == 0).sum()), "constant": int((status == 1).sum()), "ld": int((status == 2).sum()),
           "phase_ms_median": {k: statistics.median(v) for k, v in phases.items()},
           "phase_ms_all": phases, "ld_prune_call_ms": prune_wall, "corr_banded_call_ms": banded_wall}
    for k, v in phases.items():
        print(f"  {k}: {statistics.median(v):.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    print(f"  cusk_ld_prune call: {statistics.median(prune_wall):.1f} ms;  cusk_corr_banded call: {statistics.median(banded_wall):.1f} ms")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
