"""Times of the ordinal-trait kernels beside the pair-count pass on the same rows.

    python tools/ordinal_time.py [--markers 10000] [--individuals 16384] [--traits 20] [--ordinal 4] [--levels 4] [--reps 5]

Device-resident .bed rows and phenotypes; per repetition one `cusk_pair_counts` call (wall clock around the call, which
returns when the counts are on the host), one `cusk_ordinal_tables` call (wall clock, and the table kernel alone from the
library's events) and one `cusk_polychoric_fit` over the k x q tables it produced (wall clock and kernel).  Prints one
JSON line with the medians.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=10000)
    ap.add_argument("--individuals", type=int, default=16384)
    ap.add_argument("--traits", type=int, default=20)
    ap.add_argument("--ordinal", type=int, default=4)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import cigwas_amd as cg

    rng = np.random.Generator(np.random.PCG64(1))
    k, N, p, q = a.markers, a.individuals, a.traits, a.ordinal
    # genotypes with a planted effect on the ordinal traits, 1 % missing calls
    maf = rng.uniform(0.05, 0.5, (k, 1))
    dosage = (rng.random((k, N)) < maf).astype(np.int8) + (rng.random((k, N)) < maf).astype(np.int8)
    code = np.array([3, 2, 0], np.uint8)[dosage]
    code[rng.random((k, N)) < 0.01] = 1
    pad = (-N) % 4
    code = np.pad(code, ((0, 0), (0, pad)))
    bed = (code[:, 0::4] | (code[:, 1::4] << 2) | (code[:, 2::4] << 4) | (code[:, 3::4] << 6)).astype(np.uint8)
    phen = rng.standard_normal((p, N)).astype(np.float32)
    ord_ix = np.arange(q, dtype=np.int32)
    for t in ord_ix:
        liab = phen[t] + 0.05 * dosage[t].astype(np.float32)
        phen[t] = np.searchsorted(np.quantile(liab, np.linspace(0, 1, a.levels + 1)[1:-1]), liab).astype(np.float32)
    phen[rng.random((p, N)) < 0.05] = np.nan
    levels, nlev = cg.ordinal_levels(phen, ord_ix)
    eng = cg.Engine(0)
    bed_d, phen_d = cg.DeviceArray(bed), cg.DeviceArray(phen)
    t_pc, t_tab, t_tab_k, t_fit, t_fit_k = [], [], [], [], []
    for rep in range(a.reps + 1):  # the first repetition warms up
        t0 = time.perf_counter()
        eng.pair_counts(bed_d, phen_d, N, p, k=k)
        t1 = time.perf_counter()
        mxo, _ = eng.ordinal_tables(bed_d, phen_d, N, p, ord_ix, levels, nlev, k=k)
        t2 = time.perf_counter()
        r, se, st = eng.polychoric_fit(mxo.reshape(k * q, 3, 8))
        t3 = time.perf_counter()
        ms = eng.ordinal_timing()
        if rep:
            t_pc.append((t1 - t0) * 1e3), t_tab.append((t2 - t1) * 1e3), t_fit.append((t3 - t2) * 1e3)
            t_tab_k.append(ms[0]), t_fit_k.append(ms[1])
    med = lambda v: float(np.median(v))
    print(json.dumps(dict(markers=k, individuals=N, traits=p, ordinal=q, levels=a.levels, reps=a.reps,
                          pair_counts_call_ms=med(t_pc), ordinal_tables_call_ms=med(t_tab), table_kernel_ms=med(t_tab_k),
                          polychoric_fit_call_ms=med(t_fit), fit_kernel_ms=med(t_fit_k), tables=int(k * q),
                          fitted=int((st == 0).sum()), boundary=int((st == 1).sum()), degenerate=int((st == 2).sum()))))
    bed_d.free()
    phen_d.free()
    eng.close()


if __name__ == "__main__":
    main()
