#!/usr/bin/env python3
"""Device time of cusk_marker_pair_sizes beside the correlation build of the same rows.

k contiguous markers x N individuals (default 10,000 x 16,384, 0.1 % missing calls), device-resident .bed.  The engine runs
on a torch stream so that torch's events (HIP events) bracket the call on the stream it launches on; one warm-up call,
then `--repeats` timed ones: median and spread (max - min) in ms.  The yardstick comes from the same process: the SNP x SNP
part of cusk_corr_build on the same rows (cusk_corr_timing, FP4 form by default), median and spread of as many builds.
Only the k x k corner of the size matrix is allocated (ld = k), and the build writes a (k + 1)^2 matrix with one trait.
Last line: one JSON object."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=10000)
    ap.add_argument("--individuals", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch

    import cigwas_amd as cg
    from cigwas_amd import synth

    k, N = args.markers, args.individuals
    rng = np.random.default_rng(7)
    G = rng.binomial(2, 0.3, (k, N)).astype(np.int8)
    G[rng.random((k, N)) < 0.001] = -1
    bed = synth.pack_bed(G)
    means, stds = synth.bed_stats(G)
    phen = rng.standard_normal((1, N)).astype(np.float32)
    torch.cuda.set_device(args.device)
    stream = torch.cuda.Stream()
    eng = cg.Engine(args.device, stream.cuda_stream)
    bed_d = cg.DeviceArray(bed)
    out = cg.DeviceArray(nbytes=4 * k * k)
    Cd = cg.DeviceArray(nbytes=4 * (k + 1) * (k + 1))

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        eng.marker_pair_sizes(bed_d, N, out.ptr, k, k=k, m_total=k)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    timed()
    pair = [timed() for _ in range(args.repeats)]
    got = out.download(np.float32, (k, k))
    V = (G[:64] >= 0).astype(np.int64)
    assert np.array_equal(got[:64, :64], (V @ V.T).astype(np.float32)) and np.array_equal(got, got.T)
    build = []
    for i in range(args.repeats + 1):
        eng.corr_build(bed, phen, k, N, 1, means, stds, Cd.ptr)
        if i:
            build.append(float(eng.corr_timing()[1]))
    res = {"markers": k, "individuals": N,
           "marker_pair_sizes_ms": {"median": round(statistics.median(pair), 4), "spread": round(max(pair) - min(pair), 4),
                                    "repeats": [round(v, 4) for v in pair]},
           "corr_build_mxm_ms": {"median": round(statistics.median(build), 4), "spread": round(max(build) - min(build), 4),
                                 "repeats": [round(v, 4) for v in build]}}
    print(f"cusk_marker_pair_sizes {res['marker_pair_sizes_ms']}\ncorrelation build, marker x marker {res['corr_build_mxm_ms']}")
    print(json.dumps(res))
    for a in (bed_d, out, Cd):
        a.free()
    eng.close()


if __name__ == "__main__":
    main()
