#!/usr/bin/env python3
"""Wall-clock phases of `mps sumstats` and the cost of the indexed correlation build beside the contiguous one.

    python tools/sumstats_time.py [--markers 40000] [--samples 16384] [--traits 20] [--selected 5000] [--repeats 5]
                                  [--se] [--no-mps]

Writes a synthetic PLINK set (binomial dosages, 0.1 % missing) + .phen + prep files to a temporary directory, then
  1. runs `mps sumstats` with CUSK_TIMING=1 once to warm up and `--repeats` times more, and prints the median of every
     phase mark (load, staging, indexed build with its device times, pack, genome-wide mxp, file writing);
  2. in this process, with the .bed resident in HBM: `cusk_corr_build_indexed` on the selected markers against
     `cusk_corr_build` on the same rows made contiguous on the host and uploaded beforehand -- warm-up, `--repeats`
     calls each, median of the call's wall clock and of the SNP x SNP kernel's HIP-event time -- and
     `cusk_pack_lower_tri` to the host;
  3. the count pass (`cusk_pair_counts`: trait masks, marker x trait and trait x trait counts, download) on the selected
     rows, resident and contiguous, beside the marker x trait build of the same rows (`cusk_corr_build` without a
     matrix), both as the call's wall clock; and the count pass's share of the HBM peak, counting the .bed rows and the
     trait masks once each.
`--se` runs `mps sumstats ... se` in step 1 (one more phase mark: the genome-wide pair counts), `--no-mps` skips step 1.
The difference between the two build calls is the row gather (k * ceil(N/4) bytes read and written) plus the upload of
the index list.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(d, m, N, p, rng):
    from cigwas_amd import synth

    maf = rng.uniform(0.05, 0.5, m)
    G = np.empty((m, N), np.int8)
    for i0 in range(0, m, 2048):
        g = rng.binomial(2, maf[i0:i0 + 2048, None], (min(2048, m - i0), N)).astype(np.int8)
        g[rng.random(g.shape) < 0.001] = -1
        G[i0:i0 + 2048] = g
    bed = synth.pack_bed(G)
    means, stds = synth.bed_stats(G)
    stem = os.path.join(d, "geno")
    synth.write_bfiles(stem, bed, N, means, stds, ["1"] * (m // 2) + ["2"] * (m - m // 2))
    Y = rng.standard_normal((p, N)).astype(np.float32)
    synth.write_phen_fast(os.path.join(d, "y.phen"), Y)
    return stem, os.path.join(d, "y.phen"), bed, np.ascontiguousarray(Y).reshape(-1), means, stds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=40000)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--traits", type=int, default=20)
    ap.add_argument("--selected", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--se", action="store_true", help="step 1 with the standard-error files")
    ap.add_argument("--no-mps", action="store_true", help="skip step 1")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second the bandwidth share refers to")
    a = ap.parse_args()
    import cigwas_amd as cg
    from cigwas_amd import cli
    from cigwas_amd._lib import lib

    m, N, p, k = a.markers, a.samples, a.traits, a.selected
    rng = np.random.Generator(np.random.PCG64(11))
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        stem, phen_path, bed, phen, means, stds = write_inputs(d, m, N, p, rng)
        ixs = np.sort(rng.choice(m, size=k, replace=False)).astype(np.int32)
        ixs.tofile(os.path.join(d, "sel.ixs"))
        print(f"inputs: {m} markers x {N} individuals x {p} traits, {k} selected ({time.perf_counter() - t0:.1f} s to write)")
        out = os.path.join(d, "out")
        os.mkdir(out)
        marks = {}
        for rep in range(0 if a.no_mps else a.repeats + 1):
            r = subprocess.run([cli.MPS_PATH, "sumstats", phen_path, stem, os.path.join(d, "sel.ixs"), out] + (["se"] if a.se else []),
                               check=True,
                               capture_output=True, text=True, env=dict(os.environ, CUSK_TIMING="1"))
            if rep == 0:
                continue  # warm-up: page cache, code objects
            for line in (r.stdout + r.stderr).splitlines():
                mt = re.match(r"\[t\] (.*?): ([0-9.eE+-]+) ms", line) or re.match(r"\[hostprof\] (corr_build_indexed: gather).*: ([0-9.]+) ms", line)
                if mt:
                    marks.setdefault(mt.group(1), []).append(float(mt.group(2)))
                mt = re.match(r"\[t\] device: marker x marker ([0-9.eE+-]+) ms, marker x trait \+ trait x trait ([0-9.eE+-]+) ms", line)
                if mt:
                    marks.setdefault("device: marker x marker kernel", []).append(float(mt.group(1)))
                    marks.setdefault("device: marker x trait + trait x trait kernels", []).append(float(mt.group(2)))
        if not a.no_mps:
            print(f"mps sumstats{' se' if a.se else ''}, median of {a.repeats} runs after one warm-up (ms):")
            for name, v in marks.items():
                print(f"  {name}: {statistics.median(v):.2f}  (min {min(v):.2f}, max {max(v):.2f})")
            sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))}
            print(f"  files: {sizes}")

        eng = cg.Engine(0)
        n = k + p
        bed_d, means_d, stds_d = cg.DeviceArray(bed), cg.DeviceArray(means), cg.DeviceArray(stds)
        sel_d, smean_d, sstd_d = cg.DeviceArray(bed[ixs]), cg.DeviceArray(means[ixs]), cg.DeviceArray(stds[ixs])
        Cd = cg.DeviceArray(nbytes=4 * n * n)

        def indexed():
            eng.corr_build_indexed(bed_d, phen, ixs, m, N, p, means_d, stds_d, Cd.ptr)

        def contiguous():
            eng._check(lib().cusk_corr_build(eng.h, sel_d.ptr, phen.ctypes.data, k, N, p, smean_d.ptr, sstd_d.ptr, Cd.ptr, None))

        res = {}
        for name, fn in (("indexed", indexed), ("contiguous", contiguous)):
            fn()
            wall, mxm = [], []
            for _ in range(a.repeats):
                t = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t) * 1e3)
                mxm.append(float(eng.corr_timing()[1]))
            res[name] = (statistics.median(wall), statistics.median(mxm))
            print(f"build {name}: call {res[name][0]:.3f} ms (min {min(wall):.3f}), SNP x SNP kernel {res[name][1]:.3f} ms")
        gather_bytes = 2 * k * ((N + 3) // 4)
        print(f"indexed - contiguous = {res['indexed'][0] - res['contiguous'][0]:.3f} ms for a gather of {gather_bytes / 1e6:.1f} MB "
              f"read + written")
        eng.pack_lower_tri(Cd.ptr, n, k)
        t_pack = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            eng.pack_lower_tri(Cd.ptr, n, k)
            t_pack.append((time.perf_counter() - t) * 1e3)
        print(f"pack_lower_tri to the host ({2 * k * (k + 1) / 1e6:.1f} MB): {statistics.median(t_pack):.3f} ms")

        phen_d = cg.DeviceArray(phen)
        mxp_host = np.zeros(k * p, np.float32)

        def counts():
            eng.pair_counts(sel_d, phen_d, N, p, k=k)

        def mxp_only():
            eng._check(lib().cusk_corr_build(eng.h, sel_d.ptr, phen_d.ptr, k, N, p, smean_d.ptr, sstd_d.ptr, None, mxp_host.ctypes.data))

        pc = {}
        for name, fn in (("pair counts", counts), ("marker x trait build", mxp_only)):
            fn()
            wall = []
            for _ in range(max(a.repeats, 20)):
                t = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t) * 1e3)
            pc[name] = (statistics.median(wall), min(wall))
            print(f"{name} of {k} resident rows: call {pc[name][0]:.3f} ms (min {pc[name][1]:.3f})")
        moved = k * ((N + 3) // 4) + p * ((N + 63) // 64) * 16
        print(f"pair counts: {moved / 1e6:.1f} MB (.bed rows + trait masks, once each) in {pc['pair counts'][0]:.3f} ms = "
              f"{moved / (pc['pair counts'][0] * 1e-3) / 1e9:.1f} GB/s, {100 * moved / (pc['pair counts'][0] * 1e-3) / a.hbm_peak:.1f} % of "
              f"{a.hbm_peak / 1e12:.1f} TB/s; {pc['pair counts'][0] / pc['marker x trait build'][0]:.2f} x the marker x trait build")
        eng.close()


if __name__ == "__main__":
    main()
