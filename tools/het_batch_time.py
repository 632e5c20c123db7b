#!/usr/bin/env python3
"""Blocks per second of the whole-chromosome job at per-pair sample sizes, batched against block by block.

    python tools/het_batch_time.py [--blocks 25] [--individuals 16384] [--traits 20] [--repeats 5] [--passes 4]
                                   [--het-batch-vars 16384]

The data set is the one `bench.py --full` generates for its whole-chromosome leg (bench.write_chromosome: unequal LD
blocks of 500 SNPs on average, 20 traits), with gaps put into two traits: trait 1 is observed on 25 % of the individuals,
trait 3 on 60 %.  It is run through the block driver (run_blocks.run_job, one GPU, writer "local": every block's five
files are written) nine ways:
  1. het, one block per engine run          (`run_blocks.py --het`)
  2. het, batched                           (`run_blocks.py --het-batch-vars V`)
  3. not het, batched                       (`run_blocks.py --batch-vars V`: what the het batch lacks -- the filter, the
                                             vectorised and union-major sweeps, the level-1 row kernel -- is in here)
  4. het with the filter, one block per run (`run_blocks.py --het --het-filter`)
  5. het with the filter, batched           (`run_blocks.py --het-batch-vars V --het-filter`)
  6. ... with filter and rows, per block    (`run_blocks.py --het --het-filter --het-rows`: level 1 on the row kernel)
  7. ... with filter and rows, batched      (`run_blocks.py --het-batch-vars V --het-filter --het-rows`)
  8. ... filter, rows and markers, per block (`run_blocks.py --het --het-filter --het-rows --het-markers`: pairs of markers at
                                              the number of individuals both were genotyped on; the results differ from 6-7)
  9. ... filter, rows and markers, batched   (`run_blocks.py --het-batch-vars V --het-filter --het-rows --het-markers`)
(ways 4-5, 6-7 and 8-9 have a block set, and with it engines, of their own: the options stay set on an engine)
One repeat = `--passes` passes of the job over the chromosome, timed on the host around work that ends with the files on
disk; the nine ways alternate inside every repeat.  After one untimed warm-up repeat the tool prints, per way, the median
of `--repeats` repeats in blocks/s, the spread (max - min) of the repeats, and the mean wall-clock phases of a pass as the
pipeline reports them (ms; counts and sizes are part of corr; l1_tests / l1_exact: level-1 tests per pass and those the
row kernel's filter sent to the exact form, ways 6-7 only).  CUSK_BATCH_PROF=1 in the environment adds the batch
pipeline's own phase marks on stderr.  Last line: one JSON object with all of it."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=25)
    ap.add_argument("--individuals", type=int, default=16384)
    ap.add_argument("--traits", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--max-level", type=int, default=5)
    ap.add_argument("--max-level-two", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--het-batch-vars", type=int, default=16384)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import bench
    from cigwas_amd import run_blocks as rb
    from cigwas_amd import synth

    N, p = args.individuals, args.traits
    indir = tempfile.mkdtemp(prefix="het_batch_in_", dir=bench.input_dir_root())
    workdir = tempfile.mkdtemp(prefix="het_batch_out_")
    try:
        _phen, stem, blocks, sizes = bench.write_chromosome(indir, 0, 1, args.blocks, N, p)
        Y = synth.chromosome_traits(np.load(os.path.join(indir, "seg0.contrib.npy")))
        rng = np.random.default_rng(2024)
        Y[1, rng.permutation(N)[int(0.25 * N):]] = np.nan
        Y[3 % p, rng.permutation(N)[int(0.60 * N):]] = np.nan
        gaps = os.path.join(indir, "gaps.phen")
        synth.write_phen_fast(gaps, Y)
        os.sync()
        nb = len(sizes)
        bs_het = rb.BlockSet(gaps, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
        bs_het.set_het(True)
        bs_plain = rb.BlockSet(gaps, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
        bs_hetf = rb.BlockSet(gaps, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
        bs_hetf.set_het(True)
        bs_hetf.set_het_filter(True)
        bs_hetfr = rb.BlockSet(gaps, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
        bs_hetfr.set_het(True)
        bs_hetfr.set_het_filter(True)
        bs_hetfr.set_het_rows(True)
        bs_hetfrm = rb.BlockSet(gaps, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
        bs_hetfrm.set_het(True)
        bs_hetfrm.set_het_filter(True)
        bs_hetfrm.set_het_rows(True)
        bs_hetfrm.set_het_markers(True)
        V = args.het_batch_vars
        ways = {
            "het_per_block": dict(bs=bs_het, batch_vars=0, het=False),
            "het_batch": dict(bs=bs_het, batch_vars=V, het=True),
            "plain_batch": dict(bs=bs_plain, batch_vars=V, het=False),
            "het_filter_per_block": dict(bs=bs_hetf, batch_vars=0, het=False),
            "het_filter_batch": dict(bs=bs_hetf, batch_vars=V, het=True),
            "het_filter_rows_per_block": dict(bs=bs_hetfr, batch_vars=0, het=False),
            "het_filter_rows_batch": dict(bs=bs_hetfr, batch_vars=V, het=True),
            "het_filter_rows_markers_per_block": dict(bs=bs_hetfrm, batch_vars=0, het=False),
            "het_filter_rows_markers_batch": dict(bs=bs_hetfrm, batch_vars=V, het=True),
        }
        counter = [0]

        def one_pass(w):
            counter[0] += 1
            out = os.path.join(workdir, f"out{counter[0]}")
            os.makedirs(out)
            done, stats, _ = rb.run_job(w["bs"], out, args.device, options={"timing": 0}, writer="local", batch_vars=w["batch_vars"],
                                        blockfile=blocks, het=w["het"])
            shutil.rmtree(out)
            it = stats if w["batch_vars"] > 0 else stats.values()
            ph = {}
            for s in it:
                for key in ("ms_corr", "ms_stage1", "ms_prune", "ms_stage2", "ms_reduce"):
                    ph[key[3:]] = ph.get(key[3:], 0.0) + float(getattr(s, key))
                # level-1 tests and those a row kernel's filter sent to the exact form (het_rows; 0 otherwise), both stages
                ph["l1_tests"] = ph.get("l1_tests", 0.0) + float(s.stage[0].tests[1] + s.stage[1].tests[1])
                ph["l1_exact"] = ph.get("l1_exact", 0.0) + float(s.stage[0].rechecks[1] + s.stage[1].rechecks[1])
            return len(done), ph

        rates = {k: [] for k in ways}
        phases = {k: {} for k in ways}
        written = {}
        for rep in range(args.repeats + 1):  # repeat 0 warms every way up
            for name, w in ways.items():
                t0 = time.perf_counter()
                for _ in range(args.passes):
                    written[name], ph = one_pass(w)
                    if rep > 0:
                        for k, v in ph.items():
                            phases[name][k] = phases[name].get(k, 0.0) + v / (args.repeats * args.passes)
                dt = time.perf_counter() - t0
                if rep > 0:
                    rates[name].append(args.passes * nb / dt)
        out = {"blocks": nb, "markers": int(sum(sizes)), "individuals": N, "traits": p, "het_batch_vars": V, "repeats": args.repeats,
               "passes_per_repeat": args.passes, "ways": {}}
        for name in ways:
            r = rates[name]
            out["ways"][name] = {"blocks_per_s_median": round(statistics.median(r), 1), "spread": round(max(r) - min(r), 1),
                                 "repeats": [round(v, 1) for v in r], "blocks_written": written[name],
                                 "phase_ms_per_pass": {k: round(v, 3) for k, v in phases[name].items()}}
            print(f"{name:34s} {statistics.median(r):9.1f} blocks/s (median of {len(r)}, spread {max(r) - min(r):.1f}), "
                  f"{written[name]} of {nb} blocks written, phases/pass {out['ways'][name]['phase_ms_per_pass']}", flush=True)
        a, b = out["ways"]["het_batch"], out["ways"]["het_per_block"]
        out["het_batch_over_per_block"] = round(a["blocks_per_s_median"] / b["blocks_per_s_median"], 2)
        out["faster_by_more_than_the_spread"] = bool(a["blocks_per_s_median"] - b["blocks_per_s_median"] > max(a["spread"], b["spread"]))
        # the filter against the same way without it: ratio of the medians, and whether the gain exceeds both spreads
        # ... and the row kernel at level 1 against the filtered way without it
        for plain, filt in (("het_per_block", "het_filter_per_block"), ("het_batch", "het_filter_batch"),
                            ("het_filter_per_block", "het_filter_rows_per_block"), ("het_filter_batch", "het_filter_rows_batch"),
                            ("het_filter_rows_per_block", "het_filter_rows_markers_per_block"),
                            ("het_filter_rows_batch", "het_filter_rows_markers_batch")):
            f, g = out["ways"][filt], out["ways"][plain]
            out[filt + "_over_" + plain] = round(f["blocks_per_s_median"] / g["blocks_per_s_median"], 2)
            out[filt + "_faster_by_more_than_the_spread"] = bool(
                f["blocks_per_s_median"] - g["blocks_per_s_median"] > max(f["spread"], g["spread"]))
        bs_het.close()
        bs_plain.close()
        bs_hetf.close()
        bs_hetfr.close()
        bs_hetfrm.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(indir, ignore_errors=True)
        shutil.rmtree(workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
