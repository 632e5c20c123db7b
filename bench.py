#!/usr/bin/env python3
"""bench.py -- CI tests/sec of the MI355X-native cusk PC-skeleton engine (BASELINE.json metric).

N = 1 (default): one step = one pass of the hot path over one synthetic LD block: the complete level-ordered skeleton
search (levels 0..5: level-0 bitmap build, per-level neighbour compaction, CI sweep, separating-set finalisation) on
the block's correlation matrix, which is already resident in HBM when the timed region starts.  Workload = the
north_star headline: 10,000 SNPs x 20 traits, N = 16,384 individuals, alpha = 1e-4, max level 5; the matrix is
produced from synthetic packed .bed genotypes by this repo's own correlation build (Kendall-npn SNP x SNP, Pearson
SNP x trait / trait x trait), exactly what `cusk` feeds its sweep.  With --full the same run also checks the engine's
adjacency and separating sets against the CPU oracle on the full block (`parity`), times the CPU baselines, adds the
per-level table and rooflines, the end-to-end block and a bounded whole-chromosome pass through the multi-GPU block
driver on this one GPU (`scale`).

N > 1 (torchrun, one rank per GPU): BASELINE.json config 4, the whole-chromosome run -- 25 unequal LD blocks per GPU
(200 blocks x ~500 SNPs x 20 traits on 8 GPUs; weak scaling), written as a PLINK file set, every block through the
product's block driver (ci-gwas_amd/run_blocks.py: `cusk_blockset_*`, longest-processing-time assignment; the blocks of
a rank run in batches -- `cusk_blockset_run_batch`: correlation build, stage one, prune, stage two and reduction of all
blocks of a batch in one set of device runs; .bed staged in HBM once per GPU), no collective in the data path.  Files
(--writer rank0, the default): the per-block results are gathered to rank 0 over RCCL (the one exchange north_star names),
which writes every file; the gather and rank 0's writing are timed separately.  --writer merge: every rank writes the
files of its own blocks and the merged skeleton -- what `merge-block-outputs` reads of every block -- is gathered to rank
0, which writes merged_blocks* from memory (the library's merge); --writer local has no exchange (what the reference's
one-process-per-block runs do).  A --full line reports all three.  One step = one pass of the job over the whole chromosome.

EVERY --full line (N = 1 included) and every N > 1 line carries the same `scale` object -- the whole-chromosome job on this
many GPUs, 25 blocks per GPU -- and `scale.blocks_per_sec` is the key a scaling curve is to be built from (at N = 1 `value`
is the headline block, at N > 1 the chromosome job: not comparable with each other).

A plain run (no --full) does only what the headline figure needs: set-up, --warmup steps, the --steps timed steps, the
outputs of the last step when --dump-outputs DIR is given, and the line (metric, value, unit, ms_per_step, ...).
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

# before anything initialises HIP: the engine's two streams must not share a hardware queue with RCCL's streams
# (see ci-gwas_amd/_lib.py)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
VALU_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: peak FP32 (vector)
LDS_PEAK_GBS = 256 * 256 * 2.4  # 256 B/clk/CU (ds_read_b128) x 256 CUs x 2.4 GHz = 157 TB/s


def algorithmic_bytes(level, tests, subsets, n):
    """bytes the path moves per level if every operand came from HBM."""
    if level == 0:
        return 4.0 * n * (n - 1) / 2
    return subsets * 4.0 * (level + level * (level - 1) / 2) + tests * 4.0 * (level + 2)


def filter_flops(level, tests, subsets):
    """fp32 operations the level >= 2 sweep kernels issue (csrc/ci_fast.h, sweep_vec.hip; FMA = 2): per test one
    forward substitution against the set's Cholesky factor, l(l-1)/2 + 2l FMAs + l multiplies + 4 for the comparison
    = l(l-1) + 5l + 4; per conditioning set the factorisation and F^-1 C[S,X]: sum_i (i^2 + 2i) + l(l-1) + 3l."""
    L = level
    per_test = L * (L - 1) + 5 * L + 4
    per_set = sum(i * i + 2 * i for i in range(L)) + L * (L - 1) + 3 * L
    return tests * float(per_test) + subsets * float(per_set)


def roofline_of(level, tests, subsets, n, kernel_ms, engine, traffic=None):
    """roofline object of one launch (or one launch per degree class) of the level's dominant kernel"""
    mode = 0 if engine == "cusk" else 1
    if level <= 1:
        ab = algorithmic_bytes(level, tests, subsets, n)
        ach = ab / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
        return {
            "kernel": f"level1_rows2_kernel<{mode}, false, 256, true> (one launch per step; <.., 512, true> where that puts as many rows on a CU; the gather form <.., 256, false> when two rows of C "
                      f"do not fit a CU's LDS)" if level == 1 else "level0_wide_kernel",
            "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "traffic": traffic, "algorithmic_bytes_per_step": ab, "kernel_ms_per_step": float(kernel_ms),
            "note": "algorithmic bytes = SURVEY 8(d): 4(l+l(l-1)/2) B per subset + 4(l+2) B per test (level 0: 4 B per "
                    "pair), x the tests and subsets of one launch; duration = HIP events on the engine stream around the "
                    "kernel alone; traffic = FETCH_SIZE+WRITE_SIZE of the committed PMC passes per launch "
                    "(profiles/pmc_traffic.json)",
        }
    fl = filter_flops(level, tests, subsets)
    ach = fl / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else 0.0
    lds = (tests * 4.0 * (level + 2)) / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
    return {
        "kernel": f"sweep_vec_kernel<{level}, {mode}> (one launch per degree class)" if level < 9 else
                  f"sweep_fast_kernel<{level}, ...> (one launch per degree class)",
        "bound": "valu", "achieved": ach, "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / VALU_PEAK_TFLOPS,
        "traffic": None, "flops_per_step": fl, "kernel_ms_per_step": float(kernel_ms),
        "lds": {"achieved": lds, "peak": LDS_PEAK_GBS, "unit": "GB/s", "frac": lds / LDS_PEAK_GBS},
        "note": "levels >= 2 run from an LDS-staged sub-matrix (HBM traffic ~4 d^2 B per work item, negligible), so the "
                "bound is the fp32 vector pipe: achieved = issued filter flops (l(l-1)+5l+4 per test, FMA = 2, + the "
                "per-set Cholesky) / kernel time against the 157.3 TFLOP/s FP32 vector peak; lds = 4(l+2) B per test "
                "(one ds_read_b128 per conditioning variable feeds four tests) against 256 B/clk/CU",
    }


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def pcalg_probe():
    """BASELINE.json names pcalg::skeleton as the CPU baseline; R is not part of the image -- say so."""
    rs = shutil.which("Rscript")
    if not rs:
        return "unavailable (no Rscript on this box)"
    try:
        r = subprocess.run([rs, "-e", "library(pcalg)"], capture_output=True, timeout=30)
        return "available" if r.returncode == 0 else "unavailable (Rscript present, library(pcalg) fails)"
    except Exception as exc:  # noqa: BLE001
        return f"unavailable ({type(exc).__name__})"


# ---------------------------------------------------------------------------------------------------------------
# whole-chromosome workload through the block driver (config C4)
# ---------------------------------------------------------------------------------------------------------------
def write_chromosome(workdir, rank, world, blocks_per_gpu, N, p, dist=None):
    """Every rank generates the genotypes of its 25 blocks; rank 0 assembles the PLINK file set.  Returns
    (phen path, bfiles stem, .blocks path, sizes)."""
    from cigwas_amd import synth

    nb = blocks_per_gpu * world
    sizes = synth.chromosome_block_sizes(nb)
    G, contrib = synth.chromosome_segment(sizes, rank * blocks_per_gpu, (rank + 1) * blocks_per_gpu, N, p)
    means, stds = synth.bed_stats(G)
    synth.pack_bed(G).tofile(os.path.join(workdir, f"seg{rank}.bedpart"))
    np.save(os.path.join(workdir, f"seg{rank}.contrib.npy"), contrib)
    np.save(os.path.join(workdir, f"seg{rank}.means.npy"), means)
    np.save(os.path.join(workdir, f"seg{rank}.stds.npy"), stds)
    del G
    if dist is not None:
        dist.barrier()
    stem = os.path.join(workdir, "chr")
    if rank == 0:
        contrib = sum(np.load(os.path.join(workdir, f"seg{r}.contrib.npy")) for r in range(world))
        Y = synth.chromosome_traits(contrib)
        m = sum(sizes)
        with open(stem + ".bed", "wb") as f:
            f.write(bytes([0x6C, 0x1B, 0x01]))
            for r in range(world):
                with open(os.path.join(workdir, f"seg{r}.bedpart"), "rb") as g:
                    shutil.copyfileobj(g, f, 1 << 24)
        with open(stem + ".bim", "w") as f:
            f.write("".join(f"1\trs{i}\t0\t{1000 + i}\tA\tG\n" for i in range(m)))
        with open(stem + ".fam", "w") as f:
            f.write("".join(f"f{i} i{i} 0 0 0 -9\n" for i in range(N)))
        with open(stem + ".dim", "w") as f:
            f.write(f"{N}\t{m}\n")
        for sfx in ("means", "stds"):
            v = np.concatenate([np.load(os.path.join(workdir, f"seg{r}.{sfx}.npy")) for r in range(world)])
            with open(f"{stem}.{sfx}", "w") as f:
                f.write("".join(repr(float(x)) + "\n" for x in v.astype(np.float32)))
        synth.write_phen_fast(os.path.join(workdir, "y.phen"), Y)
        synth.write_blocks_file(os.path.join(workdir, "c.blocks"), sizes)
    if dist is not None:
        dist.barrier()
    return os.path.join(workdir, "y.phen"), stem, os.path.join(workdir, "c.blocks"), sizes


def chromosome_run(args, rank, world, device, cdev, dist, steps, warmup):
    """K passes of the job over the synthetic chromosome, for the default writer and for the other one.  Returns
    (scale object for rank 0, per-level detail of this rank's batches, seconds of the timed passes, canonical tests)."""
    import torch

    from cigwas_amd import run_blocks as rb

    N, p = args.individuals, args.traits
    # The synthetic INPUT files (350 MB per GPU's share: they are read once and staged in HBM) go to memory-backed storage
    # when the box has it: written to disk they leave the file system throttling writers for seconds -- the result files
    # of a SECOND bench run on the same box (the N = 1, 2, 4, 8 series) took 11-21 ms per pass instead of 1.9.  The
    # RESULT files of the timed passes go where a job's files go: TMPDIR / /tmp.
    if rank == 0:
        workdir = tempfile.mkdtemp(prefix="cusk_bench_", dir=os.environ.get("TMPDIR", "/tmp"))
        indir = tempfile.mkdtemp(prefix="cusk_bench_in_", dir=input_dir_root())
    else:
        workdir = indir = None
    if dist is not None:
        box = [workdir, indir]
        dist.broadcast_object_list(box, src=0)
        workdir, indir = box
    t0 = time.time()
    phen, stem, blocks, sizes = write_chromosome(indir, rank, world, args.blocks_per_gpu, N, p, dist)
    t_gen = time.time() - t0
    # the synthetic inputs were written a moment ago (hundreds of MB of dirty pages): without this the kernel's write-back
    # throttling lands on the result files of the timed passes (measured: 15-20 ms instead of 2 ms per 25 blocks)
    if rank == 0:
        os.sync()
    if dist is not None:
        dist.barrier()
    bs = rb.BlockSet(phen, stem, blocks, args.alpha, args.max_level, args.max_level_two, 1)
    bv = max(0, args.batch_vars)
    counter = [0]

    def one_pass(writer, timing=0, tm=None):
        out = None
        if rank == 0 or writer in ("local", "merge"):
            counter[0] += 1
            out = os.path.join(workdir, f"out{counter[0]}")
            os.makedirs(out, exist_ok=True)
        # timed passes run without per-level HIP events (a few microseconds of device time each); the per-level kernel
        # times of the roofline come from one untimed detail pass
        if writer == "merge" and bv <= 0:
            writer = "rank0"  # (the merge writer is part of the batched path)
        return rb.run_job(bs, out, device, inflight=args.inflight, schedule=args.schedule, collective_device=cdev,
                          options={"timing": timing}, writer=writer, batch_vars=bv, timings=tm, blockfile=blocks)

    def totals(stats):
        """(executed tests, canonical tests, phase sums) of one pass's stats (batched: list of batch stats; else per block)"""
        ex = ca = 0
        ph = {}
        it = stats if bv > 0 else stats.values()
        for s_ in it:
            ex += int(s_.tests[0]) + int(s_.tests[1])
            if bv > 0:
                ca += int(s_.canonical[0]) + int(s_.canonical[1])
            else:
                ca += int(sum(s_.stage[0].canonical_tests)) + int(sum(s_.stage[1].canonical_tests))
            for key in ("ms_corr", "ms_stage1", "ms_prune", "ms_stage2", "ms_reduce"):
                ph[key[3:]] = ph.get(key[3:], 0.0) + float(getattr(s_, key))
        return ex, ca, ph

    def timed(writer, K, W):
        for _ in range(W):
            one_pass(writer)
        if rank == 0:
            os.sync()  # the warm-up passes' files (and whatever the box wrote before) are on their way out before the clock starts
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex = ca = 0
        ph, tms = {}, {}
        done = None
        for _ in range(K):
            tm = {}
            done, stats, _owned = one_pass(writer, tm=tm)
            e_, c_, p_ = totals(stats)
            ex += e_
            ca += c_
            for k_, v_ in p_.items():
                ph[k_] = ph.get(k_, 0.0) + v_
            for k_, v_ in tm.items():
                tms[k_] = tms.get(k_, 0.0) + v_
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt, float(ex), float(ca)], dtype=torch.float64, device=cdev if cdev is not None else "cpu")
            tmax = t.clone()
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dt, ex, ca = float(tmax[0].item()), float(t[1].item()), float(t[2].item())
        nwritten = len(done) if done is not None else 0
        if writer in ("local", "merge") and dist is not None:
            t = torch.tensor([float(nwritten)], dtype=torch.float64, device=cdev if cdev is not None else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            nwritten = int(t[0].item())
        return dt, ex, ca, {k_: v_ / K for k_, v_ in ph.items()}, {k_: v_ / K * 1e3 for k_, v_ in tms.items()}, nwritten

    one_pass(args.writer)  # first pass of the process: allocations, staging of the .bed
    # --full: the untimed detail pass (per-level kernel times of the roofline) and the other writers' timed passes
    detail_stats = one_pass("local", timing=1)[1] if args.full else []
    dt, ex, ca, ph, tms, nwritten = timed(args.writer, steps, warmup)
    others = {}
    for other in ("merge", "rank0", "local") if args.full else ():
        if other == args.writer or (other == "merge" and bv <= 0):
            continue
        dt2, _ex2, _ca2, _ph2, tms2, _nw2 = timed(other, steps, 1)
        others[other] = {"blocks_per_sec": len(sizes) * steps / dt2, "ms_per_pass": dt2 / steps * 1e3,
                         "gather_ms": tms2.get("gather_s", 0.0) if other != "local" else 0.0, "write_ms": tms2.get("write_s")}
    # per-level totals over this rank's blocks (detail pass): which kernel dominates the device time
    lv_ms, lv_tests, lv_sub, nvar = np.zeros(15), np.zeros(15), np.zeros(15), 0
    for s_ in (detail_stats if bv > 0 or not detail_stats else detail_stats.values()):
        for st in (s_.stage[0], s_.stage[1]):
            for l in range(st.levels_run):
                lv_ms[l] += st.main_kernel_ms[l]
                lv_tests[l] += st.tests[l]
                lv_sub[l] += st.subsets[l]
        nvar = max(nvar, int(s_.vars_stage1) if bv > 0 else int(s_.markers) + p)
    nb = len(sizes)
    scale = {
        "workload": f"cusk whole-chromosome job through the block driver (BASELINE config 4's per-GPU share x {world}): {nb} unequal LD "
                    f"blocks ({args.blocks_per_gpu} per GPU, {int(sum(sizes))} SNPs, sizes min/mean/max "
                    f"{[int(min(sizes)), float(np.mean(sizes)), int(max(sizes))]}) x {p} traits, N={N}, alpha={args.alpha:g}, max level "
                    f"{args.max_level}, max level two {args.max_level_two}, depth 1; one pass = .bed (in HBM) -> correlations -> stage one "
                    f"-> prune -> stage two -> reduction -> result files",
        "n_gpus": world, "blocks": nb, "blocks_per_gpu": args.blocks_per_gpu, "passes": steps,
        "writer": args.writer,
        "blocks_per_sec": nb * steps / dt, "ms_per_pass": dt / steps * 1e3, "blocks_written_per_pass": nwritten,
        "gather_ms": tms.get("gather_s", 0.0) if args.writer != "local" else 0.0,
        "write_ms": tms.get("write_s"), "compute_ms": tms.get("compute_s"),
        "rank0_phase_ms_per_pass": ph,
        "ci_tests_per_sec": ca / dt, "ci_tests_per_pass": ca / steps, "executed_ci_tests_per_sec": ex / dt,
        "other_writers": others,
        "execution": (f"batched: blocks of a rank in batches of <= {bv} padded variables, one correlation build / level loop per stage / read-out "
                      f"per batch (cusk_blockset_run_batch)") if bv > 0 else "one block per engine run (cusk_blockset_run_block)",
        "batch_vars": bv, "schedule": args.schedule,
        "gather": ("writer merge: every rank writes the files of its own blocks; indices, adjacency and correlations of every block "
                   "(no separating sets) -> rank 0, which writes the merged skeleton merged_blocks* from memory (cusk_merge_packed = "
                   "merge-block-outputs).  writer rank0: the full results -> rank 0, which writes every file.  Transport: size all-gather + "
                   "one gather over "
                   + ("RCCL (backend nccl)" if cdev is not None else ("gloo" if dist is not None else "nothing (one rank)"))
                   + "; gather_ms / write_ms: rank 0's wall clock per pass for the exchange / for what it writes after it"),
        "inputs": ".bed / .phen / means / stds staged in HBM once per GPU (cusk_blockset_stage; the synthetic input files live under "
                  + input_dir_root() + "); result files written inside the timed region under " + os.environ.get("TMPDIR", "/tmp"),
        "curve_key": "scale.blocks_per_sec (same workload definition at every N: 25 blocks per GPU, weak scaling)",
        "generate_s": t_gen,
    }
    bs.close()
    if rank == 0:
        shutil.rmtree(workdir, ignore_errors=True)
        shutil.rmtree(indir, ignore_errors=True)
    return scale, (lv_ms, lv_tests, lv_sub, nvar), dt, ca


def input_dir_root():
    """where the synthetic input files of a run are written: CUSK_BENCH_INPUT_DIR, else /dev/shm when it is a writable
    directory with room, else TMPDIR / /tmp"""
    d = os.environ.get("CUSK_BENCH_INPUT_DIR")
    if d:
        return d
    try:
        st = os.statvfs("/dev/shm")
        if os.access("/dev/shm", os.W_OK) and st.f_bavail * st.f_frsize > (8 << 30):
            return "/dev/shm"
    except OSError:
        pass
    return os.environ.get("TMPDIR", "/tmp")


def e2e_block(args, bed, phen, means, stds, device):
    """BASELINE metric "wall-clock per 10k-SNP block at l <= 5": the headline block as a PLINK file set through
    cusk_blockset_run_block -- the code `mps cusk` runs (cli.cpp:521-677): correlation build from the packed genotypes (staged
    in HBM), stage one, prune, stage two (both at max level l), reduction -- plus writing the five result files."""
    from cigwas_amd import run_blocks as rb
    from cigwas_amd import synth
    from cigwas_amd.skeleton import Engine

    m, p, N = args.markers, args.traits, args.individuals
    d = tempfile.mkdtemp(prefix="cusk_e2e_in_", dir=input_dir_root())
    dout = tempfile.mkdtemp(prefix="cusk_e2e_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        stem = os.path.join(d, "blk")
        synth.write_bfiles(stem, bed, N, means, stds)
        synth.write_phen_fast(os.path.join(d, "y.phen"), np.asarray(phen, np.float32).reshape(p, N))
        synth.write_blocks_file(os.path.join(d, "b.blocks"), [m])
        bs = rb.BlockSet(os.path.join(d, "y.phen"), stem, os.path.join(d, "b.blocks"), args.alpha, args.max_level, args.max_level, 1)
        eng = Engine(device)
        eng.set_option("timing", 0)
        bs.stage(eng)
        out = os.path.join(dout, "out")
        os.makedirs(out)
        walls, phases = [], {}
        os.sync()  # (the input files were written a moment ago: keep their write-back out of the result files' way)
        for k in range(6):
            outk = os.path.join(out, str(k))  # a directory of its own per run: a job writes new files, it does not truncate old ones
            os.makedirs(outk)
            t0 = time.perf_counter()
            _, st, wr = bs.run_block_to_files(eng, 0, outk)  # (as `mps cusk` does: the library writes its own result)
            t2 = time.perf_counter()
            if k:  # the first call allocates
                walls.append((t2 - t0) * 1e3)
                for key in ("ms_inputs", "ms_corr", "ms_stage1", "ms_prune", "ms_stage2", "ms_reduce"):
                    phases.setdefault(key[3:], []).append(float(getattr(st, key)))
                phases.setdefault("write", []).append(wr * 1e3)
        phases = {k_: float(np.median(v_)) for k_, v_ in phases.items()}
        res = {"e2e_block_ms": float(np.median(walls)), "runs": len(walls), "phases_ms": phases, "retained_markers": int(st.retained),
               "ci_tests": [int(st.tests[0]), int(st.tests[1])], "max_level": args.max_level, "max_level_two": args.max_level,
               "path": "cusk_blockset_run_block (csrc/host/block_pipeline.h = `mps cusk`'s pipeline) + the five result files; .bed staged in HBM, "
                       "matrix never leaves the device between build and sweeps"}
        lib_release = rb.lib().cusk_blockset_release_engine
        lib_release(bs.h, eng.h)
        eng.close()
        bs.close()
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)
        shutil.rmtree(dout, ignore_errors=True)


DUMP_MAX_ROWS = {"edges": 1 << 20, "sepsets": 1 << 18}  # 16 MB + 37.7 MB of float64, + pMax and counters: < 64 MB in all


def _seeded_rows(count, cap, seed):
    """all row indices when count <= cap, else a fixed seeded sample of cap of them (ascending)"""
    if count <= cap:
        return np.arange(count)
    return np.sort(np.random.default_rng(seed).choice(count, cap, replace=False))


def dump_outputs(d, eng, Cd, st, engine):
    """--dump-outputs DIR: what the last timed step returned to its caller, as DIR/<name>.npy (float64 / float32).
    edges [E, 2] = (i, j), i < j, of the skeleton (the whole adjacency); canonical_tests = the device counter per level
    and, last, the level reached; cusk only: sepsets [R, 18] = (x, y, level, z, S[14], -1 padded) records sorted by
    (x, y), pmax_edges / pmax_sepsets = pMax at those pairs.  Above DUMP_MAX_ROWS rows a fixed seeded sample is written."""
    os.makedirs(d, exist_ok=True)
    G = eng.adjacency()
    ei, ej = np.nonzero(G)
    del G
    up = ei < ej
    ei, ej = ei[up], ej[up]
    r = _seeded_rows(len(ei), DUMP_MAX_ROWS["edges"], 1)
    ei, ej = ei[r], ej[r]
    np.save(os.path.join(d, "edges.npy"), np.stack([ei, ej], axis=1).astype(np.float64))
    np.save(os.path.join(d, "canonical_tests.npy"), np.array(list(st.canonical_tests) + [st.level], np.float64))
    if engine != "cusk":
        return
    x, y, lv, z, S = eng.sepsets()
    r = _seeded_rows(len(x), DUMP_MAX_ROWS["sepsets"], 2)
    x, y, lv, z, S = x[r], y[r], lv[r], z[r], S[r]
    rec = np.concatenate([np.stack([x, y, lv], axis=1).astype(np.float64), z.astype(np.float64)[:, None], S.astype(np.float64)], axis=1)
    np.save(os.path.join(d, "sepsets.npy"), rec)
    P = eng.pmax(Cd.ptr)
    np.save(os.path.join(d, "pmax_edges.npy"), P[ei, ej].astype(np.float32))
    np.save(os.path.join(d, "pmax_sepsets.npy"), P[x, y].astype(np.float32))


def full_block_detail(out, args, st, n, m, N, lv, main_ms, main_detail, kernel_ms, level_ms, D, corr_ms):
    """--full, block workload: the rooflines of the dominant kernel and of every level, the per-level table of the detail
    pass and the correlation build's timing, added to the line `out`"""
    # levels other than the dominant one: their kernel durations come from the detail pass
    for l in range(15):
        if l != lv:
            main_ms[l] = main_detail[l]
    # dominant kernel = the level whose sweep kernel takes the most device time; its duration comes from HIP
    # events the engine records on its own stream around that kernel alone (cusk_stats.main_kernel_ms)
    # HBM-side bytes per launch from the committed PMC passes (profiles/pmc_traffic.json: the headline block's cusk
    # engine; FETCH_SIZE corrected as the guide prescribes for gfx950, x 2 -- the run's own calibration beside it)
    traffic, traffic_detail = None, None
    tf = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(tf) and args.engine == "cusk":
        try:
            tj = json.load(open(tf))
            traffic = tj.get(f"level{lv}")
            traffic_detail = {k: v for k, v in tj.items() if k != "note" and (k.startswith(f"level{lv}") or k in ("fetch_calibration", "kernel"))}
        except Exception:  # noqa: BLE001
            traffic = None
    out["roofline"] = roofline_of(lv, st.tests[lv], st.subsets[lv], n, main_ms[lv], args.engine, traffic)
    out["roofline_counts"] = "tests and conditioning sets the dominant kernel EXECUTED in one launch (device counters)"
    out["level_rooflines"] = {str(l): {k: v for k, v in roofline_of(l, st.tests[l], st.subsets[l], n, main_ms[l], args.engine).items()
                                       if k in ("bound", "achieved", "peak", "unit", "frac", "kernel_ms_per_step", "lds")}
                              for l in range(st.levels_run) if main_ms[l] > 0}
    out["corr_roofline"] = {
        "kernel": "mxm_fp4_kernel<true> (v_mfma_scale_f32_32x32x64_f8f6f4 on e2m1 indicators, nine contingency GEMMs, "
                  "upper-triangle tiles, .bed decoded in-kernel)",
        "bound": "mfma",
        "achieved": (2.0 * 9.0 * N * m * (m - 1) / 2.0) / (corr_ms[1] * 1e-3) / 1e12 if corr_ms[1] > 0 else 0.0,
        "peak": 10000.0,
        "unit": "TOP/s",
        "frac": ((2.0 * 9.0 * N * m * (m - 1) / 2.0) / (corr_ms[1] * 1e-3) / 1e12) / 10000.0 if corr_ms[1] > 0 else 0.0,
        "dtype": "fp4 (e2m1) operands, f32 accumulation, exact for 0/1 indicators",
        "frac_of_int8_peak": ((2.0 * 9.0 * N * m * (m - 1) / 2.0) / (corr_ms[1] * 1e-3) / 1e12) / 5000.0 if corr_ms[1] > 0 else 0.0,
        "note": "ops = 2*9*N*m(m-1)/2 (SURVEY 8d); peak = dense FP4 MFMA (~10 PF, MI355X_MICROARCH.md), the pipe the kernel "
                "runs on; frac_of_int8_peak = the same rate against SURVEY 8d's 5 POPS int8 figure",
    }
    out["levels"] = {
        str(l): {"tests": int(st.tests[l]), "subsets": int(st.subsets[l]), "removed": int(st.removed[l]), "rechecks": int(st.rechecks[l]),
                 "max_degree": int(st.max_degree[l]), "sweep_ms": float(kernel_ms[l]), "level_ms": float(level_ms[l])}
        for l in range(st.levels_run)
    }
    out["levels_note"] = (f"sweep_ms / level_ms and the durations of level_rooflines other than level {lv}: detail pass of {D} untimed steps "
                          "with per-level HIP events (timing = 1); the timed steps record only the pair around the dominant kernel")
    out["corr_build_ms"] = {"decode": corr_ms[0], "snp_x_snp": corr_ms[1], "snp_trait_and_trait_trait": corr_ms[2],
                            "total_incl_h2d": corr_ms[3]}
    if traffic_detail:
        out["roofline"]["traffic_detail"] = traffic_detail
    if args.engine == "cusk" and sum(st.canonical_tests) > 0:
        # the dominant kernel's roofline on the CANONICAL tests of its level: the engine executes more tests than that
        # (lanes cannot see each other's fresh verdicts; level 1 evaluates every pair), so this is the figure that cannot be
        # inflated by doing needless work; roofline_executed = the same with the launch's own test counter
        ex_r = out["roofline"]
        out["roofline"] = roofline_of(lv, int(st.canonical_tests[lv]), int(st.subsets[lv]), n, main_ms[lv], args.engine, traffic)
        if traffic_detail:
            out["roofline"]["traffic_detail"] = traffic_detail
        out["roofline_counts"] = ("tests of the dominant kernel's level in the CANONICAL (sequential) schedule (device counter, equal to "
                                  "the oracle's count: parity.canonical_count_equal)")
        # NOT a roofline (the operands of the extra tests come from LDS, not HBM): how many tests the launch executed per second
        out["dominant_kernel_executed_tests"] = {"tests_per_launch": int(st.tests[lv]), "tests_per_sec": float(st.tests[lv]) / (main_ms[lv] * 1e-3) if main_ms[lv] > 0 else 0.0,
                                                 "bytes_equivalent_per_sec": ex_r["achieved"] * 1e9,
                                                 "note": "the launch evaluates every pair of a row (lanes cannot see each other's fresh verdicts); the byte figure prices those tests "
                                                         "with SURVEY 8(d)'s 12 B as if their operands came from HBM -- they come from LDS, so this is a rate, not a roofline fraction"}
    elif args.engine == "cuskss" and st.canonical_tests[lv] > 0:
        # hetcor engine: the finaliser of level 1 counts the canonical tests on the device (cusk_stats.canonical_tests[1]; the
        # deeper levels are not counted there): the dominant kernel's roofline is on canonical tests, as the cusk line's
        ex_r = out["roofline"]
        out["roofline"] = roofline_of(lv, int(st.canonical_tests[lv]), int(st.subsets[lv]), n, main_ms[lv], args.engine, traffic)
        out["roofline_counts"] = "tests of the dominant kernel's level in the CANONICAL (sequential) schedule (device counter of level1_apply_kernel)"
        out["dominant_kernel_executed_tests"] = {"tests_per_launch": int(st.tests[lv]), "tests_per_sec": float(st.tests[lv]) / (main_ms[lv] * 1e-3) if main_ms[lv] > 0 else 0.0,
                                                 "bytes_equivalent_per_sec": ex_r["achieved"] * 1e9, "note": "a rate, not a roofline fraction (see the cusk line)"}

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["auto", "block", "chromosome"], default="auto",
                    help="auto: the headline block at N = 1, the whole-chromosome job at N > 1")
    ap.add_argument("--markers", type=int, default=10000)
    ap.add_argument("--traits", type=int, default=20)
    ap.add_argument("--individuals", type=int, default=16384)
    ap.add_argument("--max-level", type=int, default=5)
    ap.add_argument("--max-level-two", type=int, default=14, help="chromosome workload: stage-two level bound (CLI default 14)")
    ap.add_argument("--blocks-per-gpu", type=int, default=25, help="chromosome workload: LD blocks per GPU (config C4: 200 on 8 GPUs)")
    ap.add_argument("--inflight", type=int, default=1, help="chromosome workload: blocks in flight per GPU")
    ap.add_argument("--schedule", choices=["lpt", "dynamic"], default="lpt")
    ap.add_argument("--writer", choices=["rank0", "merge", "local"], default="rank0",
                    help="chromosome workload: rank0 = one gather of the full results over RCCL, rank 0 writes every file; merge = every rank "
                         "writes the files of its own blocks and the merged skeleton (what merge-block-outputs reads of every block) is "
                         "gathered to rank 0 and written there as merged_blocks*; local = every rank writes its own blocks' files, no "
                         "exchange.  All three are measured, this one is the line's blocks_per_sec")
    ap.add_argument("--batch-vars", type=int, default=16384,
                    help="chromosome workload: blocks run in batches of at most this many padded variables (0: one block per engine run)")
    ap.add_argument("--scale-steps", type=int, default=5, help="N = 1: timed passes of the whole-chromosome leg (the `scale` object)")
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--engine", choices=["cusk", "cuskss"], default="cusk",
                    help="block workload: cusk = Skeleton engine (sepsets + pMax); cuskss = hetcor engine with uniform ESS")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo to rehearse on one GPU)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-chromosome", action="store_true", help="N = 1: skip the bounded whole-chromosome pass (the `scale` object)")
    ap.add_argument("--e2e", action="store_true", help="N = 1: the end-to-end block figure also for a non-headline configuration")
    ap.add_argument("--option", action="append", default=[], metavar="KEY=VALUE",
                    help="engine option for kernel experiments (cusk_set_option); the default run sets none")
    ap.add_argument("--cpu-sample-markers", type=int, default=10000)
    ap.add_argument("--cpu-threads", type=int, default=0, help="OpenMP threads of the CPU baseline (0 = min(16, affinity))")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: per-level detail pass and rooflines, correlation-build timing, "
                         "full-size parity against the CPU oracle and the CPU baselines, the end-to-end block, the whole-chromosome "
                         "pass (N = 1) and the other writers (chromosome workload).  A plain run sets up, warms up, times --steps "
                         "steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="block workload: after the timed steps, write what the last step returned to its caller as DIR/<name>.npy "
                         "(float32 / float64, <= 64 MB in all; see dump_outputs)")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        print(f"bench.py: --gpus {args.gpus} needs torchrun (WORLD_SIZE={world})", file=sys.stderr)
        sys.exit(2)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.workload == "chromosome" or (args.workload == "auto" and world > 1)):
        ap.error("--dump-outputs: the block workload only (the chromosome job's results are its files)")
    import torch
    import torch.distributed as dist

    ndev = torch.cuda.device_count()
    local_rank = local_rank % max(ndev, 1)
    torch.cuda.set_device(local_rank)
    cdev = None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            cdev = torch.device("cuda", local_rank)
        else:
            dist.init_process_group(args.backend)
    workload = args.workload if args.workload != "auto" else ("block" if world == 1 else "chromosome")

    if workload == "chromosome":
        scale, (lv_ms, lv_tests, lv_sub, nvar), dt, tests = chromosome_run(args, rank, world, local_rank, cdev,
                                                                           dist if world > 1 else None, args.steps, args.warmup)
        if rank == 0:
            K = args.steps
            lv = int(np.argmax(lv_ms[1:]) + 1) if lv_ms[1:].sum() > 0 else 0
            out = {
                "metric": "ci_tests_per_sec", "value": tests / dt, "unit": "CI tests/s", "n_gpus": world, "steps": K,
                "warmup": args.warmup, "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {
                    "workload": scale["workload"],
                    "blocks_per_step": scale["blocks"], "engine": "cusk", "parallelism": f"block-sharded x{world}, {args.schedule}",
                },
                "value_counts": "canonical CI tests of both stages (cusk_stats.canonical_tests: the sequential schedule, device counter); "
                                "scale.executed_ci_tests_per_sec = what the parallel sweeps executed",
                "blocks_per_sec": scale["blocks_per_sec"],
                "scaling_curve_key": scale["curve_key"],
                "scale": scale,
            }
            if args.full:
                out["roofline"] = roofline_of(lv, lv_tests[lv], lv_sub[lv], nvar, lv_ms[lv], "cusk")
                out["roofline"]["note"] = ("rank 0's batches of an untimed detail pass (per-level HIP events on), summed over batches and both stages: the level whose "
                                           "dominant kernel takes the most device time; " + out["roofline"]["note"])
            print(json.dumps(out))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ------------------------------------------------------------------------------------------------------
    # headline block workload (N = 1)
    # ------------------------------------------------------------------------------------------------------
    if world > 1:
        print("bench.py: the block workload is the single-GPU headline; N > 1 runs the chromosome workload", file=sys.stderr)
        sys.exit(2)
    import cigwas_amd as cg
    from cigwas_amd import synth

    m, p, N = args.markers, args.traits, args.individuals
    n = m + p
    t0 = time.time()
    bed, phen, means, stds, _G = synth.synth_bed_block(m, N, p, block_index=rank)
    del _G
    t_gen = time.time() - t0

    eng = cg.Engine(local_rank)
    # the matrix is written by cusk_corr_build, which mirrors every element: symmetric by construction
    eng.set_option("assume_symmetric", 1)
    for kv in args.option:
        k, v = kv.split("=")
        eng.set_option(k, int(v))
    Cd = cg.DeviceArray(nbytes=4 * n * n)
    eng.corr_build(bed, phen, m, N, p, means, stds, Cd.ptr)
    if args.full:  # a second, warm build for corr_build_ms / corr_roofline
        eng.corr_build(bed, phen, m, N, p, means, stds, Cd.ptr)
        corr_ms = [float(x) for x in eng.corr_timing()]

    Th = cg.threshold_array(N, args.alpha)
    th_het = cg.hetcor_threshold(args.alpha)

    def step():
        if args.engine == "cusk":
            return eng.run_skeleton(Cd.ptr, n, Th, args.max_level)
        return eng.run_hetcor(Cd.ptr, n, th_het, args.max_level, ess_uniform=float(N))

    if not args.full and not any(kv.split("=")[0] == "timing" for kv in args.option):
        eng.set_option("timing", 0)  # a plain run records no per-level HIP events: nothing reads them
    for _ in range(args.warmup):
        st = step()
    if args.full:
        # Detail pass (untimed): per-level events (option timing = 1: a pair around every level's sweep) for the `levels`
        # table and the per-level rooflines.  Every HIP event costs a few microseconds of device time (a dozen per step:
        # ~50 us of a 1.3 ms step), so the timed steps below record only the pair around the dominant kernel (timing = 3)
        # -- the roofline's duration is still measured live, inside the timed region, on the engine's own stream.
        D = 5
        kernel_ms = np.zeros(15)
        level_ms = np.zeros(15)
        main_detail = np.zeros(15)
        eng.set_option("timing", 1)
        for _ in range(D):
            st = step()
            kernel_ms += np.array(st.kernel_ms)
            level_ms += np.array(st.level_ms)
            main_detail += np.array(st.main_kernel_ms)
        kernel_ms /= D
        level_ms /= D
        main_detail /= D
        lv = int(np.argmax(main_detail[1:]) + 1) if st.levels_run > 1 else 0
        eng.set_option("timing", 3 if lv == 1 else 1)
    st = step()  # untimed: the first step after the last change of options (and the only one before the clock with --warmup 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tests_total = 0
    main_ms = np.zeros(15)
    for _ in range(args.steps):
        st = step()
        tests_total += sum(st.tests)
        main_ms += np.array(st.main_kernel_ms)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, eng, Cd, st, args.engine)

    K = args.steps
    main_ms /= K
    headline = (m == 10000 and p == 20 and N == 16384 and args.max_level == 5 and args.engine == "cusk")
    out = {
        "metric": "ci_tests_per_sec",
        "value": tests_total / dt,
        "unit": "CI tests/s",
        "n_gpus": world,
        "steps": K,
        "warmup": args.warmup,
        "ms_per_step": dt / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": f"{args.engine} level sweep, one LD block {m} SNPs x {p} traits, N={N}, alpha={args.alpha:g}, "
                        f"max level {args.max_level}{' (north_star headline)' if headline else ''}; correlation matrix from "
                        f"synthetic .bed (Kendall-npn/Pearson) resident in HBM",
            "blocks_per_step": 1,
            "n_variables": n,
            "engine": args.engine,
        },
        "value_counts": "executed CI tests (device counters)",
        "executed_tests_per_step": tests_total / K,
        "canonical_tests_per_step_device": int(sum(st.canonical_tests)) if args.engine == "cusk" else None,
        "canonical_tests_by_level_device": [int(v) for v in st.canonical_tests[: st.levels_run]],
        "headline_block_sweeps_per_sec": K / dt,
        "filter_violations": int(st.violations), "exact_fallbacks": int(st.exact_fallbacks),
        "synth_gen_s": t_gen,
        "full": bool(args.full),
    }
    if args.engine == "cusk" and sum(st.canonical_tests) > 0:
        # `value` = canonical CI tests (the sequential schedule of the reference algorithm, computed on the device from
        # the selected ranks and checked against the oracle's own count in --full runs) over the measured time
        out["value_executed"] = out["value"]
        out["value"] = float(sum(st.canonical_tests)) / (dt / K)
        out["value_counts"] = ("canonical CI tests (sequential schedule; cusk_stats.canonical_tests, device counter) / measured time; "
                               "value_executed = executed tests (device counters) / the same time")
    if args.full:
        full_block_detail(out, args, st, n, m, N, lv, main_ms, main_detail, kernel_ms, level_ms, D, corr_ms)
    if args.full and not args.no_cpu_baseline:
        nall = args.cpu_threads or min(16, len(os.sched_getaffinity(0)))
        from oracle import oracle as O

        ms_ = min(args.cpu_sample_markers, m)
        ix = np.concatenate([np.arange(ms_), np.arange(m, n)])
        Ch = Cd.download(np.float32, (n, n))
        sub = np.ascontiguousarray(Ch[np.ix_(ix, ix)]) if ms_ < m else Ch
        Thc = O.threshold_array(N, args.alpha)

        def run_ref(mat, threads):
            os.environ["OMP_NUM_THREADS"] = str(threads)
            tc = time.perf_counter()
            if args.engine == "cusk":
                r = O.skeleton(mat, Thc, args.max_level)
            else:
                r = O.hetcor_skeleton(mat, np.ones(mat.shape, np.int32), np.full(mat.shape, N, np.float32), th_het,
                                      args.max_level, np.zeros(mat.shape[0], np.int32))
            return r, time.perf_counter() - tc

        import ctypes as C

        try:  # the oracle reads OMP_NUM_THREADS once at load: set the team size explicitly as well
            omp = C.CDLL("libgomp.so.1")
        except OSError:
            omp = None

        def set_threads(k):
            if omp is not None:
                omp.omp_set_num_threads(int(k))

        set_threads(nall)
        ref, tcpu = run_ref(sub, nall)
        # ---- parity at the size that is timed: adjacency, level counter, separating sets vs the oracle ----
        if ms_ == m:
            G = eng.adjacency()
            par = {"adjacency_equal": bool(np.array_equal(G, ref.G)), "level_equal": bool(st.level == ref.level),
                   "edges": int(ref.G.sum() // 2)}
            del G
            if args.engine == "cusk":
                x, y, _lv, _z, S = eng.sepsets()
                rx, ry = np.nonzero(ref.sepset[:, :, 0] != -1)
                same = (len(rx) == len(x)) and np.array_equal(rx, x) and np.array_equal(ry, y) and np.array_equal(ref.sepset[rx, ry], S)
                par["sepsets_equal"] = bool(same)
                par["sepset_records"] = int(len(x))
            out["parity_checked"] = True
            out["parity_ok"] = bool(all(v for k, v in par.items() if k.endswith("_equal")))
            out["parity"] = par
            # the sequential (oracle) schedule skips tests that parallel lanes cannot know are already decided: `value`
            # is the canonical count over the measured time, the rate of executed tests is reported beside it
            out["canonical_tests_per_step"] = int(ref.tests.sum())
            out["canonical_tests_by_level"] = [int(v) for v in ref.tests[: st.levels_run]]
            if args.engine == "cusk":
                par["canonical_count_equal"] = bool(int(sum(st.canonical_tests)) == int(ref.tests.sum()))
                out["parity_ok"] = bool(out["parity_ok"] and par["canonical_count_equal"])
            else:
                if st.canonical_tests[1] > 0:
                    par["canonical_count_level1_equal"] = bool(int(st.canonical_tests[1]) == int(ref.tests[1]))
                    out["parity_ok"] = bool(out["parity_ok"] and par["canonical_count_level1_equal"])
                out["value_executed"] = out["value"]
                out["value"] = float(ref.tests.sum()) / (dt / K)
                out["value_counts"] = ("canonical CI tests (counted by the oracle on this very matrix) / measured time; "
                                       "value_executed = the engine's device counters / the same time")
        else:
            out["parity_checked"] = False
        base = {
            "value": float(ref.tests.sum()) / tcpu, "unit": "CI tests/s", "cores": nall, "kind": "port", "cpu_model": cpu_model(),
            "sample": f"oracle (C restatement of the reference's fp32 arithmetic, OpenMP over rows) on the leading {ms_} SNPs + {p} "
                      f"traits of the same matrix, levels 0..{args.max_level}: {int(ref.tests.sum())} tests in {tcpu:.2f} s",
        }
        # one thread, bounded sample (about a fifth of the block)
        m1 = min(6000, ms_)
        ix1 = np.concatenate([np.arange(m1), np.arange(m, n)])
        sub1 = np.ascontiguousarray(Ch[np.ix_(ix1, ix1)])
        set_threads(1)
        r1, t1 = run_ref(sub1, 1)
        base["one_thread"] = {"value": float(r1.tests.sum()) / t1, "cores": 1,
                              "sample": f"leading {m1} SNPs + {p} traits: {int(r1.tests.sum())} tests in {t1:.2f} s"}
        # double precision, pcalg::gaussCItest semantics (the named baseline's algorithm; pcalg itself: see probe)
        set_threads(nall)
        tc = time.perf_counter()
        r64 = O.pcstable_f64(sub, float(N), args.alpha, args.max_level)
        t64 = time.perf_counter() - tc
        base["f64_gaussCItest"] = {
            "value": float(r64.tests.sum()) / t64, "cores": nall,
            "sample": f"PC-stable in double precision, sqrt(N-|S|-3)|atanh r| <= qnorm(1-alpha/2), same matrix: "
                      f"{int(r64.tests.sum())} tests in {t64:.2f} s",
            "adjacency_entries_differing_from_fp32_reference_arithmetic": int((r64.G != ref.G).sum()),
        }
        base["pcalg"] = pcalg_probe()
        out["cpu_baseline"] = base
        del Ch, sub, sub1, ref, r64
    Cd.free()
    eng.close()
    if (args.full and headline) or args.e2e:
        out["e2e_block"] = e2e_block(args, bed, phen, means, stds, local_rank)
        out["e2e_block_ms"] = out["e2e_block"]["e2e_block_ms"]
    if args.full and not args.no_chromosome:
        a2 = argparse.Namespace(**vars(args))
        scale, _lvs, _dt, _tests = chromosome_run(a2, 0, 1, local_rank, None, None, args.scale_steps, 1)
        out["scale"] = scale
        out["scaling_curve_key"] = scale["curve_key"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
