// level_loop.hip -- host side of the level sweep: one skeleton run as a struct (LevelRun) with named steps.  The level
// loop of the reference's cusk/src/cuPC-S.cu:99-415 and hetcor-cuPC-S.cu:115-332, enqueued ahead of the device (DESIGN.md,
// "Host loop"); the decisions that need no device (kernel of a class, classes with work, outcome of the read-back) are
// functions of plain values in host/level_policy.h.
#include <algorithm>
#include <atomic>
#include <chrono>

#include "host/level_policy.h"
#include "sweep_common.h"

namespace cusk {
namespace {

#define STEP(call) do { const int rc_ = (call); if (rc_ != CUSK_OK) return rc_; } while (0)

struct LevelPlan
{
    SweepParams sp;
    FinalizeParams fp;
    long long nitems[kNumClasses];
    bool use_pair = false, use_fast = false, use_rows = false, filter_ok = true;
    size_t pair_lds = 0;
    bool redone = false;
    bool known_items = false;  // nitems[] holds the level's real class counts (row-sharded runs wait for them)
    int maxdeg_bound = 0;      // no row has more neighbours than this (newest maximum degree the host has seen)
    int staged_classes = 0;
    unsigned long long chunk0 = 0;  // conditioning sets per work item of the first degree class at this level
    bool tmaj = false;         // swept by unions T = S + Y (sweep_tmaj.hip): the work items count (l + 1)-subsets
    bool force_exact = false;  // the level is taken up again on the exact arithmetic (recheck queue overflow of a tmaj level)
};

// what kind of run this is, fixed in prepare()
struct ModeFlags
{
    bool het;         // per-pair sample sizes (hetcor with a matrix, or cusk_run_skeleton_het): a threshold per test, HET kernels
    bool het0;        // ... with Skeleton's records: no vectorised sweep, no level-1 pair kernel
    bool het0_exact;  // ... and without option het_filter: every level on the exact path
    bool sharded;     // rows split over several engines: an exchange per level, the host follows at distance 0
    bool batched;     // blocks on the diagonal of one allocation: level 0 by level0_batch_kernel, symmetric by construction
    // the size matrix is checked for bitwise symmetry (launched with level 0, read after level 1's gate); a symmetric one allows
    bool ness_checked;       // ... the union-major sweep of the deep levels at one threshold per union (option het_filter)
    bool ness_checked_rows;  // ... level 1 on the row kernel, both tests of a pair at one threshold (option het_rows)
};

struct LevelRun
{
    cusk_engine *e;
    const RunArgs &a;
    hipStream_t s = e->stream;
    const int n = a.n, words = (n + 63) / 64, last_level = std::min(kML, a.maxlevel);
    ModeFlags m = {};
    cusk_stats local = {};
    long long &item_cap = e->item_cap_cur;
    int run_seq = 0, staged_classes = 0, lookahead = 0;
    char *ctl = nullptr;  // the control block and what lies in it (kCtl*)
    LevelCounters *dcnt = nullptr;
    unsigned long long *dslots = nullptr, *dcanon = nullptr;  // counter slots, canonical test counters
    int *dsym = nullptr;                                      // level 0's asymmetry flag
    LevelPlan plan[kLevels];
    PlanArgs pa;  // of the plan enqueued last
    // Gate of a level's finalisation and of the next level's plan: "the recheck queue held every uncertain test".  A
    // level that is run (or redone) on the exact path has no queue: ~0.
    unsigned long long qcap_gate[kLevels];
    unsigned long long chunk = 0, chunk0 = 0;
    bool symmetric = false, rows_timed = false, first_pass = true;
    bool ness_symmetric = false;  // the size matrix is bitwise symmetric: means something only under m.ness_checked / _rows
    int level1_form = -1;  // cusk_engine_level1_form: the kernel level 1 was enqueued on
    int maxdeg1 = 0, maxdeg2 = -1;  // maximum degree at the start of levels 1 and 2 (-1: the host has not seen it yet)
    int start = 1;     // first level to enqueue in this pass
    int redo = 0;      // level whose recheck queue overflowed: its sweeps run again on the exact path before `start`
    int enq_last = 0, planned_last = 0;  // last level enqueued in this pass; last one whose plan kernel was (>= enq_last)
    bool closed = false, done = false;   // the host has seen a level's closed gate: nothing more is enqueued in this pass; the run is over
    int level_out = (a.maxlevel < 0) ? 0 : last_level + 1, levels_swept = 0;
    const std::chrono::steady_clock::time_point hp_t0 = std::chrono::steady_clock::now();
    std::string hp_log;  // option hostprof: host-side phase marks of the run (microseconds since entry) on stderr

    void hp_mark(const char *what)
    {
        if (!e->opt_hostprof) return;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hp_t0).count();
        char buf[64];
        std::snprintf(buf, sizeof(buf), " %s=%.1f", what, us);
        hp_log += buf;
    }
    void mark_redone(int l) { plan[l].redone = true; local.exact_fallbacks++; qcap_gate[l] = ~0ull; }  // once more, on the exact path
    int *off_of(int l) const { return (l == 1) ? e->off1.as<int>() : e->off[l & 1].as<int>(); }
    float level_threshold(int l) const { return m.het ? a.Th[0] : (a.mode == 0) ? a.Th[l] : uniform_ess_threshold(a.Th[0], a.ess_uniform, l); }

    // buffers, plan-block sequence, control block, time index
    int prepare()
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        for (auto &q : qcap_gate) q = ~0ull;
        e->n = n;
        e->words = words;
        e->mode = a.mode;
        e->have_result = false;
        e->nrec = 0;
        e->level1_form = -1;
        m.het = (a.Ness != nullptr);
        m.het0 = m.het && a.mode == 0;
        m.het0_exact = m.het0 && e->opt_het_filter == 0;
        m.sharded = e->shard_world > 1;
        m.batched = (a.row_range != nullptr);
        m.ness_checked = m.het0 && e->opt_het_filter != 0 && last_level >= 2;
        m.ness_checked_rows = m.het0 && e->opt_het_rows != 0 && last_level >= 1;
        if (m.sharded && !e->shard_fn) return fail(e, CUSK_ERR_ARG, "row sharding needs an exchange function");

        const size_t bm = sizeof(unsigned long long) * (size_t)n * words;
        CUSK_HIP(e, e->adj.ensure(bm));
        if (a.mode == 0) CUSK_HIP(e, e->adj0.ensure(bm));
        CUSK_HIP(e, e->deg.ensure(sizeof(int) * (size_t)n));
        // per-run control block (level counters, counter slots, record bases, symmetry flag): one allocation, one
        // memset, one read-back at the end (pinned mirror with the same layout)
        CUSK_HIP(e, e->counters.ensure(kCtlBytes));
        item_cap = std::max<long long>(item_cap, std::max<long long>(e->opt_item_cap, 1024));
        for (int k = 0; k < 2; k++)
        {
            CUSK_HIP(e, e->off[k].ensure(sizeof(int) * ((size_t)n + 1)));
            for (int c = 0; c < kNumClasses; c++) CUSK_HIP(e, e->items[k][c].ensure(sizeof(int2) * (size_t)item_cap));
        }
        CUSK_HIP(e, e->off1.ensure(sizeof(int) * ((size_t)n + 1)));
        // plan kernel: 8 words per 256-row block, validated by a 24-bit launch sequence number (cleared when it wraps or the buffer is new)
        const size_t need = sizeof(unsigned long long) * 8 * (((size_t)n + 255) / 256);
        const bool fresh = need > e->planblk.cap;
        CUSK_HIP(e, e->planblk.ensure(need));
        if (fresh || e->plan_seq >= 0xfffff0u)
        {
            CUSK_HIP(e, hipMemsetAsync(e->planblk.p, 0, e->planblk.cap, s));
            e->plan_seq = 0;
        }
        run_seq = ++e->run_seq;
        e->records_ready = e->z_ready = false;
        e->rec_slots = 0;
        e->last_C = a.C;
        ctl = e->counters.as<char>();
        dcnt = reinterpret_cast<LevelCounters *>(ctl + kCtlCnt);
        dslots = reinterpret_cast<unsigned long long *>(ctl + kCtlSlots);
        dcanon = reinterpret_cast<unsigned long long *>(ctl + kCtlCanon);
        dsym = reinterpret_cast<int *>(ctl + kCtlSym);
        CUSK_HIP(e, hipMemsetAsync(ctl, 0, kCtlBytes, s));
        if (a.mode == 1)
        {
            CUSK_HIP(e, e->ti.ensure(sizeof(int) * (size_t)n));
            if (a.time_index)
                CUSK_HIP(e, hipMemcpyAsync(e->ti.p, a.time_index, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
            else
                CUSK_HIP(e, hipMemsetAsync(e->ti.p, 0, sizeof(int) * (size_t)n, s));
        }
        chunk = (unsigned long long)std::max<long long>(e->opt_chunk, 256);
        chunk0 = (unsigned long long)std::max<long long>(e->opt_chunk0, 64);
        // which classes can be staged in LDS in this mode
        while (staged_classes < kNumClasses - 1 && lds_layout(kClassCap[staged_classes], m.het).total <= kLdsLimit) staged_classes++;
        if (e->opt_max_staged_classes >= 0) staged_classes = std::min(staged_classes, e->opt_max_staged_classes);  // test hook: 0 = every row through L2
        // no launch needs a number from the host, which only follows `lookahead` levels behind the device to stop enqueuing
        // once the loop has ended ("Host loop"); row-sharded runs call back every level and follow at distance 0
        lookahead = m.sharded ? 0 : std::max(0, e->opt_lookahead);
        return CUSK_OK;
    }

    int enqueue_level0()
    {
        CUSK_HIP(e, hipEventRecord(e->ev_run[0], s));
        CUSK_HIP(e, hipEventRecord(e->ev_l0[0], s));
        float th0 = a.Th[0];
        if (a.mode == 1 && !m.het) th0 = (float)((double)a.Th[0] / std::sqrt((double)a.ess_uniform - 3.0));
        if (m.batched)
            CUSK_HIP(e, launch_level0_batch(a.C, m.het0 ? a.Ness : nullptr, e->adj.as<unsigned long long>(), e->adj0.as<unsigned long long>(),
                                            e->deg.as<int>(), n, words, a.row_range, th0, s));
        else
        {
            CUSK_HIP(e, launch_level0(a.C, m.het ? a.Ness : nullptr, a.Ginit, e->adj.as<unsigned long long>(), n, words, th0,
                                      e->opt_assume_symmetric ? nullptr : dsym, s));
            // (Skeleton mode keeps the bitmap of level 0: the degree pass below writes the copy; without a level 1 nobody reads it
            // but the pMax read-out, which then needs the copy made here)
            if (a.mode == 0 && last_level < 1)
                CUSK_HIP(e, hipMemcpyAsync(e->adj0.p, e->adj.p, sizeof(unsigned long long) * (size_t)n * words, hipMemcpyDeviceToDevice, s));
        }
        // is the size matrix bitwise symmetric (inside the blocks of a batch)?  Launched with level 0, read with the round
        // trip that follows it (size_from_level1)
        if (m.ness_checked || m.ness_checked_rows)
        {
            *e->hflag = 0;
            CUSK_HIP(e, launch_ess_symmetry(a.Ness, n, a.row_range, e->hflag, s));
        }
        CUSK_HIP(e, hipEventRecord(e->ev_l1[0], s));
        hp_mark("l0_enq");
        local.max_degree[0] = n - 1;
        local.edges[0] = (long long)n * (n - 1);
        local.tests[0] = m.batched ? a.level0_pairs : (long long)n * (n - 1) / 2;
        local.canonical_tests[0] = local.tests[0];
        local.levels_run = 1;
        if (last_level >= 1 && !m.batched)
            CUSK_HIP(e, launch_degree(e->adj.as<unsigned long long>(), e->deg.as<int>(), n, words,
                                      a.mode == 0 ? e->adj0.as<unsigned long long>() : nullptr, s));
        return CUSK_OK;
    }

    int launch_sweeps(int l, bool exact_only)
    {
        LevelPlan &pl = plan[l];
        SweepParams sp = pl.sp;
        // The degree classes of a level are independent launches: the first on the engine stream, the others on the auxiliary
        // stream (tiny rows next to hub rows fill the chip better together); the streams join before the recheck pass.  Every
        // launch is persistent and reads its class's work-item count on the device (empty classes return at once).
        if (pl.use_rows && !exact_only)
        {
            CUSK_HIP(e, launch_level1_rows(a.mode, e->opt_validate != 0, pl.filter_ok && e->opt_fast != 0, sp, e->rv.as<float>(),
                                           e->rpos.p, e->sel.as<unsigned>(), e->wpre.as<int>(), e->opt_timing ? e->ev_main[0] : nullptr,
                                           e->opt_timing ? e->ev_main[1] : nullptr, e->shard_rank, e->shard_world, e->opt_l1_threads, e->opt_l1_lds_row != 0, m.sharded,
                                           a.time_index != nullptr, (a.mode == 1) ? dcanon + (size_t)l * kCounterSlots : nullptr, s,
                                           m.het0 ? e->nv.as<float>() : nullptr, &level1_form));
            rows_timed = true;
            return CUSK_OK;
        }
        if (l == 1) level1_form = (pl.use_pair && !exact_only) ? 1 : 0;
        bool may[kNumClasses];
        const int nonempty = classes_with_work(pl.known_items, pl.nitems, pl.staged_classes, pl.maxdeg_bound, kClassCap, kNumClasses, may);
        const bool fork = (nonempty > 1) && (e->opt_overlap != 0);  // (a stale degree bound forks for classes that turn out empty)
        if (fork)
        {
            CUSK_HIP(e, hipEventRecord(e->ev_fork, s));
            CUSK_HIP(e, hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
        }
        bool first = true;
        for (int c = 0; c < kNumClasses; c++)
        {
            if (!may[c]) continue;
            hipStream_t cs = (fork && !first) ? e->stream2 : s;
            first = false;
            sp.items = e->items[l & 1][c].as<int2>();
            sp.cap = kClassCap[c];
            sp.cls = c;
            sp.chunk = (c == 0) ? pl.chunk0 : chunk;
            sp.item_cap = item_cap;
            sp.grid_cap = item_cap;
            if (l >= 2 && !pl.use_pair && !pl.tmaj)
            {
                // small blocks: no more workgroups than the class can have items -- at most n rows of at most dmax neighbours
                // with ceil(C(dmax, l) / chunk) items each (the bound of the degrees the host has seen, the class capacity)
                const int dmax = std::min(pl.maxdeg_bound, kClassCap[c]);
                const unsigned long long sets = binom_sat(dmax, l);
                const unsigned long long per_row = sets / sp.chunk + 1ull;
                if (per_row < (1ull << 40)) sp.grid_cap = std::min<long long>(item_cap, (long long)(per_row * (unsigned long long)n));
            }
            sp.validate = e->opt_validate ? std::max(1, e->opt_tmaj_validate_stride) : 0;
            switch (sweep_kind(l, c, m.het, pl.use_pair, pl.tmaj, pl.use_fast, exact_only, e->opt_vec != 0, e->opt_validate != 0,
                               c < kNumClasses - 1 && sweep_vec_lds_bytes(c) <= kLdsLimit, kNumClasses, kVecMaxLevel))
            {
            case SweepKind::Pair: CUSK_HIP(e, launch_pair(a.mode, sp, pl.pair_lds, cs)); break;
            case SweepKind::Tmaj: CUSK_HIP(e, launch_sweep_tmaj(a.mode, m.het, l, sp, c, cs)); break;
            case SweepKind::Vec: CUSK_HIP(e, launch_sweep_vec(a.mode, l, sp, c, c == 0 ? e->opt_vec_threads : kThreads, cs)); break;
            case SweepKind::Fast: CUSK_HIP(e, launch_sweep_fast(a.mode, m.het, l, e->opt_validate != 0, sp, c, cs)); break;
            case SweepKind::Exact: CUSK_HIP(e, launch_sweep_exact(a.mode, m.het, l, sp, c, cs)); break;
            }
        }
        if (fork)
        {
            CUSK_HIP(e, hipEventRecord(e->ev_join, e->stream2));
            CUSK_HIP(e, hipStreamWaitEvent(s, e->ev_join, 0));
        }
        if (pl.use_fast && !exact_only) CUSK_HIP(e, launch_recheck(a.mode, m.het, l, sp, s));
        return CUSK_OK;
    }

    int launch_finalize(int l)
    {
        if (a.mode != 0) return CUSK_OK;
        plan[l].fp.qcap = qcap_gate[l];
        // separating-set records in place (level-1 slot of the pair), bitmap rows and degrees; the winners' exact z is
        // computed when somebody asks for it
        CUSK_HIP(e, cusk::launch_finalize(l, plan[l].fp, s));
        return CUSK_OK;
    }

    // row-sharded runs: join the engines' selection state after a level's sweep (unsigned MIN), then derive what the
    // sweep kernels would have left behind on a single engine
    int shard_join(int l)
    {
        LevelPlan &pl = plan[l];
        if (pl.use_fast && l >= 2)
        {  // a recheck queue that overflowed on this engine: finish its rows on the exact path now (local decision)
            CUSK_HIP(e, hipMemcpyAsync(e->hcnt + l, dcnt + l, sizeof(LevelCounters), hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipStreamSynchronize(s));
            if (e->hcnt[l].qcount > (unsigned long long)e->opt_queue_cap)
            {
                mark_redone(l);
                STEP(launch_sweeps(l, true));
            }
        }
        const size_t count = (size_t)e->hgate[l].total_edges;
        // Skeleton: the lowest passing rank per slot (64 bits; the row kernel's 32-bit form at level 1).  hetcor: one
        // 32-bit mark per slot, 0 = the edge is gone (the row kernel leaves exactly that; the other kernels clear
        // adjacency bits, which are turned into marks here): in both cases the join is an unsigned MIN
        if (a.mode == 1 && !pl.use_rows) CUSK_HIP(e, launch_marks_from_bitmap(pl.sp, e->sel.as<unsigned>(), s));
        const int elem = (pl.use_rows || a.mode == 1) ? 4 : 8;
        void *dev = (pl.use_rows || a.mode == 1) ? e->sel.p : e->best[l & 1].p;
        int rc = 0;
        if (e->shard_host_staging)
        {
            const size_t bytes = count * (size_t)elem;
            CUSK_HIP(e, e->shard_host.ensure(bytes, std::max<size_t>(bytes, 64)));
            CUSK_HIP(e, hipMemcpyAsync(e->shard_host.p, dev, bytes, hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipStreamSynchronize(s));
            rc = e->shard_fn(e->shard_user, l, e->shard_host.p, count, elem, 0, (void *)s);
            if (rc == 0) CUSK_HIP(e, hipMemcpyAsync(dev, e->shard_host.p, bytes, hipMemcpyHostToDevice, s));
        }
        else
        {
            CUSK_HIP(e, hipStreamSynchronize(s));
            rc = e->shard_fn(e->shard_user, l, dev, count, elem, 1, (void *)s);
        }
        if (rc != 0) return fail(e, CUSK_ERR_ARG, "row-shard exchange failed at level " + std::to_string(l));
        // hetcor: every engine now drops the edges any engine removed (bitmap rows and degrees, identically everywhere)
        if (a.mode == 1)
            CUSK_HIP(e, launch_level1_apply(pl.sp, e->sel.as<unsigned>(), (l == 1 && pl.use_rows) ? e->rpos.p : nullptr, false, s));
        return CUSK_OK;
    }

    // the level's plan kernel writes its gate record into pinned host memory; spin until this run's record is there
    int wait_gate(int l)
    {
        volatile int *seq = &e->hgate[l].seq;
        for (unsigned long it = 1; *seq != run_seq; it++)
        {
            if ((it & 0x3fff) == 0)
            {
                const hipError_t q = hipStreamQuery(s);
                if (q == hipSuccess)
                {
                    if (*seq == run_seq) break;
                    return fail(e, CUSK_ERR_HIP, "level " + std::to_string(l) + ": the stream drained without the level's gate record");
                }
                if (q != hipErrorNotReady) return fail(e, CUSK_ERR_HIP, std::string("stream error while waiting for a level gate: ") + hipGetErrorString(q));
            }
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return CUSK_OK;
    }

    // 1. the plan of the level from the degrees alone: offsets, work items, totals, gate (level 1 is planned for
    //    the generic kernels first: whether the matrix is symmetric is only known with the first read-back, and the
    //    row-streaming kernel does not use work items)
    int enqueue_plan(int l)
    {
        const int cs = l & 1, behind = l - 1 - lookahead;
        if (behind >= start)
        {  // follow the device at a distance: has the loop ended `lookahead` levels ago?
            STEP(wait_gate(behind));
            if ((closed = !e->hgate[behind].active)) return CUSK_OK;
        }
        if (e->opt_timing == 2) CUSK_HIP(e, hipEventRecord(e->ev_l0[l], s));
        LevelPlan &pl = plan[l];
        pl.redone = false;
        pl.known_items = false;
        const bool first_build = (l == 1 && first_pass);
        pa.deg = e->deg.as<int>();
        pa.off = off_of(l);
        for (int c = 0; c < kNumClasses; c++) pa.items[c] = e->items[cs][c].as<int2>();
        pa.n = n;
        pa.L = l;
        pa.binom = e->binom.as<unsigned long long>();
        pa.chunk = chunk;
        // the small work item only where the one-wavefront kernel runs (sweep_vec.hip); the 256-thread kernels of the
        // same class (exact path, heterogeneous thresholds, levels >= kVecMaxLevel) want long runs of consecutive ranks
        const float th_l = level_threshold(l);
        const bool vec0 = (e->opt_fast != 0) && l >= 2 && l < kVecMaxLevel && th_l >= kThMinFilter && !m.het && e->opt_vec &&
                          !e->opt_validate && staged_classes > 0;
        // levels 2-4 of an LD block hold a few thousand sets per row at most: a smaller item (fewer sets per lane in
        // turn) shortens the serial tail of every item; from level 5 on the staging of an item has to be amortised
        const unsigned long long c0 = (l <= 4) ? (unsigned long long)std::max<long long>(e->opt_chunk0_low, 64) : chunk0;
        pl.chunk0 = vec0 ? c0 : chunk;
        // deep levels by unions T = S + Y: single threshold, symmetric matrix (the inverse-based form has no
        // meaning for the two orientations of an asymmetric input), filter certified for this threshold
        pl.tmaj = (e->opt_fast != 0) && !pl.force_exact && l >= std::max(2, e->opt_tmaj_min_level) && l <= kML &&
                  th_l >= kThMinFilter && (!m.het || (m.ness_checked && ness_symmetric)) && symmetric && !m.sharded;
        if (pl.tmaj) pl.chunk0 = chunk;
        pa.chunk0 = pl.chunk0;
        pa.Lsets = pl.tmaj ? l + 1 : l;
        pa.staged_classes = staged_classes;
        pa.pair_mode = ((l == 1) && !first_build && pl.use_pair && !pl.use_rows) ? 1 : 0;
        pa.cnt = dcnt + l;
        pa.prev = (l >= 2) ? dcnt + (l - 1) : nullptr;
        pa.prev_qcap = (l >= 2) ? qcap_gate[l - 1] : ~0ull;
        pa.item_cap = item_cap;
        pa.shard_rank = e->shard_rank;
        pa.shard_world = e->shard_world;
        pa.gate = e->hgate_dev + l;
        pa.seq = run_seq;
        pa.sym = (l == 1 && !e->opt_assume_symmetric && !m.batched) ? dsym : nullptr;
        pa.blocks = e->planblk.as<unsigned long long>();
        pa.blk_seq = ++e->plan_seq;
        if (first_build && e->binom_rows <= 0)
        {  // the plan reads C(d, 1) = d only at level 1, but wants a valid table pointer
            CUSK_HIP(e, e->binom.ensure(sizeof(unsigned long long) * kBinomStride));
            pa.binom = e->binom.as<unsigned long long>();
        }
        CUSK_HIP(e, launch_plan(pa, s));
        planned_last = l;
        return CUSK_OK;
    }

    // the run's one mandatory round trip, behind the first plan of level 1: sizes of the CSR arrays and of the binomial
    // table come from the level-1 degrees; then the kernel form of level 1
    int size_from_level1()
    {
        LevelPlan &pl = plan[1];
        hp_mark("plan1_enq");
        // (the record store of a previous run is cleared while the gate record travels: the clear needs no number
        // from the device unless the store has to grow)
        int *const rec_l_before = (a.mode == 0) ? e->rec_l.as<int>() : nullptr;
        const size_t rec_l_cleared = rec_l_before ? e->rec_l.cap : 0;
        if (rec_l_cleared) CUSK_HIP(e, hipMemsetAsync(rec_l_before, 0, rec_l_cleared, s));
        STEP(wait_gate(1));
        hp_mark("gate1");
        symmetric = (e->hgate[1].sym == 0) || (e->opt_assume_symmetric != 0) || m.batched;
        // (the symmetry kernel ran before the level-1 plan on this stream: its store has landed)
        ness_symmetric = (*reinterpret_cast<volatile int *>(e->hflag) == 0);
        const long long cap_edges = std::max<long long>(e->hgate[1].total_edges, 1);  // allocation bound for the CSR arrays (edges only shrink)
        maxdeg1 = e->hgate[1].maxdeg;
        for (int k = 0; k < 2; k++)
        {
            CUSK_HIP(e, e->nbr[k].ensure(sizeof(int) * ((size_t)cap_edges + 4)));  // + room: the row kernel's 8-byte requests
            if (a.mode == 0) CUSK_HIP(e, e->best[k].ensure(sizeof(unsigned long long) * (size_t)cap_edges));
        }
        CUSK_HIP(e, e->rv.ensure(sizeof(float) * ((size_t)cap_edges + 4)));
        CUSK_HIP(e, e->rpos.ensure(sizeof(int) * 4 * (size_t)cap_edges));
        CUSK_HIP(e, e->sel.ensure(sizeof(unsigned) * (size_t)cap_edges));
        if (a.mode == 0)
        {
            CUSK_HIP(e, e->rec_x.ensure(sizeof(int) * (size_t)cap_edges));
            CUSK_HIP(e, e->rec_y.ensure(sizeof(int) * (size_t)cap_edges));
            CUSK_HIP(e, e->rec_l.ensure(sizeof(int) * (size_t)cap_edges));
            CUSK_HIP(e, e->rec_s.ensure(sizeof(int) * kML * (size_t)cap_edges));
            e->rec_cap = (long long)(e->rec_l.cap / sizeof(int));
            if ((long long)(e->rec_s.cap / (sizeof(int) * kML)) < e->rec_cap) e->rec_cap = (long long)(e->rec_s.cap / (sizeof(int) * kML));
            e->rec_slots = cap_edges;
            if (e->rec_l.as<int>() != rec_l_before || rec_l_cleared < sizeof(int) * (size_t)cap_edges)
                CUSK_HIP(e, hipMemsetAsync(e->rec_l.p, 0, sizeof(int) * (size_t)cap_edges, s));  // no records yet
            CUSK_HIP(e, e->wpre.ensure(sizeof(int) * (size_t)n * words));
        }
        CUSK_HIP(e, e->queue.ensure(sizeof(RecheckEntry) * (size_t)e->opt_queue_cap));
        // binomial table C(a, b), a <= max degree: kept on the device across runs
        if ((long long)maxdeg1 >= e->binom_rows)
        {
            const int rows = std::max(maxdeg1 + 1, 1024);
            e->binom_host.assign((size_t)rows * kBinomStride, 0ull);
            for (int aa = 0; aa < rows; aa++)
                for (int b = 0; b < kBinomStride; b++)
                    e->binom_host[(size_t)aa * kBinomStride + b] = binom_sat(aa, b);
            CUSK_HIP(e, e->binom.ensure(e->binom_host.size() * sizeof(unsigned long long)));
            CUSK_HIP(e, hipMemcpyAsync(e->binom.p, e->binom_host.data(),
                                       e->binom_host.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
            e->binom_rows = rows;
        }
        // level 1 on a symmetric matrix with a single threshold: row-streaming kernel (or the pair kernel)
        pl.pair_lds = (size_t)maxdeg1 * 20 + 16;
        pl.use_pair = !m.het && symmetric && (e->opt_pair != 0) && pl.pair_lds <= 64 * 1024;
        pl.use_rows = !m.het && symmetric && (e->opt_pair != 0) && (e->opt_rows != 0);
        // per-pair sample sizes: the HET form of the row kernel, opt-in (option het_rows) and only on a bitwise symmetric
        // size matrix; "fast" = 0 keeps level 1 on the exact sweep as it keeps the deeper levels there
        if (m.ness_checked_rows && ness_symmetric && symmetric && (e->opt_fast != 0) && (e->opt_pair != 0) && (e->opt_rows != 0))
        {
            pl.use_rows = true;
            CUSK_HIP(e, e->nv.ensure(sizeof(float) * ((size_t)cap_edges + 4)));
        }
        if (pl.use_rows) CUSK_HIP(e, e->wpre.ensure(sizeof(int) * (size_t)n * words));
        if (pl.use_pair && !pl.use_rows)
        {  // the pair kernel counts its work items differently: plan again (option rows = 0 only)
            CUSK_HIP(e, hipMemsetAsync(dcnt + 1, 0, sizeof(LevelCounters), s));
            pa.pair_mode = 1;
            pa.binom = e->binom.as<unsigned long long>();
            e->hgate[1].seq = 0;
            pa.blk_seq = ++e->plan_seq;
            CUSK_HIP(e, launch_plan(pa, s));
        }
        first_pass = false;
        return CUSK_OK;
    }

    // 2. the neighbour lists, what the host knows of the level by now (class counts, a degree bound), the kernel arguments
    int fill_params(int l)
    {
        const int cs = l & 1;
        LevelPlan &pl = plan[l];
        if (m.sharded)
        {  // the exchange below is a collective: every engine must know now whether the level runs
            STEP(wait_gate(l));
            if ((closed = !e->hgate[l].active)) return CUSK_OK;
            for (int c = 0; c < kNumClasses; c++) pl.nitems[c] = e->hgate[l].class_items[c];
            pl.known_items = true;
        }
        pl.use_fast = (e->opt_fast != 0) && (l >= 2) && !pl.force_exact && !m.het0_exact;
        // (no host dependency)
        CUSK_HIP(e, launch_fill_nbr(e->adj.as<unsigned long long>(), off_of(l), e->nbr[cs].as<int>(),
                                    (a.mode == 0 && !pl.use_rows) ? e->best[cs].as<unsigned long long>() : nullptr, n, words,
                                    (l == 1 && (pl.use_rows || a.mode == 0)) ? e->wpre.as<int>() : nullptr, dcnt + l, a.row_range, s));
        // Level 2 is where the degrees collapse: the host looks at its gate record (it travels while the device compacts the lists)
        // for the class counts and a degree bound; the stale level-1 bound forked levels 2-4 over empty classes (~20 us each)
        if (l == 2 && !m.sharded && e->opt_sync2)
        {
            STEP(wait_gate(2));
            if ((closed = !e->hgate[2].active)) return CUSK_OK;
            for (int c = 0; c < kNumClasses; c++) pl.nitems[c] = e->hgate[2].class_items[c];
            pl.known_items = !e->hgate[2].item_overflow;
            maxdeg2 = e->hgate[2].maxdeg;
        }
        // degrees only shrink: the newest level whose counters have arrived bounds every later one
        pl.maxdeg_bound = maxdeg1;
        if (maxdeg2 >= 0 && l >= 2) pl.maxdeg_bound = std::min(pl.maxdeg_bound, maxdeg2);
        const int k = l - 1 - lookahead;
        if (k >= 1 && e->hgate[k].seq == run_seq && e->hgate[k].active) pl.maxdeg_bound = std::min(pl.maxdeg_bound, e->hgate[k].maxdeg);
        pl.staged_classes = staged_classes;

        // the level's kernel arguments; whether it goes through the filter and the recheck queue
        SweepParams &sp = pl.sp;
        sp.C = a.C;
        sp.Ness = a.Ness;
        sp.n = n;
        sp.level = l;
        sp.off = off_of(l);
        sp.nbr = e->nbr[cs].as<int>();
        sp.best = e->best[cs].as<unsigned long long>();
        sp.adj = e->adj.as<unsigned long long>();
        sp.deg = e->deg.as<int>();
        sp.words = words;
        sp.items = nullptr;
        sp.binom = e->binom.as<unsigned long long>();
        sp.time_index = e->ti.as<int>();
        sp.has_ti = (a.mode == 1 && a.time_index != nullptr) ? 1 : 0;
        sp.chunk = chunk;
        sp.cap = 0;
        sp.cls = 0;
        sp.item_cap = item_cap;
        sp.grid_cap = item_cap;
        sp.cnt = dcnt + l;
        sp.row_range = a.row_range;
        sp.max_span = m.batched ? a.max_span : n;
        sp.slots = dslots + (size_t)l * kCounterSlots * 4;
        sp.th = level_threshold(l);
        const double tq = std::tanh((double)sp.th);
        sp.t2 = (float)(tq * tq);
        // The guard band of the filter (ci_fast.h) is relative; the fp32 Fisher z of the exact path carries an
        // absolute error of ~1e-7.  Below this threshold the margin between the two gets thin, so such levels
        // (N beyond ~4 million samples at alpha 1e-4) run entirely on the exact arithmetic.
        pl.filter_ok = (sp.th >= kThMinFilter);
        if (!pl.filter_ok) pl.use_fast = false;
        sp.queue = pl.use_fast ? e->queue.as<RecheckEntry>() : nullptr;
        sp.qcap = pl.use_fast ? (unsigned long long)e->opt_queue_cap : 0;
        qcap_gate[l] = pl.use_fast ? sp.qcap : ~0ull;
        FinalizeParams &fp = pl.fp;
        fp.C = a.C;
        fp.n = n;
        fp.off = sp.off;
        fp.nbr = sp.nbr;
        fp.best = sp.best;
        fp.sel = pl.use_rows ? e->sel.as<unsigned>() : nullptr;
        fp.level = l;
        fp.adj = sp.adj;
        fp.deg = sp.deg;
        fp.words = words;
        fp.binom = sp.binom;
        fp.off1 = e->off1.as<int>();
        fp.wpre1 = e->wpre.as<int>();
        fp.adj0 = e->adj0.as<unsigned long long>();
        fp.rec_x = e->rec_x.as<int>();
        fp.rec_y = e->rec_y.as<int>();
        fp.rec_l = e->rec_l.as<int>();
        fp.rec_s = e->rec_s.as<int>();
        fp.rec_cap = e->rec_cap;
        fp.meta = pl.use_rows ? e->rpos.as<int4>() : nullptr;
        fp.cnt = dcnt + l;
        fp.slots = sp.slots;  // (fp.qcap: launch_finalize)
        fp.canon = dcanon + (size_t)l * kCounterSlots;
        return CUSK_OK;
    }

    // the level's sweeps and its finaliser; exact_only: once more on the exact path after a recheck-queue overflow
    // (everything the fast pass recorded is a certified verdict and stays valid)
    int enqueue_sweeps(int l, bool exact_only)
    {
        const bool timed = !exact_only && (e->opt_timing == 1 || e->opt_timing == 2);
        if (exact_only) mark_redone(l);
        if (timed) CUSK_HIP(e, hipEventRecord(e->ev_k0[l], s));
        STEP(launch_sweeps(l, exact_only));
        if (timed) CUSK_HIP(e, hipEventRecord(e->ev_k1[l], s));
        if (m.sharded && !exact_only) STEP(shard_join(l));
        STEP(launch_finalize(l));
        if (e->opt_timing == 2) CUSK_HIP(e, hipEventRecord(e->ev_l1[l], s));
        return CUSK_OK;
    }

    // read-back of the whole control block
    int read_back()
    {
        CUSK_HIP(e, hipEventRecord(e->ev_join, e->stream2));
        CUSK_HIP(e, hipStreamWaitEvent(s, e->ev_join, 0));
        // counters, slots and record bases in one copy (hcnt, hslots, hrec_base point into the pinned mirror)
        CUSK_HIP(e, hipMemcpyAsync(e->hcnt, ctl, kCtlSym, hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipEventRecord(e->ev_run[1], s));
        hp_mark("all_enq");
        CUSK_HIP(e, hipStreamSynchronize(s));
        hp_mark("synced");
        return CUSK_OK;
    }

    // did every enqueued level run to completion?  If not: what to take up again, and from which level (start, redo)
    int decide_after_read_back()
    {
        int ended = 0;  // first level whose gate stayed closed (a level whose plan ran but whose sweeps were not enqueued included)
        for (int l = 1; l <= planned_last && !ended; l++)
            if (!e->hcnt[l].active) ended = l;
        const int last_ran = ended ? ended - 1 : enq_last;
        const ReadBack rb = after_read_back(ended, last_ran, m.sharded, plan[last_ran].use_fast && !plan[last_ran].redone, plan[last_ran].tmaj,
                                            e->hcnt[last_ran].qcount > (unsigned long long)e->opt_queue_cap, e->hcnt[ended].overflow != 0,
                                            e->hcnt[ended].item_overflow != 0);
        long long need;
        switch (rb.what)
        {
        case AfterReadBack::Done:
            levels_swept = last_ran;
            if (ended) level_out = ended - 1;  // cuPC-S.cu:154-159
            done = true;
            return CUSK_OK;
        case AfterReadBack::BinomOverflow:
            return fail(e, CUSK_ERR_OVERFLOW,
                        "C(degree, level) exceeds 2^62 at level " + std::to_string(ended) + " (max degree " +
                            std::to_string(e->hcnt[ended].maxdeg) + ")");
        case AfterReadBack::ReplanTmaj:
            plan[rb.level].force_exact = true;
            local.exact_fallbacks++;
            start = rb.level;
            break;
        case AfterReadBack::RedoExact:
            redo = rb.level;
            start = rb.level + 1;
            break;
        case AfterReadBack::GrowItems:
            need = item_cap;
            for (int c = 0; c < kNumClasses; c++) need = std::max(need, e->hcnt[ended].class_items[c]);
            item_cap = need + need / 4;
            for (int k = 0; k < 2; k++)
                for (int c = 0; c < kNumClasses; c++) CUSK_HIP(e, e->items[k][c].ensure(sizeof(int2) * (size_t)item_cap));
            start = ended;
            break;
        }
        // resume: the counters of the levels that are enqueued again start from zero, their gate records are void
        for (int l = start; l < kLevels; l++) e->hgate[l].seq = 0;
        if (start <= 2) maxdeg2 = -1;
        if (start <= last_level)
        {
            CUSK_HIP(e, hipMemsetAsync(dcnt + start, 0, sizeof(LevelCounters) * (size_t)(kLevels - start), s));
            CUSK_HIP(e, hipMemsetAsync(dslots + (size_t)start * kCounterSlots * 4, 0,
                                       sizeof(unsigned long long) * (size_t)(kLevels - start) * kCounterSlots * 4, s));
            CUSK_HIP(e, hipMemsetAsync(dcanon + (size_t)start * kCounterSlots, 0,
                                       sizeof(unsigned long long) * (size_t)(kLevels - start) * kCounterSlots, s));
        }
        return CUSK_OK;
    }

    int collect_stats()
    {
        // degrees and edge counts at the start of every level that was planned (the one at which the loop ended included)
        for (int l = 1; l <= std::min(levels_swept + 1, last_level); l++)
        {
            local.max_degree[l] = e->hcnt[l].maxdeg;
            local.edges[l] = e->hcnt[l].total_edges;
        }
        local.levels_run += levels_swept;
        float ms = 0.0f;
        CUSK_HIP(e, hipEventElapsedTime(&ms, e->ev_l0[0], e->ev_l1[0]));
        local.kernel_ms[0] = local.level_ms[0] = ms;
        const bool timed = (e->opt_timing == 1 || e->opt_timing == 2);
        for (int l = 1; l <= levels_swept; l++)
        {
            for (int k = 0; k < kCounterSlots; k++)
            {
                const unsigned long long *sl = e->hslots + ((size_t)l * kCounterSlots + k) * 4;
                local.tests[l] += (long long)sl[0];
                local.subsets[l] += (long long)sl[1];
                local.removed[l] += (long long)sl[2];
                local.violations += (long long)sl[3];
                // (hetcor: counted at level 1 by level1_apply_kernel when no time index is given; 0 elsewhere)
                if (a.mode == 0 || l == 1) local.canonical_tests[l] += (long long)e->hcanon[(size_t)l * kCounterSlots + k];
            }
            local.rechecks[l] = (long long)e->hcnt[l].qcount;
            if (timed)
            {
                CUSK_HIP(e, hipEventElapsedTime(&ms, e->ev_k0[l], e->ev_k1[l]));
                local.kernel_ms[l] = local.main_kernel_ms[l] = ms;
            }
            if (l == 1 && rows_timed && (timed || e->opt_timing == 3))
            {  // (timing = 3: the events around the level-1 row kernel only)
                CUSK_HIP(e, hipEventElapsedTime(&ms, e->ev_main[0], e->ev_main[1]));
                local.main_kernel_ms[l] = ms;
            }
            if (!timed) continue;
            // level time: plan to finaliser with timing = 2; otherwise from the end of the previous level's sweep to the
            // end of this one's (the previous finaliser, this level's plan, lists and sweep)
            if (e->opt_timing == 2)
                CUSK_HIP(e, hipEventElapsedTime(&ms, e->ev_l0[l], e->ev_l1[l]));
            else
                CUSK_HIP(e, hipEventElapsedTime(&ms, l == 1 ? e->ev_l1[0] : e->ev_k1[l - 1], e->ev_k1[l]));
            local.level_ms[l] = ms;
        }
        CUSK_HIP(e, hipEventElapsedTime(&ms, e->ev_run[0], e->ev_run[1]));
        local.total_ms = ms;
        local.level = level_out;
        e->last_levels = levels_swept;
        e->level1_form = levels_swept >= 1 ? level1_form : -1;
        e->nrec = 0;  // the dense record list is produced on request (materialize_records)
        e->have_result = true;
        return CUSK_OK;
    }
};

}  // namespace

int run_levels(cusk_engine *e, const RunArgs &a, cusk_stats *st)
{
    if (a.n <= 0 || a.C == nullptr || a.Th == nullptr) return fail(e, CUSK_ERR_ARG, "bad arguments");
    LevelRun r{e, a};
    STEP(r.prepare());
    STEP(r.enqueue_level0());
    while (!r.done)
    {
        if (r.redo > 0) STEP(r.enqueue_sweeps(r.redo, true));
        r.redo = 0;
        r.enq_last = r.planned_last = r.start - 1;
        r.closed = false;
        for (int l = r.start; l <= r.last_level; l++)
        {
            STEP(r.enqueue_plan(l));
            if (r.closed) break;
            if (l == 1 && r.first_pass) STEP(r.size_from_level1());
            STEP(r.fill_params(l));
            if (r.closed) break;
            STEP(r.enqueue_sweeps(l, false));
            r.enq_last = l;
        }
        STEP(r.read_back());
        STEP(r.decide_after_read_back());
    }
    STEP(r.collect_stats());
    if (st) *st = r.local;
    r.hp_mark("done");
    if (e->opt_hostprof) std::fprintf(stderr, "[hostprof]%s\n", r.hp_log.c_str());
    return CUSK_OK;
}

}  // namespace cusk
