// batch_pipeline.h -- MANY LD blocks through the `cusk` pipeline in one set of device runs (include/cusk_hip.h section 3:
// cusk_blockset_run_batch).
//
// The reference runs one block per `mps cusk` process (/root/reference/cusk/src/cli.cpp:507-512, README.md:62); a
// 500-SNP block is a chain of launch-latency-bound kernels that leaves an MI355X idle.  Here the blocks a GPU owns go
// through cli.cpp:521-677 TOGETHER: their correlation matrices are built by one set of launches onto the diagonal of one
// allocation (cusk_corr_build_batch_*), stage one sweeps them in ONE level loop (cusk_run_skeleton_batch), the pruned
// sub-matrices are gathered by one launch onto the diagonal of a second allocation, stage two sweeps those in one level
// loop, and one read-out brings adjacency, separating sets and correlations back.  Per block the result is the one of
// run_cusk_block (block_pipeline.h) -- the files are byte-identical (tests/test_gpu_batch.py) -- because the blocks never
// interact: a row only meets columns of its own block.
//
// run_cusk_batch is the sequence of the steps below, named like those of run_cusk_block: layout -> correlations -> sizes
// (het) -> prefilter -> size matrix (het) -> stage one -> prune + gather -> stage two -> reduction (adjacency and
// correlations, then separating sets).  Their index arithmetic is batch_plan.h, which has no engine call in it.
#pragma once
#include <thread>
#include <cstdio>
#include <cstdlib>

#include "block_pipeline.h"

namespace host {

struct BatchScratch
{
    DevMat C, C2;
    DevMat Ness, Ness2;  // batches at per-pair sample sizes: the size matrices of both stages, laid out like C and C2
};

struct BatchStats
{
    int blocks = 0, skipped = 0;
    long long markers = 0, retained = 0;
    long long vars_stage1 = 0, vars_stage2 = 0;  // padded variable counts of the two batch allocations
    long long tests[2] = {0, 0}, canonical[2] = {0, 0};
    double ms_corr = 0, ms_stage1 = 0, ms_prune = 0, ms_stage2 = 0, ms_reduce = 0;
    cusk_stats stage[2];
};

struct BatchBlockOut
{
    int block_index = -1;
    bool skipped = false;
    int num_sig = 0;
    std::string stem;
    Reduced r;
};

// CUSK_BATCH_PROF=1: wall-clock marks of run_cusk_batch on stderr (microseconds since entry)
struct BatchProf
{
    std::chrono::steady_clock::time_point p0 = std::chrono::steady_clock::now();
    std::string log;
    void mark(const char *what)
    {
        static const bool on = std::getenv("CUSK_BATCH_PROF") != nullptr;
        if (!on) return;
        char buf[64];
        std::snprintf(buf, sizeof(buf), " %s=%.0f", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - p0).count());
        log += buf;
    }
};

// what more than one step needs.  Block b = blocks[b] of the caller; k = the k-th block that passed the prefilter.
struct BatchState
{
    size_t N = 0, p = 0, bpc = 0;
    bool het = false;
    std::vector<long long> first;  // layout: first marker, marker count and first stage-one variable of block b
    std::vector<int> m, base;
    size_t n1 = 0, msum = 0, n2 = 0;            // variables of the two batch allocations, markers of the batch
    std::vector<float> mxp, mxp_ess, pxp_ess;   // marker x trait correlations; het: their sizes, one p x p table per block
    std::vector<int> kept, lo1, hi1, lo2, hi2;  // kept[k] = b; block k = variables [lo, hi) of stage one / stage two
    std::vector<std::vector<int>> P1, P2;       // what block k retains after stage one (of its m + p) / two (of P1[k])
    std::vector<uint64_t> packed;
    BatchProf prof;
};

inline void gather_rows(cusk_engine *e, const float *M_dev, size_t n, const GatherTables &g, float *out, size_t out_count,
                        int out_on_device, const char *what)
{
    if (cusk_gather_rows(e, M_dev, (int)n, g.idx.data(), g.rows(), g.row_src.data(), g.row_k.data(), g.row_first.data(),
                         g.row_out.data(), g.rows(), out, (long long)out_count, out_on_device) != CUSK_OK)
        engine_die(what, e);
}

// one batched Skeleton run over the blocks [lo[k], hi[k]) on the diagonal of the n x n matrix C; het: at the sizes Ness
inline void batch_skeleton(cusk_engine *e, const CuskInputs &in, bool het, const float *C, const float *Ness, size_t n,
                           const std::vector<int> &lo, const std::vector<int> &hi, int max_level, cusk_stats &s, const char *what)
{
    if ((het ? cusk_run_skeleton_batch_het(e, C, Ness, (int)n, (int)lo.size(), lo.data(), hi.data(), in.th_het, max_level, &s)
             : cusk_run_skeleton_batch(e, C, (int)n, (int)lo.size(), lo.data(), hi.data(), in.Th, max_level, &s)) != CUSK_OK)
        engine_die(what, e);
}

inline void sum_tests(const cusk_stats &s, long long &tests, long long &canonical)
{
    for (int l = 0; l < s.levels_run; l++)
    {
        tests += s.tests[l];
        canonical += s.canonical_tests[l];
    }
}

// ---- the steps of run_cusk_batch, in the order they run ----

// layout: which markers each block has (checked against the .bed file) and where it lies in stage one -- block b =
// variables [base[b], base[b] + m_b + p), bases multiples of 64
inline void batch_layout(const CuskInputs &in, const std::vector<int> &blocks, std::vector<BatchBlockOut> &outs, BatchState &st)
{
    const size_t B = blocks.size();
    st.first.resize(B);
    st.m.resize(B);
    for (size_t b = 0; b < B; b++)
    {
        const int bi = blocks[b];
        if (bi < 0 || (size_t)bi >= in.blocks.size()) die("block index out of range");
        const Block &blk = in.blocks[(size_t)bi];
        outs[b].block_index = bi;
        outs[b].stem = blk.file_stem();
        const size_t g0 = in.first_marker(blk);
        if (3 + (g0 + blk.size()) * st.bpc > in.bed.size) die("bed file is shorter than .dim / .bim say");
        st.first[b] = (long long)g0;
        st.m[b] = (int)blk.size();
    }
    if (!plan_layout(st.m, st.p, st.base, st.n1, st.msum)) die("batch too large");
}

// correlations: marker x trait first (prefilter, cli.cpp:550-576), the rest for the blocks that pass -- the marker x
// marker part is enqueued for every block at once and runs while the host does the prefilter
inline void batch_correlations(cusk_engine *e, const StagedInputs &staged, BatchScratch &scr, BatchState &st)
{
    scr.C.reserve(st.n1 * st.n1);
    st.mxp.resize(st.msum * st.p);
    if (cusk_corr_build_batch(e, staged.bed, staged.phen, staged.means, staged.stds, st.N, st.p, (int)st.m.size(), st.first.data(),
                              st.m.data(), st.base.data(), (int)st.n1, scr.C.p, st.mxp.data()) != CUSK_OK)
        engine_die("correlation build", e);
    st.prof.mark("mxp");
}

// sizes (het): counts of complete observations in one pass over the batch's markers (sorted for the call, mapped back to
// the order of the batch; block by block when the batch names a block twice), then per block the chain of
// block_sample_sizes with the trait x trait correlations from the block's own diagonal block (the gather waits for the
// marker x marker part of the build, which writes them)
inline void batch_sizes(cusk_engine *e, const CuskInputs &in, const StagedInputs &staged, BatchScratch &scr, BatchState &st)
{
    const size_t B = st.m.size(), p = st.p, bed_rows = (in.bed.size - 3) / st.bpc;
    std::vector<int> mxp_n(st.msum * p), pxp_n(p * p), ix;
    std::vector<size_t> row0;
    if (plan_count_pass(st.first, st.m, ix, row0))
    {
        std::vector<int> sorted_n(st.msum * p);
        if (cusk_pair_counts(e, staged.bed, staged.phen, ix.data(), ix.size(), bed_rows, st.N, p, sorted_n.data(), pxp_n.data()) != CUSK_OK)
            engine_die("pair counts (batch)", e);
        for (size_t b = 0, o = 0; b < B; o += (size_t)st.m[b] * p, b++)
            std::copy_n(sorted_n.begin() + (long)(row0[b] * p), (size_t)st.m[b] * p, mxp_n.begin() + (long)o);
    }
    else
        for (size_t b = 0, o = 0; b < B; o += (size_t)st.m[b] * p, b++)
            if (cusk_pair_counts(e, staged.bed + (size_t)st.first[b] * st.bpc, staged.phen, nullptr, (size_t)st.m[b], (size_t)st.m[b], st.N, p,
                                 mxp_n.data() + o, pxp_n.data()) != CUSK_OK)
                engine_die("pair counts (batch)", e);
    st.prof.mark("counts");
    std::vector<int> trait0(B), traits(p);
    for (size_t b = 0; b < B; b++) trait0[b] = st.base[b] + st.m[b];
    std::iota(traits.begin(), traits.end(), 0);
    GatherTables g;
    plan_gather(trait0, std::vector<std::vector<int>>(B, traits), nullptr, 0, g);
    std::vector<float> pxp(g.cells), me, pe;
    gather_rows(e, scr.C.p, st.n1, g, pxp.data(), pxp.size(), 0, "gather (trait correlations, batch)");
    st.mxp_ess.resize(st.msum * p);
    st.pxp_ess.resize(B * p * p);
    for (size_t b = 0, o = 0; b < B; o += (size_t)st.m[b] * p, b++)
    {
        block_sample_sizes(st.mxp.data() + o, mxp_n.data() + o, pxp.data() + b * p * p, pxp_n.data(), (size_t)st.m[b], p, me, pe);
        std::copy(me.begin(), me.end(), st.mxp_ess.begin() + (long)o);
        std::copy(pe.begin(), pe.end(), st.pxp_ess.begin() + (long)(b * p * p));
    }
    st.prof.mark("sizes");
}

// prefilter, cli.cpp:561-576 per block: a block without a marginally significant marker-trait correlation is skipped
inline void batch_prefilter(const CuskInputs &in, BatchState &st, std::vector<BatchBlockOut> &outs, BatchStats &bs)
{
    for (size_t b = 0, o = 0; b < st.m.size(); b++)
    {
        const size_t cnt = (size_t)st.m[b] * st.p;
        const int num_sig = st.het ? count_significant_het(st.mxp.data() + o, st.mxp_ess.data() + o, cnt, in.th_het)
                                   : count_significant(st.mxp.data() + o, cnt, in.Th[0]);
        o += cnt;
        outs[b].num_sig = num_sig;
        outs[b].skipped = (num_sig == 0);
        if (num_sig > 0)
            st.kept.push_back((int)b);
        else
            bs.skipped++;
    }
    st.prof.mark("prefilter");
}

// size matrix (het): the kept blocks' sizes onto the diagonal of an allocation shaped like C; het markers: jointly observed
// individuals per pair of markers over every block's m x m corner
inline void batch_size_matrix(cusk_engine *e, const CuskInputs &in, const StagedInputs &staged, BatchScratch &scr, BatchState &st)
{
    const int K = (int)st.kept.size();
    std::vector<int> mk, rows;
    std::vector<float> me, pe;
    compact_sizes(st.kept, st.m, st.p, st.mxp_ess, st.pxp_ess, mk, me, pe);
    scr.Ness.reserve(st.n1 * st.n1);
    if (cusk_ess_square_batch(e, me.data(), pe.data(), K, mk.data(), st.lo1.data(), st.p, (float)st.N, (int)st.n1, scr.Ness.p) != CUSK_OK)
        engine_die("sample-size matrix (batch)", e);
    if (in.het_markers)
    {
        kept_marker_rows(st.kept, st.first, st.m, rows);
        if (cusk_marker_pair_sizes_batch(e, staged.bed, rows.data(), (in.bed.size - 3) / st.bpc, st.N, K, mk.data(), st.lo1.data(),
                                         (int)st.n1, scr.Ness.p) != CUSK_OK)
            engine_die("marker pair sizes (batch)", e);
    }
    st.prof.mark("ess_square");
}

// stage one: one level loop for every kept block.  Options as in stage_one of block_pipeline.h, but for assume_symmetric:
// a batched run never verifies the symmetry of its matrices (the engine ignores the option there), so none is set
inline void batch_stage_one(cusk_engine *e, const CuskInputs &in, BatchScratch &scr, BatchState &st, cusk_stats &s)
{
    if (st.het && in.het_filter) cusk_engine_set_option(e, "het_filter", 1);  // (stays set for stage two)
    if (st.het && in.het_rows) cusk_engine_set_option(e, "het_rows", 1);      // (likewise)
    batch_skeleton(e, in, st.het, scr.C.p, scr.Ness.p, st.n1, st.lo1, st.hi1, in.max_level, s, st.het ? "Skeleton (het, batch)" : "Skeleton (batch)");
    st.prof.mark("stage1");
}

// prune + gather: what stage two keeps of every block (parent_set.cpp:8-53 per block; depth 1 looks at the trait rows
// only, so only they travel), where the blocks lie in stage two (bases multiples of 64 again), and their sub-matrices
// gathered device to device onto the diagonal of scr.C2 / scr.Ness2 (cli.cpp:62-87)
inline void batch_prune_and_gather(cusk_engine *e, const CuskInputs &in, BatchScratch &scr, BatchState &st)
{
    const size_t K = st.kept.size();
    const int p = (int)st.p;
    const bool traits_only = (in.depth == 1 && p > 0);
    size_t words = 0, pos = 0;
    for (size_t k = 0; k < K; k++) words += bits_words(traits_only ? p : st.hi1[k] - st.lo1[k], st.hi1[k] - st.lo1[k]);
    st.packed.resize(words);
    if ((traits_only ? cusk_result_adj_bits_blocks_tail(e, p, st.packed.data()) : cusk_result_adj_bits_blocks(e, st.packed.data())) != CUSK_OK)
        engine_die("adjacency (batch)", e);
    st.prof.mark("bits1");
    st.P1.resize(K);
    st.lo2.resize(K);
    st.hi2.resize(K);
    for (size_t k = 0; k < K; k++)
    {
        const int nb = st.hi1[k] - st.lo1[k];
        st.P1[k] = traits_only ? subset_variables_depth1(slice_bits(st.packed, pos, p, nb), nb, nb - p)
                               : subset_variables(slice_bits(st.packed, pos, nb, nb), nb, nb - p, in.depth);
        st.lo2[k] = (int)st.n2;
        st.hi2[k] = (int)(st.n2 + st.P1[k].size());
        st.n2 += (size_t)pad64(st.P1[k].size());
    }
    st.prof.mark("bfs1");
    GatherTables g;
    plan_gather(st.lo1, st.P1, &st.lo2, st.n2, g);
    scr.C2.reserve(st.n2 * st.n2);
    gather_rows(e, scr.C.p, st.n1, g, scr.C2.p, 0, 1, "gather (batch)");
    if (st.het)
    {  // the sizes of the retained variables, by the very index tables
        scr.Ness2.reserve(st.n2 * st.n2);
        gather_rows(e, scr.Ness.p, st.n1, g, scr.Ness2.p, 0, 1, "gather (sizes, batch)");
    }
    st.prof.mark("gather2");
}

// stage two: Skeleton again on every reduced set, each from its complete graph (stage_two of block_pipeline.h, again
// without assume_symmetric)
inline void batch_stage_two(cusk_engine *e, const CuskInputs &in, BatchScratch &scr, BatchState &st, cusk_stats &s)
{
    batch_skeleton(e, in, st.het, scr.C2.p, scr.Ness2.p, st.n2, st.lo2, st.hi2, in.max_level_two, s,
                   st.het ? "Skeleton (het, stage two, batch)" : "Skeleton (stage two, batch)");
    st.prof.mark("stage2");
}

// reduction (parent_set.cpp:84-175 per block), first part: the variables every block retains after stage two, their
// adjacency, and their correlations by one gather of dense cells
inline void batch_reduce(cusk_engine *e, const CuskInputs &in, BatchScratch &scr, BatchState &st, std::vector<BatchBlockOut> &outs,
                         BatchStats &bs)
{
    const size_t K = st.kept.size();
    size_t words = 0, pos = 0, cell = 0;
    for (size_t k = 0; k < K; k++) words += bits_words(st.hi2[k] - st.lo2[k], st.hi2[k] - st.lo2[k]);
    st.packed.resize(words);
    if (cusk_result_adj_bits_blocks(e, st.packed.data()) != CUSK_OK) engine_die("adjacency (stage two, batch)", e);
    st.prof.mark("bits2");
    st.P2.resize(K);
    for (size_t k = 0; k < K; k++)
    {
        const int kb = st.hi2[k] - st.lo2[k];
        const Bits G2 = slice_bits(st.packed, pos, kb, kb);
        st.P2[k] = subset_variables(G2, kb, kb - (int)st.p, in.depth);
        Reduced &out = outs[(size_t)st.kept[k]].r;
        out.num_var = st.P2[k].size();
        out.num_phen = st.p;
        out.max_level = ML;
        out.sep_sparse = true;  // (batch_reduce_sepsets fills the list)
        out.new_to_old = compose(st.P2[k], &st.P1[k]);
        out.G = gather_adj(G2, st.P2[k]);
        bs.retained += (long long)out.num_markers();
    }
    GatherTables g;
    plan_gather(st.lo2, st.P2, nullptr, 0, g);
    std::vector<float> corr(g.cells);
    gather_rows(e, scr.C2.p, st.n2, g, corr.data(), corr.size(), 0, "gather (results, batch)");
    for (size_t k = 0; k < K; k++)
    {
        const size_t kk = st.P2[k].size();
        outs[(size_t)st.kept[k]].r.C.assign(corr.begin() + (long)cell, corr.begin() + (long)(cell + kk * kk));
        cell += kk * kk;
    }
    st.prof.mark("adj_corr");
}

// reduction, second part: the sparse separating-set records of the stage-two run split by block and remapped as
// reduce_sepsets does, stage-two quirk included (remap_batch_records).  The sets stay a sorted list per block (Reduced::
// sep_recs, empty so far); the dense k x k x 14 arrays are only built for a caller that asks for them
inline void batch_reduce_sepsets(cusk_engine *e, BatchState &st, std::vector<BatchBlockOut> &outs)
{
    const int *x = nullptr, *y = nullptr, *rs = nullptr;  // engine-owned pinned memory
    const long long cnt = cusk_result_sepsets_view(e, &x, &y, &rs);
    if (cnt < 0) engine_die("sepsets (batch)", e);
    if (!remap_batch_records(cnt, x, y, rs, st.lo2, st.hi2, st.P1, st.P2,
                             [&](size_t k, const SepRec &q) { outs[(size_t)st.kept[k]].r.sep_recs.push_back(q); }))
        die("separating-set record outside every block");
    for (int b : st.kept) sort_sep_recs(outs[(size_t)b].r);
    st.prof.mark("sepsets");
}

// cli.cpp:521-677 for every block of `blocks` on the engine's device.  outs[i] belongs to blocks[i].
// het: every block as run_cusk_block runs it on a set at per-pair sample sizes (`mps cusk ... het`) -- counts of complete
// observations for the batch's markers in one pass, the sizes of every block through block_sample_sizes, the het
// prefilter, both stages through cusk_run_skeleton_batch_het with the sizes on the diagonal of a second allocation.
inline void run_cusk_batch(cusk_engine *e, const CuskInputs &in, const StagedInputs &staged, const std::vector<int> &blocks,
                           BatchScratch &scr, std::vector<BatchBlockOut> &outs, BatchStats &bs, bool het = false)
{
    bs = BatchStats();
    BatchState st;
    outs.assign(blocks.size(), BatchBlockOut());
    if (blocks.empty()) return;
    if (cusk_engine_bind_thread(e) != CUSK_OK) engine_die("bind thread", e);
    st.N = in.dims.num_samples;
    st.p = in.phen.num_phen;
    st.bpc = in.dims.bytes_per_col();
    st.het = het && st.p > 0;  // (without traits there is no pair with a size of its own; run_cusk_block takes the plain branch too)
    Lap lap;

    batch_layout(in, blocks, outs, st);
    bs.blocks = (int)blocks.size();
    bs.markers = (long long)st.msum;
    bs.vars_stage1 = (long long)st.n1;
    batch_correlations(e, staged, scr, st);
    if (st.het) batch_sizes(e, in, staged, scr, st);
    batch_prefilter(in, st, outs, bs);
    if (st.kept.empty())
    {
        // the marker x marker part of the build is still enqueued and reads the engine's pinned table staging, which the
        // next batch overwrites: nothing may be in flight when this returns
        float one;
        if (cusk_engine_download(e, &one, scr.C.p, sizeof(one)) != CUSK_OK) engine_die("correlation build (batch)", e);
        bs.ms_corr = lap();
        return;
    }
    st.prof.mark("mxm_enq");
    bs.ms_corr = lap();

    plan_kept(st.kept, st.m, st.base, st.p, st.lo1, st.hi1);
    if (st.het)
    {
        batch_size_matrix(e, in, staged, scr, st);
        bs.ms_corr += lap();
    }
    batch_stage_one(e, in, scr, st, bs.stage[0]);
    sum_tests(bs.stage[0], bs.tests[0], bs.canonical[0]);
    bs.ms_stage1 = lap();

    batch_prune_and_gather(e, in, scr, st);
    bs.vars_stage2 = (long long)st.n2;
    bs.ms_prune = lap();

    batch_stage_two(e, in, scr, st, bs.stage[1]);
    sum_tests(bs.stage[1], bs.tests[1], bs.canonical[1]);
    bs.ms_stage2 = lap();

    batch_reduce(e, in, scr, st, outs, bs);
    batch_reduce_sepsets(e, st, outs);
    bs.ms_reduce = lap();
    if (!st.prof.log.empty()) std::fprintf(stderr, "[batchprof]%s\n", st.prof.log.c_str());
}

}  // namespace host
