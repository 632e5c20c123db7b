// block_pipeline.h -- one LD block through the `cusk` pipeline, shared by the `mps cusk` command (one block per
// process, cli.cpp:432-678 of the reference) and by the multi-GPU block driver (many blocks per process:
// include/cusk_hip.h section 3, ci-gwas_amd/run_blocks.py).  Both callers run exactly this code, so the files of a
// sharded whole-chromosome run are byte-identical to those of per-block `mps cusk` invocations by construction.
//
// Host code against the C ABI only (no HIP headers): correlation build and both skeleton stages run on the engine's
// device, the matrix never leaves HBM between them, adjacency comes back as a bitmap, separating sets as sparse
// records, only the retained sub-matrix is gathered to the host.  run_cusk_block is the sequence of the steps below; the
// rules they apply live in prefilter.h, square_inputs.h and reduce.h.
#pragma once
#include <chrono>
#include <memory>

#include "geno_inputs.h"
#include "prefilter.h"
#include "reduce.h"
#include "square_inputs.h"

namespace host {

// what `mps cusk` loads before it turns to its block (cli.cpp:458-497); loaded once, shared by all blocks
struct CuskInputs
{
    std::string phen_path, bfiles, block_path;
    float alpha = 0.0f;
    int max_level = 0, max_level_two = 0, depth = 1;
    std::string full_corrmats_dir;  // not empty: also write <stem>.all_corrs there (cli.cpp:651-658)
    Phen phen;
    BedDims dims;
    BimInfo bim;
    std::vector<Block> blocks;
    float Th[ML + 1];
    // `mps cusk ... het`: every pair with a trait at the number of individuals it was observed on (run_cusk_block's het
    // branch); th_het = the alpha/2 quantile the per-test thresholds are formed from
    bool het = false;
    float th_het = 0.0f;
    // `mps cusk ... het filter`: the het runs set engine option het_filter (levels >= 2 through the filter and the
    // recheck queue instead of the exact path alone); same results
    bool het_filter = false;
    // `mps cusk ... het rows`: the het runs set engine option het_rows (level 1 on the row kernel at per-pair sample sizes
    // when the size matrix is symmetric); same results
    bool het_rows = false;
    // `mps cusk ... het markers`: a pair of markers is tested at the number of individuals both were observed on
    // (cusk_marker_pair_sizes over the marker x marker part of the size matrix) instead of N; results change
    bool het_markers = false;
    MappedFile bed;
    // all markers' means / stds, read once when several blocks are run from one process (empty: line-range reads)
    std::vector<float> means_all, stds_all;

    // cli.cpp:458-497 (path checks, .phen, .dim, .bim, .blocks with the bounds check, thresholds)
    void load(std::ostream *log)
    {
        if (log) *log << "Checking paths" << std::endl;
        check_prep_paths(bfiles);
        check_bed_magic(bfiles);
        check_path(phen_path);
        check_path(block_path);
        load_phen_dims(phen_path, bfiles, phen, dims);
        bim = read_bim(bfiles + ".bim");
        if (log) *log << "Found " << phen.num_phen << " phenotypes" << std::endl;
        if (log) *log << "Loading blocks" << std::endl;
        blocks = read_blocks(block_path);
        if (log) *log << "Found " << blocks.size() << " blocks" << std::endl;
        for (const Block &b : blocks)
            if (b.first >= bim.markers_on(b.chr) || b.last >= bim.markers_on(b.chr))
                die("block out of bounds with first_ix: " + std::to_string(b.first) + " last_ix: " + std::to_string(b.last));
        cusk_threshold_array((int)dims.num_samples, alpha, Th);
        th_het = cusk_hetcor_threshold(alpha);
        map_bed(bed, bfiles, dims, 0);
    }
    void load_all_marker_stats()
    {
        means_all = read_floats_line_range(bfiles + ".means", 0, std::numeric_limits<size_t>::max());
        stds_all = read_floats_line_range(bfiles + ".stds", 0, std::numeric_limits<size_t>::max());
    }
    size_t first_marker(const Block &b) const { return bim.start_of(b.chr) + b.first; }
};

struct BlockStats
{
    int skipped = 0;         // cli.cpp:572-576: no marginally significant marker-trait correlation, no output
    int num_sig = 0;
    long long markers = 0;   // block size
    long long retained = 0;  // markers in the written result
    long long tests[2] = {0, 0};  // CI tests of stage one / stage two (SURVEY.md 8d definition)
    cusk_stats stage[2];
    // wall-clock phases, ms: inputs (bed slice, means, stds), correlation build, stage one, prune + gather,
    // stage two, reduction
    double ms_inputs = 0, ms_corr = 0, ms_stage1 = 0, ms_prune = 0, ms_stage2 = 0, ms_reduce = 0;
    // het runs, both part of ms_corr: the count pass (cusk_pair_counts), and the size chain on the host + cusk_ess_square
    double ms_counts = 0, ms_ess = 0;
};

// per-caller device scratch that survives from block to block
struct BlockScratch
{
    DevMat C, C2;
    DevMat Ness, Ness2;  // het runs: the sample-size matrices of the block and of its stage-two set
    // the NEXT block's correlation matrix, being built on the engine's third stream while this block is swept
    // (cusk_corr_build_begin / _end): pending >= 0 = its block index, pending_m = its marker count
    DevMat Cnext;
    int pending = -1;
    size_t pending_m = 0;
    void swap_next()
    {
        std::swap(C.p, Cnext.p);
        std::swap(C.cap, Cnext.cap);
    }
};

// ms since the last call (or since construction)
struct Lap
{
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double operator()()
    {
        const auto now = std::chrono::steady_clock::now();
        const double v = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return v;
    }
};

// ---- the steps of run_cusk_block, in the order they run ----

// inputs: where the block's genotypes, the phenotypes and the block's means / stds are read from
struct BlockRows
{
    const unsigned char *bed = nullptr;
    const float *phen = nullptr, *means = nullptr, *stds = nullptr;
    std::vector<float> means_v, stds_v;  // line-range reads, when neither `staged` nor means_all holds them
};

inline void block_inputs(const CuskInputs &in, const Block &block, const StagedInputs *staged, BlockRows &r)
{
    const size_t m = block.size(), g0 = in.first_marker(block), g1 = g0 + m - 1;
    const size_t bpc = in.dims.bytes_per_col();
    if (3 + (g1 + 1) * bpc > in.bed.size) die("bed file is shorter than .dim / .bim say");
    r.bed = in.bed.data + 3 + g0 * bpc;  // io.cpp:238-249
    r.phen = in.phen.data.data();
    if (staged)
    {  // device-resident inputs: no per-block PCIe traffic
        r.bed = staged->bed + g0 * bpc;
        r.phen = staged->phen;
        r.means = staged->means + g0;
        r.stds = staged->stds + g0;
    }
    else if (!in.means_all.empty())
    {
        if (g1 >= in.means_all.size() || g1 >= in.stds_all.size()) die("block size and number of means or stds differ");
        r.means = in.means_all.data() + g0;
        r.stds = in.stds_all.data() + g0;
    }
    else
    {
        r.means_v = read_floats_line_range(in.bfiles + ".means", g0, g1);
        r.stds_v = read_floats_line_range(in.bfiles + ".stds", g0, g1);
        if (r.means_v.size() != m || r.stds_v.size() != m) die("block size and number of means or stds differ");
        r.means = r.means_v.data();
        r.stds = r.stds_v.data();
    }
}

// correlation build: the block's n x n matrix into scr.C and its marker x trait part to the host -- waited for when it was
// built ahead, beside the previous block's sweeps; built now otherwise
inline void block_correlations(cusk_engine *e, const CuskInputs &in, int block_index, const BlockRows &r, size_t m, BlockScratch &scr,
                               std::vector<float> &mxp)
{
    const size_t N = in.dims.num_samples, p = in.phen.num_phen, n = m + p;
    if (scr.pending == block_index && scr.pending_m == m)
    {
        scr.pending = -1;
        scr.swap_next();
        if (cusk_corr_build_end(e, mxp.data()) != CUSK_OK) engine_die("correlation build (end)", e);
        return;
    }
    if (scr.pending >= 0)
    {  // a build for another block is in flight (the caller changed its mind): let it finish, drop it
        scr.pending = -1;
        if (cusk_corr_build_end(e, nullptr) != CUSK_OK) engine_die("correlation build (end)", e);
    }
    scr.C.reserve(n * n);
    if (cusk_corr_build(e, r.bed, r.phen, m, N, p, r.means, r.stds, scr.C.p, mxp.data()) != CUSK_OK)
        engine_die("correlation build", e);
}

// build-ahead: the correlation build of blocks[next_index] is started now that this block's own matrix is complete, and
// runs beside this block's sweeps
inline void build_next_ahead(cusk_engine *e, const CuskInputs &in, const StagedInputs &staged, int next_index, BlockScratch &scr)
{
    const size_t N = in.dims.num_samples, p = in.phen.num_phen, bpc = in.dims.bytes_per_col();
    const Block &nb = in.blocks[next_index];
    const size_t m2 = nb.size(), h0 = in.first_marker(nb), n2 = m2 + p;
    if (m2 == 0 || 3 + (h0 + m2) * bpc > in.bed.size) return;
    scr.Cnext.reserve(n2 * n2);
    if (cusk_corr_build_begin(e, staged.bed + h0 * bpc, staged.phen, m2, N, p, staged.means + h0, staged.stds + h0, scr.Cnext.p) !=
        CUSK_OK)
        engine_die("correlation build (begin)", e);
    scr.pending = next_index;
    scr.pending_m = m2;
}

// sizes (het): complete-observation counts of every marker x trait and trait x trait pair of the block (resident inputs
// when staged; a correlation build started ahead runs on its own stream and buffers), the sizes `cuskss-merged --het` gives
// the same pairs, and their expansion to the n x n matrix scr.Ness on the device
inline void block_sizes(cusk_engine *e, const CuskInputs &in, const BlockRows &r, size_t m, const std::vector<float> &mxp,
                        BlockScratch &scr, std::vector<float> &mxp_ess, BlockStats &bs, Lap &lap)
{
    const size_t N = in.dims.num_samples, p = in.phen.num_phen, n = m + p;
    std::vector<float> pxp_ess;
    std::vector<int> mxp_n(m * p), pxp_n(p * p);
    if (cusk_pair_counts(e, r.bed, r.phen, nullptr, m, m, N, p, mxp_n.data(), pxp_n.data()) != CUSK_OK) engine_die("pair counts", e);
    bs.ms_counts = lap();
    std::vector<int> traits(p);
    std::iota(traits.begin(), traits.end(), (int)m);
    const std::vector<float> pxp = gather(e, scr.C.p, (int)n, traits);
    block_sample_sizes(mxp.data(), mxp_n.data(), pxp.data(), pxp_n.data(), m, p, mxp_ess, pxp_ess);
    scr.Ness.reserve(n * n);
    if (cusk_ess_square(e, mxp_ess.data(), pxp_ess.data(), m, p, (float)N, scr.Ness.p) != CUSK_OK) engine_die("sample-size matrix", e);
    // (het markers) the block's own rows once more: jointly observed individuals per pair of markers over the m x m corner
    if (in.het_markers && cusk_marker_pair_sizes(e, r.bed, nullptr, m, m, N, scr.Ness.p, n) != CUSK_OK)
        engine_die("marker pair sizes", e);
    bs.ms_ess = lap();
}

// prefilter, cli.cpp:561-576: how many marker-trait correlations are marginally significant (a block without any is skipped)
inline int block_prefilter(const CuskInputs &in, const std::vector<float> &mxp, const std::vector<float> &mxp_ess)
{
    return in.het ? count_significant_het(mxp.data(), mxp_ess.data(), mxp.size(), in.th_het)
                  : count_significant(mxp.data(), mxp.size(), in.Th[0]);
}

// stage one: Skeleton on the block's n variables
inline void stage_one(cusk_engine *e, const CuskInputs &in, int n, BlockScratch &scr, cusk_stats &st)
{
    cusk_engine_set_option(e, "assume_symmetric", 1);  // cusk_corr_build mirrors every element
    if (in.het)
    {
        if (in.het_filter) cusk_engine_set_option(e, "het_filter", 1);  // (stays set for stage two)
        if (in.het_rows) cusk_engine_set_option(e, "het_rows", 1);      // (likewise)
        if (cusk_run_skeleton_het(e, scr.C.p, scr.Ness.p, n, in.th_het, in.max_level, &st) != CUSK_OK) engine_die("Skeleton (het)", e);
    }
    else if (cusk_run_skeleton(e, scr.C.p, n, in.Th, in.max_level, &st) != CUSK_OK)
        engine_die("Skeleton", e);
}

// prune + gather: the variables stage two keeps (all traits, the markers within `depth` of one), and their sub-matrices
// gathered device to device into scr.C2 / scr.Ness2 (cli.cpp:62-87)
inline std::vector<int> prune_and_gather(cusk_engine *e, const CuskInputs &in, size_t m, BlockScratch &scr)
{
    const size_t p = in.phen.num_phen, n = m + p;
    std::vector<int> P;
    if (in.depth == 1 && p > 0)
    {  // only the trait rows travel (25 KB of the 12.6 MB bitmap of a 10k block)
        Bits T;
        T.n = (int)p;
        T.words = cusk_result_words(e);
        T.w.resize((size_t)T.n * T.words);
        if (cusk_result_adj_rows(e, (int)m, (int)p, T.w.data()) != CUSK_OK) engine_die("adjacency download", e);
        P = subset_variables_depth1(T, (int)n, (int)m);
    }
    else
    {
        Bits G = fetch_adjacency(e);
        P = subset_variables(G, (int)n, (int)m, in.depth);
    }
    const int k = (int)P.size();
    scr.C2.reserve((size_t)k * k);
    if (cusk_gather_submatrix_dev(e, scr.C.p, (int)n, P.data(), k, scr.C2.p) != CUSK_OK) engine_die("gather", e);
    if (in.het)
    {  // the sizes of the retained variables, by the same index list
        scr.Ness2.reserve((size_t)k * k);
        if (cusk_gather_submatrix_dev(e, scr.Ness.p, (int)n, P.data(), k, scr.Ness2.p) != CUSK_OK) engine_die("gather (sizes)", e);
    }
    return P;
}

// stage two: Skeleton again on the reduced set, starting from the complete graph
inline void stage_two(cusk_engine *e, const CuskInputs &in, int k, BlockScratch &scr, cusk_stats &st2)
{
    cusk_engine_set_option(e, "assume_symmetric", 0);
    if (in.het)
    {
        if (cusk_run_skeleton_het(e, scr.C2.p, scr.Ness2.p, k, in.th_het, in.max_level_two, &st2) != CUSK_OK)
            engine_die("Skeleton (het, stage two)", e);
    }
    else if (cusk_run_skeleton(e, scr.C2.p, k, in.Th, in.max_level_two, &st2) != CUSK_OK)
        engine_die("Skeleton (stage two)", e);
}

// reduction: the stage-two result in the numbering of the variables it retains; P = stage one's retained variables
inline void reduce_block(cusk_engine *e, const CuskInputs &in, const std::vector<int> &P, BlockScratch &scr, Reduced &out)
{
    const size_t p = in.phen.num_phen;
    const int k = (int)P.size();
    Bits G2 = fetch_adjacency(e);
    std::vector<int> P2 = subset_variables(G2, k, k - (int)p, in.depth);
    out = Reduced();
    out.num_var = P2.size();
    out.num_phen = p;
    out.max_level = ML;
    out.new_to_old = compose(P2, &P);
    out.G = gather_adj(G2, P2);
    out.C = gather(e, scr.C2.p, k, P2);
    // (the sets as a list; the 18 MB dense array only for callers that ask for it, the .sep file is streamed)
    out.sep_sparse = reduce_sepsets_sparse(e, P2, ML, &P, out.sep_recs);
    if (!out.sep_sparse) out.S = reduce_sepsets(e, P2, ML, &P);
}

// cli.cpp:521-677 for blocks[block_index] on the engine's device.  Returns false when the block is skipped.
// next_index >= 0 (block driver, device-resident inputs): the correlation build of that block is started as soon as this
// block's own matrix is complete and runs beside this block's sweeps; the call for block next_index then only waits for it.
inline bool run_cusk_block(cusk_engine *e, const CuskInputs &in, int block_index, BlockScratch &scr, Reduced &out,
                           std::string &stem, BlockStats &bs, std::ostream *log, const StagedInputs *staged = nullptr,
                           int next_index = -1)
{
    if (block_index < 0 || (size_t)block_index >= in.blocks.size()) die("block index out of range");
    if (cusk_engine_bind_thread(e) != CUSK_OK) engine_die("bind thread", e);  // the scratch matrices go to e's device
    const Block &block = in.blocks[block_index];
    stem = block.file_stem();
    const size_t m = block.size(), p = in.phen.num_phen, n = m + p;
    bs = BlockStats();
    bs.markers = (long long)m;
    Lap lap;
    if (log)
    {
        *log << "\nProcessing block " << block_index + 1 << " / " << in.blocks.size() << std::endl;
        *log << "Block size: " << m << std::endl;
        *log << "Loading bed data" << std::endl;
    }
    BlockRows rows;
    block_inputs(in, block, staged, rows);
    bs.ms_inputs = lap();

    if (log)
    {
        *log << "Checking for significant marker - phen correlations" << std::endl;
        *log << "Computing all correlations" << std::endl;
    }
    std::vector<float> mxp(m * p), mxp_ess;
    block_correlations(e, in, block_index, rows, m, scr, mxp);
    if (staged && p > 0 && next_index >= 0 && (size_t)next_index < in.blocks.size() && next_index != block_index)
        build_next_ahead(e, in, *staged, next_index, scr);
    bs.ms_corr = lap();
    if (in.het && p > 0)
    {
        block_sizes(e, in, rows, m, mxp, scr, mxp_ess, bs, lap);
        bs.ms_corr += bs.ms_counts + bs.ms_ess;
    }
    bs.num_sig = block_prefilter(in, mxp, mxp_ess);
    if (bs.num_sig > 0)
    {
        if (log) *log << "Found " << bs.num_sig << " marker - phen correlations. Proceeding." << std::endl;
    }
    else
    {
        if (log) *log << "No significant correlations found. Skipping block." << std::endl;
        bs.skipped = 1;
        return false;
    }
    if (!in.full_corrmats_dir.empty())
    {  // cli.cpp:27,651-658 (compile-time switch WRITE_FULL_CORRMATS in the reference)
        std::vector<float> full(n * n);
        if (cusk_dev_download(full.data(), scr.C.p, sizeof(float) * n * n) != CUSK_OK) engine_die("correlation matrix download", e);
        write_binary(make_path(in.full_corrmats_dir, stem, ".all_corrs"), full.data(), full.size());
    }

    if (log) *log << "Running cuPC" << std::endl;
    cusk_stats &st = bs.stage[0];
    stage_one(e, in, (int)n, scr, st);
    bs.ms_stage1 = lap();
    for (int l = 0; l < st.levels_run; l++)
    {
        bs.tests[0] += st.tests[l];
        if (log)
            *log << "level " << l << ": max degree " << st.max_degree[l] << ", " << st.tests[l] << " tests, "
                 << st.level_ms[l] * 1e-3 << " s" << std::endl;
    }
    const std::vector<int> P = prune_and_gather(e, in, m, scr);
    bs.ms_prune = lap();
    // (the stage-one separating sets of cli.cpp:673 are never read again: stage two recomputes them)

    if (log) *log << "Starting second cusk stage" << std::endl;
    cusk_stats &st2 = bs.stage[1];
    stage_two(e, in, (int)P.size(), scr, st2);
    bs.ms_stage2 = lap();
    for (int l = 0; l < st2.levels_run; l++) bs.tests[1] += st2.tests[l];
    reduce_block(e, in, P, scr, out);
    bs.retained = (long long)out.num_markers();
    if (log) *log << "Retained " << out.num_markers() << " markers" << std::endl;
    bs.ms_reduce = lap();
    return true;
}

}  // namespace host
