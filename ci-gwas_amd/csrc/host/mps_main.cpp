// mps_main.cpp -- `mps`-compatible host program for the cusk path on MI355X.
//
// Same positional argv contracts, stdout milestones, exit codes and output files as the
// reference's native CLI (/root/reference/cusk/apps/mps.cpp:17-121, src/cli.cpp:194-346,
// :432-678), so that ci-gwas.py (or this repo's cli shim) can call it unchanged:
//   mps cusk   <.phen> <bfiles> <.blocks> <alpha> <max-level> <max-level-two> <depth> <outdir> <block-index> [het] [filter] [rows] [markers]
//   mps cuskss <mxm> <mxp> <mxp_se> <pxp> <pxp_se> <time_index> <block_index> <blockfile>
//              <marker_indices> <alpha> <l1> <l2> <depth> <num_samples> <outdir>   ("NULL" = absent)
// and two commands the reference does not have, for users who hold the genotypes (see SUMSTATS_USAGE):
//   mps sumstats   <.phen> <bfiles> <marker-indices|NULL> <outdir> [se] [ordinal=<1-based,...>]
//   mps cuskss-bed <.phen> <bfiles> <marker-indices> <time_index|NULL> <alpha> <l1> <l2> <depth> <outdir> [het] [markers] [ordinal=<1-based,...>]
//   mps prune      <bfiles> <out-stem> <r-max> <window>   (see PRUNE_USAGE)
// Differences by design: the correlation matrix never leaves HBM between the build and the
// sweep, adjacency comes back as a bitmap, separating sets as sparse records, only the
// retained sub-matrix is gathered to the host, and files are written with one fwrite each.
// `mps prep` / `mps block` are outside this build's scope and say so.
#include <chrono>
#include <algorithm>
#include <cstring>
#include <filesystem>
#include <memory>
#include <numeric>
#include <set>

#include "../../../include/cusk_hip.h"
#include "block_pipeline.h"
#include "host_io.h"
#include "ordinal_host.h"

using namespace host;

namespace {

// ---------------------------------------------------------------------------------------
// mps cusk   (cli.cpp:432-678)
// ---------------------------------------------------------------------------------------
const char *CUSK_USAGE = R"(
Run the skeleton search on a single block of a block diagonal genomic covariance matrix.

usage: mps cusk <.phen> <bfiles> <.blocks> <alpha> <max-level> <max-level-two> <depth> <outdir> <block-index> [het] [filter] [rows] [markers]

arguments:
    het             test every marker-trait and trait-trait pair at the number of individuals it was observed on (.phen
                    with NA entries): prefilter, both skeleton stages and the separating sets of the block; the sizes are
                    those `cuskss-bed ... het` uses for the same pairs.  Same five output files.
    filter          (after het) levels >= 2 of both stages through the filter and the recheck queue instead of the exact
                    path alone (engine option het_filter).  Same five output files.
    rows            (after het, before or after filter) level 1 of both stages on the row-streaming kernel at per-pair
                    sample sizes (engine option het_rows).  Same five output files.
    markers         (after het, in any order with filter and rows) test every pair of markers at the number of individuals
                    both were genotyped on (.bed code 01 = missing) instead of all of them.  The files change where
                    markers have missing calls.
)";

// wall-clock phase marks, printed as "[t] <phase>: <ms> ms" when CUSK_TIMING is set (tools/e2e_block.py)
struct PhaseTimer
{
    bool on = std::getenv("CUSK_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::cout << "[t] " << what << ": " << std::chrono::duration<double, std::milli>(now - last).count() << " ms (at "
                  << std::chrono::duration<double, std::milli>(now - t0).count() << ")" << std::endl;
        last = now;
    }
};

int cmd_cusk(int argc, char **argv)
{
    CuskInputs in;
    std::string outdir;
    int block_index = 0;
    if (!parse_cusk_args(argc, argv, in, outdir, block_index))
    {
        std::cout << CUSK_USAGE << std::endl;
        std::exit(1);
    }
    std::cout << "Got args: \n.phen: " << in.phen_path << "\nbfiles: " << in.bfiles << "\n.blocks: " << in.block_path
              << "\nalpha: " << in.alpha << "\nmax_level: " << in.max_level << "\nmax_level_two: " << in.max_level_two
              << "\ndepth: " << in.depth << "\noutdir: " << outdir << "\nblock-index: " << block_index << std::endl;
    if (in.het) std::cout << "het: per-pair sample sizes" << (in.het_filter ? ", levels >= 2 through the filter" : "")
                          << (in.het_rows ? ", level 1 on the row kernel" : "") << (in.het_markers ? ", marker pairs at their own counts" : "")
                          << std::endl;

    PhaseTimer tm;
    check_path(outdir);
    in.load(&std::cout);  // cli.cpp:458-497
    tm.mark("load phen, dim, bim, blocks; map bed");
    if (block_index < 0 || (size_t)block_index >= in.blocks.size()) die("block index out of range");
    std::cout << "Number of levels: " << in.max_level << std::endl;
    std::cout << "Setting level thr for cuPC: " << std::endl;
    for (int i = 0; i <= std::min(in.max_level, ML); ++i) std::cout << "\t Level: " << i << " thr: " << in.Th[i] << std::endl;
    if (in.het) std::cout << "het: every test at quantile " << in.th_het << " / sqrt(mean pair size - level - 3) instead" << std::endl;
    if (std::getenv("CUSK_WRITE_FULL_CORRMATS")) in.full_corrmats_dir = outdir;

    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    tm.mark("engine create");
    // the one block of this invocation through the pipeline the block driver runs for every block of a chromosome
    BlockScratch scratch;
    Reduced out;
    std::string stem;
    BlockStats bs;
    const bool kept = run_cusk_block(e, in, block_index, scratch, out, stem, bs, &std::cout);
    // (a level 1 that ran on the row kernel forms no conditioning sets: subsets[1] = 0 beside tests[1] > 0)
    if (in.het_rows)
        for (int k = 0; k < 2; k++)
            std::cout << "het rows: stage " << (k + 1) << " level 1 " << (bs.stage[k].tests[1] > 0 && bs.stage[k].subsets[1] == 0 ? "on the row kernel" : "not on the row kernel")
                      << ", " << bs.stage[k].rechecks[1] << " of " << bs.stage[k].tests[1] << " tests sent to the exact form" << std::endl;
    if (tm.on)
    {
        std::cout << "[t] inputs (bed slice, means, stds): " << bs.ms_inputs << " ms\n[t] correlation build (H2D + kernels + mxp D2H): "
                  << bs.ms_corr << " ms" << std::endl;
        if (in.het)
            std::cout << "[t] of which pair counts: " << bs.ms_counts << " ms\n[t] of which size chain + sample-size matrix: " << bs.ms_ess
                      << " ms" << std::endl;
        if (kept)
        {
            std::cout << "[t] skeleton stage one: " << bs.ms_stage1 << " ms\n[t] adjacency fetch + prune + sub-matrix gather: "
                      << bs.ms_prune << " ms\n[t] skeleton stage two: " << bs.ms_stage2 << " ms\n[t] stage-two reduction: "
                      << bs.ms_reduce << " ms" << std::endl;
            const cusk_stats &st = bs.stage[1];
            for (int l = 0; l < st.levels_run; l++)
                std::cout << "[t] stage two level " << l << ": max degree " << st.max_degree[l] << ", " << st.edges[l]
                          << " edges, " << st.tests[l] << " tests, " << st.subsets[l] << " sets, " << st.rechecks[l]
                          << " rechecks, sweep " << st.kernel_ms[l] << " ms, level " << st.level_ms[l] << " ms" << std::endl;
            std::cout << "[t] filter contradictions (option validate): stage one " << bs.stage[0].violations << ", stage two "
                      << st.violations << "; exact fallbacks " << bs.stage[0].exact_fallbacks << " / " << st.exact_fallbacks << std::endl;
        }
        tm.mark("block pipeline");
    }
    if (kept)
    {
        write_reduced(out, make_path(outdir, stem, ""), true);
        tm.mark("write outputs");
    }
    cusk_engine_destroy(e);
    tm.mark("engine destroy");
    return 0;
}

// ---------------------------------------------------------------------------------------
// mps cuskss   (mps.cpp:31-101, cli.cpp:29-60, :89-173, :194-346)
// ---------------------------------------------------------------------------------------
struct GC
{
    size_t num_var = 0, num_phen = 0;
    std::vector<int> new_to_old;
    std::vector<int> G;      // empty = complete graph
    std::vector<float> C;    // num_var^2
    std::vector<float> ess;  // num_var^2 when heterogeneous, else empty
    size_t num_markers() const { return num_var - num_phen; }
};

// run_cusk, cli.cpp:29-60: hetcor_skeleton, prune to depth, extract the retained sub-matrices.  C_resident: the
// num_var^2 matrix where a correlation build left it in HBM (gc.C is empty then); otherwise gc.C is uploaded.
GC run_cusk(cusk_engine *e, const GC &gc, float th, float ess_uniform, bool het, int depth, int max_level,
            const std::vector<int> &time_index_traits, const float *C_resident = nullptr)
{
    const int n = (int)gc.num_var;
    std::vector<int> ti(n, 0);
    for (size_t i = gc.num_markers(), r = 0; i < gc.num_var; i++, r++) ti[i] = time_index_traits[r];
    std::unique_ptr<DevMat> uploaded;
    if (!C_resident) uploaded.reset(new DevMat(gc.C));
    const float *Cd = C_resident ? C_resident : uploaded->p;
    std::unique_ptr<DevMat> Nd;
    if (het) Nd.reset(new DevMat(gc.ess));
    int *Gd = nullptr;
    if (!gc.G.empty())
    {
        Gd = static_cast<int *>(cusk_dev_alloc(sizeof(int) * gc.G.size()));
        if (!Gd || cusk_dev_upload(Gd, gc.G.data(), sizeof(int) * gc.G.size()) != CUSK_OK) engine_die("upload G", e);
    }
    cusk_stats st;
    if (cusk_run_hetcor(e, Cd, het ? Nd->p : nullptr, ess_uniform, Gd, n, th, max_level, ti.data(), &st) != CUSK_OK)
        engine_die("hetcor_skeleton", e);
    cusk_dev_free(Gd);
    Bits G = fetch_adjacency(e);
    std::vector<int> P = subset_variables(G, n, (int)gc.num_markers(), depth);
    GC out;
    out.num_var = P.size();
    out.num_phen = gc.num_phen;
    out.new_to_old = compose(P, &gc.new_to_old);
    out.G = gather_adj(G, P);
    out.C = gather(e, Cd, n, P);
    if (het) out.ess = gather(e, Nd->p, n, P);
    return out;
}

void write_gc(const GC &gc, const std::string &base)
{
    Reduced r;
    r.num_var = gc.num_var;
    r.num_phen = gc.num_phen;
    r.max_level = ML;  // cli.cpp:58 passes ML
    r.new_to_old = gc.new_to_old;
    r.G = gc.G;
    r.C = gc.C;
    write_reduced(r, base, false);
    // heterogeneous runs: the sample sizes of the retained variables beside .corr, same order (float32, num_var^2), for
    // sepselect --het
    if (!gc.ess.empty()) write_binary(base + ".ess", gc.ess.data(), gc.ess.size());
}

int cmd_cuskss(int argc, char **argv)
{
    if (argc < 17) die("usage: mps cuskss <mxm> <mxp> <mxp_se> <pxp> <pxp_se> <time_index> <block_index> <blockfile> "
                       "<marker_indices> <alpha> <max_level_one> <max_level_two> <depth> <num_samples> <outdir>");
    const std::string mxm_path = argv[2], mxp_path = argv[3], mxp_se_path = argv[4], pxp_path = argv[5],
                      pxp_se_path = argv[6], time_index_path = argv[7];
    const int block_index = std::stoi(argv[8]);
    const std::string blockfile_path = argv[9], marker_index_path = argv[10];
    const float alpha = std::stof(argv[11]);
    const int max_level_one = std::stoi(argv[12]), max_level_two = std::stoi(argv[13]), depth = std::stoi(argv[14]);
    const float num_samples = (float)std::stoi(argv[15]);
    const std::string outdir = argv[16];
    const bool merged = marker_index_path != "NULL", hetcor = mxp_se_path != "NULL", trait_only = mxm_path == "NULL",
               two_stage = max_level_two > 0, time_indexed = time_index_path != "NULL";
    check_path(pxp_path);
    check_path(outdir);
    if (merged)
        check_path(marker_index_path);
    else
        check_path(blockfile_path);
    if (hetcor || merged || !trait_only)
    {
        check_path(mxm_path);
        check_path(mxp_path);
    }
    if (hetcor)
    {
        check_path(mxp_se_path);
        check_path(pxp_se_path);
    }
    if (time_indexed) check_path(time_index_path);

    std::cout << "Loading input files" << std::endl;
    Block block;
    std::vector<size_t> rows;
    if (merged)
    {
        std::cout << "Loading marker indices" << std::endl;
        for (int v : read_binary<int>(marker_index_path)) rows.push_back((size_t)v);
    }
    else
    {
        std::cout << "Loading block file" << std::endl;
        const std::vector<Block> blocks = read_blocks(blockfile_path);
        if (block_index < 0 || (size_t)block_index >= blocks.size()) die("block index out of range");
        block = blocks[block_index];
        for (size_t r = block.first_global(); r <= block.last_global(); r++) rows.push_back(r);
    }
    std::cout << "Loading pxp" << std::endl;
    const Pxp pxp = load_pxp(pxp_path, hetcor ? pxp_se_path : std::string(), num_samples);
    const size_t p = pxp.num_phen;
    std::vector<int> time_index_traits(p, 1);
    if (time_indexed)
    {
        std::cout << "Loading time_indices" << std::endl;
        time_index_traits = read_ints_lines(time_index_path);
        if (time_index_traits.size() < p) die("time index file has fewer lines than traits");
    }
    const float th = cusk_hetcor_threshold(alpha);
    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);

    GC gc;
    gc.num_phen = p;
    if (trait_only)
    {  // cli.cpp:225-256
        gc.num_var = p;
        gc.C = pxp.corr;
        if (hetcor) gc.ess = pxp.ess;
        gc.new_to_old.resize(p);
        std::iota(gc.new_to_old.begin(), gc.new_to_old.end(), 0);
        std::cout << "Starting first cusk stage" << std::endl;
        gc = run_cusk(e, gc, th, num_samples, hetcor, depth, max_level_one, time_index_traits);
        write_gc(gc, make_path(outdir, "trait_only", ""));
        std::cout << "Retained " << gc.num_markers() << " markers" << std::endl;
        cusk_engine_destroy(e);
        return 0;
    }
    std::cout << "Loading mxm" << std::endl;
    const size_t m = mxm_num_markers(mxm_path);
    std::cout << "Loading mxp summary stats" << std::endl;
    const Mxp mxp = load_mxp(mxp_path, hetcor ? mxp_se_path : std::string(), rows);
    if (pxp.num_phen != mxp.num_phen) die("Numbers of traits seem to differ between pxp and mxp");
    if (m != mxp.num_markers)
        die("Numbers of markers seem to differ between mxm and mxp\nmxp: " + std::to_string(mxp.num_markers) + " x " +
            std::to_string(mxp.num_phen) + "\nmxm: " + std::to_string(m) + " x " + std::to_string(m));
    std::cout << "Merging correlations into single matrix" << std::endl;
    // make_square_cuskss_inputs, cli.cpp:89-173: markers first, then traits
    const size_t n = m + p;
    gc.num_var = n;
    gc.C.assign(n * n, 1.0f);
    load_mxm_into(mxm_path, m, gc.C.data(), n);
    if (hetcor) gc.ess.assign(n * n, num_samples);
    for (size_t i = 0; i < m; i++)
        for (size_t k = 0; k < p; k++)
        {
            gc.C[i * n + m + k] = gc.C[(m + k) * n + i] = mxp.corr[i * p + k];
            if (hetcor) gc.ess[i * n + m + k] = gc.ess[(m + k) * n + i] = mxp.ess[i * p + k];
        }
    for (size_t a = 0; a < p; a++)
        for (size_t b = 0; b < p; b++)
        {
            gc.C[(m + a) * n + m + b] = pxp.corr[a * p + b];
            if (hetcor) gc.ess[(m + a) * n + m + b] = pxp.ess[a * p + b];
        }
    gc.new_to_old.resize(n);
    std::iota(gc.new_to_old.begin(), gc.new_to_old.end(), 0);
    std::cout << "Starting first cusk stage" << std::endl;
    gc = run_cusk(e, gc, th, num_samples, hetcor, depth, max_level_one, time_index_traits);
    if (two_stage)
    {
        std::cout << "Starting second cusk stage" << std::endl;
        gc = run_cusk(e, gc, th, num_samples, hetcor, depth, max_level_two, time_index_traits);
    }
    std::cout << "Retained " << gc.num_markers() << " markers" << std::endl;
    write_gc(gc, make_path(outdir, merged ? "cuskss_merged" : block.file_stem(), ""));
    cusk_engine_destroy(e);
    return 0;
}

// ---------------------------------------------------------------------------------------
// mps sumstats / mps cuskss-bed: the inputs of `cuskss` on the merged marker set, from genotypes.  The reference has
// no such command: its cuskss reads mxm / mxp / pxp files (cli.cpp:194-346) and leaves making them to the user.
// ---------------------------------------------------------------------------------------
const char *SUMSTATS_USAGE = R"(
Compute the summary statistics cuskss reads (mxm, mxp, pxp) from genotypes and phenotypes.

usage: mps sumstats <.phen> <bfiles> <marker-indices|NULL> <outdir> [se] [ordinal=<1-based,...>]

arguments:
    .phen           path to standardized phenotype tsv
    bfiles          stem of .bed, .bim, .fam fileset (with the .dim, .means, .stds of mps prep)
    marker-indices  ascending global marker indices (int32 binary, merged_blocks.ixs) whose LD goes to mxm; NULL = all
    outdir          receives mxm.bin, mxp.txt (all markers), pxp.txt
    se              also write mxp_se.txt and pxp_se.txt: standard errors from the number of individuals each pair was
                    observed on (.phen with NA), for cuskss --mxp-se / --pxp-se
    ordinal=...     (after se) 1-based numbers of the traits that are ordinal (2 to 8 distinct values): every pair with one of
                    them gets its polychoric (marker or ordinal partner) or polyserial (continuous partner) correlation
                    and that estimator's standard error instead of the Pearson value and the count's
)";

const char *CUSKSS_BED_USAGE = R"(
Run cuskss on the markers selected in all blocks, with the correlations computed from genotypes on the device.

usage: mps cuskss-bed <.phen> <bfiles> <marker-indices> <time_index|NULL> <alpha> <max_level_one> <max_level_two> <depth> <outdir> [het] [markers] [ordinal=<1-based,...>]

    het             test every marker-trait and trait-trait pair at the number of individuals it was observed on (.phen
                    with NA) instead of all of them: the result of cuskss on the files of `mps sumstats ... se`
    markers         (after het) also every pair of markers at the number of individuals both were genotyped on (.bed code
                    01 = missing) instead of all of them; cuskss_merged.ess carries those counts in its marker x marker part
    ordinal=...     (after het) 1-based numbers of the ordinal traits: polychoric / polyserial correlations and their
                    standard errors for every pair with one of them; the result of cuskss on the files of
                    `mps sumstats ... se ordinal=...`
)";

// .phen, the prep files and the marker selection; the arrays every kernel reads are copied to the device once
struct GenoInputs
{
    Phen phen;
    std::vector<std::string> trait_names, chr, snp, ref;
    BedDims dims;
    MappedFile bed;
    std::vector<float> means, stds;
    std::vector<int> ixs;
    unsigned char *bed_d = nullptr;
    float *phen_d = nullptr, *means_d = nullptr, *stds_d = nullptr;
    size_t N() const { return dims.num_samples; }
    size_t m() const { return dims.num_markers; }
    size_t p() const { return phen.num_phen; }
    size_t k() const { return ixs.size(); }
    // the .bed rows where the kernels find them: HBM, or the file mapping when the device has no room for all of them
    // (the same entry points take either)
    const unsigned char *bed_rows() const { return bed_d ? bed_d : bed.data + 3; }

    void load(const std::string &phen_path, const std::string &bfiles, const std::string &index_path, bool want_bim)
    {
        std::cout << "Checking paths" << std::endl;
        for (const char *sfx : {".bed", ".dim", ".means", ".stds", ".bim"}) check_path(bfiles + sfx);
        check_path(phen_path);
        if (index_path != "NULL") check_path(index_path);
        if (!bed_has_valid_magic(bfiles + ".bed")) die("unexpected magic number in bed file.");
        phen = load_phen(phen_path);
        {
            std::ifstream f(phen_path);
            std::string header;
            std::getline(f, header);
            const auto w = split_ws(header);
            if (w.size() != phen.num_phen + 2) die("header and rows of the .phen file differ in width");
            trait_names.assign(w.begin() + 2, w.end());
        }
        dims = read_dims(bfiles + ".dim");
        if (phen.num_samples != dims.num_samples) die("different num samples in phen and dims");
        std::cout << "Found " << phen.num_phen << " phenotypes" << std::endl;
        if (phen.num_phen == 0 || m() == 0 || N() == 0) die("nothing to correlate");
        means = read_floats_line_range(bfiles + ".means", 0, std::numeric_limits<size_t>::max());
        stds = read_floats_line_range(bfiles + ".stds", 0, std::numeric_limits<size_t>::max());
        if (means.size() != m() || stds.size() != m()) die("number of markers and number of means or stds differ");
        bed.open(bfiles + ".bed");
        if (bed.size < 3 + m() * dims.bytes_per_col()) die(".bed file is smaller than .dim says");
        if (want_bim)
        {  // columns 1, 2, 5 of the .bim: the `chr snp ref` columns of an mxp file
            std::ifstream f(bfiles + ".bim");
            std::string line;
            while (std::getline(f, line))
            {
                const auto w = split_ws(line);
                if (w.size() < 5) continue;
                chr.push_back(w[0]);
                snp.push_back(w[1]);
                ref.push_back(w[4]);
            }
            if (chr.size() != m()) die("number of markers in .bim and .dim differ");
        }
        if (index_path == "NULL")
        {
            ixs.resize(m());
            std::iota(ixs.begin(), ixs.end(), 0);
        }
        else
        {
            std::cout << "Loading marker indices" << std::endl;
            ixs = read_binary<int>(index_path);
            if (ixs.empty()) die("marker index file is empty");
            for (size_t i = 0; i < ixs.size(); i++)
                if (ixs[i] < 0 || (size_t)ixs[i] >= m() || (i > 0 && ixs[i] <= ixs[i - 1]))
                    die("marker indices must be ascending, distinct and smaller than the number of markers");
        }
        if (k() + p() > (size_t)std::numeric_limits<int>::max() / 2) die("too many variables");
    }

    void stage(cusk_engine *e)
    {
        auto up = [&](const void *src, size_t bytes, const char *what) -> void * {
            void *d = cusk_dev_alloc(bytes);
            if (!d || cusk_dev_upload(d, src, bytes) != CUSK_OK) engine_die(what, e);
            return d;
        };
        phen_d = static_cast<float *>(up(phen.data.data(), sizeof(float) * phen.data.size(), "upload phenotypes"));
        means_d = static_cast<float *>(up(means.data(), sizeof(float) * means.size(), "upload means"));
        stds_d = static_cast<float *>(up(stds.data(), sizeof(float) * stds.size(), "upload stds"));
        const size_t bed_bytes = m() * dims.bytes_per_col();
        bed_d = static_cast<unsigned char *>(cusk_dev_alloc(bed_bytes));
        if (!bed_d)
            std::cout << "The .bed (" << bed_bytes << " bytes) does not fit the device: reading it from the host" << std::endl;
        else if (cusk_dev_upload(bed_d, bed.data + 3, bed_bytes) != CUSK_OK)
            engine_die("upload .bed", e);
    }

    // n x n matrix (selected markers, then traits) built where the sweep reads it
    void build_square(cusk_engine *e, float *C_dev, float *mxp_host = nullptr)
    {
        if (cusk_corr_build_indexed(e, bed_rows(), phen_d, ixs.data(), k(), m(), N(), p(), means_d, stds_d, C_dev, mxp_host) !=
            CUSK_OK)
            engine_die("correlation build", e);
    }

    ~GenoInputs()
    {
        cusk_dev_free(bed_d);
        cusk_dev_free(phen_d);
        cusk_dev_free(means_d);
        cusk_dev_free(stds_d);
    }
};

// Polychoric / polyserial estimates of every pair with an ordinal trait (`ordinal=`), as float32 the files hold: r and se
// are formed in double on the device and rounded once, here.
struct OrdinalTraitEstimates
{
    std::vector<float> r, se;  // p x q: trait a with ordinal trait spec.ix[t]; its own entry is not set
};

OrdinalSpec load_ordinal_spec(const std::string &arg, const GenoInputs &in)
{
    try
    {
        return ordinal_levels(parse_ordinal_arg(arg, in.p()), in.phen.data.data(), in.N(), in.trait_names);
    }
    catch (const std::exception &ex)
    {
        die(ex.what());
    }
    return OrdinalSpec();
}

OrdinalTraitEstimates ordinal_trait_estimates(cusk_engine *e, const GenoInputs &in, const OrdinalSpec &spec)
{
    const size_t p = in.p(), q = spec.q();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    OrdinalTraitEstimates out;
    out.r.assign(p * q, nan);
    out.se.assign(p * q, nan);
    std::vector<int> oxo(q * q * 64);
    if (cusk_ordinal_tables(e, nullptr, in.phen_d, nullptr, 0, 0, in.N(), p, spec.ix.data(), q, spec.levels.data(), spec.nlev.data(),
                            nullptr, oxo.data()) != CUSK_OK)
        engine_die("ordinal trait tables", e);
    std::vector<double> r(q * q), se(q * q);
    std::vector<int> status(q * q);
    if (cusk_polychoric_fit(e, oxo.data(), q * q, 8, 8, r.data(), se.data(), status.data()) != CUSK_OK)
        engine_die("polychoric fit (traits)", e);
    for (size_t a = 0; a < q; a++)
        for (size_t b = a + 1; b < q; b++)
        {  // one fit per pair, mirrored: the two orientations of a table need not agree to the last bit
            out.r[(size_t)spec.ix[a] * q + b] = out.r[(size_t)spec.ix[b] * q + a] = (float)r[a * q + b];
            out.se[(size_t)spec.ix[a] * q + b] = out.se[(size_t)spec.ix[b] * q + a] = (float)se[a * q + b];
        }
    std::vector<int> cont;
    for (size_t t = 0; t < p; t++)
        if (std::find(spec.ix.begin(), spec.ix.end(), (int)t) == spec.ix.end()) cont.push_back((int)t);
    if (!cont.empty())
    {
        const size_t nc = cont.size();
        r.resize(nc * q), se.resize(nc * q), status.resize(nc * q);
        if (cusk_polyserial_fit(e, in.phen_d, in.N(), p, cont.data(), nc, spec.ix.data(), q, spec.levels.data(), spec.nlev.data(),
                                r.data(), se.data(), status.data()) != CUSK_OK)
            engine_die("polyserial fit", e);
        for (size_t c = 0; c < nc; c++)
            for (size_t t = 0; t < q; t++)
            {
                out.r[(size_t)cont[c] * q + t] = (float)r[c * q + t];
                out.se[(size_t)cont[c] * q + t] = (float)se[c * q + t];
            }
    }
    return out;
}

// r and se (rows x q, float32) of the markers `marker_ix` (NULL: rows 0 .. rows-1 of bed) with every ordinal trait
void ordinal_marker_estimates(cusk_engine *e, const GenoInputs &in, const OrdinalSpec &spec, const unsigned char *bed, const int *marker_ix,
                              size_t rows, size_t m_total, float *r_out, float *se_out)
{
    const size_t q = spec.q();
    std::vector<int> tab(rows * q * 24);
    if (cusk_ordinal_tables(e, bed, in.phen_d, marker_ix, rows, m_total, in.N(), in.p(), spec.ix.data(), q, spec.levels.data(),
                            spec.nlev.data(), tab.data(), nullptr) != CUSK_OK)
        engine_die("ordinal marker tables", e);
    std::vector<double> r(rows * q), se(rows * q);
    std::vector<int> status(rows * q);
    if (cusk_polychoric_fit(e, tab.data(), rows * q, 3, 8, r.data(), se.data(), status.data()) != CUSK_OK)
        engine_die("polychoric fit (markers)", e);
    for (size_t i = 0; i < rows * q; i++)
    {
        r_out[i] = (float)r[i];
        se_out[i] = (float)se[i];
    }
}

int cmd_sumstats(int argc, char **argv)
{
    if (argc < 6)
    {
        std::cout << SUMSTATS_USAGE << std::endl;
        std::exit(1);
    }
    const std::string phen_path = argv[2], bfiles = argv[3], index_path = argv[4], outdir = argv[5];
    const bool with_se = argc > 6;
    if (with_se && std::string(argv[6]) != "se") die(std::string("sumstats: unknown trailing argument ") + argv[6]);
    const bool with_ordinal = argc > 7;
    if (with_ordinal && std::string(argv[7]).compare(0, 8, "ordinal=") != 0) die(std::string("sumstats: unknown trailing argument ") + argv[7]);
    if (argc > 8) die(std::string("sumstats: unknown trailing argument ") + argv[8]);
    PhaseTimer tm;
    check_path(outdir);
    GenoInputs in;
    in.load(phen_path, bfiles, index_path, true);
    tm.mark("load phen, dim, means, stds, bim, indices; map bed");
    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    if (tm.on) cusk_engine_set_option(e, "hostprof", 1);
    in.stage(e);
    tm.mark("engine create + inputs to the device");
    const size_t k = in.k(), p = in.p(), m = in.m(), n = k + p;

    std::cout << "Computing correlations of " << k << " selected markers and " << p << " traits" << std::endl;
    DevMat C(n * n);
    in.build_square(e, C.p);
    if (tm.on)
    {
        float ms4[4];
        cusk_corr_timing(e, ms4);
        std::cout << "[t] device: marker x marker " << ms4[1] << " ms, marker x trait + trait x trait " << ms4[2] << " ms" << std::endl;
    }
    tm.mark("indexed build (gather + mxm + mxp + pxp)");
    std::vector<float> tri(k * (k + 1) / 2);
    if (cusk_pack_lower_tri(e, C.p, n, k, tri.data(), 0) != CUSK_OK) engine_die("pack mxm", e);
    tm.mark("pack lower triangle + copy to host");
    std::vector<int> traits(p);
    std::iota(traits.begin(), traits.end(), (int)k);
    const std::vector<float> pxp = gather(e, C.p, (int)n, traits);

    std::cout << "Computing marker-trait correlations of all " << m << " markers" << std::endl;
    std::vector<float> mxp(m * p);
    const size_t chunk = 16384, clb = in.dims.bytes_per_col();
    for (size_t c0 = 0; c0 < m; c0 += chunk)
    {
        const size_t mc = std::min(chunk, m - c0);
        if (cusk_corr_build(e, in.bed_rows() + c0 * clb, in.phen_d, mc, in.N(), p, in.means_d + c0, in.stds_d + c0, nullptr,
                            &mxp[c0 * p]) != CUSK_OK)
            engine_die("marker-trait correlations", e);
    }
    tm.mark("genome-wide mxp");
    std::vector<int> mxp_n, pxp_n;
    if (with_se)
    {
        std::cout << "Counting complete observations per pair" << std::endl;
        mxp_n.resize(m * p);
        pxp_n.resize(p * p);
        for (size_t c0 = 0; c0 < m; c0 += chunk)
        {
            const size_t mc = std::min(chunk, m - c0);
            if (cusk_pair_counts(e, in.bed_rows() + c0 * clb, in.phen_d, nullptr, mc, mc, in.N(), p, &mxp_n[c0 * p],
                                 c0 == 0 ? pxp_n.data() : nullptr) != CUSK_OK)
                engine_die("pair counts", e);
        }
        tm.mark("genome-wide pair counts");
    }

    // ordinal traits: their columns of mxp / mxp_se and their rows and columns of pxp / pxp_se are replaced
    std::vector<float> pxp_out = pxp, mxp_se, pxp_se;
    if (with_ordinal)
    {
        const OrdinalSpec spec = load_ordinal_spec(argv[7], in);
        const size_t q = spec.q();
        std::cout << "Estimating polychoric / polyserial correlations of " << q << " ordinal traits" << std::endl;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        mxp_se.resize(m * p);
        for (size_t i = 0; i < m * p; i++) mxp_se[i] = std::isnan(mxp[i]) ? nan : cusk_se_from_count(mxp[i], mxp_n[i]);
        pxp_se.assign(p * p, nan);
        for (size_t a = 0; a < p; a++)
            for (size_t b = 0; b < p; b++)
                if (a != b && !std::isnan(pxp[a * p + b])) pxp_se[a * p + b] = cusk_se_from_count(pxp[a * p + b], pxp_n[a * p + b]);
        const OrdinalTraitEstimates te = ordinal_trait_estimates(e, in, spec);
        for (size_t t = 0; t < q; t++)
            for (size_t a = 0; a < p; a++)
                if (a != (size_t)spec.ix[t])
                {
                    const size_t o = (size_t)spec.ix[t];
                    pxp_out[a * p + o] = pxp_out[o * p + a] = te.r[a * q + t];
                    pxp_se[a * p + o] = pxp_se[o * p + a] = te.se[a * q + t];
                }
        std::vector<float> r(chunk * q), se(chunk * q);
        for (size_t c0 = 0; c0 < m; c0 += chunk)
        {
            const size_t mc = std::min(chunk, m - c0);
            ordinal_marker_estimates(e, in, spec, in.bed_rows() + c0 * clb, nullptr, mc, mc, r.data(), se.data());
            for (size_t i = 0; i < mc; i++)
                for (size_t t = 0; t < q; t++)
                {
                    mxp[(c0 + i) * p + spec.ix[t]] = r[i * q + t];
                    mxp_se[(c0 + i) * p + spec.ix[t]] = se[i * q + t];
                }
        }
        tm.mark("ordinal tables + fits");
    }

    std::cout << "Writing mxm.bin, mxp.txt, pxp.txt" << std::endl;
    auto cstrs = [](const std::vector<std::string> &v) {
        std::vector<const char *> out(v.size());
        for (size_t i = 0; i < v.size(); i++) out[i] = v[i].c_str();
        return out;
    };
    const auto chr = cstrs(in.chr), snp = cstrs(in.snp), ref = cstrs(in.ref), names = cstrs(in.trait_names);
    char err[512] = "";
    if (cusk_sumstats_write(outdir.c_str(), tri.data(), k, mxp.data(), m, p, pxp_out.data(), chr.data(), snp.data(), ref.data(),
                            names.data(), err, sizeof(err)) != CUSK_OK)
        die(err);
    if (with_ordinal)
    {
        std::cout << "Writing mxp_se.txt, pxp_se.txt" << std::endl;
        if (cusk_sumstats_write_se_values(outdir.c_str(), mxp_se.data(), m, p, pxp_se.data(), chr.data(), snp.data(), ref.data(),
                                          names.data(), err, sizeof(err)) != CUSK_OK)
            die(err);
    }
    else if (with_se)
    {
        std::cout << "Writing mxp_se.txt, pxp_se.txt" << std::endl;
        if (cusk_sumstats_write_se(outdir.c_str(), mxp.data(), mxp_n.data(), m, p, pxp.data(), pxp_n.data(), chr.data(), snp.data(),
                                   ref.data(), names.data(), err, sizeof(err)) != CUSK_OK)
            die(err);
    }
    tm.mark("write files");
    cusk_engine_destroy(e);
    std::cout << "Done." << std::endl;
    return 0;
}

int cmd_cuskss_bed(int argc, char **argv)
{
    if (argc < 11)
    {
        std::cout << CUSKSS_BED_USAGE << std::endl;
        std::exit(1);
    }
    const std::string phen_path = argv[2], bfiles = argv[3], index_path = argv[4], time_index_path = argv[5];
    const float alpha = std::stof(argv[6]);
    const int max_level_one = std::stoi(argv[7]), max_level_two = std::stoi(argv[8]), depth = std::stoi(argv[9]);
    const std::string outdir = argv[10];
    const bool het = argc > 11;
    if (het && std::string(argv[11]) != "het") die(std::string("cuskss-bed: unknown trailing argument ") + argv[11]);
    bool het_markers = false;
    std::string ordinal_arg;
    for (int a = 12; a < argc; a++)
    {  // after het: markers, then ordinal=...
        const std::string w = argv[a];
        if (w == "markers" && a == 12)
            het_markers = true;
        else if (w.compare(0, 8, "ordinal=") == 0 && a + 1 == argc)
            ordinal_arg = w;
        else
            die(std::string("cuskss-bed: unknown trailing argument ") + argv[a]);
    }
    if (index_path == "NULL") die("cuskss-bed needs marker indices");
    check_path(outdir);
    const bool time_indexed = time_index_path != "NULL";
    if (time_indexed) check_path(time_index_path);
    GenoInputs in;
    in.load(phen_path, bfiles, index_path, false);
    const size_t k = in.k(), p = in.p(), n = k + p;
    const float num_samples = (float)in.N();
    std::vector<int> time_index_traits(p, 1);
    if (time_indexed)
    {
        std::cout << "Loading time_indices" << std::endl;
        time_index_traits = read_ints_lines(time_index_path);
        if (time_index_traits.size() < p) die("time index file has fewer lines than traits");
    }
    const float th = cusk_hetcor_threshold(alpha);
    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    in.stage(e);

    std::cout << "Computing correlations of " << k << " selected markers and " << p << " traits" << std::endl;
    GC gc;
    gc.num_phen = p;
    gc.num_var = n;
    gc.new_to_old.resize(n);
    std::iota(gc.new_to_old.begin(), gc.new_to_old.end(), 0);
    {
        DevMat C(n * n);
        std::vector<float> mxp;
        if (het) mxp.resize(k * p);
        in.build_square(e, C.p, het ? mxp.data() : nullptr);
        if (het)
        {
            // The sample sizes `cuskss` would load from the files of `mps sumstats ... se` (load_mxp, load_pxp and
            // make_square_cuskss_inputs, cli.cpp:89-173): N between markers; the count of complete observations, through
            // the standard error the file would hold, between a marker or trait and a trait; NaN where the correlation
            // is NaN and on the trait diagonal (pxp_se holds nan there).  pxp is read as the loader reads it: the
            // upper triangle, mirrored.
            std::cout << "Counting complete observations per pair" << std::endl;
            std::vector<int> traits(p);
            std::iota(traits.begin(), traits.end(), (int)k);
            const std::vector<float> pxp = gather(e, C.p, (int)n, traits);
            std::vector<int> mxp_n(k * p), pxp_n(p * p);
            if (cusk_pair_counts(e, in.bed_rows(), in.phen_d, in.ixs.data(), k, in.m(), in.N(), p, mxp_n.data(), pxp_n.data()) !=
                CUSK_OK)
                engine_die("pair counts", e);
            const float nan = std::numeric_limits<float>::quiet_NaN();
            auto ess_of = [&](float r, int count) { return std::isnan(r) ? nan : cusk_ess_from_se(r, cusk_se_from_count(r, count)); };
            gc.ess.assign(n * n, num_samples);
            if (het_markers)
            {  // between markers: the individuals both were genotyped on, counted on the device into a k x k scratch
                DevMat Nmm(k * k);
                std::vector<float> cnt(k * k);
                if (cusk_marker_pair_sizes(e, in.bed_rows(), in.ixs.data(), k, in.m(), in.N(), Nmm.p, k) != CUSK_OK)
                    engine_die("marker pair sizes", e);
                if (cusk_dev_download(cnt.data(), Nmm.p, sizeof(float) * k * k) != CUSK_OK) engine_die("marker pair sizes (download)", e);
                for (size_t i = 0; i < k; i++) std::copy_n(&cnt[i * k], k, &gc.ess[i * n]);
            }
            for (size_t i = 0; i < k; i++)
                for (size_t t = 0; t < p; t++)
                    gc.ess[i * n + k + t] = gc.ess[(k + t) * n + i] = ess_of(mxp[i * p + t], mxp_n[i * p + t]);
            for (size_t a = 0; a < p; a++)
            {
                gc.ess[(k + a) * n + k + a] = nan;
                for (size_t b = a + 1; b < p; b++)
                    gc.ess[(k + a) * n + k + b] = gc.ess[(k + b) * n + k + a] = ess_of(pxp[a * p + b], pxp_n[a * p + b]);
            }
        }
        if (!ordinal_arg.empty())
        {
            // what `mps sumstats ... se ordinal=` writes for the pairs with an ordinal trait, through the same rounding to
            // float32 and the same chain to a sample size; the matrix on the device gets the estimates in place
            const OrdinalSpec spec = load_ordinal_spec(ordinal_arg, in);
            const size_t q = spec.q();
            std::cout << "Estimating polychoric / polyserial correlations of " << q << " ordinal traits" << std::endl;
            const float nan = std::numeric_limits<float>::quiet_NaN();
            auto ess_of_se = [&](float r, float se) { return std::isnan(r) ? nan : cusk_ess_from_se(r, se); };
            const OrdinalTraitEstimates te = ordinal_trait_estimates(e, in, spec);
            std::vector<float> mr(k * q), mse(k * q), cross(n);
            ordinal_marker_estimates(e, in, spec, in.bed_rows(), in.ixs.data(), k, in.m(), mr.data(), mse.data());
            for (size_t t = 0; t < q; t++)
            {
                const size_t o = k + (size_t)spec.ix[t];
                for (size_t i = 0; i < k; i++)
                {
                    cross[i] = mr[i * q + t];
                    gc.ess[i * n + o] = gc.ess[o * n + i] = ess_of_se(mr[i * q + t], mse[i * q + t]);
                }
                for (size_t a = 0; a < p; a++)
                {
                    if (k + a == o)
                    {
                        cross[o] = 1.0f;
                        continue;
                    }
                    cross[k + a] = te.r[a * q + t];
                    gc.ess[(k + a) * n + o] = gc.ess[o * n + k + a] = ess_of_se(te.r[a * q + t], te.se[a * q + t]);
                }
                if (cusk_matrix_set_cross(e, C.p, n, o, cross.data()) != CUSK_OK) engine_die("ordinal correlations into the matrix", e);
            }
        }
        // what the loaders of the three files do to a NaN correlation (host_io.h: load_mxm_into, load_mxp, load_pxp)
        if (cusk_nan_to_zero(e, C.p, n * n) != CUSK_OK) engine_die("NaN -> 0", e);
        std::cout << "Starting first cusk stage" << std::endl;
        gc = run_cusk(e, gc, th, num_samples, het, depth, max_level_one, time_index_traits, C.p);
    }
    if (max_level_two > 0)
    {
        std::cout << "Starting second cusk stage" << std::endl;
        gc = run_cusk(e, gc, th, num_samples, het, depth, max_level_two, time_index_traits);
    }
    std::cout << "Retained " << gc.num_markers() << " markers" << std::endl;
    write_gc(gc, make_path(outdir, "cuskss_merged", ""));
    cusk_engine_destroy(e);
    return 0;
}

const char *MPS_USAGE = R"(
usage: mps <command> [<args>]

commands:
    cusk                    Run the skeleton search on a single block of block diagonal genomic covariance matrix
    cuskss                  Run the skeleton search on a block of markers and traits with pre-computed correlations.
    sumstats                Compute the correlation files cuskss reads (mxm, mxp, pxp; with `se` also mxp_se, pxp_se) from genotypes and phenotypes
    cuskss-bed              cuskss on the merged marker selection with the correlations computed from genotypes
    block                   Tile the marker x marker correlation matrix of every chromosome into LD blocks
    prep                    Prepare input (PLINK) .bed file for cusk: .dim, .means, .stds, .modes
    prune                   Drop constant markers and LD-prune a fileset (goes in front of prep)
)";

}  // namespace

// ---------------------------------------------------------------------------------------
// mps block   (cli.cpp:348-411)
// ---------------------------------------------------------------------------------------
const char *BLOCK_USAGE = R"(
Tile marker x marker correlation matrix

usage: mps block <bfiles> <max-block-size> <device-mem-gb> <corr-width>

arguments:
    bfiles          stem of .bed, .bim, .fam fileset
    max-block-size  maximum number of markers per block
    device-mem-gb   maximum memory available on gpu in GB
    corr-width      max distance at which to compute correlations
)";

int cmd_block(int argc, char **argv)
{
    if (argc < 6)
    {
        std::cout << BLOCK_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2];
    const int max_block_size = std::stoi(argv[3]);
    const float device_mem_gb = std::stof(argv[4]);
    const size_t corr_width = (size_t)std::stoi(argv[5]);
    PhaseTimer tm;

    std::cout << "Checking paths" << std::endl;
    for (const char *sfx : {".bed", ".bim", ".fam"}) check_path(bfiles + sfx);
    if (!bed_has_valid_magic(bfiles + ".bed")) die("unexpected magic number in bed file.");
    const BimInfo bim = read_bim(bfiles + ".bim");
    const size_t N = count_lines(bfiles + ".fam");  // BedDims(BfilesBase), io.h:41-45
    const size_t bytes_per_marker = (N + 3) / 4;
    const std::string out_path = bfiles + "_m" + std::to_string(max_block_size) + ".blocks";  // bfiles_base.h:35

    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    for (const std::string &cid : bim.chr_ids)
    {
        const size_t m = bim.markers_on(cid);
        const size_t mem_host_gb = (size_t)(((double)(m * bytes_per_marker) + (double)corr_width * (double)m * 4.0) * 1e-9);
        std::cout << "[Chr " << cid << "]: At least " << mem_host_gb << " GB in host memory required." << std::endl;
        std::cout << "[Chr " << cid << "]: Loading bed data for " << m << " markers." << std::endl;
        Block whole;
        whole.chr = cid;
        whole.first = 0;
        whole.last = m - 1;
        BedDims dims;
        dims.num_samples = N;
        dims.num_markers = bim.num_lines;
        const std::vector<unsigned char> bed = read_bed_block(bfiles + ".bed", whole, dims, bim);
        tm.mark("read chromosome");

        std::cout << "[Chr " << cid << "]: Computing correlations." << std::endl;
        {  // corr_host.cu:73-91: the reference sizes a marker batch from the device memory it is told about
            const double mem_bytes = (double)device_mem_gb * 1e9;
            size_t batch = (size_t)std::floor(mem_bytes / (double)(bytes_per_marker + corr_width * 4));
            if (batch > m) batch = m;
            if (batch < corr_width)
            {
                std::printf("Maximal batch size (%zu) < corr width (%zu). Decrease distance threshold or increase device memory. \n",
                            batch, corr_width);
                std::exit(1);
            }
        }
        std::vector<float> row_sums(m);
        if (cusk_corr_banded(e, bed.data(), m, N, corr_width, row_sums.data(), nullptr) != CUSK_OK)
            engine_die("banded correlations", e);
        tm.mark("banded correlations + row sums (device)");
        std::cout << "[Chr " << cid << "]: Computing row sums." << std::endl;
        std::cout << "[Chr " << cid << "]: Making blocks." << std::endl;
        std::vector<long long> first(m), last(m);  // a chromosome has at most m blocks
        size_t num_blocks = 0;
        if (cusk_block_chr(e, row_sums.data(), m, max_block_size, first.data(), last.data(), m, &num_blocks) != CUSK_OK)
            engine_die("Hanning smoothing", e);
        tm.mark("smoothing (device) + minima + bisection");
        std::cout << "[Chr " << cid << "]: Partitioned into " << num_blocks << " blocks." << std::endl;
        std::cout << "[Chr " << cid << "]: Writing blocks to output file." << std::endl;
        std::ofstream fout(out_path, std::ios::out | std::ios::app);  // io.cpp:266-277: appends
        for (size_t b = 0; b < num_blocks; b++) fout << cid << "\t" << first[b] << "\t" << last[b] << std::endl;
    }
    cusk_engine_destroy(e);
    std::cout << "Done." << std::endl;
    return 0;
}

// ---------------------------------------------------------------------------------------
// mps prune   (not in the reference, whose README leaves both preconditions to the user)
// ---------------------------------------------------------------------------------------
const char *PRUNE_USAGE = R"(
Drop markers without recorded variation and LD-prune a fileset on the correlation the skeleton tests

usage: mps prune <bfiles> <out-stem> <r-max> <window>

arguments:
    bfiles          stem of .bed, .bim, .fam fileset
    out-stem        stem of the pruned fileset (.bed, .bim, .fam) and of .prune.in / .prune.out; not bfiles itself
    r-max           a marker is dropped when |r| >= r-max with an earlier kept marker of its chromosome within the
                    window; in (0, 1]; r is the banded Kendall-npn correlation of `mps block`
    window          number of following markers every marker is compared with (at most 4096)

Markers are walked in .bim order per chromosome and the first kept marker wins (PLINK's --indep-pairwise keeps the marker
with the higher minor allele frequency and prunes on the Pearson r^2 of the dosages).  A marker with at most one
genotype among its non-missing calls is dropped as constant and blocks no other marker.
)";

int cmd_prune(int argc, char **argv)
{
    if (argc != 6)
    {
        std::cout << PRUNE_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2], out_stem = argv[3];
    float r_max = 0.0f;
    long long window = 0;
    try
    {
        r_max = std::stof(argv[4]);
        window = std::stoll(argv[5]);
    }
    catch (const std::exception &)
    {
        die("r-max and window must be numbers");
    }
    if (!(r_max > 0.0f && r_max <= 1.0f)) die("r-max must be in (0, 1]");
    if (window < 1 || window > CUSK_PRUNE_MAX_WINDOW) die("window must be between 1 and " + std::to_string(CUSK_PRUNE_MAX_WINDOW));
    if (out_stem == bfiles) die("out-stem must differ from bfiles");
    for (const char *sfx : {".bed", ".bim", ".fam"})
    {  // another spelling of the same stem, or a link: found before the device work, cusk_prune_write checks again
        std::error_code ec;
        if (std::filesystem::equivalent(out_stem + sfx, bfiles + sfx, ec) && !ec) die("out-stem must differ from bfiles: " + out_stem + sfx + " is the input file");
    }
    PhaseTimer tm;

    std::cout << "Checking paths" << std::endl;
    for (const char *sfx : {".bed", ".bim", ".fam"}) check_path(bfiles + sfx);
    if (!bed_has_valid_magic(bfiles + ".bed")) die("unexpected magic number in bed file.");
    const BimInfo bim = read_bim(bfiles + ".bim");
    const size_t N = count_lines(bfiles + ".fam");
    if (bim.num_lines == 0 || N == 0) die("empty .bim or .fam file");

    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    std::vector<unsigned char> status(bim.num_lines);
    for (size_t c = 0; c < bim.chr_ids.size(); c++)
    {
        // (by position, not by id: the statuses of a chromosome id that occurs twice must not land on its first run)
        const std::string &cid = bim.chr_ids[c];
        const size_t m = bim.num_on_chr[c], start = bim.chr_start[c];
        std::vector<unsigned char> bed(m * ((N + 3) / 4));
        {
            std::ifstream f(bfiles + ".bed", std::ios::binary);
            f.seekg(3 + (std::streamoff)(start * ((N + 3) / 4)));
            if (!f.read(reinterpret_cast<char *>(bed.data()), (std::streamsize)bed.size())) die("bed file is shorter than its .bim and .fam say");
        }
        tm.mark("read chromosome");
        if (cusk_ld_prune(e, bed.data(), m, N, (size_t)window, r_max, status.data() + start, nullptr) != CUSK_OK)
            engine_die("ld prune", e);
        tm.mark("banded correlations, counts, bitmap, scan (device)");
        size_t n[3] = {0, 0, 0};
        for (size_t j = 0; j < m; j++) n[status[start + j]]++;
        std::cout << "[Chr " << cid << "]: " << m << " markers: " << n[CUSK_PRUNE_KEEP] << " kept, " << n[CUSK_PRUNE_CONSTANT]
                  << " constant, " << n[CUSK_PRUNE_LD] << " dropped for LD." << std::endl;
    }
    cusk_engine_destroy(e);
    if (cusk_prune_write(bfiles.c_str(), out_stem.c_str(), status.data(), status.size()) != CUSK_OK) die("cannot write the pruned fileset " + out_stem);
    tm.mark("write fileset");
    std::cout << "Done." << std::endl;
    return 0;
}

// ---------------------------------------------------------------------------------------
// mps prep   (cli.cpp:680-708, prep.cpp:15-76 compute_bed_col_stats_no_impute, :159-203 prep_bed_no_impute)
// ---------------------------------------------------------------------------------------
// Per marker over its non-missing genotypes: mean = sum / (float)count, population standard deviation with the
// squared deviations accumulated in single precision in sample order, most frequent genotype (ties to the lower
// one).  Host code like the reference's (one streaming pass over the .bed; nothing here is worth a device launch);
// the arithmetic is kept operation for operation because cusk's Pearson correlations divide by these numbers.
const char *PREP_USAGE = R"(
Prepare input (PLINK) .bed file for cusk

usage: mps prep <.bfiles>

arguments:
    .bfiles filestem of .bed, .bim, .fam fileset
)";

int cmd_prep(int argc, char **argv)
{
    if (argc != 3 || std::string(argv[2]) == "--help" || std::string(argv[2]) == "-h")
    {
        std::cout << PREP_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2];
    for (const char *sfx : {".bed", ".bim", ".fam"}) check_path(bfiles + sfx);
    if (!bed_has_valid_magic(bfiles + ".bed"))
    {
        std::cout << "Invalid prefix bytes in bed" << std::endl;
        std::exit(1);
    }
    const size_t N = count_lines(bfiles + ".fam");
    const size_t M = count_lines(bfiles + ".bim");
    std::cout << "Writing dim file." << std::endl;
    {
        std::ofstream fout(bfiles + ".dim");
        fout << N << "\t" << M << std::endl;
    }
    const size_t bytes_per_marker = (N + 3) / 4;
    std::vector<unsigned char> col(bytes_per_marker);
    std::vector<float> means, stds;
    std::vector<int> modes;
    std::ifstream bed(bfiles + ".bed", std::ios::binary);
    bed.seekg(3);
    std::cout << "Computing means, stds, modes." << std::endl;
    // PLINK codes, low bits first (bed_lut.h): 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
    static const int kValue[4] = {2, 0, 1, 0};
    size_t lc = 0;
    while (bed.read(reinterpret_cast<char *>(col.data()), (std::streamsize)bytes_per_marker))
    {
        if (lc % 100000 == 0) std::cout << "Processing marker " << lc + 1 << " / " << M << std::endl;
        int counts[3] = {0, 0, 0};
        size_t sum = 0, missing = 0;
        for (size_t i = 0; i < N; i++)
        {
            const int code = (col[i >> 2] >> (2 * (i & 3))) & 3;
            if (code == 1)
                missing++;
            else
            {
                counts[kValue[code]]++;
                sum += (size_t)kValue[code];
            }
        }
        int mode = 0;
        for (int g = 1; g < 3; g++)
            if (counts[g] > counts[mode]) mode = g;
        const float mean = sum / (float)(N - missing);
        float ss = 0.0f;
        for (size_t i = 0; i < N; i++)
        {
            const int code = (col[i >> 2] >> (2 * (i & 3))) & 3;
            if (code != 1) ss += ((float)kValue[code] - mean) * ((float)kValue[code] - mean);
        }
        means.push_back(mean);
        stds.push_back(std::sqrt(ss / (float)(N - missing)));
        modes.push_back(mode);
        lc++;
    }
    std::cout << "Writing stats to files." << std::endl;
    {
        std::ofstream f(bfiles + ".means");
        for (float v : means) f << v << std::endl;
    }
    {
        std::ofstream f(bfiles + ".stds");
        for (float v : stds) f << v << std::endl;
    }
    {
        std::ofstream f(bfiles + ".modes");
        for (int v : modes) f << v << std::endl;
    }
    std::cout << "Done." << std::endl;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 1)
    {
        std::cout << MPS_USAGE << std::endl;
        return EXIT_SUCCESS;
    }
    const std::string cmd = argv[1];
    try
    {
        if (cmd == "cusk") return cmd_cusk(argc, argv);
        if (cmd == "cuskss") return cmd_cuskss(argc, argv);
        if (cmd == "sumstats") return cmd_sumstats(argc, argv);
        if (cmd == "cuskss-bed") return cmd_cuskss_bed(argc, argv);
        if (cmd == "block") return cmd_block(argc, argv);
        if (cmd == "prep") return cmd_prep(argc, argv);
        if (cmd == "prune") return cmd_prune(argc, argv);
    }
    catch (const Fatal &f)
    {  // bad input: message + status 1, as the reference's loaders and argument checks do (cli.cpp:185-192)
        std::cerr << f.what() << std::endl;
        return 1;
    }
    catch (const EngineError &f)
    {  // device failure: gpuerrors.h:6-15
        std::fprintf(stderr, "mps: %s\n", f.what());
        return EXIT_FAILURE;
    }
    std::cout << MPS_USAGE << std::endl;
    return EXIT_SUCCESS;
}
