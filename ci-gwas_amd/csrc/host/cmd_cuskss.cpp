// cmd_cuskss.cpp -- mps cuskss (mps.cpp:31-101, cli.cpp:89-173, :194-346 of the reference): the skeleton search on
// pre-computed correlation files, markers of one block or of the merged selection, then the traits.
#include <numeric>

#include "cuskss_run.h"
#include "mps.h"
#include "square_inputs.h"

using namespace host;

int host::cmd_cuskss(int argc, char **argv)
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
    const std::vector<int> time_index_traits = load_time_index(time_index_path, p);
    const float th = cusk_hetcor_threshold(alpha);
    cusk_engine *e = open_engine();

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
    if (hetcor) gc.ess = square_sample_sizes(mxp.ess, pxp.ess, m, p, num_samples);
    for (size_t i = 0; i < m; i++)
        for (size_t k = 0; k < p; k++) gc.C[i * n + m + k] = gc.C[(m + k) * n + i] = mxp.corr[i * p + k];
    for (size_t a = 0; a < p; a++) std::copy_n(&pxp.corr[a * p], p, &gc.C[(m + a) * n + m]);
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
