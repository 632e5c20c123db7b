// cmd_cusk.cpp -- mps cusk (cli.cpp:432-678 of the reference): one LD block through block_pipeline.h, the code the block
// driver runs for every block of a chromosome.
#include "block_pipeline.h"
#include "mps.h"
#include "trailing_words.h"

using namespace host;

namespace {

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

// argv of `mps cusk` (cli.cpp:432-456 plus the optional trailing `het`, which the words `filter`, `rows` and `markers` may
// follow in any order, each at most once): false = too few arguments (the caller prints the usage text and exits with 1)
bool parse_cusk_args(int argc, char **argv, CuskInputs &in, std::string &outdir, int &block_index)
{
    if (argc < 11) return false;
    in.phen_path = argv[2];
    in.bfiles = argv[3];
    in.block_path = argv[4];
    in.alpha = std::stof(argv[5]);
    in.max_level = std::stoi(argv[6]);
    in.max_level_two = std::stoi(argv[7]);
    in.depth = std::stoi(argv[8]);
    outdir = argv[9];
    block_index = std::stoi(argv[10]);
    parse_trailing_words("cusk", argc, argv, 11,
                         {{"het", 0, &in.het, nullptr},
                          {"filter", TrailingWord::kAnywhere, &in.het_filter, nullptr},
                          {"rows", TrailingWord::kAnywhere, &in.het_rows, nullptr},
                          {"markers", TrailingWord::kAnywhere, &in.het_markers, nullptr}});
    return true;
}

}  // namespace

int host::cmd_cusk(int argc, char **argv)
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

    cusk_engine *e = open_engine();
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
