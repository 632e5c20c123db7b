// mps_main.cpp -- `mps`-compatible host program for the cusk path on MI355X: the dispatch to the commands (cmd_<name>.cpp).
//
// Same positional argv contracts, stdout milestones, exit codes and output files as the reference's native CLI
// (cusk/apps/mps.cpp:17-121, src/cli.cpp:194-346, :348-411, :432-708), so that ci-gwas.py (or this repo's cli shim) can
// call it unchanged:
//   mps prep   <bfiles>
//   mps block  <bfiles> <max-block-size> <device-mem-gb> <corr-width>
//   mps cusk   <.phen> <bfiles> <.blocks> <alpha> <max-level> <max-level-two> <depth> <outdir> <block-index> [het] [filter] [rows] [markers]
//   mps cuskss <mxm> <mxp> <mxp_se> <pxp> <pxp_se> <time_index> <block_index> <blockfile>
//              <marker_indices> <alpha> <l1> <l2> <depth> <num_samples> <outdir>   ("NULL" = absent)
// and five commands the reference does not have:
//   mps sumstats   <.phen> <bfiles> <marker-indices|NULL> <outdir> [se] [ordinal=<1-based,...>]
//   mps cuskss-bed <.phen> <bfiles> <marker-indices> <time_index|NULL> <alpha> <l1> <l2> <depth> <outdir> [het] [markers] [ordinal=<1-based,...>]
//   mps prune      <bfiles> <out-stem> <r-max> <window>
//   mps prep-phen  <bfiles> <table> <out> <covar|NULL> [ordinal=<1-based,...>]
//   mps check-phen <bfiles> <.phen>
// Differences by design: the correlation matrix never leaves HBM between the build and the
// sweep, adjacency comes back as a bitmap, separating sets as sparse records, only the
// retained sub-matrix is gathered to the host, and files are written with one fwrite each.
#include <cstdio>
#include <string>

#include "engine_util.h"
#include "host_io.h"
#include "mps.h"

using namespace host;

namespace {

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
    prep-phen               Match a trait table to the .fam, remove covariates from the traits and standardise them
    check-phen              Check that a .phen is row-aligned to the .fam and standardised (status 1 if not)
)";

}  // namespace

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
        if (cmd == "prep-phen") return cmd_prep_phen(argc, argv);
        if (cmd == "check-phen") return cmd_check_phen(argc, argv);
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
