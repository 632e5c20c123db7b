// cmd_cuskss_bed.cpp -- mps cuskss-bed: cuskss on the merged marker selection with the correlations computed from genotypes
// on the device -- the result of `mps sumstats` followed by `mps cuskss` without the files in between.  The reference has
// no such command.
#include "cuskss_run.h"
#include "mps.h"
#include "ordinal_estimates.h"
#include "square_inputs.h"
#include "trailing_words.h"

using namespace host;

namespace {

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

}  // namespace

int host::cmd_cuskss_bed(int argc, char **argv)
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
    bool het = false, het_markers = false, with_ordinal = false;
    std::string ordinal_arg;
    parse_trailing_words("cuskss-bed", argc, argv, 11,
                         {{"het", 0, &het, nullptr}, {"markers", 1, &het_markers, nullptr}, {"ordinal=", TrailingWord::kLast, &with_ordinal, &ordinal_arg}});
    if (index_path == "NULL") die("cuskss-bed needs marker indices");
    check_path(outdir);
    if (time_index_path != "NULL") check_path(time_index_path);
    GenoInputs in;
    in.load(phen_path, bfiles, index_path, false);
    const size_t k = in.k(), p = in.p(), n = k + p;
    const float num_samples = (float)in.N();
    const std::vector<int> time_index_traits = load_time_index(time_index_path, p);
    const float th = cusk_hetcor_threshold(alpha);
    cusk_engine *e = open_engine();
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
            if (cusk_pair_counts(e, in.bed_rows(), in.dev.phen, in.ixs.data(), k, in.m(), in.N(), p, mxp_n.data(), pxp_n.data()) !=
                CUSK_OK)
                engine_die("pair counts", e);
            std::vector<float> mxp_ess, pxp_ess, cnt;
            block_sample_sizes(mxp.data(), mxp_n.data(), pxp.data(), pxp_n.data(), k, p, mxp_ess, pxp_ess);
            if (het_markers)
            {  // between markers: the individuals both were genotyped on, counted on the device into a k x k scratch
                DevMat Nmm(k * k);
                cnt.resize(k * k);
                if (cusk_marker_pair_sizes(e, in.bed_rows(), in.ixs.data(), k, in.m(), in.N(), Nmm.p, k) != CUSK_OK)
                    engine_die("marker pair sizes", e);
                if (cusk_dev_download(cnt.data(), Nmm.p, sizeof(float) * k * k) != CUSK_OK) engine_die("marker pair sizes (download)", e);
            }
            gc.ess = square_sample_sizes(mxp_ess, pxp_ess, k, p, num_samples, het_markers ? cnt.data() : nullptr);
        }
        if (with_ordinal)
        {
            // what `mps sumstats ... se ordinal=` writes for the pairs with an ordinal trait, through the same rounding to
            // float32 and the same chain to a sample size; the matrix on the device gets the estimates in place
            const OrdinalSpec spec = load_ordinal_spec(ordinal_arg, in);
            const size_t q = spec.q();
            std::cout << "Estimating polychoric / polyserial correlations of " << q << " ordinal traits" << std::endl;
            const OrdinalTraitEstimates te = ordinal_trait_estimates(e, in, spec);
            std::vector<float> mr(k * q), mse(k * q), cross(q * n);
            ordinal_marker_estimates(e, in, spec, in.bed_rows(), in.ixs.data(), k, in.m(), mr.data(), mse.data());
            visit_ordinal_pairs(spec.ix, k, mr.data(), mse.data(), p, &te, OrdinalSquareSink(spec.ix, k, p, cross.data(), gc.ess.data()));
            for (size_t t = 0; t < q; t++)
                if (cusk_matrix_set_cross(e, C.p, n, k + (size_t)spec.ix[t], &cross[t * n]) != CUSK_OK)
                    engine_die("ordinal correlations into the matrix", e);
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
