// cmd_sumstats.cpp -- mps sumstats: the inputs of `cuskss` on the merged marker set (mxm, mxp, pxp and their standard
// errors), from genotypes.  The reference has no such command: its cuskss reads these files (cli.cpp:194-346) and leaves
// making them to the user.
#include "mps.h"
#include "ordinal_estimates.h"
#include "square_inputs.h"
#include "trailing_words.h"

using namespace host;

namespace {

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

std::vector<const char *> cstrs(const std::vector<std::string> &v)
{
    std::vector<const char *> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i].c_str();
    return out;
}

}  // namespace

int host::cmd_sumstats(int argc, char **argv)
{
    if (argc < 6)
    {
        std::cout << SUMSTATS_USAGE << std::endl;
        std::exit(1);
    }
    const std::string phen_path = argv[2], bfiles = argv[3], index_path = argv[4], outdir = argv[5];
    bool with_se = false, with_ordinal = false;
    std::string ordinal_arg;
    parse_trailing_words("sumstats", argc, argv, 6, {{"se", 0, &with_se, nullptr}, {"ordinal=", 1, &with_ordinal, &ordinal_arg}});
    PhaseTimer tm;
    check_path(outdir);
    GenoInputs in;
    in.load(phen_path, bfiles, index_path, true);
    tm.mark("load phen, dim, means, stds, bim, indices; map bed");
    cusk_engine *e = open_engine();
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
        if (cusk_corr_build(e, in.bed_rows() + c0 * clb, in.dev.phen, mc, in.N(), p, in.dev.means + c0, in.dev.stds + c0, nullptr,
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
            if (cusk_pair_counts(e, in.bed_rows() + c0 * clb, in.dev.phen, nullptr, mc, mc, in.N(), p, &mxp_n[c0 * p],
                                 c0 == 0 ? pxp_n.data() : nullptr) != CUSK_OK)
                engine_die("pair counts", e);
        }
        tm.mark("genome-wide pair counts");
    }

    // ordinal traits: their columns of mxp / mxp_se and their rows and columns of pxp / pxp_se are replaced
    std::vector<float> pxp_out = pxp, mxp_se, pxp_se;
    if (with_ordinal)
    {
        const OrdinalSpec spec = load_ordinal_spec(ordinal_arg, in);
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
        std::vector<float> r(chunk * q), se(chunk * q);
        for (size_t c0 = 0; c0 < m; c0 += chunk)
        {  // (the chunks are about device memory; the pairs between traits go with the first)
            const size_t mc = std::min(chunk, m - c0);
            ordinal_marker_estimates(e, in, spec, in.bed_rows() + c0 * clb, nullptr, mc, mc, r.data(), se.data());
            visit_ordinal_pairs(spec.ix, mc, r.data(), se.data(), p, c0 == 0 ? &te : nullptr,
                                OrdinalFileSink{&mxp[c0 * p], &mxp_se[c0 * p], pxp_out.data(), pxp_se.data(), p});
        }
        tm.mark("ordinal tables + fits");
    }

    std::cout << "Writing mxm.bin, mxp.txt, pxp.txt" << std::endl;
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
