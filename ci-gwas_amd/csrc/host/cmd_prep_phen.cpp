// cmd_prep_phen.cpp -- mps prep-phen / mps check-phen (not in the reference, whose README leaves "make sure that the trait
// values are standardized" to the user and whose cusk/scripts/phen_prep.py only reindexes and checks): a trait table matched
// to the .fam by IID, residualised on covariates and standardised on the device (cusk_phen_adjust states the rule), written
// as a .phen the rest of the workflow can take as it is; and the check of an existing .phen.
#include <cmath>
#include <filesystem>

#include "engine_util.h"
#include "host_io.h"
#include "mps.h"
#include "phen_table.h"
#include "trailing_words.h"

using namespace host;

namespace {

const char *PREP_PHEN_USAGE = R"(
Match a trait table to the .fam, remove covariates from the traits and standardise them

usage: mps prep-phen <bfiles> <table> <out> <covar|NULL> [ordinal=<1-based,...>] [rint|rint=<offset>]

arguments:
    bfiles          stem of .bed, .bim, .fam fileset; only the .fam is read
    table           trait table: header FID IID <traits> (ids in either order, IID may be EID), NA for missing
    out             the .phen to write: one row per individual of the .fam, in its order; <out>.prep.tsv beside it
    covar           covariate table in the format of the trait table (at most 63 numeric columns), or NULL
    ordinal=...     1-based numbers of the traits that are ordinal: standardised only, never residualised
    rint            rank-based inverse normal transform of every trait that is not ordinal, behind the step above;
                    rint=<offset> sets the offset c of (rank - c) / (n + 1 - 2c), 0 <= c <= 0.5 (default 0.375, Blom)

Every trait is regressed on the covariates (with an intercept) over the individuals that have the trait and every covariate,
and the residuals are standardised to mean 0 and population standard deviation 1; without covariates, and for ordinal traits,
the values themselves are.  Individuals without the trait (or, for an adjusted trait, without a covariate) get NA.
With rint the ranks are taken on those standardised residuals as float32, the values the file would hold without it: ties
get their average rank, the normal scores are standardised again, and <out>.prep.tsv gains the columns rint_mean rint_sd.
)";

const char *CHECK_PHEN_USAGE = R"(
Check that a .phen has the rows of the .fam in its order and standardised traits

usage: mps check-phen <bfiles> <phen>

Exit status 1 when the row count or an IID differs from the .fam, or a trait has |mean| >= 0.1 or |sd - 1| >= 0.1.
)";

bool same_file(const std::string &a, const std::string &b)
{
    std::error_code ec;
    return a == b || (std::filesystem::equivalent(a, b, ec) && !ec);
}

AlignedPhen load_aligned(const std::string &path, const FamIds &fam)
{
    return align_phen_table(read_phen_table(path), &fam);
}

std::string fmt(double v)
{
    if (std::isnan(v)) return "NA";
    char b[64];
    std::snprintf(b, sizeof(b), "%.9g", v);
    return b;
}

}  // namespace

int host::cmd_prep_phen(int argc, char **argv)
{
    if (argc < 6)
    {
        std::cout << PREP_PHEN_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2], table_path = argv[3], out_path = argv[4], covar_path = argv[5];
    bool with_ordinal = false;
    std::string ordinal_arg;
    bool rint_word = false, rint_offset_word = false;
    std::string rint_arg;
    parse_trailing_words("prep-phen", argc, argv, 6,
                         {{"ordinal=", 0, &with_ordinal, &ordinal_arg},
                          {"rint", TrailingWord::kFree, &rint_word, nullptr},
                          {"rint=", TrailingWord::kFree, &rint_offset_word, &rint_arg}});
    if (rint_word && rint_offset_word) die("prep-phen: give rint or rint=<offset>, not both");
    const bool with_rint = rint_word || rint_offset_word;
    double rint_offset = 0.375;
    if (rint_offset_word)
    {
        const std::string tok = rint_arg.substr(5);
        char *end = nullptr;
        rint_offset = std::strtod(tok.c_str(), &end);
        if (tok.empty() || *end != '\0' || !(rint_offset >= 0.0 && rint_offset <= 0.5)) die("prep-phen: rint offset '" + tok + "' is not a number in [0, 0.5]");
    }
    const bool with_covar = covar_path != "NULL";
    const std::string fam_path = bfiles + ".fam";
    check_path(fam_path);
    check_path(table_path);
    if (with_covar) check_path(covar_path);
    if (same_file(out_path, table_path) || (with_covar && same_file(out_path, covar_path)) || same_file(out_path, fam_path))
        die("prep-phen: out names one of the inputs");
    PhaseTimer tm;

    const FamIds fam = read_fam_ids(fam_path);
    if (fam.n() == 0) die("empty .fam file");
    const AlignedPhen Y = load_aligned(table_path, fam);
    if (Y.p() == 0) die(table_path + " has no trait column");
    std::cout << "Traits: " << Y.p() << " columns; " << Y.matched << " of " << fam.n() << " individuals of the .fam found, "
              << Y.dropped << " rows of the table dropped." << std::endl;
    AlignedPhen X;
    if (with_covar)
    {
        X = load_aligned(covar_path, fam);
        if (X.p() == 0) die(covar_path + " has no covariate column");
        if (X.p() > CUSK_PHEN_MAX_COVAR) die("at most " + std::to_string(CUSK_PHEN_MAX_COVAR) + " covariates are supported, " + covar_path + " has " + std::to_string(X.p()));
        std::cout << "Covariates: " << X.p() << " columns; " << X.matched << " of " << fam.n() << " individuals of the .fam found, "
                  << X.dropped << " rows of the table dropped." << std::endl;
    }
    tm.mark("read and align tables");
    const size_t p = Y.p(), c = X.p(), N = fam.n();
    std::vector<unsigned char> adjust(p, with_covar ? 1 : 0), transform(p, with_rint ? 1 : 0);
    if (with_ordinal)
    {
        std::istringstream ss(ordinal_arg.substr(ordinal_arg.find('=') + 1));
        std::string tok;
        size_t listed = 0;
        while (std::getline(ss, tok, ','))
        {
            char *end = nullptr;
            const long v = std::strtol(tok.c_str(), &end, 10);
            if (tok.empty() || *end != '\0' || v < 1 || (size_t)v > p) die("prep-phen: ordinal trait number '" + tok + "' is not in 1 .. " + std::to_string(p));
            adjust[(size_t)v - 1] = 0;
            transform[(size_t)v - 1] = 0;
            ++listed;
        }
        if (listed == 0) die("prep-phen: ordinal= without trait numbers");
    }

    cusk_engine *e = open_engine();
    std::vector<float> out(p * N);
    std::vector<int> n(p), status(p);
    std::vector<double> mean(p), sd(p), r2(p), beta(p * (c + 1));
    const int rc = cusk_phen_adjust(e, Y.data.data(), with_covar ? X.data.data() : nullptr, N, p, c, adjust.data(), out.data(), n.data(),
                                    mean.data(), sd.data(), beta.data(), r2.data(), status.data());
    if (rc == CUSK_ERR_ARG)
    {
        std::string msg = cusk_last_error(e);
        const size_t at = msg.find("covariate ");
        if (at != std::string::npos)
        {  // the message counts columns; name the one meant
            const size_t j = (size_t)std::atoi(msg.c_str() + at + 10);
            if (j < c) msg += " (" + X.names[j] + ")";
        }
        cusk_engine_destroy(e);
        die("prep-phen: " + msg);
    }
    if (rc != CUSK_OK) engine_die("prep-phen", e);
    if (tm.on)
    {
        float ms[5];
        cusk_phen_timing(e, ms);
        std::cout << "[t] device: scaling " << ms[0] << " ms, gram " << ms[1] << " ms, solve " << ms[2] << " ms, moments " << ms[3]
                  << " ms, standardise " << ms[4] << " ms" << std::endl;
    }
    tm.mark("adjust and standardise (device, with copies)");
    std::string refused;
    for (size_t t = 0; t < p; t++)
        if (status[t] != CUSK_PHEN_OK)
            refused += "\n  " + Y.names[t] + ": " +
                       (status[t] == CUSK_PHEN_SINGULAR
                            ? "the covariates are collinear on the " + std::to_string(n[t]) + " individuals that have this trait"
                            : "too few individuals (" + std::to_string(n[t]) + ") or no variation");
    // the transform of what the file would hold without it; a trait refused above is already named
    std::vector<double> rint_mean(p), rint_sd(p);
    if (with_rint && refused.empty())
    {
        std::vector<float> scores(p * N);
        std::vector<int> rint_n(p), rint_status(p);
        if (cusk_phen_rint(e, out.data(), N, p, transform.data(), rint_offset, scores.data(), rint_n.data(), rint_mean.data(), rint_sd.data(),
                           rint_status.data(), nullptr) != CUSK_OK)
            engine_die("prep-phen", e);
        if (tm.on)
        {
            float ms[4];
            cusk_phen_rint_timing(e, ms);
            std::cout << "[t] device: rint keys " << ms[0] << " ms, sort " << ms[1] << " ms, ranks " << ms[2] << " ms, moments and standardise "
                      << ms[3] << " ms" << std::endl;
        }
        for (size_t t = 0; t < p; t++)
            if (rint_status[t] != CUSK_PHEN_OK)
                refused += "\n  " + Y.names[t] + ": too few individuals (" + std::to_string(rint_n[t]) + ") or no variation to rank";
        out.swap(scores);
        tm.mark("rank-based inverse normal transform (device, with copies)");
    }
    cusk_engine_destroy(e);
    if (!refused.empty()) die("prep-phen: nothing written; these traits cannot be prepared:" + refused);

    write_phen_file(out_path, fam, Y.names, out.data());
    CheckedTextFile rep(out_path + ".prep.tsv");
    std::string text = std::string("trait\tmode\tn\tmean\tsd\tr2") + (with_rint ? "\trint_mean\trint_sd" : "") + "\n";
    for (size_t t = 0; t < p; t++)
    {
        const std::string mode = adjust[t] ? (transform[t] ? "adjusted+rint" : "adjusted") : (transform[t] ? "rint" : "standardised");
        text += Y.names[t] + "\t" + mode + "\t" + std::to_string(n[t]) + "\t" + fmt(mean[t]) + "\t" + fmt(sd[t]) + "\t" + fmt(r2[t]);
        if (with_rint) text += "\t" + fmt(rint_mean[t]) + "\t" + fmt(rint_sd[t]);
        text += "\n";
    }
    rep.put(text);
    rep.close();
    tm.mark("write files");
    std::cout << "Wrote " << out_path << " and " << out_path << ".prep.tsv" << std::endl;
    std::cout << "Done." << std::endl;
    return 0;
}

int host::cmd_check_phen(int argc, char **argv)
{
    if (argc != 4)
    {
        std::cout << CHECK_PHEN_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2], phen_path = argv[3], fam_path = bfiles + ".fam";
    check_path(fam_path);
    check_path(phen_path);
    const FamIds fam = read_fam_ids(fam_path);
    if (fam.n() == 0) die("empty .fam file");
    const PhenTable table = read_phen_table(phen_path);
    const AlignedPhen Y = align_phen_table(table, &fam);
    if (Y.p() == 0) die(phen_path + " has no trait column");
    bool ok = true;
    if (table.n() != fam.n())
    {
        ok = false;
        std::cout << "rows: " << table.n() << " in " << phen_path << ", " << fam.n() << " in " << fam_path << std::endl;
    }
    else if (!Y.in_order)
    {
        ok = false;
        size_t i = 0;
        while (i < fam.n() && table.iid[i] == fam.iid[i]) i++;
        std::cout << "rows: IID " << table.iid[i] << " on data line " << i + 1 << " where the .fam has " << fam.iid[i] << std::endl;
    }
    // the moments of the rows as the file has them: a file in another order is reported for that, not for its values
    const AlignedPhen raw = align_phen_table(table, nullptr);
    const size_t p = raw.p(), N = raw.N;
    std::vector<int> n(p, 0);
    std::vector<double> mean(p, std::nan("")), sd(p, std::nan(""));
    if (N > 0)
    {
        cusk_engine *e = open_engine();
        if (cusk_phen_moments(e, raw.data.data(), N, p, n.data(), mean.data(), sd.data()) != CUSK_OK) engine_die("check-phen", e);
        cusk_engine_destroy(e);
    }
    for (size_t t = 0; t < p; t++)
        if (!(std::fabs(mean[t]) < 0.1 && std::fabs(sd[t] - 1.0) < 0.1))
        {
            ok = false;
            std::cout << "trait " << raw.names[t] << ": n " << n[t] << ", mean " << fmt(mean[t]) << ", sd " << fmt(sd[t]) << ": not standardised" << std::endl;
        }
    std::cout << (ok ? "check-phen: row-aligned and standardised." : "check-phen: FAILED.") << std::endl;
    return ok ? 0 : 1;
}
