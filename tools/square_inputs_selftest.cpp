// square_inputs_selftest.cpp -- the sample-size chain, its expansion to the square matrix and the ordinal overlay
// (csrc/host/square_inputs.h), and the trailing-word parser (csrc/host/trailing_words.h), under the host sanitizers.  Every
// function is checked against its rule restated for one cell at a time -- which inputs the cell comes from, through which
// chain -- and compared by bit pattern, NaNs included.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/square_inputs_selftest.cpp
//       ci-gwas_amd/csrc/host/sumstats_api.cpp -o square_inputs_selftest        (one command line)
#include "../ci-gwas_amd/csrc/host/square_inputs.h"
#include "../ci-gwas_amd/csrc/host/trailing_words.h"

#include <cstdio>
#include <cstring>
#include <sstream>

using namespace host;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }
static const float kNaN = std::numeric_limits<float>::quiet_NaN();

// ---- inputs of one case ----
struct Case
{
    const char *name;
    size_t k, p;
    std::vector<int> ix;  // ordinal traits
    bool corner;
    int special;  // 0 none, 1 NaN in mxp, 2 NaN in the upper triangle of pxp only, 3 counts of 3 or less, 4 NaN estimate
};

struct Inputs
{
    size_t k, p, q;
    std::vector<int> ix;
    std::vector<float> mxp, pxp, corner, mr, mse;
    std::vector<int> mxp_n, pxp_n;
    OrdinalTraitEstimates te;
    float uniform = 400.0f;
    int t_of(size_t trait) const
    {
        for (size_t t = 0; t < q; t++)
            if ((size_t)ix[t] == trait) return (int)t;
        return -1;
    }
};

static float unit(unsigned &s)  // in (-0.9, 0.9)
{
    s = s * 1664525u + 1013904223u;
    return ((float)(s >> 8) / (float)(1u << 24) - 0.5f) * 1.8f;
}

static Inputs make_inputs(const Case &c)
{
    Inputs in;
    in.k = c.k, in.p = c.p, in.q = c.ix.size(), in.ix = c.ix;
    const size_t k = c.k, p = c.p, q = in.q;
    unsigned s = 12345u + (unsigned)(k * 31 + p * 7 + q);
    in.mxp.resize(k * p), in.mxp_n.resize(k * p), in.pxp.resize(p * p), in.pxp_n.resize(p * p);
    for (size_t i = 0; i < k * p; i++) in.mxp[i] = unit(s), in.mxp_n[i] = 200 + (int)(i * 13 % 150);
    // the square as the device leaves it: the two triangles differ, so that reading the wrong one shows
    for (size_t i = 0; i < p * p; i++) in.pxp[i] = unit(s), in.pxp_n[i] = 150 + (int)(i * 17 % 200);
    for (size_t a = 0; a < p; a++) in.pxp[a * p + a] = 1.0f;
    if (c.corner)
    {
        in.corner.resize(k * k);
        for (size_t i = 0; i < k * k; i++) in.corner[i] = 300.0f + (float)(i * 5 % 90);
    }
    in.mr.resize(k * q), in.mse.resize(k * q);
    for (size_t i = 0; i < k * q; i++) in.mr[i] = unit(s), in.mse[i] = 0.02f + 0.05f * std::fabs(unit(s));
    // p x q, one value per unordered pair of ordinal traits (one fit per pair, mirrored), the own entry not set
    in.te.r.assign(p * q, kNaN), in.te.se.assign(p * q, kNaN);
    for (size_t a = 0; a < p; a++)
        for (size_t t = 0; t < q; t++)
        {
            const size_t o = (size_t)c.ix[t];
            if (a == o) continue;
            const int ta = in.t_of(a);
            if (ta >= 0 && a > o)
            {
                in.te.r[a * q + t] = in.te.r[o * q + (size_t)ta], in.te.se[a * q + t] = in.te.se[o * q + (size_t)ta];
                continue;
            }
            in.te.r[a * q + t] = unit(s), in.te.se[a * q + t] = 0.03f + 0.05f * std::fabs(unit(s));
        }
    if (c.special == 1) in.mxp[(k - 1) * p] = kNaN;
    if (c.special == 2) in.pxp[0 * p + 1] = kNaN, in.pxp[1 * p + 0] = 0.25f;
    if (c.special == 3)
        for (size_t i = 0; i < k * p; i++) in.mxp_n[i] = (int)(i % 4), in.pxp_n[i % (p * p)] = (int)((i + 1) % 4);
    if (c.special == 4) in.mr[0] = kNaN, in.te.r[(c.ix[0] == 0 ? 1 : 0) * q] = kNaN;
    return in;
}

// ---- the rules, one cell at a time ----
static float chain_count(float r, int count) { return std::isnan(r) ? kNaN : cusk_ess_from_se(r, cusk_se_from_count(r, count)); }
static float chain_se(float r, float se) { return std::isnan(r) ? kNaN : cusk_ess_from_se(r, se); }
static float se_of_count(float r, int count) { return std::isnan(r) ? kNaN : cusk_se_from_count(r, count); }

// r and se of the pair (variable v, variable w) of the square numbering, v != w, at least one a trait; overlay: with the
// ordinal estimates
static void pair_estimate(const Inputs &in, size_t v, size_t w, bool overlay, float &r, float &se)
{
    const size_t k = in.k, p = in.p, q = in.q;
    if (v > w) std::swap(v, w);  // now w is a trait
    const size_t b = w - k;
    if (v < k)
    {  // marker v, trait b
        const int t = overlay ? in.t_of(b) : -1;
        r = t >= 0 ? in.mr[v * q + (size_t)t] : in.mxp[v * p + b];
        se = t >= 0 ? in.mse[v * q + (size_t)t] : se_of_count(r, in.mxp_n[v * p + b]);
        return;
    }
    const size_t a = v - k;  // traits a < b: the upper triangle is what the loader reads
    const int tb = overlay ? in.t_of(b) : -1, ta = overlay ? in.t_of(a) : -1;
    if (tb >= 0)
        r = in.te.r[a * q + (size_t)tb], se = in.te.se[a * q + (size_t)tb];
    else if (ta >= 0)
        r = in.te.r[b * q + (size_t)ta], se = in.te.se[b * q + (size_t)ta];
    else
        r = in.pxp[a * p + b], se = se_of_count(r, in.pxp_n[a * p + b]);
}

static float expected_size(const Inputs &in, size_t v, size_t w, bool overlay)
{
    const size_t k = in.k, p = in.p;
    if (v < k && w < k) return in.corner.empty() ? in.uniform : in.corner[v * k + w];
    if (v == w) return kNaN;
    if (!overlay)
    {  // the count's chain, from the cell's own count
        const size_t lo = std::min(v, w), hi = std::max(v, w);
        return lo < k ? chain_count(in.mxp[lo * p + hi - k], in.mxp_n[lo * p + hi - k])
                      : chain_count(in.pxp[(lo - k) * p + hi - k], in.pxp_n[(lo - k) * p + hi - k]);
    }
    float r, se;
    pair_estimate(in, v, w, true, r, se);
    const bool ordinal = (v >= k && in.t_of(v - k) >= 0) || (w >= k && in.t_of(w - k) >= 0);
    return ordinal ? chain_se(r, se) : expected_size(in, v, w, false);
}

static void run_case(const Case &c)
{
    const Inputs in = make_inputs(c);
    const size_t k = in.k, p = in.p, q = in.q, n = k + p;
    int before = failures;

    // the chain and its expansion
    std::vector<float> mxp_ess, pxp_ess;
    block_sample_sizes(in.mxp.data(), in.mxp_n.data(), in.pxp.data(), in.pxp_n.data(), k, p, mxp_ess, pxp_ess);
    EXPECT(mxp_ess.size() == k * p && pxp_ess.size() == p * p);
    std::vector<float> ess = square_sample_sizes(mxp_ess, pxp_ess, k, p, in.uniform, c.corner ? in.corner.data() : nullptr);
    EXPECT(ess.size() == n * n);
    for (size_t v = 0; v < n; v++)
        for (size_t w = 0; w < n; w++) EXPECT(same_bits(ess[v * n + w], expected_size(in, v, w, false)));

    // the overlay, square layout
    std::vector<float> cross(q * n, -7.0f);
    visit_ordinal_pairs(in.ix, k, in.mr.data(), in.mse.data(), p, &in.te, OrdinalSquareSink(in.ix, k, p, cross.data(), ess.data()));
    for (size_t v = 0; v < n; v++)
        for (size_t w = 0; w < n; w++) EXPECT(same_bits(ess[v * n + w], expected_size(in, v, w, true)));
    for (size_t t = 0; t < q; t++)
        for (size_t v = 0; v < n; v++)
        {
            float r = 1.0f, se = 0.0f;
            if (v != k + (size_t)in.ix[t]) pair_estimate(in, v, k + (size_t)in.ix[t], true, r, se);
            EXPECT(same_bits(cross[t * n + v], r));
        }

    // the overlay, file layout: over the Pearson values and the counts' standard errors, all rows at once and in two chunks
    std::vector<float> fm[2], fms[2], fp[2], fps[2];
    for (int chunked = 0; chunked < 2; chunked++)
    {
        fm[chunked] = in.mxp, fp[chunked] = in.pxp;
        fms[chunked].resize(k * p), fps[chunked].assign(p * p, kNaN);
        for (size_t i = 0; i < k * p; i++) fms[chunked][i] = se_of_count(in.mxp[i], in.mxp_n[i]);
        for (size_t a = 0; a < p; a++)
            for (size_t b = 0; b < p; b++)
                if (a != b) fps[chunked][a * p + b] = se_of_count(in.pxp[a * p + b], in.pxp_n[a * p + b]);
        const size_t cut = chunked ? k / 2 : k;
        for (size_t c0 = 0; c0 < k; c0 += (c0 == 0 && cut ? cut : k))
        {
            const size_t rows = (c0 == 0 && cut ? cut : k - c0);
            visit_ordinal_pairs(in.ix, rows, in.mr.data() + c0 * q, in.mse.data() + c0 * q, p, c0 == 0 ? &in.te : nullptr,
                                OrdinalFileSink{fm[chunked].data() + c0 * p, fms[chunked].data() + c0 * p, fp[chunked].data(), fps[chunked].data(), p});
        }
    }
    for (size_t i = 0; i < k; i++)
        for (size_t b = 0; b < p; b++)
        {
            float r, se;
            pair_estimate(in, i, k + b, true, r, se);
            for (int ch = 0; ch < 2; ch++) EXPECT(same_bits(fm[ch][i * p + b], r) && same_bits(fms[ch][i * p + b], se));
        }
    for (size_t a = 0; a < p; a++)
        for (size_t b = 0; b < p; b++)
        {
            // a pair without an ordinal trait keeps what the square held in that very cell (the file holds both triangles)
            float r = in.pxp[a * p + b], se = a == b ? kNaN : se_of_count(r, in.pxp_n[a * p + b]);
            if (a != b && (in.t_of(a) >= 0 || in.t_of(b) >= 0)) pair_estimate(in, k + a, k + b, true, r, se);
            for (int ch = 0; ch < 2; ch++) EXPECT(same_bits(fp[ch][a * p + b], r) && same_bits(fps[ch][a * p + b], se));
        }

    // both layouts from the same estimates: every pair with an ordinal trait agrees, correlation and size
    for (size_t t = 0; t < q; t++)
    {
        const size_t o = (size_t)in.ix[t];
        for (size_t i = 0; i < k; i++)
        {
            EXPECT(same_bits(cross[t * n + i], fm[0][i * p + o]));
            EXPECT(same_bits(ess[i * n + k + o], size_from_se(fm[0][i * p + o], fms[0][i * p + o])));
            EXPECT(same_bits(ess[(k + o) * n + i], ess[i * n + k + o]));
        }
        for (size_t a = 0; a < p; a++)
        {
            if (a == o) continue;
            EXPECT(same_bits(cross[t * n + k + a], fp[0][a * p + o]) && same_bits(fp[0][a * p + o], fp[0][o * p + a]));
            EXPECT(same_bits(ess[(k + a) * n + k + o], size_from_se(fp[0][a * p + o], fps[0][a * p + o])));
            EXPECT(same_bits(ess[(k + o) * n + k + a], size_from_se(fp[0][o * p + a], fps[0][o * p + a])));
        }
    }
    if (failures != before) std::printf("  in case: %s\n", c.name);
}

static void test_square_inputs()
{
    const Case cases[] = {
        {"k=1 p=1", 1, 1, {}, false, 0},
        {"k=1 p=1, the trait ordinal (q = p)", 1, 1, {0}, false, 0},
        {"k=2 p=3", 2, 3, {}, false, 0},
        {"k=2 p=3, ordinal 3,1 in that order", 2, 3, {2, 0}, true, 0},
        {"k=3 p=2 q=1, first trait ordinal", 3, 2, {0}, false, 0},
        {"k=3 p=2 q=1, last trait ordinal", 3, 2, {1}, false, 0},
        {"q = p = 3: no continuous trait", 2, 3, {0, 1, 2}, false, 0},
        {"NaN correlation in mxp", 3, 2, {1}, false, 1},
        {"NaN in the upper triangle of pxp only", 2, 3, {2}, false, 2},
        {"NaN in the upper triangle of pxp only, no ordinal trait", 2, 3, {}, false, 2},
        {"marker-pair corner present", 3, 2, {0}, true, 0},
        {"marker-pair corner present, no ordinal trait", 3, 2, {}, true, 0},
        {"marker-pair corner absent", 3, 2, {}, false, 0},
        {"counts of 3 or less", 3, 2, {}, false, 3},
        {"counts of 3 or less, last trait ordinal", 3, 2, {1}, true, 3},
        {"NaN estimates", 3, 2, {1}, false, 4},
    };
    for (const Case &c : cases) run_case(c);
}

// ---- trailing words: what each command's parser does with a tail, as the commands behaved before they shared a parser ----
struct Tail
{
    const char *cmd, *tail;
    const char *words;     // accepted: the words that end up set, in the command's own order; refused: NULL
    const char *refused;   // the argument the message names
};

static const Tail kTails[] = {
    // mps cusk: het first, then filter / rows / markers in any order, each at most once
    {"cusk", "", "", nullptr},
    {"cusk", "het", "het", nullptr},
    {"cusk", "het filter", "het filter", nullptr},
    {"cusk", "het rows", "het rows", nullptr},
    {"cusk", "het markers", "het markers", nullptr},
    {"cusk", "het filter rows", "het filter rows", nullptr},
    {"cusk", "het rows filter", "het filter rows", nullptr},
    {"cusk", "het filter markers", "het filter markers", nullptr},
    {"cusk", "het markers filter", "het filter markers", nullptr},
    {"cusk", "het rows markers", "het rows markers", nullptr},
    {"cusk", "het markers rows", "het rows markers", nullptr},
    {"cusk", "het filter rows markers", "het filter rows markers", nullptr},
    {"cusk", "het filter markers rows", "het filter rows markers", nullptr},
    {"cusk", "het rows filter markers", "het filter rows markers", nullptr},
    {"cusk", "het rows markers filter", "het filter rows markers", nullptr},
    {"cusk", "het markers filter rows", "het filter rows markers", nullptr},
    {"cusk", "het markers rows filter", "het filter rows markers", nullptr},
    {"cusk", "het filter filter", nullptr, "filter"},
    {"cusk", "het rows filter rows", nullptr, "rows"},
    {"cusk", "het het", nullptr, "het"},
    {"cusk", "filter", nullptr, "filter"},
    {"cusk", "filter het", nullptr, "filter"},
    {"cusk", "markers het rows", nullptr, "markers"},
    {"cusk", "het se", nullptr, "se"},
    {"cusk", "het ordinal=1", nullptr, "ordinal=1"},
    {"cusk", "het filter rows markers x", nullptr, "x"},
    {"cusk", "het filter rows markers filter", nullptr, "filter"},
    // mps sumstats: se, then ordinal=...
    {"sumstats", "", "", nullptr},
    {"sumstats", "se", "se", nullptr},
    {"sumstats", "se ordinal=2", "se ordinal=2", nullptr},
    {"sumstats", "se ordinal=", "se ordinal=", nullptr},  // (the list is parsed later, with its own messages)
    {"sumstats", "ordinal=2", nullptr, "ordinal=2"},
    {"sumstats", "ordinal=2 se", nullptr, "ordinal=2"},
    {"sumstats", "se se", nullptr, "se"},
    {"sumstats", "se x", nullptr, "x"},
    {"sumstats", "se ordinal=2 x", nullptr, "x"},
    {"sumstats", "se ordinal=2 ordinal=3", nullptr, "ordinal=3"},
    {"sumstats", "het", nullptr, "het"},
    // mps cuskss-bed: het, then markers, then ordinal=... (which must be last)
    {"cuskss-bed", "", "", nullptr},
    {"cuskss-bed", "het", "het", nullptr},
    {"cuskss-bed", "het markers", "het markers", nullptr},
    {"cuskss-bed", "het ordinal=1", "het ordinal=1", nullptr},
    {"cuskss-bed", "het markers ordinal=1,3", "het markers ordinal=1,3", nullptr},
    {"cuskss-bed", "markers", nullptr, "markers"},
    {"cuskss-bed", "markers het", nullptr, "markers"},
    {"cuskss-bed", "ordinal=1", nullptr, "ordinal=1"},
    {"cuskss-bed", "het het", nullptr, "het"},
    {"cuskss-bed", "het markers markers", nullptr, "markers"},
    {"cuskss-bed", "het ordinal=1 markers", nullptr, "ordinal=1"},
    {"cuskss-bed", "het ordinal=1 ordinal=2", nullptr, "ordinal=1"},
    {"cuskss-bed", "het markers ordinal=1 x", nullptr, "ordinal=1"},
    {"cuskss-bed", "het markers x", nullptr, "x"},
    {"cuskss-bed", "het x ordinal=1", nullptr, "x"},
    {"cuskss-bed", "het filter", nullptr, "filter"},
};

static void test_trailing_words()
{
    for (const Tail &c : kTails)
    {
        std::vector<std::string> args{"mps", c.cmd, "positional"};
        std::istringstream ss(c.tail);
        for (std::string w; ss >> w;) args.push_back(w);
        std::vector<char *> argv;
        for (std::string &a : args) argv.push_back(&a[0]);
        const std::string cmd = c.cmd;
        bool het = true, filter = true, rows = true, markers = true, se = true, ordinal = true;  // (the parser clears them)
        std::string text, got, refused;
        try
        {
            if (cmd == "cusk")
            {
                parse_trailing_words("cusk", (int)argv.size(), argv.data(), 3,
                                     {{"het", 0, &het, nullptr},
                                      {"filter", TrailingWord::kAnywhere, &filter, nullptr},
                                      {"rows", TrailingWord::kAnywhere, &rows, nullptr},
                                      {"markers", TrailingWord::kAnywhere, &markers, nullptr}});
                got = std::string(het ? "het " : "") + (filter ? "filter " : "") + (rows ? "rows " : "") + (markers ? "markers " : "");
            }
            else if (cmd == "sumstats")
            {
                parse_trailing_words("sumstats", (int)argv.size(), argv.data(), 3, {{"se", 0, &se, nullptr}, {"ordinal=", 1, &ordinal, &text}});
                got = std::string(se ? "se " : "") + (ordinal ? text + " " : "");
            }
            else
            {
                parse_trailing_words("cuskss-bed", (int)argv.size(), argv.data(), 3,
                                     {{"het", 0, &het, nullptr}, {"markers", 1, &markers, nullptr}, {"ordinal=", TrailingWord::kLast, &ordinal, &text}});
                got = std::string(het ? "het " : "") + (markers ? "markers " : "") + (ordinal ? text + " " : "");
            }
            if (!got.empty()) got.pop_back();
        }
        catch (const Fatal &f)
        {
            refused = f.what();
        }
        const bool ok = c.words ? (refused.empty() && got == c.words) : (refused == cmd + ": unknown trailing argument " + c.refused);
        if (!ok) std::printf("  mps %s ... %s: got '%s', message '%s'\n", c.cmd, c.tail, got.c_str(), refused.c_str());
        EXPECT(ok);
    }
}

int main()
{
    test_square_inputs();
    test_trailing_words();
    if (failures) return 1;
    std::printf("square_inputs_selftest: ok\n");
    return 0;
}
