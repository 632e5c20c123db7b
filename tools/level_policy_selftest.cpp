// level_policy_selftest.cpp -- the decisions of the level loop (csrc/host/level_policy.h) tabulated against the rules as
// the loop had them inline before they got names: the kernel of a (level, class), the classes that can hold work, what
// follows the read-back, the saturating binomial.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/level_policy_selftest.cpp -o level_policy_selftest
//   ./level_policy_selftest
#include "../ci-gwas_amd/csrc/host/level_policy.h"

#include <cstdio>
#include <initializer_list>

using namespace cusk;

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

// the engine's constants (cusk_internal.h, sweep_common.h), restated: this program includes no HIP header
constexpr int kNumClasses = 5, kVecMaxLevel = 9;
constexpr int kClassCap[kNumClasses] = {39, 63, 127, 191, 1 << 30};

// the if / else chain of the sweep launches as it stood in the loop, in its order (the mode is handed to the launchers and
// takes no part in the choice)
static SweepKind chain(int /*mode*/, bool het, int l, int c, bool use_pair, bool tmaj, bool use_fast, bool exact_only, bool vec,
                       bool validate, bool lds_fits)
{
    if (use_pair && !exact_only)
        return SweepKind::Pair;
    else if (tmaj && use_fast && !exact_only)
        return SweepKind::Tmaj;
    else if (use_fast && !exact_only && !het && vec && !validate && c < kNumClasses - 1 && lds_fits && l < kVecMaxLevel)
        return SweepKind::Vec;
    else if (use_fast && !exact_only)
        return SweepKind::Fast;
    else
        return SweepKind::Exact;
}

static SweepKind kind(bool het, int l, int c, bool use_pair, bool tmaj, bool use_fast, bool exact_only, bool vec, bool validate,
                      bool lds_fits = true)
{
    return sweep_kind(l, c, het, use_pair, tmaj, use_fast, exact_only, vec, validate, lds_fits, kNumClasses, kVecMaxLevel);
}

static void test_sweep_kind()
{
    int seen[5] = {0, 0, 0, 0, 0};
    for (int mode = 0; mode < 2; mode++)
        for (int het = 0; het < 2; het++)
            for (int l : {1, 2, 5, 7, 14})
                for (int c = 0; c < kNumClasses; c++)
                    for (int bits = 0; bits < 128; bits++)
                    {
                        const bool use_pair = bits & 1, tmaj = bits & 2, use_fast = bits & 4, exact_only = bits & 8, vec = bits & 16,
                                   validate = bits & 32, fits = bits & 64;
                        const SweepKind want = chain(mode, het, l, c, use_pair, tmaj, use_fast, exact_only, vec, validate, fits);
                        EXPECT(kind(het, l, c, use_pair, tmaj, use_fast, exact_only, vec, validate, fits) == want);
                        seen[(int)want]++;
                    }
    for (int k : seen) EXPECT(k > 0);
    // rows of the table by hand: (het, level, class, pair, tmaj, fast, exact_only, vec, validate)
    EXPECT(kind(false, 1, 0, true, false, false, false, true, false) == SweepKind::Pair);    // level 1, option rows = 0
    EXPECT(kind(false, 1, 0, true, false, false, true, true, false) == SweepKind::Exact);    // ... redone
    EXPECT(kind(false, 1, 2, false, false, false, false, true, false) == SweepKind::Exact);  // level 1 without the pair kernel
    EXPECT(kind(false, 2, 0, false, false, true, false, true, false) == SweepKind::Vec);
    EXPECT(kind(false, 5, 3, false, false, true, false, true, false) == SweepKind::Vec);
    EXPECT(kind(false, 5, 4, false, false, true, false, true, false) == SweepKind::Fast);  // the last class is never staged
    EXPECT(kind(false, 5, 0, false, false, true, false, true, false, false) == SweepKind::Fast);  // LDS carve too large
    EXPECT(kind(false, 5, 0, false, false, true, false, false, false) == SweepKind::Fast);  // vec = 0
    EXPECT(kind(false, 5, 0, false, false, true, false, true, true) == SweepKind::Fast);    // validate = 1
    EXPECT(kind(true, 5, 0, false, false, true, false, true, false) == SweepKind::Fast);    // a threshold per test
    EXPECT(kind(false, 14, 0, false, false, true, false, true, false) == SweepKind::Fast);  // l >= kVecMaxLevel
    EXPECT(kind(false, 7, 0, false, true, true, false, true, false) == SweepKind::Tmaj);
    EXPECT(kind(true, 14, 4, false, true, true, false, true, true) == SweepKind::Tmaj);
    EXPECT(kind(false, 7, 0, false, true, false, false, true, false) == SweepKind::Exact);  // fast = 0 wins over tmaj
    EXPECT(kind(false, 7, 0, false, true, true, true, true, false) == SweepKind::Exact);    // the redo of any level
    EXPECT(kind(true, 2, 1, false, false, false, false, true, false) == SweepKind::Exact);  // het without het_filter
}

static void test_classes()
{
    auto mask = [](bool known, const long long *nitems, int staged, int bound) {
        bool may[kNumClasses];
        const int nonempty = classes_with_work(known, nitems, staged, bound, kClassCap, kNumClasses, may);
        int m = 0, cnt = 0;
        for (int c = 0; c < kNumClasses; c++) m = m * 2 + may[c], cnt += may[c];
        EXPECT(cnt == nonempty);
        return m;
    };
    const long long none[kNumClasses] = {0, 0, 0, 0, 0};
    // every class staged but the last: a class can hold work when the bound reaches its smallest degree (bits: class 0 first)
    const struct { int bound, want; } full[] = {{0, 0b10000},   {39, 0b10000},  {40, 0b11000},  {63, 0b11000},  {64, 0b11100},
                                                {127, 0b11100}, {128, 0b11110}, {191, 0b11110}, {192, 0b11111}, {5000, 0b11111}};
    for (const auto &t : full) EXPECT(mask(false, none, kNumClasses - 1, t.bound) == t.want);
    // nothing staged (option max_staged_classes = 0): every row goes to the last class
    for (int bound : {0, 39, 40, 63, 64, 127, 128, 191, 192, 5000}) EXPECT(mask(false, none, 0, bound) == 0b00001);
    // two classes staged (the doubled LDS layout of the HET kernels stages fewer): rows beyond the second cap go to the last
    EXPECT(mask(false, none, 2, 39) == 0b10000);
    EXPECT(mask(false, none, 2, 63) == 0b11000);
    EXPECT(mask(false, none, 2, 64) == 0b11001);
    EXPECT(mask(false, none, 2, 192) == 0b11001);
    // the level's real counts, once the host has them, replace the bound
    const long long some[kNumClasses] = {0, 5, 0, 0, 2};
    EXPECT(mask(true, some, kNumClasses - 1, 5000) == 0b01001);
    EXPECT(mask(true, some, 0, 0) == 0b01001);
    EXPECT(mask(true, none, kNumClasses - 1, 5000) == 0);
}

static void test_read_back()
{
    auto is = [](ReadBack r, AfterReadBack what, int level) { return r.what == what && r.level == level; };
    // arguments: ended, last_ran, sharded, fast_pending, tmaj, queue_overflow, binom_overflow, item_overflow
    EXPECT(is(after_read_back(0, 5, false, true, false, false, false, false), AfterReadBack::Done, 5));  // every level ran
    EXPECT(is(after_read_back(4, 3, false, true, false, false, false, false), AfterReadBack::Done, 3));  // no row with > 4 neighbours
    EXPECT(is(after_read_back(1, 0, false, false, false, false, false, false), AfterReadBack::Done, 0));
    EXPECT(is(after_read_back(4, 3, false, true, false, true, false, false), AfterReadBack::RedoExact, 3));
    EXPECT(is(after_read_back(0, 3, false, true, false, true, false, false), AfterReadBack::RedoExact, 3));  // ... of the last level
    EXPECT(is(after_read_back(7, 6, false, true, true, true, false, false), AfterReadBack::ReplanTmaj, 6));
    EXPECT(is(after_read_back(4, 3, false, false, false, true, false, false), AfterReadBack::Done, 3));  // redone already, or exact
    EXPECT(is(after_read_back(2, 1, false, true, false, true, false, false), AfterReadBack::Done, 1));   // level 1 has no queue
    EXPECT(is(after_read_back(3, 2, false, true, false, false, false, true), AfterReadBack::GrowItems, 3));
    EXPECT(is(after_read_back(3, 2, false, true, false, false, true, false), AfterReadBack::BinomOverflow, 3));
    EXPECT(is(after_read_back(3, 2, false, true, false, false, true, true), AfterReadBack::BinomOverflow, 3));
    EXPECT(is(after_read_back(3, 2, false, true, false, true, true, true), AfterReadBack::RedoExact, 2));  // the overflowed queue first
    EXPECT(is(after_read_back(0, 3, false, true, false, false, true, true), AfterReadBack::Done, 3));  // flags of level 0 mean nothing
    // a row-sharded run never redoes after the read-back (it finished the level on the exact path before its exchange)
    EXPECT(is(after_read_back(4, 3, true, true, false, true, false, false), AfterReadBack::Done, 3));
    EXPECT(is(after_read_back(0, 3, true, true, true, true, false, false), AfterReadBack::Done, 3));
    EXPECT(is(after_read_back(3, 2, true, true, false, true, false, true), AfterReadBack::GrowItems, 3));
    EXPECT(is(after_read_back(3, 2, true, true, false, true, true, false), AfterReadBack::BinomOverflow, 3));
}

static void test_binom()
{
    const unsigned long long cap = 1ull << 62;
    EXPECT(binom_sat(5, 2) == 10 && binom_sat(10, 0) == 1 && binom_sat(10, 10) == 1);
    EXPECT(binom_sat(3, 5) == 0 && binom_sat(3, -1) == 0);
    EXPECT(binom_sat(39, 14) == 15084504396ull && binom_sat(63, 14) == 37387265592825ull);
    EXPECT(binom_sat(127, 8) == 1340346236625ull && binom_sat(191, 11) == 230566421070146343ull);
    EXPECT(binom_sat(191, 180) == binom_sat(191, 11));
    // at saturation: the cap itself, never a wrapped product
    EXPECT(binom_sat(1000, 14) == cap && binom_sat(100, 50) == cap && binom_sat(1023, 15) == cap);
    EXPECT(binom_sat(2147483647, 15) == cap && binom_sat(2147483647, 2147483647 - 15) == cap);
    for (int n = 0; n < 1024; n++)
        for (int k = 0; k < 16; k++) EXPECT(binom_sat(n, k) <= cap && (n == 0 || binom_sat(n, k) >= binom_sat(n - 1, k)));
    // the uniform-size threshold: alpha/2 quantile over sqrt(N - l - 3) while the float sum of (int)N stays exact
    EXPECT(uniform_ess_threshold(3.0f, 103.0f, 0) == 0.3f);
    EXPECT(uniform_ess_threshold(3.0f, 117.9f, 14) == 0.3f);
}

int main()
{
    test_sweep_kind();
    test_classes();
    test_read_back();
    test_binom();
    std::printf(failures ? "level_policy_selftest: %d FAILED\n" : "level_policy_selftest: ok\n", failures);
    return failures ? 1 : 0;
}
