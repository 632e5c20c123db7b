// blocking_selftest.cpp -- host side of `mps block` (csrc/host/blocking.h) under the host sanitizers: the window weights,
// the cut at strict minima and the window bisection, with a stand-in for the device smoothing that restates the kernel's
// loop and checks every index it forms.  Edge profiles (constant, monotone, saw-tooth, NaN, zeros, LD-like noise) from
// one marker up, at maximum block sizes below, at and far above the profile's length.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/blocking_selftest.cpp -o blocking_selftest
//   ./blocking_selftest
#include "../ci-gwas_amd/csrc/host/blocking.h"

#include <cstdio>
#include <limits>
#include <random>

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

static int smooth_calls = 0;
static std::vector<int> windows_seen;

// hanning_smooth_kernel of corr_banded.hip, one "thread" per centre
static std::vector<double> smooth_stand_in(const std::vector<float> &v, const std::vector<double> &w)
{
    const long long n = (long long)v.size();
    const int window = (int)w.size();
    smooth_calls++;
    windows_seen.push_back(window);
    EXPECT(n >= 1 && window >= 1);  // what cusk_hanning_smooth accepts
    EXPECT(window % 2 == 1);        // the bisection only asks for odd windows
    std::vector<double> out((size_t)n);
    const long long margin = window / 2;
    for (long long c = 0; c < n; c++)
    {
        double acc = 0.0;
        if (c >= margin && c < n - margin)
            for (int i = 0; i < window; i++) acc += w.at((size_t)i) * (double)v.at((size_t)(c - margin + i));
        out[(size_t)c] = acc;
    }
    return out;
}

static bool is_cover(const std::vector<ChrBlock> &b, size_t n)
{
    if (b.empty() || b.front().first != 0 || b.back().last != n - 1) return false;
    for (size_t k = 0; k < b.size(); k++)
    {
        if (b[k].first > b[k].last) return false;
        if (k + 1 < b.size() && b[k + 1].first != b[k].last + 1) return false;
    }
    return true;
}

static std::vector<float> profile(const char *kind, size_t n, std::mt19937 &rng)
{
    std::vector<float> v(n);
    const std::string k = kind;
    std::normal_distribution<float> noise(0.0f, 0.8f);
    for (size_t i = 0; i < n; i++)
    {
        if (k == "constant") v[i] = 7.5f;
        if (k == "increasing") v[i] = 1.0f + 0.25f * (float)i;
        if (k == "decreasing") v[i] = 1.0f + 0.25f * (float)(n - 1 - i);
        if (k == "sawtooth") v[i] = (i % 2) ? 3.0f : 1.0f;
        if (k == "zeros") v[i] = 0.0f;
        if (k == "noise" || k == "nan")
            v[i] = (20.0f + 10.0f * std::sin((float)i / 37.0f)) * ((i / 40) % 2 ? 0.4f : 1.0f) + noise(rng);
    }
    if (k == "nan")
        for (size_t i : {(size_t)0, n / 3, n / 2, n / 2 + 1, n - 1}) v[i] = std::numeric_limits<float>::quiet_NaN();
    return v;
}

int main()
{
    // weights: ends and middle of the window; window 1 is 0 / 0
    EXPECT(hanning_weights(0).empty() && hanning_weights(-3).empty());
    EXPECT(std::isnan(hanning_weights(1)[0]));
    {
        const std::vector<double> w = hanning_weights(3);
        EXPECT(w.size() == 3 && w[0] == 0.0 && w[1] == 1.0 && w[2] == 0.0);
        const std::vector<double> w5 = hanning_weights(5);
        EXPECT(w5[0] == 0.0 && w5[2] == 1.0 && w5[1] > 0.49 && w5[1] < 0.51 && w5[4] == 0.0);
        for (int window : {2, 4, 101, 333})
            for (double x : hanning_weights(window)) EXPECT(x >= 0.0 && x <= 1.0 && (double)(float)((0.5 - x) * 2.0) == (0.5 - x) * 2.0);
    }
    // cut at strict minima that follow a higher value
    {
        EXPECT(cut_at_minima({1.0}).size() == 1 && cut_at_minima({1.0, 2.0}).size() == 1);
        const std::vector<ChrBlock> b = cut_at_minima({0.0, 3.0, 1.0, 2.0, 2.0, 5.0, 4.0, 6.0, 0.0});
        EXPECT(b.size() == 3 && b[0].last == 2 && b[1].first == 3 && b[1].last == 6 && b[2].last == 8);
        const std::vector<ChrBlock> flat = cut_at_minima({0.0, 3.0, 1.0, 1.0, 3.0, 0.0});  // a flat bottom is cut at its last point
        EXPECT(flat.size() == 2 && flat[0].last == 3);
        EXPECT(cut_at_minima({0.0, 1.0, 2.0, 2.0, 3.0, 0.0}).size() == 1);  // a dip needs a higher value before it
        const double nan = std::numeric_limits<double>::quiet_NaN();
        EXPECT(cut_at_minima({nan, nan, nan, nan}).size() == 1);
        EXPECT(is_cover(cut_at_minima({0.0, 3.0, nan, 2.0, 1.0, 5.0, 0.0}), 7));
    }
    // the bisection over the edge profiles
    std::mt19937 rng(11);
    const char *kinds[] = {"constant", "increasing", "decreasing", "sawtooth", "zeros", "noise", "nan"};
    const size_t sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 100, 101, 301, 1000};
    int stalled = 0, within = 0;
    for (const char *kind : kinds)
        for (size_t n : sizes)
        {
            if (std::string(kind) == "nan" && n < 8) continue;  // five distinct NaN positions
            const std::vector<float> v = profile(kind, n, rng);
            for (int maxb : {1, (int)std::max<size_t>(2, n / 6), (int)(2 * n / 5), (int)(n / 2), (int)n, (int)n + 101})
            {
                if (maxb < 1) continue;
                smooth_calls = 0;
                windows_seen.clear();
                const std::vector<ChrBlock> b = blocks_of_chromosome(v, maxb, smooth_stand_in);
                EXPECT(is_cover(b, n));
                EXPECT(smooth_calls >= 1 && smooth_calls <= 40);  // a bisection over at most 2^31 windows
                for (int w : windows_seen) EXPECT(w >= (n >= 3 ? 3 : 1) && (size_t)w <= std::max<size_t>(n, 1));
                size_t largest = 0;
                for (const ChrBlock &x : b) largest = std::max(largest, x.size());
                const bool ok = std::abs((int)largest - maxb) <= 100 && (int)largest <= maxb;
                (ok ? within : stalled)++;
                const std::string k = kind;
                if (k == "constant" || k == "zeros" || n <= 3) EXPECT(b.size() == 1);
                std::printf("%-10s n=%-4zu max=%-4d windows=%-2d blocks=%zu largest=%zu %s:", kind, n, maxb, smooth_calls, b.size(),
                            largest, ok ? "tolerance" : "stalled");
                for (size_t q = 0; q < b.size() && q < 6; q++) std::printf(" %zu-%zu", b[q].first, b[q].last);
                std::printf(b.size() > 6 ? " ...\n" : "\n");
            }
        }
    EXPECT(stalled > 10 && within > 10);
    std::printf(failures ? "blocking_selftest: %d FAILED\n" : "blocking_selftest: ok\n", failures);
    return failures ? 1 : 0;
}
