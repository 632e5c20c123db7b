// rint_selftest.cpp -- the integer arithmetic of cusk_phen_rint (csrc/rint_math.h, which the device kernels of phen_rint.hip
// compile from the same text) under the host sanitizers: the key map on special values, the bitonic network executed on
// the CPU in the shape the kernels run it (tiles sorted on their own, then per merge size the steps across tiles and the
// steps inside a tile) against std::sort, and rank2 from the two searches against a counting loop.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/rint_selftest.cpp -o rint_selftest
//   ./rint_selftest
#include "../ci-gwas_amd/csrc/rint_math.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace cusk::rintm;

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

static uint32_t key_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return rint_key(b);
}

// one tile: the steps j < tile of merge sizes k_lo .. k_hi, as rint_tile_kernel runs them (every pair of a step, then the next)
static void tile_steps(std::vector<uint32_t> &keys, size_t base, size_t tile, size_t k_lo, size_t k_hi)
{
    for (size_t k = k_lo; k <= k_hi; k <<= 1)
        for (size_t j = std::min(k, tile) / 2; j > 0; j >>= 1)
            for (size_t t = 0; t < tile / 2; t++)
            {
                const size_t i = rint_pair_low(t, j), q = rint_partner(i, j);
                EXPECT(i < q && q < tile);
                uint32_t &a = keys.at(base + i), &b = keys.at(base + q);
                if (rint_exchange(a, b, rint_ascending(base + i, k))) std::swap(a, b);
            }
}

// the host's launch sequence of phen_rint.hip over one row of npad keys
static void network_sort(std::vector<uint32_t> &keys, size_t tile)
{
    const size_t npad = keys.size();
    for (size_t b = 0; b < npad; b += tile) tile_steps(keys, b, tile, 2, tile);
    for (size_t k = 2 * tile; k <= npad; k <<= 1)
    {
        for (size_t j = k / 2; j >= tile; j >>= 1)
            for (size_t t = 0; t < npad / 2; t++)
            {
                const size_t i = rint_pair_low(t, j), q = rint_partner(i, j);
                EXPECT(i < q && q < npad);
                uint32_t &a = keys.at(i), &c = keys.at(q);
                if (rint_exchange(a, c, rint_ascending(i, k))) std::swap(a, c);
            }
        for (size_t b = 0; b < npad; b += tile) tile_steps(keys, b, tile, k, k);
    }
}

static void check_keys()
{
    const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
    // strictly ascending as floats
    const float v[] = {-FLT_MAX, -1.0f, -FLT_MIN, -2 * den, -den, 0.0f, den, 2 * den, FLT_MIN, 1.0f, std::nextafter(1.0f, 2.0f), FLT_MAX};
    const size_t n = sizeof(v) / sizeof(v[0]);
    for (size_t a = 0; a + 1 < n; a++) EXPECT(key_of(v[a]) < key_of(v[a + 1]));
    EXPECT(key_of(-0.0f) == key_of(0.0f));
    EXPECT(key_of(-den) < key_of(-0.0f) && key_of(-0.0f) < key_of(den));  // neighbours across zero
    EXPECT(key_of(FLT_MAX) == 0xFF7FFFFFu && key_of(FLT_MAX) < kMissingKey);
    EXPECT(key_of(-FLT_MAX) == 0x00800000u);
    EXPECT(key_of(inf) == kMissingKey && key_of(-inf) == kMissingKey);
    EXPECT(key_of(std::nanf("")) == kMissingKey && key_of(-std::nanf("")) == kMissingKey);
    uint32_t odd = 0xFFC12345u;  // a negative NaN with a payload
    EXPECT(rint_key(odd) == kMissingKey);
    // random pairs: the order of the keys is the order of the floats
    std::mt19937 rng(7);
    for (int it = 0; it < 200000; it++)
    {
        uint32_t ba = rng(), bb = rng();
        float a, b;
        std::memcpy(&a, &ba, 4);
        std::memcpy(&b, &bb, 4);
        if (!std::isfinite(a) || !std::isfinite(b)) continue;
        EXPECT((a < b) == (rint_key(ba) < rint_key(bb)) && (a == b) == (rint_key(ba) == rint_key(bb)));
    }
}

static void check_network()
{
    std::mt19937 rng(11);
    const size_t tile = 16;  // a stand-in for the tile of the kernels
    std::vector<size_t> sizes;
    for (size_t N = 1; N <= 300; N++) sizes.push_back(N);
    for (size_t N : {511u, 512u, 513u, 1023u, 1025u}) sizes.push_back(N);
    for (size_t N : sizes)
        for (int kind = 0; kind < 4; kind++)
        {
            const size_t npad = rint_npad(N, tile);
            EXPECT(npad >= N && npad >= tile && (npad & (npad - 1)) == 0 && (npad == tile || npad / 2 < N));
            std::vector<uint32_t> keys(npad, kMissingKey);
            for (size_t i = 0; i < N; i++)
                keys[i] = kind == 0 ? (uint32_t)rng() : kind == 1 ? (uint32_t)(rng() % 5) : kind == 2 ? (uint32_t)i : (uint32_t)(N - i);
            if (kind == 0 && N > 2) keys[N / 2] = kMissingKey;  // a missing value inside the row
            std::vector<uint32_t> want = keys;
            std::sort(want.begin(), want.end());
            network_sort(keys, tile);
            EXPECT(keys == want);
        }
    // the tile as large as the row, and a tile of two
    for (size_t tile2 : {2u, 64u})
    {
        std::vector<uint32_t> keys(64), want;
        for (auto &k : keys) k = rng() % 40;
        want = keys;
        std::sort(want.begin(), want.end());
        network_sort(keys, tile2);
        EXPECT(keys == want);
    }
}

static void check_ranks()
{
    std::mt19937 rng(13);
    for (uint32_t n : {0u, 1u, 2u, 3u, 17u, 64u, 257u})
        for (uint32_t distinct : {1u, 2u, 7u, 1000000u})
        {
            std::vector<uint32_t> v(n);
            for (auto &x : v) x = rng() % distinct + 5;
            std::vector<uint32_t> sorted = v;
            std::sort(sorted.begin(), sorted.end());
            sorted.resize(n + 3, kMissingKey);  // the padding behind the observed keys is never read as one of them
            for (uint32_t i = 0; i < n; i++)
            {
                uint32_t lo = 0, eq = 0;
                for (uint32_t j = 0; j < n; j++)
                {
                    lo += v[j] < v[i];
                    eq += v[j] == v[i];
                }
                const uint32_t lower = rint_lower(sorted.data(), n, v[i]);
                const uint32_t upper = lower + rint_upper(sorted.data() + lower, n - lower, v[i]);
                EXPECT(lower == lo && upper == lo + eq);
                EXPECT(upper == rint_upper(sorted.data(), n, v[i]));
                EXPECT(rint_rank2(lower, upper) == 2 * lo + eq + 1);
            }
            EXPECT(rint_lower(sorted.data(), n, 0) == 0 && rint_upper(sorted.data(), n, 0) == 0);
            EXPECT(rint_lower(sorted.data(), n, 0xFFFFFFF0u) == n && rint_upper(sorted.data(), n, 0xFFFFFFF0u) == n);
        }
    // the largest row: rank2 of the last of 2^31 - 1 distinct values is 2 n and fits 32 bits
    const uint32_t n = 0x7FFFFFFFu;
    EXPECT(rint_rank2(n - 1, n) == 2 * n);
    EXPECT(rint_trait_bytes(500000, 8192) == 4 * ((size_t)1 << 19) + 4 * 500000);
    EXPECT(rint_npad(n, 8192) == (size_t)1 << 31);
}

int main()
{
    check_keys();
    check_network();
    check_ranks();
    if (failures)
    {
        std::printf("rint_selftest: %d failures\n", failures);
        return 1;
    }
    std::printf("rint_selftest ok\n");
    return 0;
}
