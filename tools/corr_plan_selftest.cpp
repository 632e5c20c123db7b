// corr_plan_selftest.cpp -- the tables of the batched correlation build (csrc/host/corr_plan.h) tabulated against the
// rules as the build had them inline: which blocks are refused, the 32-marker tiles of phase one in block order, the upper
// triangle of 64-marker tiles per kept block of phase two, and a staging area whose tables start at 16-byte multiples and
// do not overlap.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/corr_plan_selftest.cpp -o corr_plan_selftest
//   ./corr_plan_selftest
#include "../ci-gwas_amd/csrc/host/corr_plan.h"

#include <cstdio>

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

static_assert(sizeof(CorrBatchBlock) == 24 && sizeof(CorrTile2) == 8 && sizeof(CorrTile4) == 16, "the kernels' table layouts");

constexpr int kBlocks = 8;
static const int kMarkers[kBlocks] = {1, 31, 32, 33, 63, 64, 65, 200};
static const size_t kTraits = 5;

// blocks at multiples of 64 variables, first markers that are no multiples of anything
static void layout(long long *first, int *base, size_t &n)
{
    int b = 0;
    long long f = 3;
    for (int k = 0; k < kBlocks; k++)
    {
        first[k] = f;
        base[k] = b;
        f += kMarkers[k] + 1;
        b = (b + kMarkers[k] + (int)kTraits + 63) / 64 * 64;
    }
    n = (size_t)b;
}

// offsets: 16-byte multiples, tables in order and disjoint, everything inside `total`; write() fills exactly those ranges
static void check_layout(const CorrBatchPlan &pl, int phase)
{
    const size_t b_blk = sizeof(CorrBatchBlock) * pl.blocks.size();
    const size_t b_t = phase == 1 ? sizeof(CorrTile2) * pl.tiles2.size() : sizeof(CorrTile4) * pl.tiles4.size();
    const size_t b_k = sizeof(int) * pl.kept.size();
    EXPECT(pl.o_tiles % 16 == 0 && pl.o_kept % 16 == 0);
    EXPECT(b_blk <= pl.o_tiles && pl.o_tiles + b_t <= pl.o_kept && pl.o_kept + b_k + 16 <= pl.total);
    EXPECT(pl.o_tiles < b_blk + 16 && pl.o_kept < pl.o_tiles + b_t + 16 && pl.total < pl.o_kept + b_k + 32);  // no more than the padding
    std::vector<char> h(pl.total, (char)0x5a);
    pl.write(h.data());
    EXPECT(std::memcmp(h.data(), pl.blocks.data(), b_blk) == 0);
    EXPECT(b_t == 0 || std::memcmp(h.data() + pl.o_tiles, phase == 1 ? (const void *)pl.tiles2.data() : (const void *)pl.tiles4.data(), b_t) == 0);
    EXPECT(b_k == 0 || std::memcmp(h.data() + pl.o_kept, pl.kept.data(), b_k) == 0);
    for (size_t i = b_blk; i < pl.o_tiles; i++) EXPECT(h[i] == (char)0x5a);
    for (size_t i = pl.o_tiles + b_t; i < pl.o_kept; i++) EXPECT(h[i] == (char)0x5a);
    for (size_t i = pl.o_kept + b_k; i < pl.total; i++) EXPECT(h[i] == (char)0x5a);
}

static void test_phase_one()
{
    long long first[kBlocks];
    int base[kBlocks];
    size_t n;
    layout(first, base, n);
    CorrBatchPlan pl;
    const unsigned char keep_none[kBlocks] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const unsigned char *keep : {(const unsigned char *)nullptr, keep_none})  // phase one builds every block, whatever is kept
    {
        EXPECT(corr_batch_plan(1, kBlocks, first, kMarkers, base, keep, kTraits, n, pl));
        EXPECT(pl.blocks.size() == (size_t)kBlocks && pl.tiles4.empty() && pl.kept.empty());
        long long moff = 0;
        size_t t = 0;
        for (int b = 0; b < kBlocks; b++)
        {
            const CorrBatchBlock &bb = pl.blocks[(size_t)b];
            EXPECT(bb.bed_row0 == (unsigned long long)first[b] && bb.m == kMarkers[b] && bb.base == base[b] && bb.mxp_off == moff);
            moff += kMarkers[b];
            const int want = (kMarkers[b] + 31) / 32;  // 1, 1, 1, 2, 2, 2, 3, 7
            for (int k = 0; k < want; k++, t++) EXPECT(t < pl.tiles2.size() && pl.tiles2[t].block == b && pl.tiles2[t].tile == k);
            EXPECT((want - 1) * 32 < kMarkers[b] && kMarkers[b] <= want * 32);
        }
        EXPECT(t == pl.tiles2.size() && t == 19 && pl.markers == moff && moff == 489);
        check_layout(pl, 1);
    }
}

static void test_phase_two()
{
    long long first[kBlocks];
    int base[kBlocks];
    size_t n;
    layout(first, base, n);
    const unsigned char keep_some[kBlocks] = {1, 0, 0, 1, 0, 1, 1, 1}, keep_none[kBlocks] = {0, 0, 0, 0, 0, 0, 0, 0},
                        keep_all[kBlocks] = {1, 1, 1, 1, 1, 1, 1, 9};
    const unsigned char *masks[4] = {nullptr, keep_all, keep_some, keep_none};
    const size_t want_tiles[4] = {1 + 1 + 1 + 1 + 1 + 1 + 3 + 10, 19, 1 + 1 + 1 + 3 + 10, 0};
    for (int k = 0; k < 4; k++)
    {
        CorrBatchPlan pl;
        EXPECT(corr_batch_plan(2, kBlocks, first, kMarkers, base, masks[k], kTraits, n, pl));
        EXPECT(pl.tiles2.empty() && pl.tiles4.size() == want_tiles[k] && pl.blocks.size() == (size_t)kBlocks && pl.markers == 489);
        size_t t = 0, kk = 0;
        for (int b = 0; b < kBlocks; b++)
        {
            if (masks[k] && !masks[k][b]) continue;
            EXPECT(kk < pl.kept.size() && pl.kept[kk] == b);
            kk++;
            const int tl = (kMarkers[b] + 63) / 64;  // 1 ... 1, 2 (65), 4 (200)
            for (int bi = 0; bi < tl; bi++)
                for (int bj = bi; bj < tl; bj++, t++)
                {
                    EXPECT(t < pl.tiles4.size());
                    if (t >= pl.tiles4.size()) continue;
                    const CorrTile4 &q = pl.tiles4[t];
                    EXPECT(q.block == b && q.bi == bi && q.bj == bj && q.pad == 0);
                }
        }
        EXPECT(t == pl.tiles4.size() && kk == pl.kept.size());
        EXPECT((k == 3) == pl.kept.empty());
        check_layout(pl, 2);
    }
}

static void test_refused_blocks()
{
    CorrBatchPlan pl;
    const long long first[2] = {0, 70};
    const int base[2] = {0, 128};
    const int ok[2] = {64, 59}, over[2] = {64, 60}, zero[2] = {64, 0}, neg[2] = {-3, 59};
    const int bad_base[2] = {-64, 128};
    for (int phase = 1; phase <= 2; phase++)
    {
        EXPECT(corr_batch_plan(phase, 2, first, ok, base, nullptr, 5, 192, pl));     // 128 + 59 + 5 = 192: the last variable fits
        EXPECT(!corr_batch_plan(phase, 2, first, over, base, nullptr, 5, 192, pl));  // one marker more overruns the allocation
        EXPECT(!corr_batch_plan(phase, 2, first, ok, base, nullptr, 6, 192, pl));    // and so does one trait more
        EXPECT(!corr_batch_plan(phase, 2, first, zero, base, nullptr, 5, 192, pl));
        EXPECT(!corr_batch_plan(phase, 2, first, neg, base, nullptr, 5, 192, pl));
        EXPECT(!corr_batch_plan(phase, 2, first, ok, bad_base, nullptr, 5, 192, pl));
    }
    const unsigned char drop_bad[2] = {1, 0};  // a refused block is refused even when it is not kept
    EXPECT(!corr_batch_plan(2, 2, first, over, base, drop_bad, 5, 192, pl));
}

int main()
{
    test_phase_one();
    test_phase_two();
    test_refused_blocks();
    if (failures)
    {
        std::printf("corr_plan_selftest: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("corr_plan_selftest: ok\n");
    return 0;
}
