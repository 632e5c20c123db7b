// corr_plan.h -- the tables of the batched correlation build (corr_build.hip: batch_mxp, batch_mxm) as functions of plain
// values: which blocks are accepted, the tiles of each phase and where the tables lie in the staging area.  No HIP, no
// engine state, so that the stand-alone program tools/corr_plan_selftest.cpp tabulates them under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace cusk {

constexpr int kMT = 64;  // markers per tile side of the SNP x SNP matrix kernels (the SNP x trait ones take 32)
struct CorrBatchBlock  // one LD block of a batch
{
    unsigned long long bed_row0;  // first marker of the block (row of the staged .bed; index into mean / sd)
    int m;                        // markers of the block
    int base;                     // first variable of the block in the batch allocation
    long long mxp_off;            // first marker of the block in the compact marker x trait output
};
struct CorrTile2 { int block, tile; };         // 32-marker tile of a block; the kernels read an int2
struct CorrTile4 { int block, bi, bj, pad; };  // tile (bi, bj), bi <= bj, of a block; the kernels read an int4

struct CorrBatchPlan
{
    std::vector<CorrBatchBlock> blocks;
    std::vector<CorrTile2> tiles2;  // phase one: the 32-marker tiles of every block, in block order
    std::vector<CorrTile4> tiles4;  // phase two: the upper triangle of kMT tiles of every kept block
    std::vector<int> kept;          // phase two: the kept blocks
    long long markers = 0;          // of all blocks: rows of the compact marker x trait output
    size_t o_tiles = 0, o_kept = 0, total = 0;  // staging area: blocks at 0, tiles, kept list; 16-byte aligned, 16 bytes of slack
    void write(char *h) const
    {
        std::memcpy(h, blocks.data(), sizeof(CorrBatchBlock) * blocks.size());
        if (!tiles2.empty()) std::memcpy(h + o_tiles, tiles2.data(), sizeof(CorrTile2) * tiles2.size());
        if (!tiles4.empty()) std::memcpy(h + o_tiles, tiles4.data(), sizeof(CorrTile4) * tiles4.size());
        if (!kept.empty()) std::memcpy(h + o_kept, kept.data(), sizeof(int) * kept.size());
    }
};

// phase 1: marker x trait (every block), phase 2: marker x marker (the blocks with keep[b] != 0; keep == nullptr: all).  -> false when a
// block has no markers or does not fit the n x n allocation with its p traits
inline bool corr_batch_plan(int phase, int nblk, const long long *first_marker, const int *markers, const int *base,
                            const unsigned char *keep, size_t p, size_t n, CorrBatchPlan &pl)
{
    pl = CorrBatchPlan();
    pl.blocks.resize((size_t)nblk);
    for (int b = 0; b < nblk; b++)
    {
        if (markers[b] <= 0 || base[b] < 0 || (size_t)base[b] + (size_t)markers[b] + p > n) return false;
        pl.blocks[(size_t)b] = CorrBatchBlock{(unsigned long long)first_marker[b], markers[b], base[b], pl.markers};
        pl.markers += markers[b];
    }
    for (int b = 0; b < nblk; b++)
    {
        for (int t = 0; phase == 1 && t < (markers[b] + 31) / 32; t++) pl.tiles2.push_back(CorrTile2{b, t});
        if (phase == 1 || (keep && !keep[b])) continue;
        pl.kept.push_back(b);
        const int tl = (markers[b] + kMT - 1) / kMT;
        for (int bi = 0; bi < tl; bi++)
            for (int bj = bi; bj < tl; bj++) pl.tiles4.push_back(CorrTile4{b, bi, bj, 0});
    }
    auto align16 = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
    pl.o_tiles = align16(sizeof(CorrBatchBlock) * pl.blocks.size());
    pl.o_kept = pl.o_tiles + align16(sizeof(CorrTile2) * pl.tiles2.size() + sizeof(CorrTile4) * pl.tiles4.size());
    pl.total = pl.o_kept + align16(sizeof(int) * pl.kept.size()) + 16;
    return true;
}

}  // namespace cusk
