// marker_pairs.hip -- per-pair numbers of jointly observed individuals BETWEEN MARKERS, written as the marker x marker part
// of a sample-size matrix (cusk_marker_pair_sizes / cusk_marker_pair_sizes_batch of include/cusk_hip.h).
//
// cusk_ess_square gives every pair of markers the size n_uniform; the correlation of the pair was formed on the
// individuals for which neither marker is missing (.bed code 01).  This file computes that number for all pairs of k rows,
//   count(i, j) = #{individuals < N: code(i) != 01 and code(j) != 01},
// exactly, in integers, and stores (float)count -- exact below 2^24 -- over the k x k corner of the matrix.
//
// Two kernels.  marker_valid_pack_kernel turns every row into one validity bit per individual: a lane takes 16 bytes of
// the row (64 individuals), forms ~(lo & ~hi) on the even bits, squeezes the even bits together and stores one 64-bit
// word, zero from individual N on.  Rows of ceil(N / 4) bytes start at any byte; the loads are the aligned 16-byte loads of
// pair_count_kernel (pair_counts.hip): the two aligned chunks a lane's 16 row bytes lie in, shifted into place with
// v_alignbyte, and a chunk is only touched when it holds a byte of the row.  The packed rows are padded with zero words to a
// multiple of kMpSlab words, so the count kernel needs no guard along a row.
//
// marker_pair_count_kernel gives a workgroup of 256 threads one 64 x 64 tile of pairs (ti <= tj of one block; the tile's
// linear index is decoded on the device) and the whole loop over the individuals, so there are no atomics and nothing
// depends on the schedule.  Slabs of kMpSlab words of the 64 + 64 rows are staged in LDS word-major ([word][row], row
// stride 65 words: the stores of a 16-lane group then fall on distinct banks, the reads of a wave are 16 consecutive words
// or a broadcast); thread (tx, ty) keeps the 4 x 4 counters of rows ty + 16 u against rows tx + 16 v and adds
// popcount(a & b) per word.  The next slab travels from global memory to registers while this one is counted.  At the end
// the tile goes through LDS once more so that both the tile and its mirror image are stored along rows of the matrix; the
// two stores write the same float, which makes the matrix bitwise symmetric by construction (ess_symmetry_kernel).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cusk_internal.h"

namespace cusk {

constexpr int kMpTile = 64;   // pairs per side of a workgroup's tile
constexpr int kMpSlab = 16;   // 64-bit words of a row staged per step
constexpr int kMpLdsRow = 65; // stride (words) of one word index in LDS; also the stride (ints) of the result tile

// one block of markers: packed rows row0 .. row0 + m, its corner at out + out_off (leading dimension ld), tiles tile0 ..
// tile0 + T (T + 1) / 2 of the launch
struct MpBlock
{
    long long out_off;
    int row0, m, tile0, T;
};

template <int Q>
__device__ __forceinline__ void mp_shifted_chunk(const unsigned (&W)[8], unsigned b, unsigned (&o)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_alignbyte(W[Q + j + 1], W[Q + j], b);
}

// the 16 even bits of x, squeezed together
__device__ __forceinline__ unsigned mp_even_bits(unsigned x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    x = (x | (x >> 8)) & 0x0000ffffu;
    return x;
}

// bits[r * wp + c], c < wp: validity of individuals 64 c .. 64 c + 63 of row r (ix ? ix[r] : r of bed, rows of clb bytes);
// one thread per word, `groups` = ceil(N / 64) words carry individuals, the rest is padding
__global__ void __launch_bounds__(256) marker_valid_pack_kernel(const unsigned char *__restrict__ bed, const int *__restrict__ ix,
                                                                size_t clb, size_t rows, size_t N, size_t groups, size_t wp,
                                                                unsigned long long *__restrict__ bits)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= rows * wp) return;
    const size_t r = q / wp, c = q - r * wp;
    unsigned long long word = 0;
    if (c < groups)
    {
        const size_t src = ix ? (size_t)ix[r] : r;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(bed) + src * clb;
        const unsigned sh = (unsigned)(addr & 15u), qq = sh >> 2, b = sh & 3u;
        const uint4 *al = reinterpret_cast<const uint4 *>(addr - sh);  // aligned chunk c holds row bytes 16 c - sh .. + 15
        const size_t nal = (sh + clb + 15) / 16;                       // aligned chunks with a byte of the row in them
        // c < groups: row byte 16 c exists (64 c < N) and lies in aligned chunk c
        const uint4 lo = al[c];
        uint4 hi = make_uint4(0u, 0u, 0u, 0u);
        if (sh && c + 1 < nal) hi = al[c + 1];
        const unsigned W[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned o[4];
        switch (qq)
        {
        case 0: mp_shifted_chunk<0>(W, b, o); break;
        case 1: mp_shifted_chunk<1>(W, b, o); break;
        case 2: mp_shifted_chunk<2>(W, b, o); break;
        default: mp_shifted_chunk<3>(W, b, o); break;
        }
        unsigned h[4];
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = mp_even_bits(~o[j] | (o[j] >> 1));  // anything but 01 (missing)
        word = (unsigned long long)(h[0] | (h[1] << 16)) | ((unsigned long long)(h[2] | (h[3] << 16)) << 32);
        const size_t left = N - 64 * c;  // individuals from 64 c on: what lies beyond N (row padding, the next row) is dropped
        if (left < 64) word &= (1ull << left) - 1ull;
    }
    bits[q] = word;
}

// tile q of a triangle: tj = the largest t with t (t + 1) / 2 <= q, ti = q - tj (tj + 1) / 2 <= tj
__device__ __forceinline__ void mp_tile_of(int q, int &ti, int &tj)
{
    int t = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
    while ((long long)t * (t + 1) / 2 > q) t--;
    while ((long long)(t + 1) * (t + 2) / 2 <= q) t++;
    tj = t;
    ti = q - (int)((long long)t * (t + 1) / 2);
}

__global__ void __launch_bounds__(256) marker_pair_count_kernel(const unsigned long long *__restrict__ bits, size_t wp,
                                                                const MpBlock *__restrict__ blk, int nblk, size_t ld,
                                                                float *__restrict__ out)
{
    __shared__ unsigned long long lds[2 * kMpSlab * kMpLdsRow];  // A slab, B slab; afterwards the 64 x 65 result tile
    unsigned long long *sa = lds, *sb = lds + kMpSlab * kMpLdsRow;

    int b = 0;
    while (b + 1 < nblk && blk[b + 1].tile0 <= (int)blockIdx.x) b++;
    const MpBlock k = blk[b];
    int ti, tj;
    mp_tile_of((int)blockIdx.x - k.tile0, ti, tj);
    if (tj >= k.T) return;  // (never: the grid is the sum of the triangles)

    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    // staging: thread t brings words 4 (t & 3) .. + 3 of row t >> 2 of either operand
    const int lrow = t >> 2, lw = (t & 3) * 4;
    // (rows past the block's last one are counted on its last row and never stored)
    const int ra = min(ti * kMpTile + lrow, k.m - 1), rb = min(tj * kMpTile + lrow, k.m - 1);
    const uint4 *ga = reinterpret_cast<const uint4 *>(bits + (size_t)(k.row0 + ra) * wp + lw);
    const uint4 *gb = reinterpret_cast<const uint4 *>(bits + (size_t)(k.row0 + rb) * wp + lw);
    uint4 na[2] = {ga[0], ga[1]}, nb[2] = {gb[0], gb[1]};

    int acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) acc[u][v] = 0;

    const size_t slabs = wp / kMpSlab;
    for (size_t s = 0; s < slabs; s++)
    {
        __syncthreads();  // the previous slab has been counted
        sa[(lw + 0) * kMpLdsRow + lrow] = (unsigned long long)na[0].x | ((unsigned long long)na[0].y << 32);
        sa[(lw + 1) * kMpLdsRow + lrow] = (unsigned long long)na[0].z | ((unsigned long long)na[0].w << 32);
        sa[(lw + 2) * kMpLdsRow + lrow] = (unsigned long long)na[1].x | ((unsigned long long)na[1].y << 32);
        sa[(lw + 3) * kMpLdsRow + lrow] = (unsigned long long)na[1].z | ((unsigned long long)na[1].w << 32);
        sb[(lw + 0) * kMpLdsRow + lrow] = (unsigned long long)nb[0].x | ((unsigned long long)nb[0].y << 32);
        sb[(lw + 1) * kMpLdsRow + lrow] = (unsigned long long)nb[0].z | ((unsigned long long)nb[0].w << 32);
        sb[(lw + 2) * kMpLdsRow + lrow] = (unsigned long long)nb[1].x | ((unsigned long long)nb[1].y << 32);
        sb[(lw + 3) * kMpLdsRow + lrow] = (unsigned long long)nb[1].z | ((unsigned long long)nb[1].w << 32);
        __syncthreads();
        if (s + 1 < slabs)
        {
            const size_t o = (s + 1) * (kMpSlab / 2);  // uint4 = two words
            na[0] = ga[o];
            na[1] = ga[o + 1];
            nb[0] = gb[o];
            nb[1] = gb[o + 1];
        }
#pragma unroll 4
        for (int w = 0; w < kMpSlab; w++)
        {
            unsigned long long a[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) a[u] = sa[w * kMpLdsRow + ty + 16 * u];
#pragma unroll
            for (int v = 0; v < 4; v++) c[v] = sb[w * kMpLdsRow + tx + 16 * v];
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[u][v] += __popcll(a[u] & c[v]);
        }
    }

    // the tile through LDS: res[i][j], i = row of tile ti, j = row of tile tj
    __syncthreads();
    int *res = reinterpret_cast<int *>(lds);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) res[(ty + 16 * u) * kMpLdsRow + tx + 16 * v] = acc[u][v];
    __syncthreads();
    float *corner = out + k.out_off;
    const int i0 = ti * kMpTile, j0 = tj * kMpTile;
    const int col = t & 63, r0 = t >> 6;
    // rows i0 + r of the matrix, columns j0 .. + 63: a wave stores 64 consecutive floats
    if (j0 + col < k.m)
        for (int r = r0; r < kMpTile && i0 + r < k.m; r += 4)
            corner[(size_t)(i0 + r) * ld + (size_t)(j0 + col)] = (float)res[r * kMpLdsRow + col];
    // the mirror image: rows j0 + r, columns i0 .. + 63 (a tile on the diagonal has just written all of itself)
    if (ti != tj && i0 + col < k.m)
        for (int r = r0; r < kMpTile && j0 + r < k.m; r += 4)
            corner[(size_t)(j0 + r) * ld + (size_t)(i0 + col)] = (float)res[col * kMpLdsRow + r];
}

// rows: total marker rows (sum of the blocks' m); ix: nullptr = rows 0 .. rows - 1 of bed.  blocks: filled but for tile0 / T.
static int marker_pair_sizes_run(cusk_engine *e, const char *who, const unsigned char *bed, const int *ix, size_t rows, size_t m_total,
                                 size_t N, std::vector<MpBlock> &blocks, size_t ld, float *N_dev)
{
    const std::string name(who);
    if (N >= ((size_t)1 << 24))
        return fail(e, CUSK_ERR_ARG, name + ": counts are stored as float32, exact below 2^24: too many individuals");
    if (reinterpret_cast<uintptr_t>(N_dev) & 3u) return fail(e, CUSK_ERR_ARG, name + ": the matrix must be 4-byte aligned");
    if (m_total > (size_t)0x7fffffff || rows > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, name + ": marker indices are 32-bit: too many markers");
    if (ix)
        for (size_t i = 0; i < rows; i++)
            if (ix[i] < 0 || (size_t)ix[i] >= m_total)
                return fail(e, CUSK_ERR_ARG, name + ": marker indices must lie below the number of markers (entry " + std::to_string(i) + ")");
    long long tiles = 0;
    for (MpBlock &b : blocks)
    {
        b.T = (b.m + kMpTile - 1) / kMpTile;
        b.tile0 = (int)tiles;
        tiles += (long long)b.T * (b.T + 1) / 2;
        if (tiles > (long long)(1 << 24)) return fail(e, CUSK_ERR_ARG, name + ": too many markers for one launch");  // (sqrtf in mp_tile_of)
    }
    if (tiles == 0) return CUSK_OK;
    const size_t clb = (N + 3) / 4, groups = (N + 63) / 64, wp = (groups + kMpSlab - 1) / kMpSlab * kMpSlab;
    const size_t pack_blocks = (rows * wp + 255) / 256;
    if (pack_blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, name + ": too many markers for one launch");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;

    // the rows where the pack kernel reads them: a device-resident .bed in place (through the index list), host rows
    // packed and uploaded
    const unsigned char *bed_d = bed;
    const int *ix_d = nullptr;
    const size_t o_ix = (sizeof(MpBlock) * blocks.size() + 15) & ~(size_t)15;
    const bool on_dev = is_device_pointer(bed);
    CUSK_HIP(e, e->scratch_a.ensure(o_ix + (on_dev && ix ? sizeof(int) * rows : 0)));
    char *d = e->scratch_a.as<char>();
    CUSK_HIP(e, hipMemcpyAsync(d, blocks.data(), sizeof(MpBlock) * blocks.size(), hipMemcpyHostToDevice, s));
    std::vector<unsigned char> bed_h;
    if (on_dev)
    {
        if (ix)
        {
            CUSK_HIP(e, hipMemcpyAsync(d + o_ix, ix, sizeof(int) * rows, hipMemcpyHostToDevice, s));
            ix_d = reinterpret_cast<const int *>(d + o_ix);
        }
    }
    else
    {
        const unsigned char *src = bed;
        if (ix)
        {
            bed_h.resize(rows * clb);
            for (size_t i = 0; i < rows; i++) std::memcpy(&bed_h[i * clb], bed + (size_t)ix[i] * clb, clb);
            src = bed_h.data();
        }
        CUSK_HIP(e, e->bed_dev.ensure(rows * clb));
        CUSK_HIP(e, hipMemcpyAsync(e->bed_dev.p, src, rows * clb, hipMemcpyHostToDevice, s));
        bed_d = e->bed_dev.as<unsigned char>();
    }
    CUSK_HIP(e, e->mp_bits.ensure(sizeof(unsigned long long) * rows * wp));
    hipLaunchKernelGGL(marker_valid_pack_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, s, bed_d, ix_d, clb, rows, N, groups, wp,
                       e->mp_bits.as<unsigned long long>());
    CUSK_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(marker_pair_count_kernel, dim3((unsigned)tiles), dim3(256), 0, s, e->mp_bits.as<unsigned long long>(), wp,
                       reinterpret_cast<const MpBlock *>(d), (int)blocks.size(), ld, N_dev);
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipStreamSynchronize(s));  // written when this returns; bed_h and the scratch may go
    return CUSK_OK;
}

}  // namespace cusk

using namespace cusk;

extern "C" int cusk_marker_pair_sizes(cusk_engine *e, const unsigned char *bed, const int *marker_ix, size_t k, size_t m_total, size_t N,
                                      float *N_dev, size_t ld)
{
    if (!e || !bed || !N_dev || k == 0 || N == 0 || m_total < k || ld < k) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (k > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_marker_pair_sizes: too many markers");
    if (marker_ix)
        if (const int rc = check_marker_ix(e, marker_ix, k, m_total)) return rc;
    std::vector<MpBlock> blocks(1);
    blocks[0].out_off = 0;
    blocks[0].row0 = 0;
    blocks[0].m = (int)k;
    return marker_pair_sizes_run(e, "cusk_marker_pair_sizes", bed, marker_ix, k, m_total, N, blocks, ld, N_dev);
}

extern "C" int cusk_marker_pair_sizes_batch(cusk_engine *e, const unsigned char *bed, const int *marker_ix, size_t m_total, size_t N,
                                            int nblk, const int *m, const int *base, int n, float *N_dev)
{
    if (!e || !bed || !N_dev || !m || !base || nblk <= 0 || n <= 0 || N == 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    std::vector<MpBlock> blocks;
    size_t rows = 0;
    long long prev = 0;
    for (int b = 0; b < nblk; b++)
    {
        if (m[b] < 0 || (base[b] & 63) != 0 || (long long)base[b] < prev)
            return fail(e, CUSK_ERR_ARG, "cusk_marker_pair_sizes_batch: block bases must be ascending multiples of 64, the blocks disjoint");
        const long long end = (long long)base[b] + m[b];
        if (end > (long long)n) return fail(e, CUSK_ERR_ARG, "cusk_marker_pair_sizes_batch: a block reaches beyond the n x n allocation");
        if (m[b] > 0)
        {
            MpBlock k;
            k.out_off = (long long)base[b] * n + base[b];
            k.row0 = (int)rows;
            k.m = m[b];
            k.tile0 = k.T = 0;
            blocks.push_back(k);
        }
        rows += (size_t)m[b];
        if (rows > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_marker_pair_sizes_batch: too many markers");
        prev = end;
    }
    if (rows == 0) return CUSK_OK;
    if (!marker_ix && m_total < rows) return fail(e, CUSK_ERR_ARG, "bad arguments");
    return marker_pair_sizes_run(e, "cusk_marker_pair_sizes_batch", bed, marker_ix, rows, m_total, N, blocks, (size_t)n, N_dev);
}
