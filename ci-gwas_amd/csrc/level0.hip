// level0.hip -- level 0: the adjacency bitmap from the correlations alone (single matrix, batched block-diagonal form).
// Replaces the reference's cal_Indepl0 (cusk/src/cuPC-S.cu:458-484) and its hetcor twin (src/hetcor-cuPC-S.cu).
#include <cmath>

#include "ci_exact.h"
#include "ci_fast.h"
#include "sweep_common.h"

namespace cusk {

// ---------------------------------------------------------------------------
// level 0
// ---------------------------------------------------------------------------

// adjacency bitmap <- complete graph without self loops (Skeleton) or the caller's G (hetcor)
__global__ void init_bits_kernel(unsigned long long *adj, const int *Ginit, int n, int words)
{
    const int row = blockIdx.x;
    for (int w = threadIdx.x; w < words; w += blockDim.x)
    {
        unsigned long long bits = 0;
        const int base = w * 64;
        if (Ginit == nullptr)
        {
            int valid = n - base;
            bits = (valid >= 64) ? ~0ull : ((1ull << valid) - 1ull);
        }
        else
        {
            for (int b = 0; b < 64 && base + b < n; b++)
                if (Ginit[(size_t)row * n + base + b] == 1) bits |= (1ull << b);
        }
        if (row >= base && row < base + 64) bits &= ~(1ull << (row - base));
        adj[(size_t)row * words + w] = bits;
    }
}

// One 64x64 tile of the upper triangle per workgroup (4 waves x 16 rows, lane = column):
// coalesced 256-byte row segments in, wavefront ballots out (one 64-bit adjacency word per
// tile row, plus the mirrored word through LDS).  The mirrored tile is loaded as well so that
// level 0 also answers "is C bitwise symmetric?" (level 1 then reads only the upper triangle).
// Without per-pair sample sizes the level-0 verdict z(|c|) < th is a comparison of |c| with tanh(th): outside
// a guard band around that value (c_lo, c_hi from the host, +-5e-4 relative, far above the fp32 error of the
// reference's Fisher z) two compares settle the element, inside it (and for NaN or |c| > 1, where the reference's
// formula is not monotone) the reference's arithmetic decides.  All 16 rows of a wave are requested before the
// first is evaluated.
template <bool ESS, bool SYMCHECK>
__global__ void __launch_bounds__(256) level0_kernel(const float *__restrict__ C, const float *__restrict__ N,
                                                      unsigned long long *adj, int n, int words, float th, float c_lo,
                                                      float c_hi, int tiles, int *asym_flag)
{
    __shared__ unsigned long long s_col[64];
    __shared__ float s_t[64][65];
    int t = blockIdx.x, bi = 0;
    {
        int rem = t, len = tiles;
        while (rem >= len)
        {
            rem -= len;
            len--;
            bi++;
        }
        t = bi + rem;
    }
    const int bj = t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 64) s_col[threadIdx.x] = 0ull;
    if constexpr (SYMCHECK)
    {
        for (int rr = 0; rr < 16; rr++)
        {
            const int r = wave * 16 + rr;
            const int jr = bj * 64 + r, ic = bi * 64 + lane;
            s_t[r][lane] = (jr < n && ic < n) ? C[(size_t)jr * n + ic] : 0.0f;
        }
    }
    __syncthreads();
    const int j = bj * 64 + lane;
    float cv[16];
    [[maybe_unused]] float nv[16];
#pragma unroll
    for (int rr = 0; rr < 16; rr++)
    {
        const int i = bi * 64 + wave * 16 + rr;
        const bool in = (i < n && j < n && i < j);
        cv[rr] = in ? C[(size_t)i * n + j] : 0.0f;
        if constexpr (ESS) nv[rr] = in ? N[(size_t)i * n + j] : 4.0f;
    }
    unsigned long long colbits = 0ull;
    bool asym = false;
#pragma unroll
    for (int rr = 0; rr < 16; rr++)
    {
        const int r = wave * 16 + rr;
        const int i = bi * 64 + r;
        bool rm = false;
        if (i < n && j < n && i < j)
        {
            const float c = cv[rr];
            if constexpr (SYMCHECK)
            {
                const float ct = s_t[lane][r];
                asym |= (__float_as_uint(c) != __float_as_uint(ct)) && !((c != c) && (ct != ct));
            }
            if constexpr (ESS)
            {
                // per-pair threshold th / sqrt(N_ij - 3): a single-precision estimate of z sqrt(N_ij - 3) settles the
                // element unless it falls within 1e-3 of th (or the threshold is too small for that band, or an
                // operand is unusual); only then the reference's double-precision threshold and Fisher z are formed
                const float nm3 = nv[rr] - 3.0f;
                const float ac = fabsf(c);
                int fastv = 2;
                if (nm3 > 0.0f && nm3 < 3.0e38f && ac < 1.0f && th * __frsqrt_rn(nm3) >= kThMinFilter)
                {
                    const float sest = 0.5f * fabsf(__logf((1.0f + ac) / (1.0f - ac))) * __fsqrt_rn(nm3);
                    if (sest < th * (1.0f - 1e-3f))
                        fastv = 1;
                    else if (sest > th * (1.0f + 1e-3f))
                        fastv = 0;
                }
                if (fastv == 2)
                {
                    const float lth = (float)((double)th / sqrt((double)nv[rr] - 3.0));
                    rm = z_below<false>(c, lth);
                }
                else
                    rm = (fastv == 1);
            }
            else
            {
                const float ac = fabsf(c);
                if (ac < c_lo)
                    rm = true;
                else if (ac > c_hi && ac <= 1.0f)
                    rm = false;
                else
                    rm = z_below<false>(c, th);
            }
        }
        const unsigned long long m = __ballot(rm);
        if (lane == 0 && m != 0ull) atomicAnd(&adj[(size_t)i * words + bj], ~m);
        if (rm) colbits |= (1ull << r);
    }
    if constexpr (SYMCHECK)
    {
        if (__ballot(asym) != 0ull && lane == 0) *asym_flag = 1;
    }
    if (colbits) atomicOr(&s_col[lane], colbits);
    __syncthreads();
    if (threadIdx.x < 64)
    {
        const unsigned long long m = s_col[threadIdx.x];
        const int jj = bj * 64 + threadIdx.x;
        if (m != 0ull && jj < n) atomicAnd(&adj[(size_t)jj * words + bi], ~m);
    }
}

// Wide-tile form for the common case (one threshold, symmetry not checked): 64 rows x 256 columns per workgroup,
// so every row contributes a contiguous 1 KB to the stream instead of 256 B (DRAM pages are opened for a useful
// amount of data).  Lane l of a wave takes columns l, l+64, l+128, l+192 of its 16 rows: four coalesced 256-byte
// loads per row whose ballots are directly the four bitmap words; the mirrored words go through LDS.
constexpr int kL0Cols = 256;

// The tile in a fifth of the instructions of its first form (round 3).  That form spent ~3,900 instructions per wave on
// its 64 elements (PMC: 1,950 vector + 2,000 scalar; the launch was bound by instruction issue at 2.3 TB/s, not by the
// stream): per element a conditional single-lane store with its own address, the word-ownership logic, a need-bit.  Here an
// element costs a compare (its ballot IS the bitmap word), three instructions that park the word in lane 4 rr + q, two
// for the mirrored bit and three for "does anything of this lane need the exact comparison": the 64 words
// of the wave leave in ONE store instruction (lane L owns word (rr, q) = (L / 4, L % 4), ownership logic evaluated
// once per lane), and the exact pass -- entered by about one wave in 250 -- walks the flagged lanes' elements again.
// EDGE = the tile touches the diagonal or the matrix border (index clamps and per-element validity); interior tiles
// (nine in ten) run without either.
template <bool EDGE>
__device__ __forceinline__ void level0_tile(const float *__restrict__ C, unsigned long long *adj, int n, int words, float th,
                                            float c_lo, float c_hi, int bi, int bj, int complete_graph,
                                            unsigned long long *s_col)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = bi * 64 + wave * 16, j0 = bj * kL0Cols + lane;
    float cv[16][4];
    if constexpr (EDGE)
    {
#pragma unroll
        for (int rr = 0; rr < 16; rr++)
        {
            const size_t ro = (size_t)min(i0 + rr, n - 1) * n;
#pragma unroll
            for (int q = 0; q < 4; q++) cv[rr][q] = C[ro + min(j0 + q * 64, n - 1)];
        }
    }
    else
    {
        const float *base = C + (size_t)i0 * n + j0;
#pragma unroll
        for (int rr = 0; rr < 16; rr++)
#pragma unroll
            for (int q = 0; q < 4; q++) cv[rr][q] = base[(size_t)rr * n + q * 64];
    }
    // |c| within (slightly more than) the guard band <=> | |c| - mid | <= hw: the lane keeps the smallest such distance and
    // the largest |c| it saw (|c| > 1 is where the reference's formula is not monotone) and is "flagged" by either -- a
    // superset of the elements the exact pass decides (it applies the band test itself again, element by
    // element).  NaN is never flagged: it fails `|c| < c_lo` here and every comparison of the exact form, so the edge
    // stays either way.  (The accumulations are kept dependent chains by empty asm statements: OR-ing 64 independent
    // terms lets the compiler build a tree at the end, which keeps all 64 ballots alive -- 700 scalar-register spills.)
    const float mid = 0.5f * (c_lo + c_hi), hw = (c_hi - c_lo) * 0.51f + 1e-30f;
    float dmin = 3.0e38f, amax = 0.0f;
    unsigned wlo = 0u, whi = 0u;
    unsigned cb[4] = {0u, 0u, 0u, 0u};  // bit 15 - rr: element (rr, q) of this lane's column goes
#pragma unroll
    for (int rr = 0; rr < 16; rr++)
    {
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
            const float ac = fabsf(cv[rr][q]);
            bool rm = ac < c_lo;
            if constexpr (EDGE)
            {
                const int i = i0 + rr, j = j0 + q * 64;
                rm = rm && (i < n && j < n && i < j);
            }
            const unsigned long long m = __ballot(rm);
            const bool mine = lane == rr * 4 + q;
            wlo = mine ? (unsigned)m : wlo;
            whi = mine ? (unsigned)(m >> 32) : whi;
            cb[q] = (cb[q] << 1) | (rm ? 1u : 0u);
            asm volatile("" : "+v"(cb[q]), "+v"(wlo), "+v"(whi));  // (opaque: chains stay chains, element by element)
            dmin = fminf(dmin, fabsf(ac - mid));
            amax = fmaxf(amax, ac);
        }
        asm volatile("" : "+v"(dmin), "+v"(amax));
    }
    {
        // Every bitmap word has one owner except those that straddle the diagonal: word (row, w) with w > row / 64 is
        // decided entirely here (plain store of the complete word), w < row / 64 entirely by a mirrored tile; only
        // w == row / 64 collects bits from both sides and needs the atomic.  (With a caller-supplied starting graph
        // the words are not all ones: atomics throughout.)
        const int i = i0 + (lane >> 2), w = bj * 4 + (lane & 3);
        const unsigned long long m = ((unsigned long long)whi << 32) | wlo;
        if (m != 0ull)  // (EDGE: m is empty for rows and columns outside the matrix)
        {
            unsigned long long *dst = &adj[(size_t)i * words + w];
            if (complete_graph && w != (i >> 6))
            {
                const int nv = n - w * 64;
                *dst = ((nv >= 64) ? ~0ull : ((1ull << nv) - 1ull)) & ~m;
            }
            else
                atomicAnd(dst, ~m);
        }
    }
    const bool flagged = (dmin <= hw) || (amax > 1.0f);
    if (__ballot(flagged) != 0ull)
    {
        // exact pass (uniform branch, a fraction of a percent of the waves on unrelated markers, more along the diagonal
        // of an LD block where |c| reaches 1 + 1 ulp): which of the 64 elements -- still in registers -- need the
        // reference's arithmetic, then only those are decided, in one rolled loop
        unsigned need_lo = 0u, need_hi = 0u;  // bit rr * 4 + q
        [[maybe_unused]] int j0s = j0;
        asm volatile("" : "+v"(j0s));  // (likewise: the validity masks of the fast pass are not kept either)
#pragma unroll
        for (int rr = 0; rr < 16; rr++)
        {
#pragma unroll
            for (int q = 0; q < 4; q++)
            {
                float cq = cv[rr][q];
                asm volatile("" : "+v"(cq));  // (a value of its own: the fast pass's 64 compare masks are not kept for this)
                const float ac = fabsf(cq);
                bool need = !(ac < c_lo) && !(ac > c_hi && ac <= 1.0f);  // in the band, |c| > 1, NaN
                if constexpr (EDGE)
                {
                    const int i = i0 + rr, j = j0s + q * 64;
                    need = need && (i < n && j < n && i < j);
                }
                if (rr * 4 + q < 32)
                    need_lo |= need ? (1u << ((rr * 4 + q) & 31)) : 0u;
                else
                    need_hi |= need ? (1u << ((rr * 4 + q) & 31)) : 0u;
                asm volatile("" : "+v"(need_lo), "+v"(need_hi));
            }
        }
        // this wave's plain stores above are performed before the read-modify-writes below touch the same words
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        unsigned long long nm = ((unsigned long long)need_hi << 32) | need_lo;
        while (nm != 0ull)
        {
            const int e = __builtin_ctzll(nm);
            nm &= nm - 1ull;
            const int rr = e >> 2, q = e & 3;
            const int i = i0 + rr, j = j0 + q * 64;
            const float c = C[(size_t)i * n + j];
            if (z_below<false>(c, th))
            {
                atomicAnd(&adj[(size_t)i * words + bj * 4 + q], ~(1ull << lane));  // j % 64 == lane
                atomicOr(&s_col[q * 64 + lane], 1ull << (wave * 16 + rr));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (cb[q]) atomicOr(&s_col[q * 64 + lane], (unsigned long long)(__brev(cb[q]) >> 16) << (wave * 16));
}

__global__ void __launch_bounds__(256) level0_wide2_kernel(const float *__restrict__ C, unsigned long long *adj, int n, int words,
                                                            float th, float c_lo, float c_hi, int col_tiles, int complete_graph)
{
    __shared__ unsigned long long s_col[kL0Cols];
    // tile (bi, bj): rows [64 bi, +64), columns [256 bj, +256); only tiles that reach right of the diagonal
    int bi = 0, t = blockIdx.x;
    for (;;)
    {
        // row block bi has col_tiles - (bi / 4) column tiles (its first one contains the diagonal)
        const int len = col_tiles - (bi >> 2);
        if (t < len) break;
        t -= len;
        bi++;
    }
    const int bj = (bi >> 2) + t;
    s_col[threadIdx.x] = 0ull;
    __syncthreads();
    const bool interior = (bj * kL0Cols > bi * 64 + 63) && (bi * 64 + 64 <= n) && (bj * kL0Cols + kL0Cols <= n);
    if (interior)
        level0_tile<false>(C, adj, n, words, th, c_lo, c_hi, bi, bj, complete_graph, s_col);
    else
        level0_tile<true>(C, adj, n, words, th, c_lo, c_hi, bi, bj, complete_graph, s_col);
    __syncthreads();
    {
        const unsigned long long m = s_col[threadIdx.x];
        const int jj = bj * kL0Cols + threadIdx.x;
        if (m != 0ull && jj < n)
        {
            unsigned long long *dst = &adj[(size_t)jj * words + bi];
            if (complete_graph && bi != (jj >> 6))
                *dst = ~m;  // all 64 rows of block bi lie above row jj and exist
            else
                atomicAnd(dst, ~m);
        }
    }
}

hipError_t launch_level0(const float *C, const float *Ness, const int *Ginit, unsigned long long *adj, int n, int words,
                         float th, int *asym_flag, hipStream_t st)
{
    hipLaunchKernelGGL(init_bits_kernel, dim3(n), dim3(64), 0, st, adj, Ginit, n, words);
    const int tiles = words;
    const long long ntile = (long long)tiles * (tiles + 1) / 2;
    const dim3 grid((unsigned)ntile), block(256);
    // guard band of the |c| comparison; thresholds below kThMinFilter get an empty fast range (exact everywhere)
    float c_lo = 0.0f, c_hi = 2.0f;
    if (th >= kThMinFilter)
    {
        const double tq = std::tanh((double)th);
        c_lo = (float)(tq * (1.0 - 5e-4));
        c_hi = (float)(tq * (1.0 + 5e-4));
    }
    if (!Ness && !asym_flag)
    {
        const int col_tiles = (n + kL0Cols - 1) / kL0Cols;
        long long nt = 0;
        for (int bi = 0; bi < tiles; bi++) nt += col_tiles - (bi >> 2);
        hipLaunchKernelGGL(level0_wide2_kernel, dim3((unsigned)nt), block, 0, st, C, adj, n, words, th, c_lo, c_hi, col_tiles,
                           Ginit == nullptr ? 1 : 0);
    }
    else if (Ness && asym_flag)
        hipLaunchKernelGGL((level0_kernel<true, true>), grid, block, 0, st, C, Ness, adj, n, words, th, c_lo, c_hi, tiles,
                           asym_flag);
    else if (Ness)
        hipLaunchKernelGGL((level0_kernel<true, false>), grid, block, 0, st, C, Ness, adj, n, words, th, c_lo, c_hi, tiles,
                           asym_flag);
    else
        hipLaunchKernelGGL((level0_kernel<false, true>), grid, block, 0, st, C, Ness, adj, n, words, th, c_lo, c_hi, tiles,
                           asym_flag);
    return hipGetLastError();
}

// Level 0 at per-pair sample sizes: is the pair with correlation c and size nij removed at th / sqrt(nij - 3)?  A
// single-precision estimate of z sqrt(nij - 3) settles the element unless it falls within 1e-3 of th (or the threshold is
// too small for that band, or an operand is unusual); only then the reference's double-precision threshold and Fisher z
// are formed.  A NaN or negative radicand gives a NaN threshold: the comparison is false, the edge stays.  These are the
// statements of level0_kernel<true, SYM> above, one for one (that kernel is left as it is): a batch must decide every pair
// as the block alone does, and tests/test_gpu_cusk_het_batch.py holds the two together block by block.
__device__ __forceinline__ bool het_pair_removed(float c, float nij, float th)
{
    const float nm3 = nij - 3.0f;
    const float ac = fabsf(c);
    int fastv = 2;
    if (nm3 > 0.0f && nm3 < 3.0e38f && ac < 1.0f && th * __frsqrt_rn(nm3) >= kThMinFilter)
    {
        const float sest = 0.5f * fabsf(__logf((1.0f + ac) / (1.0f - ac))) * __fsqrt_rn(nm3);
        if (sest < th * (1.0f - 1e-3f))
            fastv = 1;
        else if (sest > th * (1.0f + 1e-3f))
            fastv = 0;
    }
    if (fastv == 2)
    {
        const float lth = (float)((double)th / sqrt((double)nij - 3.0));
        return z_below<false>(c, lth);
    }
    return fastv == 1;
}

// Block-diagonal level 0 (batched runs: many small LD blocks along the diagonal of one allocation, bases multiples of 64,
// so no bitmap word straddles two blocks).  One wave per row: the words of the row's own block come from C[row, lo..hi)
// (coalesced 256-byte pieces, ballots = bitmap words), every other word of the row is zero -- the cross-block pairs do not
// exist.  The verdict is cal_Indepl0's (cuPC-S.cu:458-484) evaluated per ordered pair; the reference evaluates i < j and
// mirrors, which is the same thing on a bitwise symmetric matrix (the batched correlation build and the device gather of
// a symmetric matrix write both triangles from one value).  Writes the live bitmap, its level-0 copy and the degrees.
// HET: the verdict of level0_kernel<true, *> at the sizes N[row, lo..hi) (same stride, same aligned 256-byte pieces); N is
// bitwise symmetric inside the blocks like C (cusk_ess_square_batch, cusk_gather_rows), so the ordered pairs agree.  N is
// the last argument and every het statement is compiled out of the <false> form: its code is the untemplated kernel's.
template <bool HET>
__global__ void __launch_bounds__(256) level0_batch_kernel(const float *__restrict__ C, unsigned long long *adj,
                                                            unsigned long long *adj0, int *deg, int n, int words,
                                                            const int2 *__restrict__ row_range, float th, float c_lo, float c_hi,
                                                            const float *__restrict__ N)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int2 rg = row_range[row];
    const int w_lo = rg.x >> 6, w_hi = (rg.y + 63) >> 6;  // empty range: w_lo >= w_hi
    unsigned long long *arow = adj + (size_t)row * words, *arow0 = adj0 ? adj0 + (size_t)row * words : nullptr;
    for (int w = lane; w < words; w += 64)
        if (w < w_lo || w >= w_hi || rg.y <= rg.x)
        {
            arow[w] = 0ull;
            if (arow0) arow0[w] = 0ull;
        }
    int d = 0;
    if (rg.y > rg.x)
    {
        const float *crow = C + (size_t)row * n;
        for (int w = w_lo; w < w_hi; w++)
        {
            const int col = w * 64 + lane;
            const bool valid = col < rg.y && col != row;
            const float c = crow[valid ? col : row];
            bool rm;
            if constexpr (HET)
            {
                const float nij = valid ? N[(size_t)row * n + col] : 4.0f;
                rm = valid && het_pair_removed(c, nij, th);
            }
            else
            {
                const float ac = fabsf(c);
                if (ac < c_lo)
                    rm = true;
                else if (ac > c_hi && ac <= 1.0f)
                    rm = false;
                else
                    rm = z_below<false>(c, th);
            }
            const unsigned long long m = __ballot(valid && !rm);
            if (lane == 0)
            {
                arow[w] = m;
                if (arow0) arow0[w] = m;
            }
            d += __popcll(m);
        }
    }
    if (lane == 0) deg[row] = d;
}

// Ness != nullptr: per-pair thresholds th / sqrt(N_ij - 3) (th = the alpha/2 quantile), the batched het run
hipError_t launch_level0_batch(const float *C, const float *Ness, unsigned long long *adj, unsigned long long *adj0, int *deg, int n,
                               int words, const int2 *row_range, float th, hipStream_t st)
{
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (Ness)
    {
        hipLaunchKernelGGL(level0_batch_kernel<true>, grid, block, 0, st, C, adj, adj0, deg, n, words, row_range, th, 0.0f, 2.0f, Ness);
        return hipGetLastError();
    }
    float c_lo = 0.0f, c_hi = 2.0f;
    if (th >= kThMinFilter)
    {
        const double tq = std::tanh((double)th);
        c_lo = (float)(tq * (1.0 - 5e-4));
        c_hi = (float)(tq * (1.0 + 5e-4));
    }
    hipLaunchKernelGGL(level0_batch_kernel<false>, grid, block, 0, st, C, adj, adj0, deg, n, words, row_range, th, c_lo, c_hi,
                       static_cast<const float *>(nullptr));
    return hipGetLastError();
}

}  // namespace cusk
