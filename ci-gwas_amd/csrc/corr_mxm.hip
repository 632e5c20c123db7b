// corr_mxm.hip -- SNP x SNP correlations from packed .bed (the marker x marker part of the reference's cu_corr_pearson_npn,
// cusk/src/corr_host.cu:1023-1197, kernel src/corr_kernels.cu:478-565): Kendall tau-b from the 3x3 genotype contingency
// table over jointly non-missing individuals, mapped by sin(pi/2 tau); three kernel forms that count the same table.
#include <type_traits>
#include <cmath>

#include "corr_kernels.h"

namespace cusk {

// ---------------------------------------------------------------------------
// decode: .bed bytes -> three bit planes per marker (1 bit / individual)
//   plane 0: genotype == 1, plane 1: genotype == 2, plane 2: non-missing
// ---------------------------------------------------------------------------
__global__ void bed_to_bitplanes_kernel(const unsigned char *__restrict__ bed, unsigned long long *planes, size_t m,
                                        size_t N, size_t clb, size_t w64)
{
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= m * w64) return;
    const size_t mk = gid / w64, w = gid - mk * w64;
    unsigned long long b1 = 0, b2 = 0, bv = 0;
    const unsigned char *src = bed + mk * clb + w * 16;
    for (int byte = 0; byte < 16; byte++)
    {
        const size_t bi = w * 16 + byte;
        if (bi >= clb) break;
        const unsigned v = src[byte];
        for (int j = 0; j < 4; j++)
        {
            const size_t smp = bi * 4 + j;
            if (smp >= N) break;
            const unsigned code = (v >> (2 * j)) & 3u;
            const unsigned long long bit = 1ull << (byte * 4 + j);
            if (code == 2u) b1 |= bit;
            if (code == 0u) b2 |= bit;
            if (code != 1u) bv |= bit;
        }
    }
    planes[(0 * m + mk) * w64 + w] = b1;
    planes[(1 * m + mk) * w64 + w] = b2;
    planes[(2 * m + mk) * w64 + w] = bv;
}

// sin(x) in double precision for the arguments this file has, |x| <= pi/2 (x = pi/2 tau): the two kernel polynomials of
// fdlibm (k_sin.c / k_cos.c, error < 1 ulp) and sin x = sign(x) cos(pi/2 - |x|) above pi/4, the difference formed from the
// two-part pi/2 of e_rem_pio2.c.  The library routine spends ~300 double-precision instructions per call on the general
// argument reduction; sixteen calls per lane made the epilogue of the SNP x SNP kernels as long as 64 K-blocks of matrix
// products.  The result is rounded to float by the caller: it can differ from the library's only where the two doubles
// straddle a float rounding boundary, as the library's own last bit already may against the host's libm (the oracle).
// NaN stays NaN; anything outside the range (rounding can put |tau| a few ulps above 1) goes to the library.
__device__ __forceinline__ double sin_quarter_turn(double x)
{
    const double ax = fabs(x);
    if (!(ax <= 1.6)) return sin(x);
    if (ax <= 0.78539816339744830962)
    {
        const double z = x * x, v = z * x;
        const double r = 8.33333333332248946124e-03 +
                         z * (-1.98412698298579493134e-04 +
                              z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
        return x + v * (-1.66666666666666324348e-01 + z * r);
    }
    const double y = (1.57079632679489655800e+00 - ax) + 6.12323399573676603587e-17;
    const double z = y * y;
    const double r = z * (4.16666666666666019037e-02 +
                          z * (-1.38888888888741095749e-03 +
                               z * (2.48015872894767294178e-05 +
                                    z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double c = 1.0 - (0.5 * z - z * r);
    return x < 0.0 ? -c : c;
}

// tau-b -> sin(pi/2 tau) in the reference's fp32 operation order (corr_kernels.cu:544-564)
__device__ __forceinline__ float npn_from_counts(const float *s)
{
    float p = ((s[0] * (s[4] + s[5] + s[7] + s[8])) + (s[1] * (s[5] + s[8])) + (s[3] * (s[7] + s[8])) + (s[4] * s[8]));
    float q = ((s[1] * (s[3] + s[6])) + (s[2] * (s[3] + s[4] + s[6] + s[7])) + (s[4] * s[6]) + (s[5] * (s[6] + s[7])));
    float t = ((s[0] * (s[1] + s[2])) + (s[1] * s[2]) + (s[3] * (s[4] + s[5])) + (s[4] * s[5]) + (s[6] * (s[7] + s[8])) +
               (s[7] * s[8]));
    float u = ((s[0] * (s[3] + s[6])) + (s[1] * (s[4] + s[7])) + (s[2] * (s[5] + s[8])) + (s[3] * s[6]) + (s[4] * s[7]) +
               (s[5] * s[8]));
    float kendall = (p - q) / sqrtf((p + q + t) * (p + q + u));
    return (float)sin_quarter_turn(M_PI / 2 * (double)kendall);
}

// counts for a 32 x 32 tile of marker pairs (upper triangle of tiles), 2 x 2 pairs per thread
constexpr int kKW = 8;  // 64-bit words per staged K chunk
__global__ void __launch_bounds__(256) mxm_popcount_kernel(const unsigned long long *__restrict__ planes, float *C,
                                                            size_t m, size_t w64, size_t n, int tiles)
{
    __shared__ unsigned long long sa[3][kTile][kKW + 1];
    __shared__ unsigned long long sb[3][kTile][kKW + 1];
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
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // pair sub-tile (2 rows x 2 cols)
    unsigned cnt[2][2][9];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int c = 0; c < 9; c++) cnt[a][b][c] = 0;

    for (size_t w0 = 0; w0 < w64; w0 += kKW)
    {
        for (int e = threadIdx.x; e < 3 * kTile * kKW; e += 256)
        {
            const int pl = e / (kTile * kKW), r = (e / kKW) % kTile, k = e % kKW;
            const size_t w = w0 + k;
            const size_t ma = (size_t)bi * kTile + r, mb = (size_t)bj * kTile + r;
            sa[pl][r][k] = (ma < m && w < w64) ? planes[((size_t)pl * m + ma) * w64 + w] : 0ull;
            sb[pl][r][k] = (mb < m && w < w64) ? planes[((size_t)pl * m + mb) * w64 + w] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kKW; k++)
        {
            unsigned long long a1[2], a2[2], av[2], b1[2], b2[2], bv[2];
#pragma unroll
            for (int u = 0; u < 2; u++)
            {
                a1[u] = sa[0][ty * 2 + u][k];
                a2[u] = sa[1][ty * 2 + u][k];
                av[u] = sa[2][ty * 2 + u][k];
                b1[u] = sb[0][tx * 2 + u][k];
                b2[u] = sb[1][tx * 2 + u][k];
                bv[u] = sb[2][tx * 2 + u][k];
            }
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                {
                    // raw products; the table cells are formed from them in the epilogue
                    cnt[a][b][0] += __popcll(a1[a] & b1[b]);
                    cnt[a][b][1] += __popcll(a1[a] & b2[b]);
                    cnt[a][b][2] += __popcll(a2[a] & b1[b]);
                    cnt[a][b][3] += __popcll(a2[a] & b2[b]);
                    cnt[a][b][4] += __popcll(a1[a] & bv[b]);
                    cnt[a][b][5] += __popcll(a2[a] & bv[b]);
                    cnt[a][b][6] += __popcll(av[a] & b1[b]);
                    cnt[a][b][7] += __popcll(av[a] & b2[b]);
                    cnt[a][b][8] += __popcll(av[a] & bv[b]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
        {
            const size_t i = (size_t)bi * kTile + ty * 2 + a, j = (size_t)bj * kTile + tx * 2 + b;
            if (i < m && j < m && i < j)
            {
                const unsigned *c = cnt[a][b];
                const unsigned n11 = c[0], n12 = c[1], n21 = c[2], n22 = c[3], n1v = c[4], n2v = c[5], nv1 = c[6],
                               nv2 = c[7], nvv = c[8];
                float s[9];
                // s[3*va + vb], va/vb = genotype value of the row/column marker
                s[4] = (float)n11;
                s[5] = (float)n12;
                s[7] = (float)n21;
                s[8] = (float)n22;
                s[3] = (float)(n1v - n11 - n12);
                s[6] = (float)(n2v - n21 - n22);
                s[1] = (float)(nv1 - n11 - n21);
                s[2] = (float)(nv2 - n12 - n22);
                s[0] = (float)(nvv - n1v - n2v - (nv1 - n11 - n21) - (nv2 - n12 - n22));
                const float r = npn_from_counts(s);
                C[i * n + j] = r;
                C[j * n + i] = r;
            }
        }
}

// ---------------------------------------------------------------------------
// SNP x SNP contingency counts as an int8 MFMA GEMM, decoded from .bed on the fly.
//
// Every cell of the 3x3 table of a marker pair is a dot product over individuals of two 0/1
// indicator vectors.  With the planes X in {[g==1], [g==2], [non-missing]} the nine products
// X_a(rows) . X_b(cols)^T are nine int8 GEMMs with exact int32 accumulation
// (v_mfma_i32_32x32x32_i8: 32x32 outputs, 32 individuals per instruction).
//
// Workgroup = 256 threads = 4 waves (2x2), output tile 64 x 64 marker pairs, K block = 128
// individuals.  Per K block each thread loads 16 bytes of packed .bed (64 individuals of one of
// the 128 tile markers), expands them with bit logic + one multiply per 4 individuals into the
// three int8 planes and stores them to LDS in MFMA fragment order (48 KB: [plane][k-step][half]
// [row] x 16 B, so every fragment is one conflict-free ds_read_b128).  Each wave then issues
// 4 k-steps x 9 MFMAs on its 32 x 32 sub-tile (9 accumulators = 144 VGPRs).  HBM traffic is the
// packed .bed itself (2 bits per genotype); the int8 planes exist only in LDS.  Two workgroups
// per CU overlap one's decode with the other's MFMAs.  The epilogue converts the counts to
// floats and applies the reference's tau-b -> sin(pi/2 tau) formula in its fp32 operation order,
// writing both triangles of the square matrix with coalesced rows (transpose through LDS).
// Only tiles of the upper triangle are launched.
// ---------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kKB = 128;   // individuals per K block
constexpr int kKS = kKB / 32;

// 16 genotype indicator bits at even positions of x -> 16 bytes of 0/1
__device__ __forceinline__ v4i expand16(unsigned x)
{
    v4i o;
    o.x = (int)((((x)&0x55u) * 0x00041041u) & 0x01010101u);
    o.y = (int)((((x >> 8) & 0x55u) * 0x00041041u) & 0x01010101u);
    o.z = (int)((((x >> 16) & 0x55u) * 0x00041041u) & 0x01010101u);
    o.w = (int)((((x >> 24) & 0x55u) * 0x00041041u) & 0x01010101u);
    return o;
}

__global__ void __launch_bounds__(256, 2) mxm_mfma_kernel(const unsigned char *__restrict__ bed, float *C, size_t m, size_t N,
                                                           size_t clb, size_t n, int tiles)
{
    __shared__ v4i sA[3][kKS][2][kMT];
    __shared__ v4i sB[3][kKS][2][kMT];
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // decode role: tile-local marker (0..63 rows of A, 64..127 rows of B) and 64-individual half of the K block
    const int row_l = tid >> 1, q = tid & 1;
    const size_t mk = (row_l < kMT) ? (size_t)bi * kMT + row_l : (size_t)bj * kMT + (row_l - kMT);
    const bool row_ok = mk < m;
    const unsigned char *rowp = bed + mk * clb;
    v4i(*dst)[kKS][2][kMT] = (row_l < kMT) ? sA : sB;
    const int rr = row_l & (kMT - 1);

    v16i acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0;

    const size_t nkb = (N + kKB - 1) / kKB;
    auto load16 = [&](size_t kb) -> uint4 {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        const size_t off = kb * (kKB / 4) + (size_t)q * 16;
        if (row_ok && off < clb)
        {
            const unsigned char *src = rowp + off;
            if (off + 16 <= clb && ((reinterpret_cast<uintptr_t>(src) & 3u) == 0))
            {
                const unsigned *s4 = reinterpret_cast<const unsigned *>(src);
                w = make_uint4(s4[0], s4[1], s4[2], s4[3]);
            }
            else
            {
                unsigned tmp[4] = {0u, 0u, 0u, 0u};
                for (size_t b = 0; b < 16 && off + b < clb; b++) tmp[b >> 2] |= (unsigned)src[b] << (8 * (b & 3));
                w = make_uint4(tmp[0], tmp[1], tmp[2], tmp[3]);
            }
        }
        return w;
    };
    uint4 w = load16(0);
    for (size_t kb = 0; kb < nkb; kb++)
    {
        const unsigned wu[4] = {w.x, w.y, w.z, w.w};
        const size_t base = kb * kKB + (size_t)q * 64;
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            // 16 individuals; those at or beyond N (padding bits, or past the file) count as missing
            const size_t s0 = base + 16 * u;
            const unsigned nv = (!row_ok || s0 >= N) ? 0u : (unsigned)min((size_t)16, N - s0);
            const unsigned msk = (nv >= 16u) ? 0x55555555u : (((1u << (2 * nv)) - 1u) & 0x55555555u);
            const unsigned lo = wu[u] & 0x55555555u, hi = (wu[u] >> 1) & 0x55555555u;
            const unsigned b1 = hi & ~lo & msk;         // code 10 -> genotype 1
            const unsigned b2 = ~hi & ~lo & msk;        // code 00 -> genotype 2
            const unsigned bv = (hi | ~lo) & msk;       // anything but 01 (missing)
            const int ks = 2 * q + (u >> 1), h = u & 1;
            dst[0][ks][h][rr] = expand16(b1);
            dst[1][ks][h][rr] = expand16(b2);
            dst[2][ks][h][rr] = expand16(bv);
        }
        if (kb + 1 < nkb) w = load16(kb + 1);  // in flight while the MFMAs run
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kKS; ks++)
        {
            v4i a[3], b[3];
#pragma unroll
            for (int pl = 0; pl < 3; pl++)
            {
                a[pl] = sA[pl][ks][lane >> 5][wr * 32 + (lane & 31)];
                b[pl] = sB[pl][ks][lane >> 5][wc * 32 + (lane & 31)];
            }
#pragma unroll
            for (int pa = 0; pa < 3; pa++)
#pragma unroll
                for (int pb = 0; pb < 3; pb++)
                    acc[pa][pb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[pa], b[pb], acc[pa][pb], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *scratch = reinterpret_cast<float *>(&sA[0][0][0][0]) + wave * (32 * 33);
    const size_t i0 = (size_t)bi * kMT + wr * 32, j0 = (size_t)bj * kMT + wc * 32;
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const int rl = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), cl = lane & 31;
        const size_t i = i0 + rl, j = j0 + cl;
        float r = 0.0f;
        if (i < m && j < m && i < j)
        {
            const unsigned n11 = acc[0][0][e], n12 = acc[0][1][e], n21 = acc[1][0][e], n22 = acc[1][1][e],
                           n1v = acc[0][2][e], n2v = acc[1][2][e], nv1 = acc[2][0][e], nv2 = acc[2][1][e],
                           nvv = acc[2][2][e];
            float s[9];
            s[4] = (float)n11;
            s[5] = (float)n12;
            s[7] = (float)n21;
            s[8] = (float)n22;
            s[3] = (float)(n1v - n11 - n12);
            s[6] = (float)(n2v - n21 - n22);
            s[1] = (float)(nv1 - n11 - n21);
            s[2] = (float)(nv2 - n12 - n22);
            s[0] = (float)(nvv - n1v - n2v - (nv1 - n11 - n21) - (nv2 - n12 - n22));
            r = npn_from_counts(s);
            C[i * n + j] = r;
        }
        scratch[cl * 33 + rl] = r;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const int jl = 2 * e + (lane >> 5), il = lane & 31;
        const size_t i = i0 + il, j = j0 + jl;
        if (i < m && j < m && i < j) C[j * n + i] = scratch[jl * 33 + il];
    }
}

// ---------------------------------------------------------------------------
// The same nine contingency GEMMs on the FP4 matrix pipe (v_mfma_scale_f32_32x32x64_f8f6f4, twice the int8
// rate).  The operands are 0/1 indicators, so e2m1 holds them exactly and the f32 accumulation is exact (counts
// <= 2^24).  Two observations make the decode almost free:
//   * a dot product over individuals does not care about their ORDER, as long as both operands use the same
//     one.  A plane word has its 16 indicator bits at the even bit positions; (x & 0x11111111) is already a
//     valid word of eight 4-bit elements (individuals 0,2,4,...) and ((x >> 2) & 0x11111111) the other eight:
//     two ANDs and a shift instead of a bit-spreading multiply per four individuals;
//   * the element those masks produce is 0b0001 = 0.5 in e2m1, so every product is 0.25 and the accumulator
//     holds count/4, exactly; the epilogue multiplies by 4.
// Workgroup = 4 waves (2x2), tile 64 x 64 marker pairs, K block = 256 individuals = four MFMA steps of 64; each
// thread decodes 128 individuals of one tile marker per block (32 bytes of .bed) into 3 planes x 4 fragments of
// 16 bytes, stored in fragment order ([plane][k-step][lane half][row]), 48 KB for both operands.
// ---------------------------------------------------------------------------
typedef int v8i __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Workgroup barrier that only drains the LDS queue.  __syncthreads() also waits for every outstanding global
// load (vmcnt(0)), which would cancel the two-blocks-ahead .bed requests of the K loop below.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int kKB4 = 256;        // individuals per K block
constexpr int kKS4 = kKB4 / 64;  // MFMA steps per K block

// band_w = 0: square output C[n x n], both triangles, upper-triangle tiles enumerated along blockIdx.x.
// band_w > 0 (mps block): banded output C[i * band_w + (j - i - 1)] for 0 < j - i <= band_w, tile (blockIdx.x,
// blockIdx.x + blockIdx.y).
// btile != nullptr (cusk_corr_build_batch): many LD blocks in one launch -- workgroup w computes tile (btile[w].y, btile[w].z)
// of block btile[w].x, whose genotypes start at marker bblk[..].bed_row0 of `bed` and whose matrix lies on the diagonal of
// the n x n batch allocation at variable bblk[..].base.
template <bool FAST>
__global__ void __launch_bounds__(256, 2) mxm_fp4_kernel(const unsigned char *__restrict__ bed_in, float *C_in, size_t m_in, size_t N,
                                                          size_t clb, size_t n, int tiles, size_t band_w,
                                                          const int4 *__restrict__ btile, const CorrBatchBlock *__restrict__ bblk)
{
    __shared__ v4i sA[3][kKS4][2][kMT];
    __shared__ v4i sB[3][kKS4][2][kMT];
    int t = blockIdx.x, bi = 0;
    const unsigned char *__restrict__ bed = bed_in;
    float *C = C_in;
    size_t m = m_in;
    if (btile != nullptr)
    {
        const int4 bt = btile[blockIdx.x];
        const CorrBatchBlock bb = bblk[bt.x];
        bed = bed_in + bb.bed_row0 * clb;
        C = C_in + (size_t)bb.base * n + bb.base;
        m = (size_t)bb.m;
        bi = bt.y;
        t = bt.z;
    }
    else if (band_w == 0)
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
    else
    {
        bi = blockIdx.x;
        t = bi + (int)blockIdx.y;
        if (t >= tiles) return;
    }
    const int bj = t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // decode role: tile-local marker (0..63 rows of A, 64..127 rows of B) and 128-individual half of the K block
    const int row_l = tid >> 1, q = tid & 1;
    const size_t mk = (row_l < kMT) ? (size_t)bi * kMT + row_l : (size_t)bj * kMT + (row_l - kMT);
    const bool row_ok = mk < m;
    const unsigned char *rowp = bed + (row_ok ? mk : 0) * clb;
    v4i(*dst)[kKS4][2][kMT] = (row_l < kMT) ? sA : sB;
    const int rr = row_l & (kMT - 1);

    v16f acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;

    const size_t nkb = (N + kKB4 - 1) / kKB4;
    // 32 bytes of the marker's row: individuals [kb*256 + q*128, +128)
    auto load32 = [&](size_t kb, unsigned (&w)[8]) {
        const size_t off = kb * (kKB4 / 4) + (size_t)q * 32;
#pragma unroll
        for (int u = 0; u < 8; u++) w[u] = 0u;
        if (row_ok && off < clb)
        {
            const unsigned char *src = rowp + off;
            if (off + 32 <= clb && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0))
            {
                const uint4 lo = reinterpret_cast<const uint4 *>(src)[0], hi = reinterpret_cast<const uint4 *>(src)[1];
                w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w;
                w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
            }
            else
            {
                for (size_t b = 0; b < 32 && off + b < clb; b++) w[b >> 2] |= (unsigned)src[b] << (8 * (b & 3));
            }
        }
    };
    const int scale1 = 0x7f7f7f7f;  // E8M0 127 = 2^0 for every block
    // one K block: decode 128 individuals of this thread's marker into LDS fragments ...
    auto decode = [&](size_t kb, const unsigned (&w)[8], auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;  // every individual of the block exists (kb < N / 256)
        const size_t base = kb * kKB4 + (size_t)q * 128;
#pragma unroll
        for (int u2 = 0; u2 < 4; u2++)
        {
            // two code words = 32 individuals = one fragment (k-step 2q + (u2 >> 1), lane half u2 & 1) per plane
            unsigned pe[3][2], po[3][2];
#pragma unroll
            for (int z = 0; z < 2; z++)
            {
                const int u = 2 * u2 + z;
                // individuals at or beyond N (padding bits, or past the file) count as missing
                unsigned msk;
                if constexpr (FULL)
                    msk = row_ok ? 0x55555555u : 0u;
                else
                {
                    const size_t s0 = base + 16 * u;
                    const unsigned nv = (!row_ok || s0 >= N) ? 0u : (unsigned)min((size_t)16, N - s0);
                    msk = (nv >= 16u) ? 0x55555555u : (((1u << (2 * nv)) - 1u) & 0x55555555u);
                }
                const unsigned lo = w[u] & 0x55555555u, hi = (w[u] >> 1) & 0x55555555u;
                const unsigned pl[3] = {hi & ~lo & msk,     // code 10 -> genotype 1
                                        ~hi & ~lo & msk,    // code 00 -> genotype 2
                                        (hi | ~lo) & msk};  // anything but 01 (missing)
#pragma unroll
                for (int k = 0; k < 3; k++)
                {
                    pe[k][z] = pl[k] & 0x11111111u;
                    po[k][z] = (pl[k] >> 2) & 0x11111111u;
                }
            }
            const int ks = 2 * q + (u2 >> 1), h = u2 & 1;
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                v4i f;
                f.x = (int)pe[k][0];
                f.y = (int)po[k][0];
                f.z = (int)pe[k][1];
                f.w = (int)po[k][1];
                dst[k][ks][h][rr] = f;
            }
        }
    };
    // ... and the 4 x 9 products of this wave's 32 x 32 sub-tile
    auto products = [&]() {
#pragma unroll
        for (int ks = 0; ks < kKS4; ks++)
        {
            v8i a[3], b[3];
#pragma unroll
            for (int pl = 0; pl < 3; pl++)
            {
                const v4i fa = sA[pl][ks][lane >> 5][wr * 32 + (lane & 31)];
                const v4i fb = sB[pl][ks][lane >> 5][wc * 32 + (lane & 31)];
                a[pl] = v8i{fa.x, fa.y, fa.z, fa.w, 0, 0, 0, 0};
                b[pl] = v8i{fb.x, fb.y, fb.z, fb.w, 0, 0, 0, 0};
            }
#pragma unroll
            for (int pa = 0; pa < 3; pa++)
#pragma unroll
                for (int pb = 0; pb < 3; pb++)
                    acc[pa][pb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[pa], b[pb], acc[pa][pb], 4, 4, 0, scale1, 0,
                                                                                  scale1);
        }
    };
    // Full K blocks of 16-byte aligned rows (FAST, checked by the launcher) are requested two blocks ahead with
    // unconditional loads into two alternating register sets: .bed comes from L2/HBM with a latency of several
    // K blocks' worth of MFMAs.  Rows without a marker read row 0 and are masked in the decode.
    size_t kb0 = 0;
    if constexpr (FAST)
    {
        const size_t nfull = N / kKB4;
        const uint4 *row4 = reinterpret_cast<const uint4 *>(rowp) + 2 * q;
        // The requests are issued as inline assembly so that NO compiler-generated s_waitcnt covers them: hipcc
        // drains the whole load queue (vmcnt(0)) at the first use inside a loop, which would serialise request and
        // use again.  Each register set is waited for explicitly, with exactly the other set's two loads allowed
        // to stay in flight, and everything is drained before the registers can be reused after the loop.
#define CUSK_BED_REQUEST(kb_, lo_, hi_)                                                                          \
    {                                                                                                          \
        const uint4 *src_ = row4 + (kb_) * (kKB4 / 64);                                                        \
        asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16"            \
                     : "=&v"(lo_), "=&v"(hi_)                                                                  \
                     : "v"(src_)                                                                               \
                     : "memory");                                                                              \
    }
#define CUSK_BED_WAIT_OLDER(lo_, hi_) asm volatile("s_waitcnt vmcnt(2)" : "+v"(lo_), "+v"(hi_)::"memory")
        if (nfull > 0)
        {
            v4u alo, ahi, blo, bhi;  // native vectors: register operands of the assembly
            unsigned w[8];
            CUSK_BED_REQUEST(0, alo, ahi);
            CUSK_BED_REQUEST(min((size_t)1, nfull - 1), blo, bhi);
            for (size_t kb = 0; kb < nfull; kb += 2)
            {
                CUSK_BED_WAIT_OLDER(alo, ahi);
                w[0] = alo.x, w[1] = alo.y, w[2] = alo.z, w[3] = alo.w;
                w[4] = ahi.x, w[5] = ahi.y, w[6] = ahi.z, w[7] = ahi.w;
                decode(kb, w, std::true_type{});
                CUSK_BED_REQUEST(min(kb + 2, nfull - 1), alo, ahi);
                lds_barrier();
                products();
                lds_barrier();
                if (kb + 1 >= nfull) break;
                CUSK_BED_WAIT_OLDER(blo, bhi);
                w[0] = blo.x, w[1] = blo.y, w[2] = blo.z, w[3] = blo.w;
                w[4] = bhi.x, w[5] = bhi.y, w[6] = bhi.z, w[7] = bhi.w;
                decode(kb + 1, w, std::true_type{});
                CUSK_BED_REQUEST(min(kb + 3, nfull - 1), blo, bhi);
                lds_barrier();
                products();
                lds_barrier();
            }
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(alo), "+v"(ahi), "+v"(blo), "+v"(bhi)::"memory");
#undef CUSK_BED_REQUEST
#undef CUSK_BED_WAIT_OLDER
            kb0 = nfull;
        }
    }
    for (size_t kb = kb0; kb < nkb; kb++)
    {
        unsigned w[8];
        load32(kb, w);
        decode(kb, w, std::false_type{});
        __syncthreads();
        products();
        __syncthreads();
    }

    // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *scratch = reinterpret_cast<float *>(&sA[0][0][0][0]) + wave * (32 * 33);
    const size_t i0 = (size_t)bi * kMT + wr * 32, j0 = (size_t)bj * kMT + wc * 32;
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const int rl = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), cl = lane & 31;
        const size_t i = i0 + rl, j = j0 + cl;
        float r = 0.0f;
        if (i < m && j < m && i < j)
        {
            // every product was 0.5 * 0.5: the accumulators hold count / 4 exactly
            const unsigned n11 = (unsigned)(acc[0][0][e] * 4.0f), n12 = (unsigned)(acc[0][1][e] * 4.0f),
                           n21 = (unsigned)(acc[1][0][e] * 4.0f), n22 = (unsigned)(acc[1][1][e] * 4.0f),
                           n1v = (unsigned)(acc[0][2][e] * 4.0f), n2v = (unsigned)(acc[1][2][e] * 4.0f),
                           nv1 = (unsigned)(acc[2][0][e] * 4.0f), nv2 = (unsigned)(acc[2][1][e] * 4.0f),
                           nvv = (unsigned)(acc[2][2][e] * 4.0f);
            float s[9];
            s[4] = (float)n11;
            s[5] = (float)n12;
            s[7] = (float)n21;
            s[8] = (float)n22;
            s[3] = (float)(n1v - n11 - n12);
            s[6] = (float)(n2v - n21 - n22);
            s[1] = (float)(nv1 - n11 - n21);
            s[2] = (float)(nv2 - n12 - n22);
            s[0] = (float)(nvv - n1v - n2v - (nv1 - n11 - n21) - (nv2 - n12 - n22));
            r = npn_from_counts(s);
            if (band_w == 0)
                C[i * n + j] = r;
            else if (j - i - 1 < band_w)
                C[i * band_w + (j - i - 1)] = r;
        }
        scratch[cl * 33 + rl] = r;
    }
    if (band_w != 0) return;  // no mirrored triangle in the banded layout (uniform per launch)
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const int jl = 2 * e + (lane >> 5), il = lane & 31;
        const size_t i = i0 + il, j = j0 + jl;
        if (i < m && j < m && i < j) C[j * n + i] = scratch[jl * 33 + il];
    }
}

__global__ void unit_diag_kernel(float *C, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) C[i * n + i] = 1.0f;
}

// upper triangle (without diagonal) of the rows/cols [lo, lo+cnt) of C into a linear array
__global__ void extract_tri_kernel(const float *__restrict__ C, float *out, size_t lo, size_t cnt, size_t n)
{
    const size_t i = blockIdx.y;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt || j >= cnt || j <= i) return;
    const size_t lin = i * (cnt - 1) - (i * (i - 1)) / 2 + (j - i - 1);
    out[lin] = C[(lo + i) * n + lo + j];
}

// per block: the trait x trait correlations (computed once, the same for every block: cli.cpp:597-649 writes them into
// every block's matrix) and the unit diagonal
__global__ void __launch_bounds__(256) batch_finish_kernel(float *C, size_t n, const CorrBatchBlock *__restrict__ bblk,
                                                            const int *__restrict__ kept, const float *__restrict__ pxp, int p)
{
    const CorrBatchBlock bb = bblk[kept[blockIdx.x]];
    float *Cb = C + (size_t)bb.base * n + bb.base;
    const int nb = bb.m + p;
    for (int i = threadIdx.x; i < nb; i += 256) Cb[(size_t)i * n + i] = 1.0f;
    for (int e = threadIdx.x; e < p * p; e += 256)
    {
        const int a = e / p, b = e % p;
        if (a != b) Cb[(size_t)(bb.m + a) * n + bb.m + b] = pxp[(size_t)a * p + b];
    }
}
// ---- launchers (corr_kernels.h) ----
static_assert(sizeof(CorrTile4) == sizeof(int4), "CorrTile4 is read as int4");

void launch_mxm_fp4(hipStream_t s, const MxmFp4Args &a)
{
    const int tiles = (int)((a.m + kMT - 1) / kMT);  // 0 with a tile table
    const dim3 grid = a.btile ? dim3((unsigned)a.ntab)
                              : (a.band_w ? dim3((unsigned)tiles, (unsigned)((a.band_w + kMT - 1) / kMT + 1))
                                          : dim3((unsigned)((long long)tiles * (tiles + 1) / 2)));
    auto *k = bed_rows16(a.bed, a.clb) ? mxm_fp4_kernel<true> : mxm_fp4_kernel<false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a.bed, a.C, a.m, a.N, a.clb, a.n, tiles, a.band_w, reinterpret_cast<const int4 *>(a.btile),
                       a.bblk);
}

void launch_mxm_int8(hipStream_t s, const unsigned char *bed, float *C, size_t m, size_t N, size_t clb, size_t n)
{
    const int tiles = (int)((m + kMT - 1) / kMT);
    hipLaunchKernelGGL(mxm_mfma_kernel, dim3((unsigned)((long long)tiles * (tiles + 1) / 2)), dim3(256), 0, s, bed, C, m, N, clb, n, tiles);
}

int launch_mxm_popcount(cusk_engine *e, hipStream_t s, const unsigned char *bed, float *C, size_t m, size_t N, size_t clb, size_t n,
                        hipEvent_t between)
{
    const size_t w64 = (N + 63) / 64;
    CUSK_HIP(e, e->planes.ensure(sizeof(unsigned long long) * 3 * m * w64));
    unsigned long long *planes = e->planes.as<unsigned long long>();
    hipLaunchKernelGGL(bed_to_bitplanes_kernel, dim3((unsigned)((m * w64 + 255) / 256)), dim3(256), 0, s, bed, planes, m, N, clb, w64);
    if (between) CUSK_HIP(e, hipEventRecord(between, s));
    const int tiles = (int)((m + kTile - 1) / kTile);
    hipLaunchKernelGGL(mxm_popcount_kernel, dim3((unsigned)((long long)tiles * (tiles + 1) / 2)), dim3(256), 0, s, planes, C, m, w64, n, tiles);
    return CUSK_OK;
}

void launch_unit_diag(hipStream_t s, float *C, size_t n) { hipLaunchKernelGGL(unit_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, C, n); }

void launch_extract_tri(hipStream_t s, const float *C, float *out, size_t lo, size_t cnt, size_t n)
{
    hipLaunchKernelGGL(extract_tri_kernel, dim3((unsigned)((cnt + 255) / 256), (unsigned)cnt), dim3(256), 0, s, C, out, lo, cnt, n);
}

void launch_batch_finish(hipStream_t s, float *C, size_t n, const CorrBatchBlock *bblk, const int *kept, size_t nkept, const float *pxp, size_t p)
{
    hipLaunchKernelGGL(batch_finish_kernel, dim3((unsigned)nkept), dim3(256), 0, s, C, n, bblk, kept, pxp, (int)p);
}

}  // namespace cusk
