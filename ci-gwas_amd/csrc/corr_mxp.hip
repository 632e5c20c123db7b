// corr_mxp.hip -- SNP x trait and trait x trait correlations (the reference's cu_marker_phen_corr_pearson and those parts of
// cu_corr_pearson_npn, cusk/src/corr_host.cu:1023-1197; kernels src/corr_kernels.cu:157-238, :285-343).  mxp: Pearson with
// precomputed marker mean/std, NaN traits skipped, in scalar, f32 MFMA and bf16 split forms; pxp: sum(y_a y_b) / #jointly-valid.
#include <algorithm>

#include "corr_kernels.h"

namespace cusk {

// one wave per marker, all traits: Pearson of corr_kernels.cu:157-238
__global__ void __launch_bounds__(256) mxp_kernel(const unsigned char *__restrict__ bed, const float *__restrict__ phen,
                                                   const float *__restrict__ mean, const float *__restrict__ sd, float *C,
                                                   float *mxp, size_t m, size_t N, size_t p, size_t clb, size_t n,
                                                   size_t p0, size_t pcount)
{
    const size_t mk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (mk >= m) return;
    float sgy[kMaxPhenRegs], sy[kMaxPhenRegs], sn[kMaxPhenRegs];
#pragma unroll
    for (int k = 0; k < kMaxPhenRegs; k++) sgy[k] = sy[k] = sn[k] = 0.0f;
    for (size_t bi = lane; bi < clb; bi += 64)
    {
        const unsigned v = bed[mk * clb + bi];
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const size_t smp = bi * 4 + j;
            if (smp >= N) break;
            const unsigned code = (v >> (2 * j)) & 3u;
            const float valid = (code != 1u) ? 1.0f : 0.0f;
            const float g = (code == 0u) ? 2.0f : ((code == 2u) ? 1.0f : 0.0f);
#pragma unroll
            for (int k = 0; k < kMaxPhenRegs; k++)
            {
                if ((size_t)k < pcount)
                {
                    const float y = phen[(p0 + k) * N + smp];
                    if (!(y != y))
                    {
                        sgy[k] += valid * g * y;
                        sy[k] += valid * y;
                        sn[k] += valid;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMaxPhenRegs; k++)
    {
        if ((size_t)k < pcount)
        {
            float a = sgy[k], b = sy[k], c = sn[k];
            for (int o = 32; o > 0; o >>= 1)
            {
                a += __shfl_xor(a, o);
                b += __shfl_xor(b, o);
                c += __shfl_xor(c, o);
            }
            if (lane == 0)
            {
                const float r = (a - mean[mk] * b) / (c * sd[mk]);
                const size_t t = p0 + k;
                if (C)
                {
                    C[mk * n + m + t] = r;
                    C[(m + t) * n + mk] = r;
                }
                if (mxp) mxp[mk * p + t] = r;
            }
        }
    }
}

// SNP x trait Pearson as an exact-f32 MFMA contraction over individuals (corr_kernels.cu:157-238 gives the
// formula: r = (sum g y - mean_g sum y) / (n sd_g) over the individuals where genotype and trait are both
// present).  With A = [genotype dosage | non-missing flag] (markers x individuals, decoded from .bed in
// registers) and B = [trait, NaN -> 0 | NaN flag] (individuals x traits) the three sums are A_g B_y, A_v B_y and
// A_v B_nan: v_mfma_f32_32x32x2_f32 accumulates each as a k-ordered chain of f32 FMAs (exact f32, the matrix
// pipe runs at the f32 vector rate but leaves the vector ALU to the decoding and needs 48 accumulator registers
// instead of 3 per marker-trait pair).
//
// Workgroup = 8 waves, output tile 32 markers x 32 traits; wave w owns the w-th eighth of the individuals
// (split-K) and the eight partial tiles are added in a fixed order through LDS, so the result is deterministic.
// Operand lane maps of the 32x32x2 form: lane l holds A[row l&31][k = l>>5] and B[k = l>>5][col l&31], one f32
// each: lane (i, k) walks marker i and takes individuals 2q+k of each byte (two MFMA steps per .bed byte), lane
// (j, k) walks trait row j with float4 loads.  The NaN product is only issued for 16-individual groups that
// contain a NaN.

// FAST: every marker row of the .bed block is dword-aligned and every trait row 16-byte aligned (N % 4 == 0 and
// aligned bases, checked by the launcher), so full 16-individual groups are fetched with one dword + four
// float4 loads, unconditionally, two groups in flight.  Anything else (odd N, the last partial group) goes
// through the bounds-checked fetch.
template <bool FAST>
__global__ void __launch_bounds__(64 * kMxpWaves) mxp_mfma_kernel(const unsigned char *__restrict__ bed,
                                                                  const float *__restrict__ phen,
                                                                  const float *__restrict__ mean,
                                                                  const float *__restrict__ sd, float *C, float *mxp, size_t m,
                                                                  size_t N, size_t p, size_t clb, size_t n, size_t p0,
                                                                  int pcount, const int2 *__restrict__ mtile,
                                                                  const CorrBatchBlock *__restrict__ bblk)
{
    __shared__ float s_part[kMxpWaves / 2][3][16][64];  // partial accumulators of the upper half of the waves
    __shared__ float s_sv[kMxpWaves][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, kh = lane >> 5;
    size_t tile32 = blockIdx.x;
    if (mtile != nullptr)
    {  // batched build: tile mtile[w].y of block mtile[w].x (see mxm_fp4_kernel)
        const int2 mt = mtile[blockIdx.x];
        const CorrBatchBlock bb = bblk[mt.x];
        bed += bb.bed_row0 * clb;
        mean += bb.bed_row0;
        sd += bb.bed_row0;
        if (C) C += (size_t)bb.base * n + bb.base;
        if (mxp) mxp += (size_t)bb.mxp_off * p;
        m = (size_t)bb.m;
        tile32 = (size_t)mt.y;
    }
    const size_t mk = tile32 * 32 + r32;  // A side: this lane's marker
    const bool mok = mk < m;
    const unsigned char *rowp = bed + (mok ? mk : 0) * clb;
    const bool tok = r32 < pcount;  // B side: this lane's trait
    const float *yrow = phen + (p0 + (tok ? r32 : 0)) * N;
    // Lanes without a marker / trait still feed the MFMA (row i of A only reaches row i of the product, column j
    // of B only column j, and those are never written); their genotypes are forced to "missing".

    v16f acc_gy, acc_vy, acc_vn;
#pragma unroll
    for (int r = 0; r < 16; r++) acc_gy[r] = acc_vy[r] = acc_vn[r] = 0.0f;
    float sv = 0.0f;

    // bounds-checked operands of group g: individuals at or beyond N count as missing / zero
    auto fetch_checked = [&](size_t g, unsigned &w, float (&y)[16]) {
        const size_t s0 = g * 16, off = g * 4;
        w = 0u;
        for (size_t bb = 0; bb < 4; bb++) w |= (unsigned)((mok && off + bb < clb) ? rowp[off + bb] : 0x55u) << (8 * bb);
#pragma unroll
        for (int q = 0; q < 16; q++)
        {
            if (s0 + q >= N) w = (w & ~(3u << (2 * q))) | (1u << (2 * q));
            y[q] = (tok && s0 + q < N) ? yrow[s0 + q] : 0.0f;
        }
    };
    auto fetch_fast = [&](size_t g, unsigned &w, float (&y)[16]) {
        w = reinterpret_cast<const unsigned *>(rowp)[g];
        const float4 *y4 = reinterpret_cast<const float4 *>(yrow) + g * 4;
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
            const float4 v = y4[q];
            y[4 * q] = v.x;
            y[4 * q + 1] = v.y;
            y[4 * q + 2] = v.z;
            y[4 * q + 3] = v.w;
        }
    };
    // 8 MFMA steps of one group; lane (row r32, half kh) supplies individual 2 st + kh in step st
    auto multiply = [&](unsigned w, const float (&y)[16]) {
        const unsigned wk = (mok ? w : 0x55555555u) >> (2 * kh);
        bool has_nan = false;
#pragma unroll
        for (int q = 0; q < 16; q++) has_nan = has_nan || (y[q] != y[q]);
        const bool any_nan = __ballot(has_nan && tok) != 0ull;
#pragma unroll
        for (int st = 0; st < 8; st++)
        {
            const unsigned code = (wk >> (4 * st)) & 3u;           // 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
            const float av = (float)((0xdu >> code) & 1u);         // non-missing flag
            const float ag = (float)((0x12u >> (2 * code)) & 3u);  // dosage, 0 when missing
            const float yq = kh ? y[2 * st + 1] : y[2 * st];
            const float by = (yq != yq) ? 0.0f : yq;
            sv += av;
            acc_gy = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, by, acc_gy, 0, 0, 0);
            acc_vy = __builtin_amdgcn_mfma_f32_32x32x2f32(av, by, acc_vy, 0, 0, 0);
        }
        // the NaN count product only for groups that contain a NaN, in its own loop: a branch around the
        // products above would make the compiler copy the 32 accumulator registers at every join
        if (any_nan)
        {
#pragma unroll
            for (int st = 0; st < 8; st++)
            {
                const unsigned code = (wk >> (4 * st)) & 3u;
                const float av = (float)((0xdu >> code) & 1u);
                const float yq = kh ? y[2 * st + 1] : y[2 * st];
                acc_vn = __builtin_amdgcn_mfma_f32_32x32x2f32(av, (yq != yq) ? 1.0f : 0.0f, acc_vn, 0, 0, 0);
            }
        }
    };

    // the wave's range of 16-individual groups
    const size_t groups = (N + 15) / 16;
    const size_t gper = (groups + kMxpWaves - 1) / kMxpWaves;
    const size_t g_begin = min(groups, (size_t)wave * gper), g_end = min(groups, g_begin + gper);
    size_t g_fast_end = g_begin;
    if constexpr (FAST)
    {
        g_fast_end = max(g_begin, min(g_end, N / 16));  // full groups of this wave
        if (g_begin < g_fast_end)
        {
            unsigned w0, w1;
            float y0[16], y1[16];
            fetch_fast(g_begin, w0, y0);
            for (size_t g = g_begin; g < g_fast_end; g += 2)
            {
                // unconditional request of the following group (clamped), then the products of the older set
                fetch_fast(min(g + 1, g_fast_end - 1), w1, y1);
                __builtin_amdgcn_sched_barrier(0);
                multiply(w0, y0);
                if (g + 1 >= g_fast_end) break;
                fetch_fast(min(g + 2, g_fast_end - 1), w0, y0);
                __builtin_amdgcn_sched_barrier(0);
                multiply(w1, y1);
            }
        }
    }
    for (size_t g = g_fast_end; g < g_end; g++)
    {
        unsigned w;
        float y[16];
        fetch_checked(g, w, y);
        multiply(w, y);
    }
    // ---- split-K reduction in a fixed order: waves 4..7 -> 0..3, then 2,3 -> 0,1, then 1 -> 0 ----
    s_sv[wave][lane] = sv;
    for (int half = kMxpWaves / 2; half >= 1; half >>= 1)
    {
        __syncthreads();
        if (wave >= half && wave < 2 * half)
        {
#pragma unroll
            for (int r = 0; r < 16; r++)
            {
                s_part[wave - half][0][r][lane] = acc_gy[r];
                s_part[wave - half][1][r][lane] = acc_vy[r];
                s_part[wave - half][2][r][lane] = acc_vn[r];
            }
        }
        __syncthreads();
        if (wave < half)
        {
#pragma unroll
            for (int r = 0; r < 16; r++)
            {
                acc_gy[r] += s_part[wave][0][r][lane];
                acc_vy[r] += s_part[wave][1][r][lane];
                acc_vn[r] += s_part[wave][2][r][lane];
            }
        }
    }
    if (wave != 0) return;
    // non-missing count per marker: both k halves of all waves, fixed order
    float svm = 0.0f;
#pragma unroll
    for (int wv = 0; wv < kMxpWaves; wv++) svm += s_sv[wv][r32] + s_sv[wv][r32 + 32];
    // C/D layout: col (trait) = lane & 31, row (marker) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    s_sv[0][lane] = svm;  // lanes i and i+32 hold the same value for marker i
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const size_t t = p0 + r32;
#pragma unroll
    for (int r = 0; r < 16; r++)
    {
        const int il = (r & 3) + 8 * (r >> 2) + 4 * kh;
        const size_t mi = tile32 * 32 + il;
        if (mi < m && tok)
        {
            const float cnt = s_sv[0][il] - acc_vn[r];
            const float rr = (acc_gy[r] - mean[mi] * acc_vy[r]) / (cnt * sd[mi]);
            if (C)
            {
                C[mi * n + m + t] = rr;
                C[(m + t) * n + mi] = rr;
            }
            if (mxp) mxp[mi * p + t] = rr;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 3: the same three sums on the bf16 matrix pipe (16x the rate of the f32 form above, whose 8 + 8 K = 2 products
// per 16 individuals bound the kernel at 0.41 ms for 13,700 markers x 20 traits -- as long as the 64 x more work of the
// SNP x SNP kernel of a batch).  A trait value is split EXACTLY into three bf16 pieces, y = hi + mid + lo (8 + 8 + 8
// significant bits), the dosage {0, 1, 2} and the flags {0, 1} are bf16 numbers anyway, so every product is exact in f32
// and only the order of the f32 additions differs from the chain above (the reference's own order is that of its block
// reduction, corr_kernels.cu:157-238; the bar is its test tolerance, 1e-5: tests/test_gpu_parity.py).
//   B fragments (mxp_split_kernel, once per build): bf16 columns c = q * 21 + t for piece q of trait t (columns 0..62),
//     64 + t = NaN flag of trait t, 85 = 1 for every individual < N; zero beyond N (padded to 64 individuals), so the
//     padding bits of a .bed row never count whatever they decode to; stored fragment-major (see the kernel).
//   Workgroup = 4 waves (one per SIMD, so that a wave may hold 160 accumulator registers) = split-K over the individuals,
//     TWO marker tiles of 32 per wave (they share the B fragments:
//     half the L2 traffic; with a tile table the two tiles may belong to different blocks of a batch -- the traits are the
//     same for all).  Per 16 individuals and tile: G x P0, G x P1, V x P0, V x P1, V x F = five
//     v_mfma_f32_32x32x16_bf16.  A fragment of a lane (marker r32, half kh): individuals 8 kh .. 8 kh + 7 = two bytes of
//     the row; a nibble (two 2-bit codes) becomes one dword of two bf16 through v_perm_b32 with the code as byte selector
//     into a 4-entry table (low bytes in one source, high bytes in the other): 6 vector instructions per dword pair (g, v).
//   The four partial tiles are added in a fixed order through LDS (deterministic), then every thread finishes a few
//   (marker, trait) pairs: pieces summed (hi + mid) + lo, r = (sum g y - mean_g sum y) / (n sd_g).
// ---------------------------------------------------------------------------------------------------------------
typedef __bf16 mxb_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned mxb_u4 __attribute__((ext_vector_type(4)));
constexpr int kMxbOnes = 64 + kMxbTraits;

// One thread per (column tile k, group g, lane): the 16 bytes that lane (column k * 32 + (lane & 31), half lane >> 5) of a
// wave feeds to the MFMA of group g -- eight consecutive individuals of one column -- stored at ((k * G + g) * 64 + lane) * 8,
// so a wave's fragment load is one contiguous kilobyte.  G = groups, a multiple of four (the kernel requests four at a time).
__global__ void __launch_bounds__(256) mxp_split_kernel(const float *__restrict__ phen, size_t N, size_t G, size_t p0, int pc,
                                                         unsigned short *__restrict__ Bq)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= 3 * G * 64) return;
    const int lane = (int)(id & 63);
    const size_t g = (id >> 6) % G;
    const int k = (int)((id >> 6) / G);
    const int c = k * 32 + (lane & 31);
    const size_t i0 = g * 16 + 8 * (size_t)(lane >> 5);
    // column c: piece q of trait t (c = q * 21 + t < 63), NaN flag of trait c - 64, the ones column, or nothing
    const int q = c < 63 ? c / kMxbTraits : -1;
    const int t = c < 63 ? c % kMxbTraits : c - 64;
    unsigned short out[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
    {
        const size_t i = i0 + j;
        unsigned short v = 0;
        if (i < N)
        {
            if (c == kMxbOnes)
                v = 0x3f80;  // 1.0
            else if (c != 63 && c < kMxbOnes && t < pc)
            {
                const float y = phen[(p0 + t) * N + i];
                if (q < 0)
                    v = (y != y) ? 0x3f80 : 0;
                else if (y == y)
                {
                    const float hi = __uint_as_float(__float_as_uint(y) & 0xffff0000u);
                    const float r1 = (hi - hi == 0.0f) ? y - hi : 0.0f;  // exact; an infinite value stays in the first piece
                    const float mid = __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
                    const float r2 = r1 - mid;  // exact, at most 8 significant bits
                    v = (unsigned short)(__float_as_uint(q == 0 ? hi : (q == 1 ? mid : r2)) >> 16);
                }
            }
        }
        out[j] = v;
    }
    mxb_u4 o;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = (unsigned)out[2 * j] | ((unsigned)out[2 * j + 1] << 16);
    *reinterpret_cast<mxb_u4 *>(Bq + id * 8) = o;
}

struct MxbTile
{
    long long c_off;    // element offset of the block's matrix inside C
    long long mxp_off;  // element offset of the block's rows inside mxp
    long long row0;     // first marker row of the block in the .bed / mean / sd arrays
    int m, tile32, valid, pad;
};

template <bool FAST>
__global__ void __launch_bounds__(64 * kMxbWaves) mxp_bf16_kernel(const unsigned char *__restrict__ bed, const unsigned short *__restrict__ Bq,
                                                        const float *__restrict__ mean, const float *__restrict__ sd, float *C,
                                                        float *mxp, size_t m_in, size_t G, size_t p, size_t clb, size_t n,
                                                        size_t p0, int pcount, int ntiles, const int2 *__restrict__ mtile,
                                                        const CorrBatchBlock *__restrict__ bblk)
{
    __shared__ float s_red[kMxbWaves][16][64];  // the partial copies of one accumulator tile
    __shared__ float s_out[2][5][32][33];  // reduced tiles: [marker tile][product][marker][column]
    __shared__ MxbTile s_tile[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, kh = lane >> 5;
    if (tid < 2)
    {
        MxbTile t;
        const int T = 2 * (int)blockIdx.x + tid;
        t.valid = T < ntiles ? 1 : 0;
        t.c_off = 0;
        t.mxp_off = 0;
        t.row0 = 0;
        t.m = (int)m_in;
        t.tile32 = T;
        t.pad = 0;
        if (t.valid && mtile != nullptr)
        {  // batched build: tile mtile[T].y of block mtile[T].x
            const int2 mt = mtile[T];
            const CorrBatchBlock bb = bblk[mt.x];
            t.row0 = (long long)bb.bed_row0;
            t.c_off = (long long)bb.base * (long long)n + bb.base;
            t.mxp_off = (long long)bb.mxp_off * (long long)p;
            t.m = bb.m;
            t.tile32 = mt.y;
        }
        s_tile[tid] = t;
    }
    __syncthreads();
    const unsigned char *rowp[2];
    bool mok[2];
#pragma unroll
    for (int u = 0; u < 2; u++)
    {
        const MxbTile t = s_tile[u];
        const long long mk = (long long)t.tile32 * 32 + r32;
        mok[u] = t.valid && mk < t.m;
        rowp[u] = bed + (size_t)(t.row0 + (mok[u] ? mk : 0)) * clb;
    }
    v16f acc[2][5];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int a = 0; a < 5; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[u][a][r] = 0.0f;

    // the wave's range of groups, in fours (G is a multiple of four)
    const size_t gper = ((G / 4 + kMxbWaves - 1) / kMxbWaves) * 4;
    const size_t g_begin = min(G, (size_t)wave * gper), g_end = min(G, g_begin + gper);
    const unsigned short *bq = Bq + (size_t)lane * 8;
    // FAST (rows of the .bed block 16-byte aligned): the four dwords of four consecutive groups in one request per marker
    // row -- a request of 64 lanes in 64 different rows costs the address unit one cycle per lane whatever its width
    auto fetch_a4 = [&](int u, size_t g0, unsigned (&w)[4]) {
        if constexpr (FAST)
        {
            const mxb_u4 v = reinterpret_cast<const mxb_u4 *>(rowp[u])[g0 >> 2];
            w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
        }
        else
        {
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                unsigned x = 0u;
                for (size_t bb = 0; bb < 4; bb++) x |= (unsigned)(((g0 + j) * 4 + bb < clb) ? rowp[u][(g0 + j) * 4 + bb] : 0x55u) << (8 * bb);
                w[j] = x;
            }
        }
    };
    auto fetch_b = [&](size_t g, mxb_u4 (&b)[3]) {
#pragma unroll
        for (int k = 0; k < 3; k++) b[k] = *reinterpret_cast<const mxb_u4 *>(bq + ((size_t)k * G + g) * 512);
    };
    // eight 2-bit codes -> eight bf16 dosages and eight bf16 non-missing flags
    // code 00 -> dosage 2 (0x4000), 01 -> missing (0, flag 0), 10 -> 1 (0x3f80), 11 -> 0; flag 1.0 = 0x3f80
    auto decode = [&](unsigned x, mxb_u4 &ag, mxb_u4 &av) {
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const unsigned nib = x >> (4 * j);
            const unsigned t = (nib & 3u) | ((nib & 0xcu) << 14);  // c0 | c1 << 16
            const unsigned sel = t * 0x0101u + 0x04000400u;        // bytes [c0, 4 + c0, c1, 4 + c1]: low byte, high byte per value
            ag[j] = __builtin_amdgcn_perm(0x003f0040u, 0x00800000u, sel);
            av[j] = __builtin_amdgcn_perm(0x3f3f003fu, 0x80800080u, sel);
        }
    };
    auto multiply = [&](const unsigned (&w)[2], const mxb_u4 (&b)[3]) {
        const mxb_bf8 b0 = __builtin_bit_cast(mxb_bf8, b[0]), b1 = __builtin_bit_cast(mxb_bf8, b[1]), b2 = __builtin_bit_cast(mxb_bf8, b[2]);
#pragma unroll
        for (int u = 0; u < 2; u++)
        {
            const unsigned x = mok[u] ? ((w[u] >> (16 * kh)) & 0xffffu) : 0x5555u;
            mxb_u4 ag, av;
            decode(x, ag, av);
            const mxb_bf8 g8 = __builtin_bit_cast(mxb_bf8, ag), v8 = __builtin_bit_cast(mxb_bf8, av);
            acc[u][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8, b0, acc[u][0], 0, 0, 0);
            acc[u][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g8, b1, acc[u][1], 0, 0, 0);
            acc[u][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v8, b0, acc[u][2], 0, 0, 0);
            acc[u][3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v8, b1, acc[u][3], 0, 0, 0);
            acc[u][4] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v8, b2, acc[u][4], 0, 0, 0);
        }
    };
    if (g_begin < g_end)
    {
        // One loop body, four groups (64 individuals) per trip: the operands of the following four are requested
        // (clamped, unconditional) before the forty products of the current four and handed over by register moves.  (An
        // exit in the middle of an unrolled pair makes the compiler keep two copies of the 160 accumulator registers and
        // move them at every join.)  The first form asked for one dword per lane and group and for B columns N apart: five
        // requests of 64 scattered addresses per group and wave kept the address unit busier than the products kept the
        // matrix pipe (184 us); now two scattered 16-byte requests and twelve contiguous kilobytes per four groups.
        unsigned wc[2][4], wn[2][4];
        mxb_u4 bc[4][3], bn[4][3];
        auto fetch4 = [&](size_t g0, unsigned (&w)[2][4], mxb_u4 (&bb)[4][3]) {
            fetch_a4(0, g0, w[0]);
            fetch_a4(1, g0, w[1]);
#pragma unroll
            for (int j = 0; j < 4; j++) fetch_b(g0 + j, bb[j]);
        };
        fetch4(g_begin, wc, bc);
        for (size_t g = g_begin; g < g_end; g += 4)
        {
            fetch4(min(g + 4, g_end - 4), wn, bn);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const unsigned wj[2] = {wc[0][j], wc[1][j]};
                multiply(wj, bc[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                wc[0][j] = wn[0][j];
                wc[1][j] = wn[1][j];
#pragma unroll
                for (int kk = 0; kk < 3; kk++) bc[j][kk] = bn[j][kk];
            }
        }
    }
    // ---- split-K reduction, tile by tile, waves 0, 1, ... in that order ----
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int a = 0; a < 5; a++)
        {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; r++) s_red[wave][r][lane] = acc[u][a][r];
            __syncthreads();
            for (int e = tid; e < 16 * 64; e += 64 * kMxbWaves)
            {
                const int r = e >> 6, l = e & 63;
                float v = s_red[0][r][l];
#pragma unroll
                for (int wv = 1; wv < kMxbWaves; wv++) v += s_red[wv][r][l];
                // C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
                s_out[u][a][(r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][l & 31] = v;
            }
        }
    __syncthreads();
    // ---- every thread finishes a few (tile, marker, trait) triples ----
    for (int idx = tid; idx < 2 * 32 * pcount; idx += 64 * kMxbWaves)
    {
        const int t = idx % pcount, i = (idx / pcount) & 31, u = idx / (pcount * 32);
        const MxbTile tt = s_tile[u];
        const long long mi = (long long)tt.tile32 * 32 + i;
        if (!tt.valid || mi >= tt.m) continue;
        float sgy[3], svy[3];
#pragma unroll
        for (int q = 0; q < 3; q++)
        {
            const int c = q * kMxbTraits + t;
            sgy[q] = s_out[u][c >> 5][i][c & 31];
            svy[q] = s_out[u][2 + (c >> 5)][i][c & 31];
        }
        const float gy = (sgy[0] + sgy[1]) + sgy[2], vy = (svy[0] + svy[1]) + svy[2];
        const float cnt = s_out[u][4][i][kMxbOnes - 64] - s_out[u][4][i][t];
        const size_t mg = (size_t)(tt.row0 + mi);
        const float rr = (gy - mean[mg] * vy) / (cnt * sd[mg]);
        const size_t tg = p0 + (size_t)t;
        if (C)
        {
            float *Cb = C + tt.c_off;
            Cb[(size_t)mi * n + (size_t)tt.m + tg] = rr;
            Cb[((size_t)tt.m + tg) * n + (size_t)mi] = rr;
        }
        if (mxp) mxp[(size_t)tt.mxp_off + (size_t)mi * p + tg] = rr;
    }
}

// one workgroup per trait pair (a < b): corr_kernels.cu:285-343
__global__ void __launch_bounds__(256) pxp_kernel(const float *__restrict__ phen, float *C, size_t m, size_t N, size_t p,
                                                   size_t n)
{
    __shared__ float ss[256], sc[256];
    size_t lin = blockIdx.x, a = 0, len = p - 1;
    while (lin >= len)
    {
        lin -= len;
        len--;
        a++;
    }
    const size_t b = a + 1 + lin;
    float s = 0.0f, c = 0.0f;
    for (size_t i = threadIdx.x; i < N; i += 256)
    {
        const float va = phen[a * N + i], vb = phen[b * N + i];
        if (!((va != va) || (vb != vb)))
        {
            s += va * vb;
            c += 1.0f;
        }
    }
    ss[threadIdx.x] = s;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1)
    {
        if ((int)threadIdx.x < o)
        {
            ss[threadIdx.x] += ss[threadIdx.x + o];
            sc[threadIdx.x] += sc[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
    {
        const float r = ss[0] / sc[0];
        C[(m + a) * n + m + b] = r;
        C[(m + b) * n + m + a] = r;
    }
}
// ---- launchers (corr_kernels.h) ----
static_assert(sizeof(CorrTile2) == sizeof(int2), "CorrTile2 is read as int2");

int launch_mxp(cusk_engine *e, hipStream_t s, const MxpArgs &a)
{
    const int2 *mtile = reinterpret_cast<const int2 *>(a.mtile);
    if (a.form == MxpForm::Bf16 && a.p > 0)
    {
        // the bf16 form: exact three-piece split of the traits, 21 traits per launch
        const size_t G = (a.N + 63) / 64 * 4;  // groups of 16 individuals, in fours
        CUSK_HIP(e, e->mxp_bq.ensure(sizeof(unsigned short) * kMxbCols * G * 16));
        unsigned short *bq = e->mxp_bq.as<unsigned short>();
        auto *k = bed_rows16(a.bed, a.clb) ? mxp_bf16_kernel<true> : mxp_bf16_kernel<false>;
        for (size_t p0 = 0; p0 < a.p; p0 += kMxbTraits)
        {
            const int pc = (int)std::min<size_t>(kMxbTraits, a.p - p0);
            hipLaunchKernelGGL(mxp_split_kernel, dim3((unsigned)((3 * G * 64 + 255) / 256)), dim3(256), 0, s, a.phen, a.N, G, p0, pc, bq);
            hipLaunchKernelGGL(k, dim3((unsigned)((a.ntiles + 1) / 2)), dim3(64 * kMxbWaves), 0, s, a.bed, bq, a.mean, a.sd, a.C, a.mxp,
                               a.m, G, a.p, a.clb, a.n, p0, pc, a.ntiles, mtile, a.bblk);
        }
    }
    for (size_t p0 = 0; p0 < a.p && a.form == MxpForm::Scalar; p0 += kMaxPhenRegs)
        hipLaunchKernelGGL(mxp_kernel, dim3((unsigned)((a.m + 3) / 4)), dim3(256), 0, s, a.bed, a.phen, a.mean, a.sd, a.C, a.mxp, a.m, a.N,
                           a.p, a.clb, a.n, p0, std::min<size_t>(kMaxPhenRegs, a.p - p0));
    if (a.form != MxpForm::F32) return CUSK_OK;
    // dword-aligned .bed rows and 16-byte aligned trait rows: the FAST form of mxp_mfma_kernel
    const bool fast = (a.clb % 4 == 0) && (a.N % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.bed) & 3u) == 0) &&
                      ((reinterpret_cast<uintptr_t>(a.phen) & 15u) == 0);
    auto *k = fast ? mxp_mfma_kernel<true> : mxp_mfma_kernel<false>;
    for (size_t p0 = 0; p0 < a.p; p0 += kMaxPhenRegs)
        hipLaunchKernelGGL(k, dim3((unsigned)a.ntiles), dim3(64 * kMxpWaves), 0, s, a.bed, a.phen, a.mean, a.sd, a.C, a.mxp, a.m, a.N, a.p,
                           a.clb, a.n, p0, (int)std::min<size_t>(kMaxPhenRegs, a.p - p0), mtile, a.bblk);
    return CUSK_OK;
}

void launch_pxp(hipStream_t s, const float *phen, float *C, size_t m, size_t N, size_t p, size_t n)
{
    if (p > 1) hipLaunchKernelGGL(pxp_kernel, dim3((unsigned)(p * (p - 1) / 2)), dim3(256), 0, s, phen, C, m, N, p, n);
}

}  // namespace cusk
