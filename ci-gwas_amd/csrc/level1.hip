// level1.hip -- level 1: the pair kernel (cross-check), the row-streaming kernel with its set-up and apply passes.
// Replaces the reference's cal_Indepl1 (cusk/src/cuPC-S.cu:486-582) and its hetcor twin (src/hetcor-cuPC-S.cu).
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>

#include "ci_exact.h"
#include "ci_fast.h"
#include "sweep_common.h"

namespace cusk {

// ---------------------------------------------------------------------------
// level 1 on a symmetric matrix with a single threshold
// ---------------------------------------------------------------------------
// A level-1 test (X ; Y | S) needs C[X,Y], C[X,S] and C[Y,S]; the first two live in row X and
// are staged once, the third is used by exactly two tests, (X;Y|S) and (X;S|Y), so staging a
// (d+1)^2 sub-matrix buys no reuse.  Lane <-> unordered neighbour pair {a<b}: ONE 4-byte gather
// of the upper-triangle element C[min,max] feeds both tests, pairs whose two tests are already
// decided are skipped without touching memory, and with ~20 VGPRs the kernel runs at full
// occupancy to hide the gather latency.  Arithmetic is the exact level-1 formula
// (cuPC-S.cu:561-566), so nothing needs rechecking.
template <int MODE>
__global__ void __launch_bounds__(kThreads) level1_pair_kernel(SweepParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long s_cnt[3];
    const int n = p.n;
    const int tid = threadIdx.x;
    if (tid < 3) s_cnt[tid] = 0ull;
    unsigned long long ntests = 0, nrem = 0;
    // persistent launch: the work items of the class are read on the device (the host does not know their number)
    const long long nitems = level_items(p);
    for (long long it = blockIdx.x; it < nitems; it += gridDim.x)
    {
    if (it != (long long)blockIdx.x) __syncthreads();  // the previous item's readers are done with the LDS copy
    const int2 item = p.items[it];
    const int X = item.x;
    const int o0 = p.off[X];
    const int d = p.off[X + 1] - o0;
    unsigned long long *s_best = reinterpret_cast<unsigned long long *>(smem);
    int *s_nbr = reinterpret_cast<int *>(smem + sizeof(unsigned long long) * d);
    float *s_m1x = reinterpret_cast<float *>(s_nbr + d);
    int *s_ti = reinterpret_cast<int *>(s_m1x + d);
    const int *g_nbr = p.nbr + o0;
    for (int k = tid; k < d; k += kThreads)
    {
        const int y = g_nbr[k];
        s_nbr[k] = y;
        s_m1x[k] = p.C[(size_t)X * n + y];
        if constexpr (MODE == 0)
            s_best[k] = p.best[o0 + k];
        else
        {
            const unsigned long long wv = p.adj[(size_t)X * p.words + (y >> 6)];
            s_best[k] = ((wv >> (y & 63)) & 1ull) ? kNone : 0ull;
            s_ti[k] = p.time_index[y];
        }
    }
    __syncthreads();
    [[maybe_unused]] int tiX = 0;
    if constexpr (MODE == 1) tiX = p.time_index[X];

    const unsigned long long npairs = (unsigned long long)d * (d - 1) / 2;
    const unsigned long long r0 = (unsigned long long)item.y * p.chunk;
    const unsigned long long cntr = min(p.chunk, npairs - r0);
    const unsigned long long q = (cntr + kThreads - 1) / kThreads;
    const unsigned long long lo = r0 + (unsigned long long)tid * q;
    const unsigned long long hi = min(r0 + cntr, lo + q);
    if (lo < hi)
    {
        // unrank the pair: row a of the strict upper triangle starts at a*d - a(a+1)/2
        auto start_of = [&](int aa) -> unsigned long long {
            return (unsigned long long)aa * d - (unsigned long long)aa * (aa + 1) / 2;
        };
        const double dd = (double)d - 0.5;
        int a = (int)(dd - sqrt(fmax(dd * dd - 2.0 * (double)lo, 0.0)));
        a = max(0, min(a, d - 2));
        while (a > 0 && start_of(a) > lo) a--;
        while (a < d - 2 && start_of(a + 1) <= lo) a++;
        int b = a + 1 + (int)(lo - start_of(a));
        auto apply = [&](int ky, int ks) {
            // edge X - nbr[ky] is separated by S = nbr[ks]
            if constexpr (MODE == 0)
            {
                const unsigned long long old = atomicMin(&p.best[o0 + ky], (unsigned long long)ks);
                atomicMin(&s_best[ky], (unsigned long long)ks);
                if (old == kNone) nrem++;
            }
            else
            {
                if (clear_edge(p.adj, p.deg, p.words, X, s_nbr[ky])) nrem++;
                s_best[ky] = 0ull;
            }
        };
        for (unsigned long long it = lo; it < hi; it++)
        {
            bool needA, needB;  // A: Y = a, S = b ; B: Y = b, S = a
            if constexpr (MODE == 0)
            {
                needA = s_best[a] >= (unsigned long long)b;
                needB = s_best[b] >= (unsigned long long)a;
            }
            else
            {
                needA = (s_best[a] == kNone) && !(s_ti[b] > max(tiX, s_ti[a]));
                needB = (s_best[b] == kNone) && !(s_ti[a] > max(tiX, s_ti[b]));
            }
            if (needA || needB)
            {
                const int ya = s_nbr[a], yb = s_nbr[b];  // ascending lists: ya < yb
                const float c = p.C[(size_t)ya * n + yb];
                const float ra = s_m1x[a], rb = s_m1x[b];
                const float hc = 1.0f - (c * c);
                if (needA)
                {
                    const float H00 = 1.0f - (rb * rb);
                    const float H01 = ra - (rb * c);
                    const float rho = H01 / (sqrtf(fabsf(H00)) * sqrtf(fabsf(hc)));
                    ntests++;
                    if (z_below<true>(rho, p.th)) apply(a, b);
                }
                if (needB)
                {
                    const float H00 = 1.0f - (ra * ra);
                    const float H01 = rb - (ra * c);
                    const float rho = H01 / (sqrtf(fabsf(H00)) * sqrtf(fabsf(hc)));
                    ntests++;
                    if (z_below<true>(rho, p.th)) apply(b, a);
                }
            }
            b++;
            if (b == d)
            {
                a++;
                b = a + 1;
            }
        }
    }
    }  // work items
    for (int o = 32; o > 0; o >>= 1)
    {
        ntests += __shfl_xor(ntests, o);
        nrem += __shfl_xor(nrem, o);
    }
    __syncthreads();
    if ((tid & 63) == 0)
    {
        atomicAdd(&s_cnt[0], ntests);
        if (MODE == 1) atomicAdd(&s_cnt[2], nrem);  // Skeleton mode counts removals when it finalises the level
    }
    __syncthreads();
    if (tid == 0)
    {
        unsigned long long *sl = p.slots + (size_t)(blockIdx.x & (kCounterSlots - 1)) * 4;
        if (s_cnt[0]) atomicAdd(&sl[0], s_cnt[0]);
        if (s_cnt[2]) atomicAdd(&sl[2], s_cnt[2]);
    }
}

// Workgroups of a persistent launch: as many as the chip holds at once for this kernel (twice that, so that a
// workgroup that drew short items does not leave its slot empty), never more than the work-item buffer holds.
unsigned persistent_grid(const void *kernel, int threads, size_t lds)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, size_t>, unsigned> cache;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(kernel, lds);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int per_cu = 0, dev = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess || per_cu <= 0)
    {
        (void)hipGetLastError();
        per_cu = 1;
    }
    if (hipGetDevice(&dev) == hipSuccess)
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    const unsigned g = (unsigned)std::max(1, per_cu) * (unsigned)cus * 2u;
    cache[key] = g;
    return g;
}

hipError_t launch_pair(int mode, const SweepParams &p, size_t lds, hipStream_t st)
{
    const void *kf = mode == 0 ? reinterpret_cast<const void *>(level1_pair_kernel<0>) : reinterpret_cast<const void *>(level1_pair_kernel<1>);
    const unsigned grid = (unsigned)std::min<long long>(persistent_grid(kf, kThreads, lds), std::max<long long>(p.grid_cap, 1));
    if (mode == 0)
        hipLaunchKernelGGL(level1_pair_kernel<0>, dim3(grid), dim3(kThreads), lds, st, p);
    else
        hipLaunchKernelGGL(level1_pair_kernel<1>, dim3(grid), dim3(kThreads), lds, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// level 1, row-streaming form (symmetric C, single threshold): HBM traffic = C once
// ---------------------------------------------------------------------------
// The pair kernel above pays one 64-byte HBM sector for every 4-byte operand C[Y,S], because a workgroup owns an
// X and its operands C[ya, yb] are scattered over as many rows as X has neighbours.  Here the loop nest is turned
// inside out: a workgroup owns one ROW ya of C and runs every level-1 test that needs an element of that row:
// for each X adjacent to ya and each later neighbour yb of X, the element C[ya,yb] feeds the two tests
// (X; ya | yb) and (X; yb | ya).  All of the workgroup's reads of C fall into that one row (and, with LD, mostly
// into a narrow window behind the diagonal), so HBM sees each touched sector once and L1/L2 serve the rest.
// Everything else those tests need is per-edge data that was compacted at level start and is read contiguously:
// the neighbour list of X, the gathered row values rv = C[X, adj(X)], and meta (position of ya inside X's list); the
// selection state sel is only written (fire-and-forget minima).

// Per CSR slot (row, k) with Y = nbr_k:  rv = C[row, Y];  meta = {Y, position of row inside Y's ascending
// list, start of Y's list, degree of Y};  sel = kNone32 (no separating set yet).
constexpr unsigned kNone32 = 0xffffffffu;

__global__ void level1_prep_kernel(const float *__restrict__ C, const int *__restrict__ off, const int *__restrict__ nbr,
                                   const unsigned long long *__restrict__ adj, const int *__restrict__ wpre, int words,
                                   float *rv, int4 *meta, unsigned *sel, int n, const LevelCounters *cnt)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n || !cnt->active) return;
    const int o0 = off[row], d = off[row + 1] - o0;
    const int rw = row >> 6;
    const unsigned long long below = (1ull << (row & 63)) - 1ull;
    for (int k = lane; k < d; k += 64)
    {
        const int y = nbr[o0 + k];
        rv[o0 + k] = C[(size_t)row * n + y];
        sel[o0 + k] = kNone32;
        // position of `row` in y's ascending list = neighbours of y below `row`: the word prefix written by
        // fill_nbr plus one popcount -- two independent loads instead of a binary search
        const int pos = wpre[(size_t)y * words + rw] + __popcll(adj[(size_t)y * words + rw] & below);
        meta[o0 + k] = make_int4(y, pos, off[y], off[y + 1] - off[y]);
    }
}

// HET sibling of level1_prep_kernel: nv = ess_term(N[row, Y]) per CSR slot, the sizes N[X, .] of the row kernel's tests
// (int-truncated once here, as ess_term does it, instead of in every step of the sweep).  The row kernel runs only on a
// bitwise symmetric N, so N[row, Y] stands for the N[Y][row] that ess_threshold_exact reads.
__global__ void level1_prep_nv_kernel(const float *__restrict__ N, const int *__restrict__ off, const int *__restrict__ nbr, float *nv,
                                      int n, const LevelCounters *cnt)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n || !cnt->active) return;
    const int o0 = off[row], d = off[row + 1] - o0;
    for (int k = lane; k < d; k += 64) nv[o0 + k] = ess_term(N[(size_t)row * n + nbr[o0 + k]]);
}

struct RowsParams
{
    const float *rv;
    const int4 *meta;
    unsigned *sel;   // level-1 selection state per CSR slot: lowest passing position (Skeleton) / 0 = edge gone (hetcor)
    int use_filter;  // 0: every test on the exact arithmetic (thresholds too small for the guard band)
    int has_ti;      // hetcor engine: a time index was given (else every index is 0 and the rule excludes nothing)
    float beta;      // half-width of the level-1 guard band on rho^2 (level1_beta)
    int shard_rank, shard_world;  // row-sharded runs: this engine streams the rows ya with ya % world == rank
    // HET form (per-pair sample sizes, level1_rows2_kernel<..., HET = true>)
    const float *nv;  // per CSR slot: ess_term(N[X, Y]), gathered at level start next to rv (level1_prep_nv_kernel)
    float th2;        // th^2: the filter's estimate of a test's threshold starts from th^2 / (mean size - 4)
    int nrow_off;     // LDSROW: the row of N follows the row of C in LDS at this distance (floats, a multiple of 4)
};

// Half-width of the level-1 guard band on rho^2.  Unlike the deeper levels (Cholesky against SVD, conditioning-dependent:
// kBeta) the two forms of the level-1 test share their operands, so the band only has to cover rounding: the exact form's
// rho carries <= 4 roundings (2.4e-7 relative), its Fisher z (two correctly rounded logs of 1 +- rho) <= 5.6e-8 absolute,
// i.e. <= 5.6e-8 / t relative in rho at the decision point |rho| = t = tanh(th); the squared form adds <= 5 roundings
// (3e-7 relative on rho^2).  Sixteen times that sum, never more than kBeta: 7.6e-5 at the headline threshold
// (t = 0.0304) instead of 2e-3 -- with the wide band a quarter of all 256-test wave steps had a lane in the band and
// went through the exact form (division, two square roots, log), which was 40 % of the kernel's vector instructions.
inline float level1_beta(float t2)
{
    const double t = std::sqrt(std::max((double)t2, 1e-30));
    return (float)std::min((double)kBeta, 16.0 * (2.0 * (2.4e-7 + 5.6e-8 / t) + 3.0e-7));
}

// Level-1 test, rho = h01 / (sqrt|h00| sqrt|hc|) against th, in the squared form with the guard band of
// ci_fast.h (level1_beta wide).  It starts from the SAME fp32 h00, h01, hc as the reference's form (identical operations), so
// unlike the deeper levels no conditioning margin is needed: the two differ by a few ulp whatever the
// operands are, as long as they are positive.  Returns pass; sure = false (inside the band, operand <= 0, NaN,
// filter off) sends the lane to level1_exact.
__device__ __forceinline__ bool level1_filter(float h00, float h01, float hc, float t2, float beta, bool ok, bool &sure)
{
    const float lhs = h01 * h01;
    const float rhs = t2 * (h00 * hc);
    const bool pass = lhs < rhs * (1.0f - beta);
    const bool fail = lhs > rhs * (1.0f + beta);
    sure = ok && (h00 > 0.0f) && (pass || fail);
    return pass;
}

__device__ __forceinline__ bool level1_exact(float h00, float h01, float hc, float th)
{
    const float rho = h01 / (sqrtf(fabsf(h00)) * sqrtf(fabsf(hc)));
    return z_below<true>(rho, th);
}

template <typename T>
__device__ __forceinline__ T ld32(const T *base, unsigned idx)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (idx << 2));
}

// ---------------------------------------------------------------------------------------------------------------
// Work of a row: for every neighbour X (list position a of the row inside X's list) the segment of later
// positions b in (a, deg X).  The segments of one staging round (THREADS neighbours) are laid end to end (block scan,
// empty ones dropped) and every wave takes a contiguous share of that flat range, 64 entries per step, so lanes stay
// busy whatever the segment lengths are; a lane finds its segment by walking the LDS prefix array from the
// wave's current segment.  The flat range counts PAIRS of positions (b, b + 1) of a segment (odd segments are padded
// by one masked position, so a pair never straddles two segments): a sweep with one position per lane is bound by
// vector-instruction issue, not by memory (136 vector instructions per 64 positions, 67 % of the SIMDs' issue cycles at
// 0.40 ms on the 10k block), and two thirds of those instructions are bookkeeping of the flattened iteration space that
// does not depend on how many positions a lane carries: the walk over the segment prefix array, slot arithmetic,
// segment-head detection, loop control.  A step is a three-stage software pipeline over five operand sets
// (CUSK_ROWS_SETS; the depth is explained at the rotation below):
//   stage A (four steps ahead): both list entries with one 8-byte load each (nbr and rv of X at b, b + 1: 4-byte
//                       aligned dwordx2);
//   stage B (one step ahead):  C[row, yb] for both -- consecutive lanes hold ascending, mostly adjacent columns of ONE
//                       row of C, staged in LDS (LDSROW) or gathered through L1/L2;
//   stage C:            the four tests as float2 pairs (v_pk_mul_f32 / v_pk_add_f32) through the branch-free filter --
//                       the same fp32 operations in the same order per element as level1_filter -- and fire-and-forget
//                       minima.
// The list entries are addressed by 32-bit byte offsets off uniform bases (the CSR arrays stay below 4 GB): scalar-base
// addressing, no 64-bit vector address arithmetic.  No selection-state reads: every pair is evaluated.  The minima do
// not depend on them, the reads were a third of the kernel's list traffic, and a state that other XCDs update past this
// XCD's L2 skipped little (measured: 0.49 -> 0.40 ms on the 10k block).
#ifndef CUSK_ROWS_SETS
#define CUSK_ROWS_SETS 5
#endif
typedef float rows_f2 __attribute__((ext_vector_type(2)));
typedef float rows_f4 __attribute__((ext_vector_type(4)));
typedef int rows_i2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float rows_f2u __attribute__((ext_vector_type(2), aligned(4)));

struct RowsStep2
{
    unsigned ia, ib;  // slots of (X, a) and of (X, b)
    int a, b, X, first_lane;
    bool in0, in1;  // position b / b + 1 is a real position of this wave's range
    rows_i2u nb;    // list entries at b, b + 1 (the second one is only meaningful when in1)
    rows_f2u rbu;
    int yb0, yb1;
    float ra;
    rows_f2 c;
    // HET: the three sizes of the lane's two pairs, int-truncated: N[X, yb] (both positions), N[X, ya], N[ya, yb]
    rows_f2u nbu;
    float na;
    rows_f2 nab;
};

// LDSROW: the columns [ya, n) of the workgroup's row of C are staged in LDS once (coalesced 16-byte loads) and the
// C[ya, yb] gathers of stage B become LDS reads: with the gathers going through L1/L2 the rows of all resident workgroups
// (40 KB each at n = 10,020, five per CU) evict each other and the per-edge streams -- 2.3 GB of L2 fills per launch for
// a 401 MB matrix, which is what bounds the kernel once the instruction count is down (37 % vector issue).  THREADS grows
// with n so that the CU keeps its waves when fewer rows fit into its 160 KB (launch_level1_rows).
//
// HET (cusk_run_skeleton_het / _batch_het with option het_rows, MODE 0 only): every test is decided at the sample sizes of
// its own three pairs.  The two tests of a lane's pair, (X; ya | yb) and (X; yb | ya), are about the same variables, and on
// a bitwise symmetric N (the engine checks: ess_symmetry_kernel) they read the same three sizes: N[X, yb] arrives with the
// list entries in stage A (rp.nv beside rp.rv), N[X, ya] per segment in the place of X in s_seg (MODE 0 never reads X), and
// N[ya, yb] lies in row ya of N, staged in LDS behind the row of C (LDSROW, already int-truncated) or read through L1/L2.
// The exact threshold of a test is RowView::ess_threshold_exact<1>: s = (N[Y][X] + N[S][X]) + N[S][Y] in float, me = s / 3,
// lth = (float)((double)th / sqrt((double)me - 1 - 3)).  Float addition commutes, so the two tests of a pair share s and lth.
// The filter judges both at a float estimate of tanh(lth)^2 that needs no square root:
//     u = th^2 / (me - 4) = lth^2,   tanh(x)^2 = u P(u)^2,   P(u) = tanh(x) / x = 1 - u/3 + 2u^2/15 - 17u^3/315 + 62u^4/2835 - ...
// and certifies a verdict only where  me - 4 >= 64,  kHetUMin <= u <= 1/16  (lth between kThMinFilter, below which no filter
// of this engine is certified, and 1/4; a mean size of a few hundred and more at the usual alpha).  Everything else -- small
// or huge sizes, a NaN or non-positive radicand -- is "not sure" and goes to level1_exact at the exact lth.
// Relative error of the estimate against tanh(lth)^2 of the exact float lth, 2^-24 = 6e-8 per rounding:
//   s:      the same three terms; summed here in the order of ess_threshold_exact, but the bound does not rely on it: two
//           additions of integers that can pass 2^24 at biobank sizes, any order within 2 x 6e-8 of any other  1.2e-7
//   me:     s * fl(1/3) against fl(s / 3): constant, product, the exact form's quotient                          1.8e-7
//   me - 4: both carried over with me / (me - 4) <= 68/64, plus the subtraction's rounding                      3.8e-7
//   u:      fl(th^2) from the host, v_rcp_f32 (1 ulp), the product                                      + 2.4e-7 = 6.2e-7
//   lth:    the exact form computes in double (1e-16) and rounds lth to float once: 6e-8 on lth, 1.2e-7 on lth^2  7.4e-7
//   tanh^2: d ln(u P^2) / d ln u lies in (0, 1] (P falls with u), so the 7.4e-7 carry over at most unchanged;
//           the series cut behind u^4 (alternating, next term 8.9e-3 u^5 <= 8.5e-9 of P); Horner in float, every inner
//           error scaled by u <= 1/16: 1e-7 on P; the square and the product with u                      + 3.4e-7 = 1.1e-6
// The band is level1_beta's own expression at the test's t = tanh(lth) (16 (2 (2.4e-7 + 5.6e-8 / t) + 3e-7), with
// 1 / t = v_rsq_f32 of the estimate; u >= kHetUMin keeps it below kBeta: 9.2e-4 at t = 2e-3) widened by kHetWiden = 4e-6,
// more than three times the 1.1e-6 above: a lane the filter certifies at the estimate lies outside level1_beta's band
// around the exact tanh(lth)^2.  tests/test_cusk_het_rows_formats.py restates estimate and band in numpy.
constexpr float kHetUMin = 4.1e-6f;   // lth^2 >= kThMinFilter^2 = 4e-6 with the estimate's error to spare
constexpr float kHetUMax = 0.0625f;   // lth <= 1/4: range of the series
constexpr float kHetDMin = 64.0f;     // me - 4
constexpr float kHetWiden = 4.0e-6f;
constexpr float kHetBeta0 = 16.0f * (2.0f * 2.4e-7f + 3.0e-7f) + kHetWiden;  // level1_beta's terms that do not depend on t
constexpr float kHetBeta1 = 16.0f * 2.0f * 5.6e-8f;                          // ... times 1 / t

template <int MODE, bool VALIDATE, int THREADS, bool LDSROW, bool HET = false>
__global__ void __launch_bounds__(THREADS) level1_rows2_kernel(SweepParams p, RowsParams rp)
{
    static_assert(!HET || MODE == 0, "per-pair sample sizes: Skeleton mode only");
    constexpr int kRowsThreads = THREADS, kRowsChunk = THREADS;
    __shared__ int4 s_seg[kRowsChunk];  // {slot of (X, a), a, C[X, row] bits, X}
    __shared__ int s_dx[kRowsChunk];    // degree of X
    __shared__ int s_pre[kRowsChunk + 1];
    __shared__ int s_wtot[2][kRowsThreads / 64];
    __shared__ unsigned long long s_cnt[HET ? 3 : 2];  // executed tests, filter violations (VALIDATE), HET: tests the filter did not certify
    extern __shared__ __attribute__((aligned(16))) float s_row[];  // LDSROW: s_row[col + sh] = C[ya, col], col >= ya
    const int n = p.n;
    // (Rows to XCDs, tried in round 3: XCD x takes the x-th and (15 - x)-th sixteenth of the rows instead of every eighth
    // row, so that an L2 keeps re-reading the lists of one region: 0.387 ms against 0.255.  Consecutive rows running at the
    // same time on all XCDs already share their lists in time, and whole regions per XCD unbalance dense and sparse ones.)
    const int ya = blockIdx.x;
    if (ya + 1 >= n) return;
    if (rp.shard_world > 1 && ya % rp.shard_world != rp.shard_rank) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kRowsThreads >> 6;
    const float *crow = p.C + (size_t)ya * n;
    [[maybe_unused]] int sh = 0;
    // LDS index = column + sh with sh = (element offset of the row) mod 4: 16-byte aligned global loads land on
    // 16-byte aligned LDS addresses whatever n is.  Only columns >= ya are ever asked for (yb follows ya in an
    // ascending list; idle lanes ask for ya itself).  The rounded-down head and rounded-up tail read at most three
    // elements of the neighbouring rows (ya >= 1 whenever the head reaches back, ya <= n - 2 always).
    // Batched runs stage the columns of the row's own block only, [ya, hi), at LDS index column - lo + sh0 (lo, the
    // block's base, is a multiple of 64 and keeps the alignment).
    // Every request is unconditional (a start past the end is clamped to the last 16-byte piece of the range: those lanes
    // repeat that piece, load and store, same bytes to the same place) and the four pieces of a pass live in four named
    // registers: with `if (iu < i_end) v[u] = ...` on an array the compiler kept the array in scratch memory and waited
    // for each load before the next (rounds 2 and 3a: 0.31 ms for this kernel instead of 0.27).  Non-temporal: the row
    // is read once, by this workgroup only, and should not push the neighbour lists and the selection words of the other
    // rows out of the L2.  The first pass (all of the row up to 16 x THREADS columns) is requested right behind the
    // per-neighbour records and before the gather that depends on them: the row streams in beside those two round trips.
    constexpr int kStep = THREADS * 4;
    [[maybe_unused]] const float *gbase = nullptr;
    [[maybe_unused]] int i_first = 0, i_end = 0, i_last = 0, i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    [[maybe_unused]] rows_f4 v0, v1, v2, v3;
    // (the activity flag and the list bounds in ONE scalar round trip: left alone, the compiler waits for the flag before it
    // asks for the bounds)
    const int act = p.cnt->active;
    const int o0 = p.off[ya], o1 = p.off[ya + 1];
    asm volatile("" ::"s"(act), "s"(o0), "s"(o1));
    if (!act) return;
    const int d = o1 - o0;
    if (d == 0) return;
    if (tid < (HET ? 3 : 2)) s_cnt[tid] = 0ull;
    int4 m = make_int4(0, 0, 0, 0);
    float mra = 0.0f;
    [[maybe_unused]] float mna = 0.0f;  // HET: ess_term(N[X, row])
    if (tid < d) m = rp.meta[o0 + tid];
    if constexpr (LDSROW)
    {
        const size_t g0 = (size_t)ya * n;
        const int sh0 = (int)(g0 & 3);
        int lo = 0, hi = n;
        if (p.row_range)
        {
            const int2 rg = p.row_range[ya];
            lo = rg.x;
            hi = rg.y;
        }
        sh = sh0 - lo;
        gbase = p.C + (g0 - sh0) + lo;  // 16-byte aligned (p.C is: checked by the launcher)
        i_end = hi - lo + sh0;
        i_last = (i_end - 1) & ~3;
        i_first = ((ya - lo + sh0) & ~3) + tid * 4;
        i0 = min(i_first, i_last), i1 = min(i_first + kStep, i_last), i2 = min(i_first + 2 * kStep, i_last), i3 = min(i_first + 3 * kStep, i_last);
        v0 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i0));
        v1 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i1));
        v2 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i2));
        v3 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i3));
        asm volatile("" ::: "memory");  // the row's requests stay between the record load and its dependent gather
    }
    if (tid < d) mra = rp.rv[m.z + m.y];  // C[X, row]
    if constexpr (HET)
        if (tid < d) mna = rp.nv[m.z + m.y];
    if constexpr (LDSROW)
    {
        *reinterpret_cast<rows_f4 *>(s_row + i0) = v0;
        *reinterpret_cast<rows_f4 *>(s_row + i1) = v1;
        *reinterpret_cast<rows_f4 *>(s_row + i2) = v2;
        *reinterpret_cast<rows_f4 *>(s_row + i3) = v3;
        for (int i = i_first + kStep * 4; i < i_end; i += kStep * 4)
        {
            i0 = min(i, i_last), i1 = min(i + kStep, i_last), i2 = min(i + 2 * kStep, i_last), i3 = min(i + 3 * kStep, i_last);
            v0 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i0));
            v1 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i1));
            v2 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i2));
            v3 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(gbase + i3));
            *reinterpret_cast<rows_f4 *>(s_row + i0) = v0;
            *reinterpret_cast<rows_f4 *>(s_row + i1) = v1;
            *reinterpret_cast<rows_f4 *>(s_row + i2) = v2;
            *reinterpret_cast<rows_f4 *>(s_row + i3) = v3;
        }
        // visible to every wave after the first barrier of the staging round below
        if constexpr (HET)
        {  // the same columns of row ya of N (same allocation shape and alignment as C: checked by the launcher), int-truncated
            // once here; they land rp.nrow_off floats behind the row of C
            const float *nbase = p.Ness + (gbase - p.C);
            float *s_nrow = s_row + rp.nrow_off;
            auto trunc4 = [](rows_f4 v) -> rows_f4 { return rows_f4{ess_term(v.x), ess_term(v.y), ess_term(v.z), ess_term(v.w)}; };
            for (int i = i_first; i < i_end; i += kStep * 4)
            {
                i0 = min(i, i_last), i1 = min(i + kStep, i_last), i2 = min(i + 2 * kStep, i_last), i3 = min(i + 3 * kStep, i_last);
                v0 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(nbase + i0));
                v1 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(nbase + i1));
                v2 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(nbase + i2));
                v3 = __builtin_nontemporal_load(reinterpret_cast<const rows_f4 *>(nbase + i3));
                *reinterpret_cast<rows_f4 *>(s_nrow + i0) = trunc4(v0);
                *reinterpret_cast<rows_f4 *>(s_nrow + i1) = trunc4(v1);
                *reinterpret_cast<rows_f4 *>(s_nrow + i2) = trunc4(v2);
                *reinterpret_cast<rows_f4 *>(s_nrow + i3) = trunc4(v3);
            }
        }
    }
    [[maybe_unused]] const float *nrow = nullptr;  // HET, gather form: row ya of N through L1/L2
    if constexpr (HET && !LDSROW) nrow = p.Ness + (size_t)ya * n;
    [[maybe_unused]] int tiA = 0;
    if constexpr (MODE == 1) tiA = p.time_index[ya];
    const bool use_filter = rp.use_filter != 0;
    const float th = p.th, t2 = p.t2, beta = rp.beta;
    [[maybe_unused]] const float th2 = rp.th2;
    unsigned ntests = 0, viol = 0;
    [[maybe_unused]] unsigned nslow = 0;  // HET: tests sent to the exact form because the filter was not sure (cusk_stats.rechecks[1])
    const bool count_by_segment = (MODE == 0) || !rp.has_ti;
    for (int kc = 0; kc < d; kc += kRowsChunk)
    {
        // ---- lay the non-empty segments of this round end to end, counted in pairs of positions ----
        const int len = (kc + tid < d) ? max(0, m.w - m.y - 1) : 0;
        const int plen = (len + 1) >> 1;
        // executed tests: without a time-index rule every position of a segment is tested in both directions -- counted
        // here once per segment instead of four flag additions per lane and step
        if (count_by_segment) ntests += 2u * (unsigned)len;
        int pos = (plen > 0) ? 1 : 0, pre = plen;
        for (int o = 1; o < 64; o <<= 1)
        {
            const int v1 = __shfl_up(pos, o), v2 = __shfl_up(pre, o);
            if (lane >= o)
            {
                pos += v1;
                pre += v2;
            }
        }
        if (kc > 0) __syncthreads();  // the previous round's readers are done with s_seg / s_pre / s_wtot
        if (lane == 63)
        {
            s_wtot[0][wave] = pos;
            s_wtot[1][wave] = pre;
        }
        __syncthreads();
        int nseg = 0, total = 0, pos0 = 0, pre0 = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++)
        {
            const int c1 = s_wtot[0][w], c2 = s_wtot[1][w];
            if (w < wave)
            {
                pos0 += c1;
                pre0 += c2;
            }
            nseg += c1;
            total += c2;
        }
        if (plen > 0)
        {
            if constexpr (HET)
                s_seg[pos0 + pos - 1] = make_int4(m.z + m.y, m.y, __float_as_int(mra), __float_as_int(mna));
            else
                s_seg[pos0 + pos - 1] = make_int4(m.z + m.y, m.y, __float_as_int(mra), m.x);
            s_dx[pos0 + pos - 1] = m.w;
            s_pre[pos0 + pos - 1] = pre0 + pre - plen;
        }
        if (tid == 0) s_pre[nseg] = total;
        if (kc + kRowsChunk + tid < d)
        {  // next round, in flight meanwhile
            m = rp.meta[o0 + kc + kRowsChunk + tid];
            mra = rp.rv[m.z + m.y];
            if constexpr (HET) mna = rp.nv[m.z + m.y];
        }
        __syncthreads();
        // ---- this wave's contiguous share of the flat range ----
        const int per = ((total + kWaves * 64 - 1) / (kWaves * 64)) * 64;
        const int f_begin = wave * per, f_end = min(total, f_begin + per);
        if (f_begin >= f_end) continue;
        int kw = 0;
        {
            int hi = nseg;  // largest kw with s_pre[kw] <= f_begin
            while (hi - kw > 1)
            {
                const int mid = (kw + hi) >> 1;
                if (s_pre[mid] <= f_begin)
                    kw = mid;
                else
                    hi = mid;
            }
        }
        // stage A: locate the lanes of a step inside the segments and request the per-slot operands.  Lanes past the
        // end of the wave's range idle on slot a of the last segment (their "neighbour" is the row itself), so every
        // request is unconditional.
        auto stage_a = [&](int base, RowsStep2 &st) {
            const int f = base + lane;
            st.in0 = f < f_end;
            int kk = kw;
            if (st.in0)
                while (s_pre[kk + 1] <= f) kk++;
            kw = __shfl(kk, 63);
            const int seg0 = s_pre[kk];
            const int4 e = s_seg[kk];
            const int dX = s_dx[kk];
            const int r = st.in0 ? 2 * (f - seg0) + 1 : 0;
            st.a = e.y;
            st.b = e.y + r;
            st.in1 = st.in0 && (st.b + 1 < dX);
            st.ra = __int_as_float(e.z);
            if constexpr (HET)
                st.na = __int_as_float(e.w);
            else
                st.X = e.w;
            st.first_lane = max(0, seg0 - base);
            st.ia = (unsigned)e.x;
            st.ib = (unsigned)(e.x + r);
            st.nb = *reinterpret_cast<const rows_i2u *>(reinterpret_cast<const char *>(p.nbr) + (st.ib << 2));
            st.rbu = *reinterpret_cast<const rows_f2u *>(reinterpret_cast<const char *>(rp.rv) + (st.ib << 2));
            if constexpr (HET) st.nbu = *reinterpret_cast<const rows_f2u *>(reinterpret_cast<const char *>(rp.nv) + (st.ib << 2));
        };
        auto stage_b = [&](RowsStep2 &st) {
            st.yb0 = st.nb.x;
            st.yb1 = st.in1 ? st.nb.y : st.nb.x;  // the entry behind an odd segment belongs to another list
            if constexpr (LDSROW)
            {
                st.c.x = s_row[st.yb0 + sh];
                st.c.y = s_row[st.yb1 + sh];
            }
            else
            {
                st.c.x = ld32<float>(crow, (unsigned)st.yb0);
                st.c.y = ld32<float>(crow, (unsigned)st.yb1);
            }
            if constexpr (HET)
            {
                if constexpr (LDSROW)
                {
                    st.nab.x = s_row[st.yb0 + sh + rp.nrow_off];
                    st.nab.y = s_row[st.yb1 + sh + rp.nrow_off];
                }
                else
                {
                    st.nab.x = ess_term(ld32<float>(nrow, (unsigned)st.yb0));
                    st.nab.y = ess_term(ld32<float>(nrow, (unsigned)st.yb1));
                }
            }
        };
        auto stage_c = [&](const RowsStep2 &cur) {
            const int a = cur.a, b = cur.b;
            const float ra = cur.ra;
            const rows_f2 c = cur.c;
            const rows_f2 rb = {cur.rbu.x, cur.rbu.y};
            bool needA0, needB0, needA1, needB1;  // A: Y = ya, S = yb ; B: Y = yb, S = ya
            if constexpr (MODE == 0)
            {
                needA0 = needB0 = cur.in0;
                needA1 = needB1 = cur.in1;
            }
            else if (rp.has_ti)
            {
                const int tiX = p.time_index[cur.X], tiB0 = p.time_index[cur.yb0], tiB1 = p.time_index[cur.yb1];
                needA0 = cur.in0 && !(tiB0 > max(tiX, tiA));
                needB0 = cur.in0 && !(tiA > max(tiX, tiB0));
                needA1 = cur.in1 && !(tiB1 > max(tiX, tiA));
                needB1 = cur.in1 && !(tiA > max(tiX, tiB1));
            }
            else
            {  // no time index given (all equal): the rule excludes nothing, and its three gathers per lane and step go
                needA0 = needB0 = cur.in0;
                needA1 = needB1 = cur.in1;
            }
            // per element exactly the operations of level1_filter: 1 - (c c), ra - (rb c), t2 ((h00) (hc)), ...
            const rows_f2 one = {1.0f, 1.0f}, rav = {ra, ra};
            const rows_f2 hc = one - (c * c);
            const rows_f2 h00a = one - (rb * rb), h01a = rav - (rb * c);
            const float h00b = 1.0f - (ra * ra);
            const rows_f2 h00bv = {h00b, h00b}, h01b = rb - (rav * c);
            // HET: the estimate of tanh(lth)^2 and the band of the header comment, per pair (both tests of a pair share them)
            std::conditional_t<HET, rows_f2, float> t2x, bex;
            [[maybe_unused]] rows_f2 ssum;  // the float sum of the pair's three sizes, in the order of ess_threshold_exact<1>
            bool okn0 = true, okn1 = true;
            if constexpr (HET)
            {
                const rows_f2 nav = {cur.na, cur.na}, nbv = {cur.nbu.x, cur.nbu.y};
                ssum = (nav + nbv) + cur.nab;
                const rows_f2 dm = ssum * 0.33333334f - 4.0f;
                const rows_f2 u = {th2 * __builtin_amdgcn_rcpf(dm.x), th2 * __builtin_amdgcn_rcpf(dm.y)};
                const rows_f2 pu = one + u * (-0.33333334f + u * (0.13333334f + u * (-0.053968254f + u * 0.021869488f)));
                t2x = u * (pu * pu);
                bex = rows_f2{kHetBeta0 + kHetBeta1 * __builtin_amdgcn_rsqf(t2x.x), kHetBeta0 + kHetBeta1 * __builtin_amdgcn_rsqf(t2x.y)};
                // (every comparison is false for a NaN: sizes whose sum or estimate is not a number are "not sure")
                okn0 = (dm.x >= kHetDMin) && (u.x >= kHetUMin) && (u.x <= kHetUMax);
                okn1 = (dm.y >= kHetDMin) && (u.y >= kHetUMin) && (u.y <= kHetUMax);
            }
            else
            {
                t2x = t2;
                bex = beta;
            }
            const rows_f2 lhsA = h01a * h01a, rhsA = t2x * (h00a * hc);
            const rows_f2 lhsB = h01b * h01b, rhsB = t2x * (h00bv * hc);
            const rows_f2 loA = rhsA * (1.0f - bex), hiA = rhsA * (1.0f + bex);
            const rows_f2 loB = rhsB * (1.0f - bex), hiB = rhsB * (1.0f + bex);
            const bool ok0 = use_filter && (hc.x > 0.0f) && okn0, ok1 = use_filter && (hc.y > 0.0f) && okn1, okb = h00b > 0.0f;
            bool passA0 = lhsA.x < loA.x, passA1 = lhsA.y < loA.y, passB0 = lhsB.x < loB.x, passB1 = lhsB.y < loB.y;
            const bool sureA0 = ok0 && (h00a.x > 0.0f) && (passA0 || lhsA.x > hiA.x);
            const bool sureA1 = ok1 && (h00a.y > 0.0f) && (passA1 || lhsA.y > hiA.y);
            const bool sureB0 = ok0 && okb && (passB0 || lhsB.x > hiB.x);
            const bool sureB1 = ok1 && okb && (passB1 || lhsB.y > hiB.y);
            if (!count_by_segment) ntests += (needA0 ? 1u : 0u) + (needB0 ? 1u : 0u) + (needA1 ? 1u : 0u) + (needB1 ? 1u : 0u);
            const bool slowA0 = needA0 && (VALIDATE || !sureA0), slowB0 = needB0 && (VALIDATE || !sureB0);
            const bool slowA1 = needA1 && (VALIDATE || !sureA1), slowB1 = needB1 && (VALIDATE || !sureB1);
            if (__ballot(slowA0 || slowB0 || slowA1 || slowB1) != 0ull)
            {  // rare: the reference's operation order
                // HET: the exact threshold of ess_threshold_exact<1> for the pair, lth = (float)((double)th / sqrt((double)me - 1 - 3))
                // with me = s / 3 and s = (N[Y][X] + N[S][X]) + N[S][Y]: (X; ya | yb) sums (na + nb) + nab and (X; yb | ya)
                // (nb + na) + nab, the same float, so one lth per pair serves both orientations.  A NaN size counts as 0
                // (ess_term).  A negative radicand (mean size below 4) gives a NaN threshold exactly as on the exact sweep:
                // z < NaN is false and the edge stays -- no special case.
                [[maybe_unused]] float lth0 = th, lth1 = th;
                if constexpr (HET)
                {
                    const float me0 = ssum.x / 3.0f, me1 = ssum.y / 3.0f;
                    lth0 = (float)((double)th / sqrt((double)me0 - 1.0 - 3.0));
                    lth1 = (float)((double)th / sqrt((double)me1 - 1.0 - 3.0));
                }
                if constexpr (HET)
                    nslow += (needA0 && !sureA0 ? 1u : 0u) + (needB0 && !sureB0 ? 1u : 0u) + (needA1 && !sureA1 ? 1u : 0u) +
                             (needB1 && !sureB1 ? 1u : 0u);
                if (slowA0)
                {
                    const bool ex = level1_exact(h00a.x, h01a.x, hc.x, HET ? lth0 : th);
                    if (VALIDATE && sureA0 && ex != passA0) viol++;
                    passA0 = ex;
                }
                if (slowB0)
                {
                    const bool ex = level1_exact(h00b, h01b.x, hc.x, HET ? lth0 : th);
                    if (VALIDATE && sureB0 && ex != passB0) viol++;
                    passB0 = ex;
                }
                if (slowA1)
                {
                    const bool ex = level1_exact(h00a.y, h01a.y, hc.y, HET ? lth1 : th);
                    if (VALIDATE && sureA1 && ex != passA1) viol++;
                    passA1 = ex;
                }
                if (slowB1)
                {
                    const bool ex = level1_exact(h00b, h01b.y, hc.y, HET ? lth1 : th);
                    if (VALIDATE && sureB1 && ex != passB1) viol++;
                    passB1 = ex;
                }
            }
            passA0 = passA0 && needA0;
            passB0 = passB0 && needB0;
            passA1 = passA1 && needA1;
            passB1 = passB1 && needB1;
            // Y = ya: positions ascend with the lane inside a segment (and b before b + 1 inside a lane), so the lowest
            // passing lane of a segment carries the segment's minimum; only that lane speaks
            const bool anyA = passA0 || passA1;
            const unsigned long long pa = __ballot(anyA);
            const unsigned long long below = pa & ((1ull << lane) - 1ull) & ~((1ull << cur.first_lane) - 1ull);
            const bool headA = anyA && (below == 0ull);
            const int bsel = passA0 ? b : b + 1;
            if constexpr (MODE == 0)
            {
                // fire-and-forget minima: nobody waits for the L2 round trip; which slots got a separating set is
                // counted once afterwards
                if (passB0) (void)__hip_atomic_fetch_min(&rp.sel[cur.ib], (unsigned)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (passB1) (void)__hip_atomic_fetch_min(&rp.sel[cur.ib + 1], (unsigned)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (headA) (void)__hip_atomic_fetch_min(&rp.sel[cur.ia], (unsigned)bsel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            else
            {
                // hetcor: the edge goes in both directions; only the slot of the ordered pair that was tested is marked
                // (level1_apply_kernel removes the edge when either direction is marked, updates bitmap and degrees once).
                // The mark is the lowest passing position, as in Skeleton mode: anything but kNone32 means "gone", and the
                // position lets level1_apply_kernel count the tests of the canonical schedule (round 2 stored plain zeros)
                if (passB0) (void)__hip_atomic_fetch_min(&rp.sel[cur.ib], (unsigned)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (passB1) (void)__hip_atomic_fetch_min(&rp.sel[cur.ib + 1], (unsigned)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (headA) (void)__hip_atomic_fetch_min(&rp.sel[cur.ia], (unsigned)bsel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        // Operand sets rotate through the stages (no register copies: every index below is a compile-time constant after
        // unrolling, so the compiler can wait for exactly the set it needs); the scheduling barriers keep the requests
        // ahead of the evaluation.  Round 3: kSets sets, the list entries requested kSets - 1 steps ahead of their
        // evaluation (rounds 1-2: three sets, two steps ahead -- a step's ~90 vector instructions cover 300 ns, the entries
        // take longer than two of those to arrive from L2, and the three waves of a SIMD, all the LDS rows allow, do not
        // cover the rest: 0.254 ms; five sets 0.242; launch_level1_rows has the other depths).
        constexpr int kSets = CUSK_ROWS_SETS;
        RowsStep2 st[kSets];
#pragma unroll
        for (int j = 0; j < kSets - 1; j++) stage_a(f_begin + 64 * j, st[j]);
        stage_b(st[0]);
        for (int base = f_begin;; base += 64 * kSets)
        {
            bool done = false;
#pragma unroll
            for (int j = 0; j < kSets; j++)
            {
                stage_a(base + 64 * (kSets - 1 + j), st[(kSets - 1 + j) % kSets]);
                stage_b(st[(j + 1) % kSets]);
                __builtin_amdgcn_sched_barrier(0);
                stage_c(st[j]);
                if (base + 64 * (j + 1) >= f_end)
                {
                    done = true;
                    break;
                }
            }
            if (done) break;
        }
    }
    for (int o = 32; o > 0; o >>= 1)
    {
        ntests += __shfl_xor(ntests, o);  // < 2^32 per wave
        if (VALIDATE) viol += __shfl_xor(viol, o);
        if constexpr (HET) nslow += __shfl_xor(nslow, o);
    }
    if (lane == 0)
    {
        if (ntests) atomicAdd(&s_cnt[0], (unsigned long long)ntests);
        if (VALIDATE && viol) atomicAdd(&s_cnt[1], (unsigned long long)viol);
        if constexpr (HET)
            if (nslow) atomicAdd(&s_cnt[2], (unsigned long long)nslow);
    }
    __syncthreads();
    if (tid == 0)
    {
        unsigned long long *sl = p.slots + (size_t)(blockIdx.x & (kCounterSlots - 1)) * 4;
        if (s_cnt[0]) atomicAdd(&sl[0], s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&sl[3], s_cnt[1]);
        // HET: the level has no recheck queue, its counter reports the tests that went to the exact form (rechecks[1]; the
        // engine compares it with a queue capacity from level 2 on only)
        if constexpr (HET)
            if (s_cnt[2]) atomicAdd(&p.cnt->qcount, s_cnt[2]);
    }
}

// hetcor mode, after the sweep: every row drops the neighbours whose slot was marked (the wave owns its bitmap row:
// word-aggregated plain read-modify-writes as in gather_records), sets its degree, and the removed directed edges
// are counted
// meta != nullptr (level 1 behind the row-streaming kernel): a slot is marked by the test of ITS ordered pair only, so the
// slot of the reverse pair is looked at as well (the edge goes when either direction found a separating variable)
__global__ void __launch_bounds__(256) level1_apply_kernel(const int *__restrict__ off, const int *__restrict__ nbr,
                                                           const unsigned *__restrict__ sel, unsigned long long *adj, int *deg,
                                                           int n, int words, unsigned long long *slots, const LevelCounters *cnt,
                                                           const int4 *__restrict__ meta, unsigned long long *canon)
{
    __shared__ int s_sum[4];
    __shared__ unsigned long long s_can[4];
    if (!cnt->active) return;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    int removed = 0;
    unsigned long long ctests = 0;
    if (row < n)
    {
        const int o0 = off[row], d = off[row + 1] - o0;
        for (int k0 = 0; k0 < d; k0 += 64)
        {
            const int k = k0 + lane;
            const bool valid = k < d;
            const int Y = valid ? nbr[o0 + k] : 0;
            const unsigned mark = valid ? sel[o0 + k] : kNone32;
            bool gone = valid && (mark != kNone32);
            // canonical (sequential) schedule of this ordered pair at level 1: the neighbour at position k is tested with the
            // positions 0, 1, ... (without k itself) up to its lowest passing one, or with all d - 1 of them
            if (canon != nullptr && valid)
                ctests += gone ? (unsigned long long)(mark + 1u - (mark > (unsigned)k ? 1u : 0u)) : (unsigned long long)(d - 1);
            if (valid && !gone && meta != nullptr)
            {
                const int4 m = meta[o0 + k];
                gone = (sel[m.z + m.y] != kNone32);
            }
            const int w = valid ? (Y >> 6) : -1 - lane;
            unsigned long long bits = gone ? (1ull << (Y & 63)) : 0ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
            {
                const unsigned long long ob = __shfl_down(bits, o);
                const int ow = __shfl_down(w, o);
                if (lane + o < 64 && ow == w) bits |= ob;
            }
            const int pw = __shfl_up(w, 1);
            if (valid && bits != 0ull && (lane == 0 || pw != w)) adj[(size_t)row * words + w] &= ~bits;
            removed += __popcll(__ballot(gone));
        }
        if (lane == 0 && removed) deg[row] = d - removed;
    }
    if (canon != nullptr)
        for (int o = 32; o > 0; o >>= 1) ctests += __shfl_xor(ctests, o);
    if (lane == 0)
    {
        s_sum[threadIdx.x >> 6] = removed;
        s_can[threadIdx.x >> 6] = ctests;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const int t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        // cusk_stats.removed: ordered pairs, as in Skeleton mode (both directions of an edge go)
        if (t && slots) atomicAdd(&slots[(size_t)(blockIdx.x & (kCounterSlots - 1)) * 4 + 2], (unsigned long long)t);
        const unsigned long long c = s_can[0] + s_can[1] + s_can[2] + s_can[3];
        if (c && canon) atomicAdd(&canon[blockIdx.x & (kCounterSlots - 1)], c);
    }
}

// hetcor mode, row-sharded runs: the sweeps of levels that do not use the row-streaming kernel clear adjacency bits
// directly; turn the bitmap back into per-slot marks (0 = the edge is gone, all ones = alive) so that the engines can
// join them with the same unsigned MIN as the Skeleton engine's selection state
__global__ void __launch_bounds__(256) marks_from_bitmap_kernel(const int *__restrict__ off, const int *__restrict__ nbr,
                                                                const unsigned long long *__restrict__ adj, unsigned *sel, int n,
                                                                int words, const LevelCounters *cnt)
{
    if (!cnt->active) return;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int o0 = off[row], d = off[row + 1] - o0;
    for (int k = lane; k < d; k += 64)
    {
        const int Y = nbr[o0 + k];
        const bool alive = (adj[(size_t)row * words + (Y >> 6)] >> (Y & 63)) & 1ull;
        sel[o0 + k] = alive ? kNone32 : 0u;
    }
}

hipError_t launch_marks_from_bitmap(const SweepParams &p, unsigned *sel, hipStream_t st)
{
    hipLaunchKernelGGL(marks_from_bitmap_kernel, dim3((p.n + 3) / 4), dim3(256), 0, st, p.off, p.nbr, p.adj, sel, p.n, p.words, p.cnt);
    return hipGetLastError();
}

hipError_t launch_level1_apply(const SweepParams &p, const unsigned *sel, const void *meta, bool count_removed, hipStream_t st)
{
    hipLaunchKernelGGL(level1_apply_kernel, dim3((p.n + 3) / 4), dim3(256), 0, st, p.off, p.nbr, sel, p.adj, p.deg, p.n, p.words,
                       count_removed ? p.slots : nullptr, p.cnt, static_cast<const int4 *>(meta), (unsigned long long *)nullptr);
    return hipGetLastError();
}

// Workgroup size of the row-streaming kernel with the row of C in LDS, or 0 for the gather form (no row fits).  Of 256 /
// 512 threads the size that puts most ROWS on a CU (at most 16 waves, 12 for the hetcor / validating forms: 125 /
// 131-137 VGPRs with five operand sets), the larger one on a tie: a row's prologue is a chain of four dependent round
// trips during which its waves have nothing to do, and only other rows on the CU fill that time.  When two rows do not
// fit (n > ~16,000) the row is gathered through L1/L2.  forced (option l1_threads): that size whenever one row fits.
// Measured at n = 10,020, round 3 with three operand sets (gather form 0.336 ms): 256 threads (three rows per CU)
// 0.255, 512 threads (two rows) 0.263, 384 threads (three rows, six waves each) 0.312, 1,024 threads (one row per
// CU) 0.383; operand sets at 256 threads: 3: 0.254, 4: 0.244, 5: 0.242, 6: 0.243, 7: 0.246, 9 (two waves per SIMD): 0.328
// het: the HET forms carry the sizes as a further operand stream (VGPR counts in DESIGN section 9): 12 waves like the
// validating forms, and row_lds holds two rows (C and N).
int level1_rows_threads(size_t row_lds, int mode, bool validate, int forced, bool het)
{
    constexpr size_t kLdsCu = 160 * 1024;
    const int max_waves = (mode == 0 && !validate && !het) ? 16 : 12;
    auto rows_per_cu = [&](int t) {
        const size_t fixed = sizeof(int4) * t + sizeof(int) * (2 * t + 1) + sizeof(int) * 2 * (t / 64) + 64;
        return std::min((int)(kLdsCu / (row_lds + fixed)), max_waves / (t / 64));
    };
    if (forced) return rows_per_cu(forced) >= 1 ? forced : 0;
    const int r256 = rows_per_cu(256), r512 = rows_per_cu(512);
    if (r512 >= 2 && r512 >= r256) return 512;
    return r256 >= 2 ? 256 : 0;
}

extern "C" int cusk_level1_rows_threads(long long row_bytes, int mode, int validate, int forced_threads)
{
    if (row_bytes < 0 || mode < 0 || mode > 2 || (forced_threads != 0 && forced_threads != 256 && forced_threads != 512)) return -1;
    // mode 2: Skeleton at per-pair sample sizes (the HET forms; row_bytes holds the rows of C and N)
    return level1_rows_threads((size_t)row_bytes, mode == 2 ? 0 : mode, validate != 0, forced_threads, mode == 2);
}

hipError_t launch_level1_rows(int mode, bool validate, bool use_filter, const SweepParams &p, float *rv, void *meta,
                              unsigned *sel, const int *wpre, hipEvent_t ev_begin, hipEvent_t ev_end, int shard_rank,
                              int shard_world, int force_threads, bool lds_row, bool defer_apply, bool has_ti,
                              unsigned long long *canon, hipStream_t st, float *nv, int *form)
{
    const int n = p.n;
    const bool het = nv != nullptr;  // per-pair sample sizes (p.Ness, bitwise symmetric): the HET forms, Skeleton mode only
    if (het && (mode != 0 || p.Ness == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(level1_prep_kernel, dim3((n + 3) / 4), dim3(256), 0, st, p.C, p.off, p.nbr, p.adj, wpre, p.words, rv,
                       static_cast<int4 *>(meta), sel, n, p.cnt);
    if (het) hipLaunchKernelGGL(level1_prep_nv_kernel, dim3((n + 3) / 4), dim3(256), 0, st, p.Ness, p.off, p.nbr, nv, n, p.cnt);
    RowsParams rp;
    rp.rv = rv;
    rp.meta = static_cast<const int4 *>(meta);
    rp.sel = sel;
    rp.use_filter = use_filter ? 1 : 0;
    rp.has_ti = has_ti ? 1 : 0;
    rp.beta = level1_beta(p.t2);
    rp.shard_rank = shard_rank;
    rp.shard_world = shard_world;
    rp.nv = nv;
    rp.th2 = (float)((double)p.th * (double)p.th);
    const dim3 grid((unsigned)n);
    if (ev_begin) (void)hipEventRecord(ev_begin, st);
    // Row of C in LDS (4 (n + 8) bytes per workgroup) unless no row fits (level1_rows_threads), the matrix is not 16-byte
    // aligned or the caller asks for the gather form (option l1_lds_row = 0).
    // HET: the row of N behind it, twice the bytes; N must be aligned as C is.
    const size_t row_floats = (size_t)(p.row_range ? p.max_span : n) + 8;
    const size_t nrow_off = (row_floats + 3) & ~(size_t)3;  // the row of N starts on a 16-byte boundary of LDS as well
    const size_t row_lds = sizeof(float) * (het ? nrow_off + row_floats : row_floats);
    rp.nrow_off = (int)nrow_off;
    int threads = 0;
    if (lds_row && (reinterpret_cast<uintptr_t>(p.C) & 15) == 0 && (!het || (reinterpret_cast<uintptr_t>(p.Ness) & 15) == 0))
        threads = level1_rows_threads(row_lds, mode, validate, force_threads, het);
    if (form) *form = threads == 256 ? 2 : threads == 512 ? 3 : 4;
#define CUSK_ROWS2_TH(M, V, T, H)                                                                                  \
    do                                                                                                            \
    {                                                                                                             \
        static size_t have = 0;                                                                                   \
        if (row_lds > have)                                                                                       \
        {                                                                                                         \
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(level1_rows2_kernel<M, V, T, true, H>),         \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_lds);                  \
            have = row_lds;                                                                                       \
        }                                                                                                         \
        hipLaunchKernelGGL((level1_rows2_kernel<M, V, T, true, H>), grid, dim3(T), row_lds, st, p, rp);              \
    } while (0)
#define CUSK_ROWS2(M, V) CUSK_ROWS2_H(M, V, false)
#define CUSK_ROWS2_H(M, V, H)                                                                                     \
    do                                                                                                            \
    {                                                                                                             \
        if (threads == 256)                                                                                       \
            CUSK_ROWS2_TH(M, V, 256, H);                                                                           \
        else if (threads == 512)                                                                                  \
            CUSK_ROWS2_TH(M, V, 512, H);                                                                           \
        else                                                                                                      \
            hipLaunchKernelGGL((level1_rows2_kernel<M, V, 256, false, H>), grid, dim3(256), 0, st, p, rp);         \
    } while (0)
    if (het && !validate)
        CUSK_ROWS2_H(0, false, true);
    else if (het)
        CUSK_ROWS2_H(0, true, true);
    else if (mode == 0 && !validate)
        CUSK_ROWS2(0, false);
    else if (mode == 0)
        CUSK_ROWS2(0, true);
    else if (!validate)
        CUSK_ROWS2(1, false);
    else
        CUSK_ROWS2(1, true);
#undef CUSK_ROWS2
#undef CUSK_ROWS2_H
#undef CUSK_ROWS2_TH
    if (ev_end) (void)hipEventRecord(ev_end, st);
    if (mode != 0 && !defer_apply)
        hipLaunchKernelGGL(level1_apply_kernel, dim3((n + 3) / 4), dim3(256), 0, st, p.off, p.nbr, sel, p.adj, p.deg, n,
                           p.words, p.slots, p.cnt, static_cast<const int4 *>(meta), has_ti ? nullptr : canon);
    return hipGetLastError();
}

}  // namespace cusk
