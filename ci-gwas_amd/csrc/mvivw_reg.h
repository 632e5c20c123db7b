// mvivw_reg.h -- the steps of the IVW regression that do not depend on where the table lives, shared by mvivw.hip (rows
// gathered from beta and weight) and mvivw_ld.hip (the whitened table, unit weights).  Each file keeps only the two
// kernels that read its table: a Gram kernel, which stages a slab of rows in LDS and calls the pieces below, and a
// residual kernel.  The solve and finish kernels read the chunk partials and `sol` alone; they are defined once, in
// mvivw.hip, and both files reach them through the launchers declared at the end.
#pragma once
#include "cusk_internal.h"
#include "host/mvivw_plan.h"

#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

namespace cusk {

constexpr int kMvTriMax = kMvMaxExposures * (kMvMaxExposures + 1) / 2;  // 8128 doubles: 63.5 KB
constexpr int kMvVec = 128;
constexpr int kMvSolLd = 2 * kMvVec + 1;  // per active outcome: theta[128], v[128], the smallest squared pivot
constexpr int kMvSumLd = kMvTriMax + kMvVec;  // per active outcome: the summed triangle G packed by rows, then b (MvBatch::gsum)
constexpr double kMvPivotMin = CUSK_PHEN_PIVOT_MIN;
constexpr double kMvNaN = std::numeric_limits<double>::quiet_NaN();
// LDS carve of the solve kernel (doubles): L[kMvTriMax], d[128], bv[128], x[128]
constexpr size_t kMvSolveLds = sizeof(double) * ((size_t)kMvTriMax + 3 * kMvVec);
static_assert(kMvChunk == CUSK_MVIVW_CHUNK && kMvMaxExposures == CUSK_MVIVW_MAX_EXPOSURES, "the header states the plan's constants");
static_assert(kMvChunk == 256, "a residual kernel gives every thread of a workgroup one row of a chunk");

struct MvBatch
{
    const double *beta;    // M x p
    const double *weight;  // M x p
    int p;
    int model;
    const int *iv;
    const int *ex;
    const MvOutcome *outs;
    double *part;     // chunk partials of the group in flight
    int *chunk_bad;   // per chunk of the call: a value that gives status 3; null: no flags (mvivw_ld.hip, whose gather tests)
    double *rpart;    // per chunk of the call: weighted residual sum of squares
    double *sol;      // per active outcome: kMvSolLd doubles
    int *status;      // per active outcome
    double *theta;    // layout of ex
    double *se;       // layout of ex
    double *stats;    // per active outcome: rss, sigma, smallest squared pivot
    // mvivw_robust.hip alone sets what follows; null: the plain regressions
    const double *rho = nullptr;  // layout of iv: the Gram kernel multiplies the weight of a list position by it
    const int *frozen = nullptr;  // per active outcome: not 0 = the Gram (rho form) and solve kernels leave it as it is
    double *dsc = nullptr;        // per active outcome: kMvVec doubles, the solve kernel's d_j = sqrt(G_jj)
    // mvivw_jackknife.hip alone sets this; null: the sums stay in LDS
    double *gsum = nullptr;  // per active outcome: kMvSumLd doubles, the chunk-ordered sums the solve kernel forms: the lower
                             // triangle of G packed by rows (k (k + 1) / 2 doubles), then b (k doubles)
};

__device__ __forceinline__ bool mv_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

// tile t of the lower triangle, counted row by row, is (ti, tj) with ti = mv_tile_row(t), tj = t - ti (ti + 1) / 2 <= ti
__device__ __forceinline__ int mv_tile_row(int t)
{
    int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    return ti;
}

// acc += A'B over the SLAB rows staged in LDS (leading dimension LD), rows ascending: `a` and `c` point at the thread's
// TS columns of the left and of the right operand
template <int TS, int LD, int SLAB>
__device__ __forceinline__ void mv_slab_walk(const double *a, const double *c, double (&acc)[TS][TS])
{
#pragma unroll 2
    for (int kk = 0; kk < SLAB; kk++)
    {
        double av[TS], cv[TS];
#pragma unroll
        for (int i = 0; i < TS; i++) av[i] = a[kk * LD + i];
#pragma unroll
        for (int j = 0; j < TS; j++) cv[j] = c[kk * LD + j];
#pragma unroll
        for (int i = 0; i < TS; i++)
#pragma unroll
            for (int j = 0; j < TS; j++) acc[i][j] = fma(av[i], cv[j], acc[i][j]);
    }
}

// tile (ti, tj) into a chunk partial: the lower triangle of the K x K Gram, packed by rows
template <int TS>
__device__ __forceinline__ void mv_store_tile(double *dst, int K, int ti, int tj, const double (&acc)[TS][TS])
{
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++)
        {
            const int r = ti * TS + i, c = tj * TS + j;
            if (r < K && c <= r) dst[r * (r + 1) / 2 + c] = acc[i][j];
        }
}

// the sum of one term per thread of a workgroup of 256, in one order: butterflies inside each wavefront, then wavefront
// 0 .. 3.  `sh`: four doubles of LDS.  The value is the sum in thread 0.
__device__ __forceinline__ double mv_block_sum(double term, double *sh)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
    if ((tid & 63) == 0) sh[tid >> 6] = term;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Steps 2 - 3 of the rule for one system in LDS, called by every thread of a workgroup of 256 with the same arguments
// (mv_solve_kernel, and mv_jk_refit_kernel of mvivw_jackknife.hip for the downdated systems).  In: L the lower triangle
// of G packed by rows, bv = b.  d_j = sqrt(G_jj), the unit-diagonal scaling, the right-looking Cholesky with the pivot
// test, both substitutions.  Returns 0 with *piv the smallest squared pivot, L the factor of the scaled Gram and bv = u,
// theta_j = u_j / d_j; 1 for a G_jj that is not positive (*piv = 0; d is not usable); 2 for a squared pivot below
// kMvPivotMin (*piv = that pivot).  x: k doubles of scratch.  The caller has synchronised after writing L and bv.
__device__ __forceinline__ int mv_factor_solve(double *L, double *d, double *bv, double *x, int k, double *piv)
{
    const int tid = threadIdx.x;
    int nonpos = 0;
    if (tid < k)
    {
        const double g = L[tid * (tid + 1) / 2 + tid];
        nonpos = !(g > 0.0);
        d[tid] = sqrt(g);
    }
    if (__syncthreads_or(nonpos))
    {  // a column of zeros
        *piv = 0.0;
        return 1;
    }
    if (tid < k)
    {
        const int rr = tid * (tid + 1) / 2;
        for (int c = 0; c < tid; c++) L[rr + c] = L[rr + c] / (d[tid] * d[c]);
        L[rr + tid] = 1.0;
    }
    __syncthreads();
    double minpiv = INFINITY;
    const int tr = tid >> 4, tc = tid & 15;
    for (int j = 0; j < k; j++)
    {
        const int jj = j * (j + 1) / 2 + j;
        const double pv = L[jj];
        if (!(pv >= minpiv)) minpiv = pv;
        if (!(pv >= kMvPivotMin))
        {  // the same for every thread
            *piv = pv;
            return 2;
        }
        const double l = sqrt(pv);
        __syncthreads();
        if (tid == 0) L[jj] = l;
        for (int r = j + 1 + tid; r < k; r += 256) L[r * (r + 1) / 2 + j] /= l;
        __syncthreads();
        for (int r = j + 1 + tr; r < k; r += 16)
        {
            const int rr = r * (r + 1) / 2;
            const double lrj = L[rr + j];
            for (int c = j + 1 + tc; c <= r; c += 16) L[rr + c] = fma(-lrj, L[c * (c + 1) / 2 + j], L[rr + c]);
        }
        __syncthreads();
    }
    // L w = D^-1 b, thread r owns row r
    double rhs = tid < k ? bv[tid] / d[tid] : 0.0;
    for (int j = 0; j < k; j++)
    {
        if (tid == j) x[j] = rhs / L[j * (j + 1) / 2 + j];
        __syncthreads();
        if (tid > j && tid < k) rhs = fma(-L[tid * (tid + 1) / 2 + j], x[j], rhs);
    }
    // L' u = w; u goes to bv, which has been read
    rhs = tid < k ? x[tid] : 0.0;
    for (int j = k - 1; j >= 0; j--)
    {
        if (tid == j) bv[j] = rhs / L[j * (j + 1) / 2 + j];
        __syncthreads();
        if (tid < j) rhs = fma(-L[j * (j + 1) / 2 + tid], bv[j], rhs);
    }
    *piv = minpiv;
    return 0;
}

// mvivw.hip: mv_solve_kernel and mv_finish_kernel for the active outcomes first .. first + nslots - 1 of b.outs.  A
// kernel is launched only from the file that defines it; the caller asks hipGetLastError.
hipError_t mv_reg_prepare();  // once per call, before the first launch: the dynamic LDS of the solve kernel
void launch_mv_solve(hipStream_t s, const MvBatch &b, int first, unsigned nslots);
void launch_mv_finish(hipStream_t s, const MvBatch &b, int first, unsigned nslots);
// mv_gram_kernel of tile class `cls` for `cnt` chunks; with_rho: the form that multiplies every weight by b.rho and
// skips the chunks of frozen outcomes (mvivw_robust.hip)
void launch_mv_gram(hipStream_t s, const MvBatch &b, int cls, const MvChunk *chunks, size_t cnt, bool with_rho);
// the plain regressions of every group of the plan, enqueued on s: Gram by class, solve, residuals, finish.  chunks: the
// plan's chunks on the device.  What cusk_mvivw runs, and step 0 of cusk_mvivw_jackknife.
hipError_t mv_plain_enqueue(hipStream_t s, const MvBatch &b, const MvPlan &plan, const MvChunk *chunks);

// What the two entry points keep per call beside their tables: the device arrays the solve and finish kernels write,
// per active outcome (na) and per exposure position (nex), and their host copies.
struct MvResults
{
    size_t na, nex, ncol;  // ncol: columns of stats
    ScopedDevBuf d_sol, d_status, d_theta, d_se, d_stats;
    std::vector<double> theta, se, stats;
    std::vector<int> status;
    MvResults(size_t na_, size_t nex_, size_t ncol_ = 3)
        : na(na_), nex(nex_), ncol(ncol_), theta(nex_, kMvNaN), se(nex_, kMvNaN), stats(na_ * ncol_, kMvNaN), status(na_, 0)
    {
    }
    hipError_t alloc(MvBatch &b)
    {
        const size_t bytes[5] = {sizeof(double) * na * kMvSolLd, sizeof(int) * na, sizeof(double) * (nex > 0 ? nex : 1),
                                 sizeof(double) * (nex > 0 ? nex : 1), sizeof(double) * na * ncol};
        DevBuf *const bufs[5] = {&d_sol, &d_status, &d_theta, &d_se, &d_stats};
        for (int i = 0; i < 5; i++)
        {
            hipError_t st = bufs[i]->ensure(bytes[i]);
            if (st != hipSuccess) return st;
        }
        b.sol = d_sol.as<double>();
        b.status = d_status.as<int>();
        b.theta = d_theta.as<double>();
        b.se = d_se.as<double>();
        b.stats = d_stats.as<double>();
        return hipSuccess;
    }
    hipError_t read_back(hipStream_t s)
    {  // enqueued; the caller synchronises
        hipError_t st = hipSuccess;
        if (nex) st = hipMemcpyAsync(theta.data(), d_theta.p, sizeof(double) * nex, hipMemcpyDeviceToHost, s);
        if (nex && st == hipSuccess) st = hipMemcpyAsync(se.data(), d_se.p, sizeof(double) * nex, hipMemcpyDeviceToHost, s);
        if (st == hipSuccess) st = hipMemcpyAsync(stats.data(), d_stats.p, sizeof(double) * na * ncol, hipMemcpyDeviceToHost, s);
        if (st == hipSuccess) st = hipMemcpyAsync(status.data(), d_status.p, sizeof(int) * na, hipMemcpyDeviceToHost, s);
        return st;
    }
};

// the caller's arrays before any result goes in: the plan's status (1 where nothing is computed), NaN everywhere else.
// Nothing of the caller's is written before this.
inline void mv_fill_unset(int nout, const std::vector<int> &plan_status, const int *ex_off, double *theta, double *se, double *stats,
                          int *status, int ncol = 3)
{
    for (int a = 0; a < nout; a++)
    {
        status[a] = plan_status[(size_t)a];
        for (int c = 0; c < ncol; c++) stats[(size_t)a * ncol + c] = kMvNaN;
        for (int c = ex_off[a]; c < ex_off[a + 1]; c++) theta[c] = se[c] = kMvNaN;
    }
}

}  // namespace cusk
