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

// mvivw.hip: mv_solve_kernel and mv_finish_kernel for the active outcomes first .. first + nslots - 1 of b.outs.  A
// kernel is launched only from the file that defines it; the caller asks hipGetLastError.
hipError_t mv_reg_prepare();  // once per call, before the first launch: the dynamic LDS of the solve kernel
void launch_mv_solve(hipStream_t s, const MvBatch &b, int first, unsigned nslots);
void launch_mv_finish(hipStream_t s, const MvBatch &b, int first, unsigned nslots);
// mv_gram_kernel of tile class `cls` for `cnt` chunks; with_rho: the form that multiplies every weight by b.rho and
// skips the chunks of frozen outcomes (mvivw_robust.hip)
void launch_mv_gram(hipStream_t s, const MvBatch &b, int cls, const MvChunk *chunks, size_t cnt, bool with_rho);

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
