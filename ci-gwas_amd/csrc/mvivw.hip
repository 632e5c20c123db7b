// mvivw.hip -- multivariable inverse-variance-weighted regressions of a merged skeleton (cusk_mvivw of
// include/cusk_hip.h, where the rule is stated; `ci-gwas mvivw`).
//
// One weighted least-squares problem through the origin per outcome: y = beta[I, o] on X = beta[I, E] with weights
// w = weight[I, o], m = |I| rows, k = |E| <= 127 columns.  Everything is IEEE double and every sum over rows has one order:
// a workgroup owns a chunk of 256 consecutive list positions and adds it in row order, the chunk partials are stored with
// plain vector stores and added in chunk order.  No floating-point atomics.
//
//   mv_gram_kernel    one workgroup per (outcome, chunk), one launch per tile class.  A slab of rows of Z = (X, y) and of
//                     W Z stands in LDS; thread t owns a TS x TS tile of the lower triangle of Z'WZ (TS = 2, 4, 8 by the
//                     number of columns, so that the tiles of the widest problem of a class fill the workgroup) in
//                     double registers and walks the slab with plain FMAs on the FP64 vector pipe.  The staging pass
//                     also notes a NaN, an infinity or a weight <= 0 among the chunk's values (status 3).
//   mv_solve_kernel   one workgroup per outcome: the ordered sum of the partials, the Gram scaled to unit diagonal as a
//                     packed triangle in LDS, right-looking Cholesky with the pivot test, both substitutions, the inverse
//                     of the factor in place and from it diag(G^-1).
//   mv_resid_kernel   one workgroup per (outcome, chunk): the weighted residual sum of squares of the chunk, one row per
//                     thread, recomputed from beta and theta
//   mv_finish_kernel  one workgroup per outcome: rss in chunk order, sigma, the standard errors by `model`
// The host (host/mvivw_plan.h) checks every index before anything is launched.
#include "cusk_internal.h"
#include "host/mvivw_plan.h"

#include <cfloat>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace cusk {

namespace {

constexpr int kMvTriMax = kMvMaxExposures * (kMvMaxExposures + 1) / 2;  // 8128 doubles: 63.5 KB
constexpr int kMvVec = 128;
constexpr int kMvSolLd = 2 * kMvVec + 1;  // per active outcome: theta[128], v[128], the smallest squared pivot
constexpr double kMvPivotMin = CUSK_PHEN_PIVOT_MIN;
static_assert(kMvChunk == CUSK_MVIVW_CHUNK && kMvMaxExposures == CUSK_MVIVW_MAX_EXPOSURES, "the header states the plan's constants");
static_assert(kMvChunk == 256, "the residual kernel gives every thread of a workgroup one row of a chunk");

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
    int *chunk_bad;   // per chunk of the call: a value that gives status 3
    double *rpart;    // per chunk of the call: weighted residual sum of squares
    double *sol;      // per active outcome: kMvSolLd doubles
    int *status;      // per active outcome
    double *theta;    // layout of ex
    double *se;       // layout of ex
    double *stats;    // per active outcome: rss, sigma, smallest squared pivot
};

__device__ __forceinline__ bool mv_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN

template <int TS, int LD, int SLAB>
__global__ void __launch_bounds__(256) mv_gram_kernel(MvBatch b, const MvChunk *__restrict__ chunks)
{
    __shared__ double zs[SLAB * LD];
    __shared__ double ws[SLAB * LD];
    __shared__ int cols[LD];
    const int tid = threadIdx.x;
    const MvChunk ch = chunks[blockIdx.x];
    const MvOutcome q = b.outs[ch.slot];
    const int k = q.k, K = k + 1, p = b.p;
    const int T = (K + TS - 1) / TS, ntiles = T * (T + 1) / 2;  // T * TS <= LD by the class table
    for (int c = tid; c < LD; c += 256) cols[c] = c < k ? b.ex[q.ex0 + c] : q.o;
    const int t = min(tid, ntiles - 1);
    int ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    const int tj = t - ti * (ti + 1) / 2;
    double acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.0;
    const int rows = min(kMvChunk, q.m - ch.chunk * kMvChunk);
    const int *ivp = b.iv + q.iv0 + (long long)ch.chunk * kMvChunk;
    int bad = 0;
    __syncthreads();
    for (int s0 = 0; s0 < rows; s0 += SLAB)
    {
        for (int idx = tid; idx < SLAB * LD; idx += 256)
        {
            const int r = idx / LD, c = idx - r * LD;
            double x = 0.0, wx = 0.0;
            if (s0 + r < rows && c < K)
            {
                const size_t base = (size_t)ivp[s0 + r] * p;
                const double w = b.weight[base + q.o];
                x = b.beta[base + cols[c]];
                wx = w * x;
                bad |= (!mv_finite(x)) | (!(w > 0.0 && w <= DBL_MAX));
            }
            zs[idx] = x;
            ws[idx] = wx;
        }
        __syncthreads();
        if (tid < ntiles)
        {
            const double *wa = ws + ti * TS, *zb = zs + tj * TS;
#pragma unroll 2
            for (int kk = 0; kk < SLAB; kk++)
            {
                double a[TS], c[TS];
#pragma unroll
                for (int i = 0; i < TS; i++) a[i] = wa[kk * LD + i];
#pragma unroll
                for (int j = 0; j < TS; j++) c[j] = zb[kk * LD + j];
#pragma unroll
                for (int i = 0; i < TS; i++)
#pragma unroll
                    for (int j = 0; j < TS; j++) acc[i][j] = fma(a[i], c[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) b.chunk_bad[q.chunk0 + ch.chunk] = bad ? 1 : 0;
    if (tid < ntiles)
    {
        const int E = K * (K + 1) / 2;
        double *dst = b.part + q.part0 + (long long)ch.chunk * E;
#pragma unroll
        for (int i = 0; i < TS; i++)
#pragma unroll
            for (int j = 0; j < TS; j++)
            {
                const int r = ti * TS + i, c = tj * TS + j;
                if (r < K && c <= r) dst[r * (r + 1) / 2 + c] = acc[i][j];
            }
    }
}

// LDS carve (doubles): L[kMvTriMax], d[128], bv[128], x[128]
constexpr size_t kMvSolveLds = sizeof(double) * ((size_t)kMvTriMax + 3 * kMvVec);

__global__ void __launch_bounds__(256) mv_solve_kernel(MvBatch b, int first)
{
    extern __shared__ double s_mem[];
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    const MvOutcome q = b.outs[slot];
    const int k = q.k, K = k + 1, E = K * (K + 1) / 2, EL = k * (k + 1) / 2;
    double *L = s_mem;
    double *d = L + kMvTriMax;
    double *bv = d + kMvVec;
    double *x = bv + kMvVec;
    double *sol = b.sol + (size_t)slot * kMvSolLd;
    int bad = 0;
    for (int c = tid; c < q.nchunks; c += 256) bad |= b.chunk_bad[q.chunk0 + c];
    if (__syncthreads_or(bad))
    {
        if (tid == 0)
        {
            b.status[slot] = 3;
            sol[2 * kMvVec] = NAN;
        }
        return;
    }
    const double *part = b.part + q.part0;
    for (int e = tid; e < E - 1; e += 256)
    {  // in chunk order; the last entry, y'Wy, is not used
        double s = 0.0;
        for (int c = 0; c < q.nchunks; c++) s += part[(size_t)c * E + e];
        if (e < EL)
            L[e] = s;
        else
            bv[e - EL] = s;
    }
    __syncthreads();
    int nonpos = 0;
    if (tid < k)
    {
        const double g = L[tid * (tid + 1) / 2 + tid];
        nonpos = !(g > 0.0);
        d[tid] = sqrt(g);
    }
    if (__syncthreads_or(nonpos))
    {  // a column of zeros
        if (tid == 0)
        {
            b.status[slot] = 2;
            sol[2 * kMvVec] = 0.0;
        }
        return;
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
        const double piv = L[jj];
        if (!(piv >= minpiv)) minpiv = piv;
        if (!(piv >= kMvPivotMin))
        {  // the same for every thread
            if (tid == 0)
            {
                b.status[slot] = 2;
                sol[2 * kMvVec] = piv;
            }
            return;
        }
        const double l = sqrt(piv);
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
    // the inverse of L in place, last column first: X_jj = 1 / L_jj, X_ij = -(sum_{c = j+1..i} X_ic L_cj) / L_jj
    for (int j = k - 1; j >= 0; j--)
    {
        const double ajj = 1.0 / L[j * (j + 1) / 2 + j];
        double s = 0.0;
        if (tid > j && tid < k)
        {
            const int rr = tid * (tid + 1) / 2;
            for (int c = j + 1; c <= tid; c++) s = fma(L[rr + c], L[c * (c + 1) / 2 + j], s);
        }
        __syncthreads();
        if (tid > j && tid < k) L[tid * (tid + 1) / 2 + j] = -s * ajj;
        if (tid == j) L[j * (j + 1) / 2 + j] = ajj;
        __syncthreads();
    }
    if (tid < k)
    {
        double v = 0.0;
        for (int i = tid; i < k; i++)
        {
            const double xi = L[i * (i + 1) / 2 + tid];
            v = fma(xi, xi, v);
        }
        sol[tid] = bv[tid] / d[tid];
        sol[kMvVec + tid] = v / (d[tid] * d[tid]);
    }
    if (tid == 0)
    {
        sol[2 * kMvVec] = minpiv;
        b.status[slot] = 0;
    }
}

__global__ void __launch_bounds__(256) mv_resid_kernel(MvBatch b, const MvChunk *__restrict__ chunks)
{
    __shared__ double th[kMvVec];
    __shared__ int cols[kMvVec];
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const MvChunk ch = chunks[blockIdx.x];
    if (b.status[ch.slot] != 0) return;  // the same for the whole workgroup; its partial is never read
    const MvOutcome q = b.outs[ch.slot];
    const int k = q.k, p = b.p;
    if (tid < k)
    {
        th[tid] = b.sol[(size_t)ch.slot * kMvSolLd + tid];
        cols[tid] = b.ex[q.ex0 + tid];
    }
    __syncthreads();
    const int pos = ch.chunk * kMvChunk + tid;
    double term = 0.0;
    if (pos < q.m)
    {
        const size_t base = (size_t)b.iv[q.iv0 + pos] * p;
        double fit = 0.0;
        for (int j = 0; j < k; j++) fit = fma(b.beta[base + cols[j]], th[j], fit);
        const double r = b.beta[base + q.o] - fit;
        term = b.weight[base + q.o] * (r * r);
    }
    // one order: butterflies inside each wavefront, then wavefront 0 .. 3
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
    if ((tid & 63) == 0) sh[tid >> 6] = term;
    __syncthreads();
    if (tid == 0) b.rpart[q.chunk0 + ch.chunk] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ void __launch_bounds__(128) mv_finish_kernel(MvBatch b, int first)
{
    __shared__ double s_sigma;
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    const MvOutcome q = b.outs[slot];
    const int st = b.status[slot];
    const double *sol = b.sol + (size_t)slot * kMvSolLd;
    if (st != 0)
    {
        if (tid < q.k)
        {
            b.theta[q.ex0 + tid] = NAN;
            b.se[q.ex0 + tid] = NAN;
        }
        if (tid == 0)
        {
            b.stats[(size_t)slot * 3] = NAN;
            b.stats[(size_t)slot * 3 + 1] = NAN;
            b.stats[(size_t)slot * 3 + 2] = sol[2 * kMvVec];
        }
        return;
    }
    if (tid == 0)
    {
        double rss = 0.0;
        for (int c = 0; c < q.nchunks; c++) rss += b.rpart[q.chunk0 + c];
        const double sigma = sqrt(rss / (double)(q.m - q.k));
        s_sigma = sigma;
        b.stats[(size_t)slot * 3] = rss;
        b.stats[(size_t)slot * 3 + 1] = sigma;
        b.stats[(size_t)slot * 3 + 2] = sol[2 * kMvVec];
    }
    __syncthreads();
    if (tid < q.k)
    {
        const bool random = b.model == 1 || (b.model == 0 && q.m >= 4);
        const double sigma = s_sigma, f = (random && sigma > 1.0) ? sigma : 1.0;
        b.theta[q.ex0 + tid] = sol[tid];
        b.se[q.ex0 + tid] = sqrt(sol[kMvVec + tid]) * f;
    }
}

int mvivw_impl(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, const int *outcome,
               const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, double *theta, double *se,
               double *stats, int *status, float *kernel_ms)
{
    const std::string who = "cusk_mvivw";
    if (!e) return CUSK_ERR_ARG;
    if (!beta || !weight || (nout > 0 && (!stats || !status))) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    MvPlan plan;
    std::string msg;
    if (mvivw_plan_build(M, p, nout, outcome, iv_off, iv, ex_off, ex, model, (size_t)e->opt_mvivw_part_bytes, plan, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (nout > 0 && ex_off[nout] > ex_off[0] && (!theta || !se)) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nout == 0) return CUSK_OK;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout];
    std::vector<double> th_h(nex, nan), se_h(nex, nan), stats_h(na * 3, nan);
    std::vector<int> st_h(na, 0);
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_iv, d_ex, d_outs, d_chunks, d_part, d_bad, d_rpart, d_sol, d_status, d_theta, d_se, d_stats;
        struct Events
        {
            hipEvent_t ev[2] = {nullptr, nullptr};
            ~Events()
            {
                for (hipEvent_t v : ev)
                    if (v) (void)hipEventDestroy(v);
            }
        } evs;
        auto up = [&](DevBuf &buf, const void *src, size_t bytes) -> hipError_t {
            hipError_t st = buf.ensure(std::max<size_t>(bytes, 8));
            if (st != hipSuccess || bytes == 0) return st;
            return hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, s);
        };
        CUSK_HIP(e, up(d_beta, beta, sizeof(double) * (size_t)M * p));
        CUSK_HIP(e, up(d_weight, weight, sizeof(double) * (size_t)M * p));
        CUSK_HIP(e, up(d_iv, iv, sizeof(int) * (size_t)iv_off[nout]));
        CUSK_HIP(e, up(d_ex, ex, sizeof(int) * nex));
        CUSK_HIP(e, up(d_outs, plan.outcomes.data(), sizeof(MvOutcome) * na));
        CUSK_HIP(e, up(d_chunks, plan.chunks.data(), sizeof(MvChunk) * plan.chunks.size()));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * plan.max_part_doubles));
        CUSK_HIP(e, d_bad.ensure(sizeof(int) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_rpart.ensure(sizeof(double) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_sol.ensure(sizeof(double) * na * kMvSolLd));
        CUSK_HIP(e, d_status.ensure(sizeof(int) * na));
        CUSK_HIP(e, d_theta.ensure(sizeof(double) * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_se.ensure(sizeof(double) * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_stats.ensure(sizeof(double) * na * 3));

        MvBatch b;
        b.beta = d_beta.as<double>();
        b.weight = d_weight.as<double>();
        b.p = p;
        b.model = model;
        b.iv = d_iv.as<int>();
        b.ex = d_ex.as<int>();
        b.outs = d_outs.as<MvOutcome>();
        b.part = d_part.as<double>();
        b.chunk_bad = d_bad.as<int>();
        b.rpart = d_rpart.as<double>();
        b.sol = d_sol.as<double>();
        b.status = d_status.as<int>();
        b.theta = d_theta.as<double>();
        b.se = d_se.as<double>();
        b.stats = d_stats.as<double>();
        CUSK_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(mv_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kMvSolveLds));
        for (hipEvent_t &v : evs.ev) CUSK_HIP(e, hipEventCreate(&v));
        CUSK_HIP(e, hipEventRecord(evs.ev[0], s));
        const MvChunk *chunks = d_chunks.as<MvChunk>();
        for (const MvGroup &g : plan.groups)
        {  // one stream: the partials of a group are read before the next group's Gram kernels overwrite them
            for (int c = 0; c < kMvClasses; c++)
            {
                const size_t cnt = g.class_first[c + 1] - g.class_first[c];
                if (cnt == 0) continue;
                const MvChunk *cl = chunks + g.class_first[c];
                if (c == 0)
                    hipLaunchKernelGGL((mv_gram_kernel<2, 44, 32>), dim3((unsigned)cnt), dim3(256), 0, s, b, cl);
                else if (c == 1)
                    hipLaunchKernelGGL((mv_gram_kernel<4, 88, 32>), dim3((unsigned)cnt), dim3(256), 0, s, b, cl);
                else
                    hipLaunchKernelGGL((mv_gram_kernel<8, 128, 16>), dim3((unsigned)cnt), dim3(256), 0, s, b, cl);
                CUSK_HIP(e, hipGetLastError());
            }
            const unsigned nslots = (unsigned)(g.last - g.first);
            const size_t nchunks = g.class_first[kMvClasses] - g.class_first[0];
            hipLaunchKernelGGL(mv_solve_kernel, dim3(nslots), dim3(256), kMvSolveLds, s, b, g.first);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(mv_resid_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, b, chunks + g.class_first[0]);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(mv_finish_kernel, dim3(nslots), dim3(128), 0, s, b, g.first);
            CUSK_HIP(e, hipGetLastError());
        }
        CUSK_HIP(e, hipEventRecord(evs.ev[1], s));
        if (nex)
        {
            CUSK_HIP(e, hipMemcpyAsync(th_h.data(), d_theta.p, sizeof(double) * nex, hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipMemcpyAsync(se_h.data(), d_se.p, sizeof(double) * nex, hipMemcpyDeviceToHost, s));
        }
        CUSK_HIP(e, hipMemcpyAsync(stats_h.data(), d_stats.p, sizeof(double) * na * 3, hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipMemcpyAsync(st_h.data(), d_status.p, sizeof(int) * na, hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipStreamSynchronize(s));
        float ms = 0.0f;
        CUSK_HIP(e, hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1]));
        if (kernel_ms) *kernel_ms = ms;
    }
    // nothing of the caller's is written before this point
    for (int a = 0; a < nout; a++)
    {
        status[a] = plan.status[(size_t)a];
        for (int c = 0; c < 3; c++) stats[(size_t)a * 3 + c] = nan;
        for (int c = ex_off[a]; c < ex_off[a + 1]; c++) theta[c] = se[c] = nan;
    }
    for (size_t slot = 0; slot < na; slot++)
    {
        const MvOutcome &q = plan.outcomes[slot];
        status[q.out] = st_h[slot];
        for (int c = 0; c < 3; c++) stats[(size_t)q.out * 3 + c] = stats_h[slot * 3 + c];
        for (int c = 0; c < q.k; c++)
        {
            theta[q.ex0 + c] = th_h[(size_t)q.ex0 + c];
            se[q.ex0 + c] = se_h[(size_t)q.ex0 + c];
        }
    }
    return CUSK_OK;
}

}  // namespace

}  // namespace cusk

extern "C" int cusk_mvivw(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout,
                          const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model,
                          double *theta, double *se, double *stats, int *status, float *kernel_ms)
{
    return cusk::mvivw_impl(e, beta, weight, M, p, nout, outcome, iv_off, iv, ex_off, ex, model, theta, se, stats, status, kernel_ms);
}
