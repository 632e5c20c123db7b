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
//                     also notes a NaN, an infinity or a weight <= 0 among the chunk's values (status 3).  Its RHO form
//                     (mvivw_robust.hip) multiplies every weight by a per-row rho.
//   mv_solve_kernel   one workgroup per outcome: the ordered sum of the partials, the Gram scaled to unit diagonal as a
//                     packed triangle in LDS, right-looking Cholesky with the pivot test, both substitutions, the inverse
//                     of the factor in place and from it diag(G^-1).
//   mv_resid_kernel   one workgroup per (outcome, chunk): the weighted residual sum of squares of the chunk, one row per
//                     thread, recomputed from beta and theta
//   mv_finish_kernel  one workgroup per outcome: rss in chunk order, sigma, the standard errors by `model`
// The host (host/mvivw_plan.h) checks every index before anything is launched.
//
// mv_gram_kernel and mv_resid_kernel read the table; what they share with their forms for the whitened table of
// mvivw_ld.hip (tile decode, slab walk, packed store, the ordered workgroup sum) stands in mvivw_reg.h.  mv_solve_kernel
// and mv_finish_kernel read no table: they serve both files, through the launchers at the end of the kernels here.
#include "mvivw_reg.h"

#include <string>

namespace cusk {

namespace {

// RHO: the form of mvivw_robust.hip.  The weight of list position i is w_i b.rho[i], the chunks of a frozen outcome are
// left alone, and the values are not tested again (the plain pass of the same call has set the flags).
template <int TS, int LD, int SLAB, bool RHO>
__global__ void __launch_bounds__(256) mv_gram_kernel(MvBatch b, const MvChunk *__restrict__ chunks)
{
    __shared__ double zs[SLAB * LD];
    __shared__ double ws[SLAB * LD];
    __shared__ int cols[LD];
    const int tid = threadIdx.x;
    const MvChunk ch = chunks[blockIdx.x];
    if constexpr (RHO)
        if (b.frozen[ch.slot]) return;  // the same for the whole workgroup
    const MvOutcome q = b.outs[ch.slot];
    const int k = q.k, K = k + 1, p = b.p;
    const int T = (K + TS - 1) / TS, ntiles = T * (T + 1) / 2;  // T * TS <= LD by the class table
    for (int c = tid; c < LD; c += 256) cols[c] = c < k ? b.ex[q.ex0 + c] : q.o;
    const int t = min(tid, ntiles - 1), ti = mv_tile_row(t), tj = t - ti * (ti + 1) / 2;
    double acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.0;
    const int rows = min(kMvChunk, q.m - ch.chunk * kMvChunk);
    const int *ivp = b.iv + q.iv0 + (long long)ch.chunk * kMvChunk;
    [[maybe_unused]] const double *rhop = RHO ? b.rho + q.iv0 + (long long)ch.chunk * kMvChunk : nullptr;
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
                double w = b.weight[base + q.o];
                if constexpr (RHO) w = w * rhop[s0 + r];
                x = b.beta[base + cols[c]];
                wx = w * x;
                bad |= (!mv_finite(x)) | (!(w > 0.0 && w <= DBL_MAX));
            }
            zs[idx] = x;
            ws[idx] = wx;
        }
        __syncthreads();
        if (tid < ntiles) mv_slab_walk<TS, LD, SLAB>(ws + ti * TS, zs + tj * TS, acc);
        __syncthreads();
    }
    if constexpr (!RHO)
    {
        bad = __syncthreads_or(bad);
        if (tid == 0) b.chunk_bad[q.chunk0 + ch.chunk] = bad ? 1 : 0;
    }
    if (tid < ntiles) mv_store_tile<TS>(b.part + q.part0 + (long long)ch.chunk * (K * (K + 1) / 2), K, ti, tj, acc);
}

__global__ void __launch_bounds__(256) mv_solve_kernel(MvBatch b, int first)
{
    extern __shared__ double s_mem[];
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    if (b.frozen && b.frozen[slot]) return;  // mvivw_robust.hip: the outcome keeps its last solution
    const MvOutcome q = b.outs[slot];
    const int k = q.k, K = k + 1, E = K * (K + 1) / 2, EL = k * (k + 1) / 2;
    double *L = s_mem;
    double *d = L + kMvTriMax;
    double *bv = d + kMvVec;
    double *x = bv + kMvVec;
    double *sol = b.sol + (size_t)slot * kMvSolLd;
    int bad = 0;
    if (b.chunk_bad)  // null: the caller has tested the values itself
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
        if (b.gsum) b.gsum[(size_t)slot * kMvSumLd + e] = s;
    }
    __syncthreads();
    double minpiv;
    const int rc = mv_factor_solve(L, d, bv, x, k, &minpiv);  // the same for every thread
    if (b.dsc && rc != 1 && tid < k) b.dsc[(size_t)slot * kMvVec + tid] = d[tid];
    if (rc != 0)
    {
        if (tid == 0)
        {
            b.status[slot] = 2;
            sol[2 * kMvVec] = minpiv;  // the pivot that failed, 0 for a G_jj that is not positive
        }
        return;
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
    const double sum = mv_block_sum(term, sh);
    if (tid == 0) b.rpart[q.chunk0 + ch.chunk] = sum;
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

}  // namespace

hipError_t mv_reg_prepare()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(mv_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kMvSolveLds);
}

void launch_mv_solve(hipStream_t s, const MvBatch &b, int first, unsigned nslots)
{
    hipLaunchKernelGGL(mv_solve_kernel, dim3(nslots), dim3(256), kMvSolveLds, s, b, first);
}

void launch_mv_finish(hipStream_t s, const MvBatch &b, int first, unsigned nslots)
{
    hipLaunchKernelGGL(mv_finish_kernel, dim3(nslots), dim3(128), 0, s, b, first);
}

namespace {
template <bool RHO>
void launch_mv_gram_form(hipStream_t s, const MvBatch &b, int cls, const MvChunk *chunks, size_t cnt)
{
    if (cls == 0)
        hipLaunchKernelGGL((mv_gram_kernel<2, 44, 32, RHO>), dim3((unsigned)cnt), dim3(256), 0, s, b, chunks);
    else if (cls == 1)
        hipLaunchKernelGGL((mv_gram_kernel<4, 88, 32, RHO>), dim3((unsigned)cnt), dim3(256), 0, s, b, chunks);
    else
        hipLaunchKernelGGL((mv_gram_kernel<8, 128, 16, RHO>), dim3((unsigned)cnt), dim3(256), 0, s, b, chunks);
}
}  // namespace

void launch_mv_gram(hipStream_t s, const MvBatch &b, int cls, const MvChunk *chunks, size_t cnt, bool with_rho)
{
    if (with_rho)
        launch_mv_gram_form<true>(s, b, cls, chunks, cnt);
    else
        launch_mv_gram_form<false>(s, b, cls, chunks, cnt);
}

hipError_t mv_plain_enqueue(hipStream_t s, const MvBatch &b, const MvPlan &plan, const MvChunk *chunks)
{
    for (const MvGroup &g : plan.groups)
    {  // one stream: the partials of a group are read before the next group's Gram kernels overwrite them
        for (int c = 0; c < kMvClasses; c++)
        {
            const size_t cnt = g.class_first[c + 1] - g.class_first[c];
            if (cnt == 0) continue;
            launch_mv_gram(s, b, c, chunks + g.class_first[c], cnt, false);
            if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
        }
        const unsigned nslots = (unsigned)(g.last - g.first);
        const size_t nchunks = g.class_first[kMvClasses] - g.class_first[0];
        launch_mv_solve(s, b, g.first, nslots);
        if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
        hipLaunchKernelGGL(mv_resid_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, b, chunks + g.class_first[0]);
        if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
        launch_mv_finish(s, b, g.first, nslots);
        if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
    }
    return hipSuccess;
}

namespace {

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
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout];
    MvResults res(na, nex);
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_iv, d_ex, d_outs, d_chunks, d_part, d_bad, d_rpart;
        ScopedEvents<2> evs;
        CUSK_HIP(e, upload_async(d_beta, beta, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_weight, weight, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_iv, iv, sizeof(int) * (size_t)iv_off[nout], s));
        CUSK_HIP(e, upload_async(d_ex, ex, sizeof(int) * nex, s));
        CUSK_HIP(e, upload_async(d_outs, plan.outcomes.data(), sizeof(MvOutcome) * na, s));
        CUSK_HIP(e, upload_async(d_chunks, plan.chunks.data(), sizeof(MvChunk) * plan.chunks.size(), s));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * plan.max_part_doubles));
        CUSK_HIP(e, d_bad.ensure(sizeof(int) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_rpart.ensure(sizeof(double) * (size_t)plan.total_chunks));

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
        CUSK_HIP(e, res.alloc(b));
        CUSK_HIP(e, mv_reg_prepare());
        CUSK_HIP(e, evs.record(0, s));
        CUSK_HIP(e, mv_plain_enqueue(s, b, plan, d_chunks.as<MvChunk>()));
        CUSK_HIP(e, evs.record(1, s));
        CUSK_HIP(e, res.read_back(s));
        CUSK_HIP(e, hipStreamSynchronize(s));
        float ms = 0.0f;
        CUSK_HIP(e, evs.elapsed(&ms, 0, 1));
        if (kernel_ms) *kernel_ms = ms;
    }
    mv_fill_unset(nout, plan.status, ex_off, theta, se, stats, status);
    for (size_t slot = 0; slot < na; slot++)
    {
        const MvOutcome &q = plan.outcomes[slot];
        status[q.out] = res.status[slot];
        for (int c = 0; c < 3; c++) stats[(size_t)q.out * 3 + c] = res.stats[slot * 3 + c];
        for (int c = 0; c < q.k; c++)
        {
            theta[q.ex0 + c] = res.theta[(size_t)q.ex0 + c];
            se[q.ex0 + c] = res.se[(size_t)q.ex0 + c];
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
