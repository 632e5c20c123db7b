// mvivw_jackknife.hip -- delete-group refits of the IVW regressions: leave-one-out estimates, PRESS and the weighted
// delete-group jackknife (cusk_mvivw_jackknife of include/cusk_hip.h, where the rule is stated; `ci-gwas mvivw --jackknife`).
//
// Step 0 is the plain call: the plan, the Gram, solve, residual and finish kernels of mvivw.hip (mv_plain_enqueue), whose
// solve kernel here also leaves the chunk-summed triangle (G, b) of every outcome in HBM (MvBatch::gsum).  Then, per batch
// of outcomes (host/mvivw_jk_plan.h):
//
//   mv_jk_refit_kernel   one workgroup of 256 threads per (outcome, group), one launch per tile class.  The group's rows
//                        of Z = (X, y) and of W Z go through LDS in slabs; thread t owns a TS x TS tile of the lower
//                        triangle of Z_g' W Z_g in double registers (mv_slab_walk, the tile classes of the Gram kernel).
//                        The slabs stand where the triangle will: after the last slab the threads write A = G - G_g packed
//                        into LDS and c = b - b_g beside it, mv_factor_solve (mvivw_reg.h, the code of the solve kernel)
//                        factors and solves in place, and a second walk over the group's rows, one row per thread, gives
//                        the prediction residuals and the group's PRESS partial.  theta_-g goes to the batch's workspace.
//   mv_jk_reduce_kernel  one workgroup per outcome: jk_status, the first failed group or the smallest pivot, PRESS in
//                        chunks of 256 groups, and per exposure (one thread each) theta_J, se_J, min, max and the most
//                        influential group, every sum over groups in chunks of 256 groups added in chunk order.
// Nothing is read by the host between the launches of a batch.  Everything is IEEE double, no floating-point atomics.
//
// LDS of the refit kernel (dynamic): max(two slabs, the packed triangle of the widest problem of the class) + d, c, x of
// 128 doubles each: 25.0 / 47.0 / 66.5 KB for the three classes, the last the solve kernel's.  With 160 KiB of LDS per
// compute unit that is 6 / 3 / 2 workgroups (24 / 12 / 8 wavefronts) per compute unit.
#include "mvivw_reg.h"

#include "host/mvivw_jk_plan.h"

#include <cstring>
#include <string>

namespace cusk {

namespace {

struct MvJk
{
    const MvJkOutcome *outs;  // per active outcome
    const int *grp;
    double *ws;      // theta_-g of the batch in flight
    double *gpress;  // per group of the batch: sum of r_i^2
    double *gpiv;    // per group of the batch: the smallest squared pivot, or the one that failed
    int *gfail;      // per group of the batch: not 0 = the pivot rule failed
    double *pres;    // layout of iv, or null
    double *jk;      // layout of ex, 4 doubles each
    int *jk_arg;     // layout of ex
    double *jk_stats;  // per active outcome: PRESS, pivot
    int *jk_status;    // per active outcome
};

template <int LD, int SLAB>
constexpr size_t mv_jk_lds()
{
    constexpr size_t slabs = (size_t)2 * SLAB * LD, tri = (size_t)(LD - 1) * LD / 2;
    return sizeof(double) * ((slabs > tri ? slabs : tri) + 3 * kMvVec);
}

template <int TS, int LD, int SLAB>
__global__ void __launch_bounds__(256) mv_jk_refit_kernel(MvBatch b, MvJk jk, const MvJkItem *__restrict__ items)
{
    extern __shared__ double s_mem[];
    __shared__ int cols[kMvVec];
    __shared__ double sh[4];
    constexpr int kRegion = (int)(mv_jk_lds<LD, SLAB>() / sizeof(double)) - 3 * kMvVec;
    static_assert(kRegion >= 2 * SLAB * LD && kRegion >= (LD - 1) * LD / 2, "slabs and triangle share the region");
    double *L = s_mem;  // first the slabs, then the packed triangle
    double *zs = s_mem, *ws = s_mem + SLAB * LD;
    double *d = s_mem + kRegion;
    double *bv = d + kMvVec;
    double *x = bv + kMvVec;
    const int tid = threadIdx.x;
    const MvJkItem it = items[blockIdx.x];
    if (b.status[it.slot] != 0) return;  // the same for the whole workgroup; the reduce kernel reads none of its values
    const MvOutcome q = b.outs[it.slot];
    const MvJkOutcome jq = jk.outs[it.slot];
    const int k = q.k, K = k + 1, p = b.p, EL = k * (k + 1) / 2;
    const int T = (K + TS - 1) / TS, ntiles = T * (T + 1) / 2;  // T * TS <= LD by the class table
    const int r0 = jk.grp[jq.grp0 + it.group], r1 = jk.grp[jq.grp0 + it.group + 1], rows = r1 - r0;
    const long long gi = jq.gi0 + it.group;
    for (int c = tid; c < kMvVec; c += 256) cols[c] = c < k ? b.ex[q.ex0 + c] : q.o;
    const int t = min(tid, ntiles - 1), ti = mv_tile_row(t), tj = t - ti * (ti + 1) / 2;
    double acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.0;
    const int *ivp = b.iv + q.iv0 + r0;
    __syncthreads();
    for (int s0 = 0; s0 < rows; s0 += SLAB)
    {  // rows past the group's end are staged as zeros: they add +0 to every sum
        for (int idx = tid; idx < SLAB * LD; idx += 256)
        {
            const int r = idx / LD, c = idx - r * LD;
            double xv = 0.0, wx = 0.0;
            if (s0 + r < rows && c < K)
            {
                const size_t base = (size_t)ivp[s0 + r] * p;
                xv = b.beta[base + cols[c]];
                wx = b.weight[base + q.o] * xv;
            }
            zs[idx] = xv;
            ws[idx] = wx;
        }
        __syncthreads();
        if (tid < ntiles) mv_slab_walk<TS, LD, SLAB>(ws + ti * TS, zs + tj * TS, acc);
        __syncthreads();
    }
    // A = G - G_g, c = b - b_g; the tile's entry (k, k), y'Wy of the group, is not used
    const double *gsum = b.gsum + (size_t)it.slot * kMvSumLd;
    if (tid < ntiles)
    {
#pragma unroll
        for (int i = 0; i < TS; i++)
#pragma unroll
            for (int j = 0; j < TS; j++)
            {
                const int r = ti * TS + i, c = tj * TS + j;
                if (r < k && c <= r)
                    L[r * (r + 1) / 2 + c] = gsum[r * (r + 1) / 2 + c] - acc[i][j];
                else if (r == k && c < k)
                    bv[c] = gsum[EL + c] - acc[i][j];
            }
    }
    __syncthreads();
    double piv;
    const int rc = mv_factor_solve(L, d, bv, x, k, &piv);  // the same for every thread
    if (tid == 0)
    {
        jk.gpiv[gi] = piv;
        jk.gfail[gi] = rc != 0;
    }
    if (rc != 0) return;
    if (tid < k)
    {
        const double th = bv[tid] / d[tid];
        x[tid] = th;
        jk.ws[jq.ws0 + (long long)it.group * k + tid] = th;
    }
    __syncthreads();
    // prediction residuals: runs of 256 consecutive rows from the group's first, each summed by mv_block_sum, in run order
    double press = 0.0;
    for (int s0 = 0; s0 < rows; s0 += 256)
    {
        double term = 0.0;
        if (s0 + tid < rows)
        {
            const size_t base = (size_t)ivp[s0 + tid] * p;
            double fit = 0.0;
            for (int j = 0; j < k; j++) fit = fma(b.beta[base + cols[j]], x[j], fit);
            const double r = sqrt(b.weight[base + q.o]) * (b.beta[base + q.o] - fit);
            if (jk.pres) jk.pres[q.iv0 + r0 + s0 + tid] = r;
            term = r * r;
        }
        press += mv_block_sum(term, sh);
        __syncthreads();
    }
    if (tid == 0) jk.gpress[gi] = press;
}

// the sum of term(g) over the groups 0 .. ng - 1: inside a chunk of kMvJkChunk groups in ascending order from zero, the
// chunk sums added in chunk order
template <typename F>
__device__ __forceinline__ double mv_jk_group_sum(int ng, F term)
{
    double tot = 0.0;
    for (int g0 = 0; g0 < ng; g0 += kMvJkChunk)
    {
        double s = 0.0;
        const int g1 = min(g0 + kMvJkChunk, ng);
        for (int g = g0; g < g1; g++) s += term(g);
        tot += s;
    }
    return tot;
}

__global__ void __launch_bounds__(256) mv_jk_reduce_kernel(MvBatch b, MvJk jk, int first)
{
    __shared__ int s_fail;
    __shared__ double s_min[256];
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    const MvOutcome q = b.outs[slot];
    const MvJkOutcome jq = jk.outs[slot];
    const int k = q.k, ng = jq.ng;
    const int plain = b.status[slot];
    int st = plain != 0 ? plain : (jq.active ? 0 : 1);
    double pivot = NAN;
    if (st == 0)
    {
        if (tid == 0) s_fail = ng;
        __syncthreads();
        double mn = INFINITY;
        for (int g = tid; g < ng; g += 256)
        {
            if (jk.gfail[jq.gi0 + g])
                atomicMin(&s_fail, g);  // an integer: the first failed group whatever the order
            else
                mn = fmin(mn, jk.gpiv[jq.gi0 + g]);
        }
        s_min[tid] = mn;
        __syncthreads();
        if (s_fail < ng)
        {
            st = 2;
            pivot = jk.gpiv[jq.gi0 + s_fail];
        }
        else
        {  // a minimum does not depend on the order it is taken in
            for (int off = 128; off > 0; off >>= 1)
            {
                if (tid < off) s_min[tid] = fmin(s_min[tid], s_min[tid + off]);
                __syncthreads();
            }
            pivot = s_min[0];
        }
    }
    if (st != 0)
    {  // the same for the whole workgroup
        if (tid < k)
        {
            for (int c = 0; c < 4; c++) jk.jk[(size_t)(q.ex0 + tid) * 4 + c] = NAN;
            jk.jk_arg[q.ex0 + tid] = -1;
        }
        if (tid == 0)
        {
            jk.jk_stats[(size_t)slot * 2] = NAN;
            jk.jk_stats[(size_t)slot * 2 + 1] = pivot;
            jk.jk_status[slot] = st;
        }
        return;
    }
    const int *gb = jk.grp + jq.grp0;
    const double m = (double)q.m;
    if (tid == 255)
    {
        const double *gp = jk.gpress + jq.gi0;
        jk.jk_stats[(size_t)slot * 2] = mv_jk_group_sum(ng, [&](int g) { return gp[g]; });
        jk.jk_stats[(size_t)slot * 2 + 1] = pivot;
        jk.jk_status[slot] = 0;
    }
    if (tid < k)
    {
        const double *tg = jk.ws + jq.ws0 + tid;  // theta_-g of this exposure: tg[g k]
        const double th = b.sol[(size_t)slot * kMvSolLd + tid];
        double lo = INFINITY, hi = -INFINITY, far = -1.0;
        int arg = 0;
        for (int g = 0; g < ng; g++)
        {
            const double v = tg[(size_t)g * k], mv = fabs(v - th);
            lo = fmin(lo, v);
            hi = fmax(hi, v);
            if (mv > far)
            {  // the first group on ties
                far = mv;
                arg = g;
            }
        }
        // theta_J = theta + sum (1 - m_g / m)(theta - theta_-g), which is ng theta - sum (1 - m_g / m) theta_-g
        const double thj = th + mv_jk_group_sum(ng, [&](int g) {
                               const double mg = (double)(gb[g + 1] - gb[g]);
                               return (1.0 - mg / m) * (th - tg[(size_t)g * k]);
                           });
        // tau_g - theta_J = (h_g - 1)(theta - theta_-g) - (theta_J - theta)
        const double shift = thj - th;
        const double var = mv_jk_group_sum(ng, [&](int g) {
                               const double h1 = m / (double)(gb[g + 1] - gb[g]) - 1.0;
                               const double dev = h1 * (th - tg[(size_t)g * k]) - shift;
                               return dev * dev / h1;
                           }) /
                           (double)ng;
        double *out = jk.jk + (size_t)(q.ex0 + tid) * 4;
        out[0] = thj;
        out[1] = sqrt(var);
        out[2] = lo;
        out[3] = hi;
        jk.jk_arg[q.ex0 + tid] = arg;
    }
}

template <int TS, int LD, int SLAB>
hipError_t mv_jk_prepare_class()
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(mv_jk_refit_kernel<TS, LD, SLAB>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_jk_lds<LD, SLAB>());
}

void launch_mv_jk_refit(hipStream_t s, const MvBatch &b, const MvJk &jk, int cls, const MvJkItem *items, size_t cnt)
{
    constexpr size_t lds0 = mv_jk_lds<44, 32>(), lds1 = mv_jk_lds<88, 32>(), lds2 = mv_jk_lds<128, 16>();
    static_assert(lds2 == kMvSolveLds, "the widest class takes the LDS of the solve kernel");
    if (cls == 0)
        hipLaunchKernelGGL((mv_jk_refit_kernel<2, 44, 32>), dim3((unsigned)cnt), dim3(256), lds0, s, b, jk, items);
    else if (cls == 1)
        hipLaunchKernelGGL((mv_jk_refit_kernel<4, 88, 32>), dim3((unsigned)cnt), dim3(256), lds1, s, b, jk, items);
    else
        hipLaunchKernelGGL((mv_jk_refit_kernel<8, 128, 16>), dim3((unsigned)cnt), dim3(256), lds2, s, b, jk, items);
}

int mvivw_jackknife_impl(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, const int *outcome,
                         const long long *iv_off, const int *iv, const int *ex_off, const int *ex, const long long *grp_off,
                         const int *grp, int model, double *theta, double *se, double *stats, int *status, double *jk_out,
                         int *jk_arg, double *jk_stats, int *jk_status, double *pres, double *refit, float *kernel_ms)
{
    const std::string who = "cusk_mvivw_jackknife";
    if (!e) return CUSK_ERR_ARG;
    if (!beta || !weight || (nout > 0 && (!stats || !status || !jk_stats || !jk_status)))
        return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    MvPlan plan;
    MvJkPlan jp;
    std::string msg;
    if (mvivw_plan_build(M, p, nout, outcome, iv_off, iv, ex_off, ex, model, (size_t)e->opt_mvivw_part_bytes, plan, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (nout > 0 && ex_off[nout] > ex_off[0] && (!theta || !se || !jk_out || !jk_arg)) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (mvivw_jk_plan_build(plan, nout, iv_off, ex_off, grp_off, grp, (size_t)e->opt_mvivw_jk_bytes, jp, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nout == 0) return CUSK_OK;
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout], niv = (size_t)iv_off[nout];
    MvResults res(na, nex);
    std::vector<double> h_jk(nex * 4, kMvNaN), h_jkstats(na * 2, kMvNaN), h_pres, h_ws;
    std::vector<int> h_arg(nex, -1), h_jkstatus(na, 0);
    // every result of the device is held back until the call has succeeded: refit per batch in h_refit
    std::vector<double> h_refit;
    if (refit) h_refit.assign((size_t)jp.refit_off[(size_t)nout], kMvNaN);
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_iv, d_ex, d_outs, d_chunks, d_part, d_bad, d_rpart, d_gsum;
        ScopedDevBuf d_jouts, d_grp, d_items, d_ws, d_gpress, d_gpiv, d_gfail, d_pres, d_jk, d_arg, d_jkstats, d_jkstatus;
        ScopedEvents<2> evs;
        CUSK_HIP(e, upload_async(d_beta, beta, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_weight, weight, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_iv, iv, sizeof(int) * niv, s));
        CUSK_HIP(e, upload_async(d_ex, ex, sizeof(int) * nex, s));
        CUSK_HIP(e, upload_async(d_outs, plan.outcomes.data(), sizeof(MvOutcome) * na, s));
        CUSK_HIP(e, upload_async(d_chunks, plan.chunks.data(), sizeof(MvChunk) * plan.chunks.size(), s));
        CUSK_HIP(e, upload_async(d_jouts, jp.outcomes.data(), sizeof(MvJkOutcome) * na, s));
        CUSK_HIP(e, upload_async(d_grp, grp, sizeof(int) * (size_t)grp_off[nout], s));
        CUSK_HIP(e, upload_async(d_items, jp.items.data(), sizeof(MvJkItem) * jp.items.size(), s));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * plan.max_part_doubles));
        CUSK_HIP(e, d_bad.ensure(sizeof(int) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_rpart.ensure(sizeof(double) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_gsum.ensure(sizeof(double) * na * kMvSumLd));
        CUSK_HIP(e, d_ws.ensure(sizeof(double) * std::max<size_t>(jp.max_ws_doubles, 1)));
        const size_t maxg = (size_t)std::max<long long>(jp.max_groups, 1);
        CUSK_HIP(e, d_gpress.ensure(sizeof(double) * maxg));
        CUSK_HIP(e, d_gpiv.ensure(sizeof(double) * maxg));
        CUSK_HIP(e, d_gfail.ensure(sizeof(int) * maxg));
        if (pres) CUSK_HIP(e, d_pres.ensure(sizeof(double) * std::max<size_t>(niv, 1)));
        CUSK_HIP(e, d_jk.ensure(sizeof(double) * 4 * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_arg.ensure(sizeof(int) * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_jkstats.ensure(sizeof(double) * 2 * na));
        CUSK_HIP(e, d_jkstatus.ensure(sizeof(int) * na));

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
        b.gsum = d_gsum.as<double>();
        CUSK_HIP(e, res.alloc(b));
        MvJk jk;
        jk.outs = d_jouts.as<MvJkOutcome>();
        jk.grp = d_grp.as<int>();
        jk.ws = d_ws.as<double>();
        jk.gpress = d_gpress.as<double>();
        jk.gpiv = d_gpiv.as<double>();
        jk.gfail = d_gfail.as<int>();
        jk.pres = pres ? d_pres.as<double>() : nullptr;
        jk.jk = d_jk.as<double>();
        jk.jk_arg = d_arg.as<int>();
        jk.jk_stats = d_jkstats.as<double>();
        jk.jk_status = d_jkstatus.as<int>();
        CUSK_HIP(e, mv_reg_prepare());
        CUSK_HIP(e, (mv_jk_prepare_class<2, 44, 32>()));
        CUSK_HIP(e, (mv_jk_prepare_class<4, 88, 32>()));
        CUSK_HIP(e, (mv_jk_prepare_class<8, 128, 16>()));
        CUSK_HIP(e, evs.record(0, s));
        CUSK_HIP(e, mv_plain_enqueue(s, b, plan, d_chunks.as<MvChunk>()));
        const MvJkItem *items = d_items.as<MvJkItem>();
        if (refit) h_ws.resize(std::max<size_t>(jp.max_ws_doubles, 1));
        for (const MvJkBatch &bt : jp.batches)
        {  // one stream: a batch's workspace is reduced (and copied) before the next batch's refits overwrite it
            for (int c = 0; c < kMvClasses; c++)
            {
                const size_t cnt = bt.class_first[c + 1] - bt.class_first[c];
                if (cnt == 0) continue;
                launch_mv_jk_refit(s, b, jk, c, items + bt.class_first[c], cnt);
                CUSK_HIP(e, hipGetLastError());
            }
            hipLaunchKernelGGL(mv_jk_reduce_kernel, dim3((unsigned)(bt.last - bt.first)), dim3(256), 0, s, b, jk, bt.first);
            CUSK_HIP(e, hipGetLastError());
            if (refit && bt.ws_doubles > 0)
            {
                CUSK_HIP(e, hipMemcpyAsync(h_ws.data(), jk.ws, sizeof(double) * bt.ws_doubles, hipMemcpyDeviceToHost, s));
                CUSK_HIP(e, hipStreamSynchronize(s));
                for (int sl = bt.first; sl < bt.last; sl++)
                {
                    const MvJkOutcome &j = jp.outcomes[(size_t)sl];
                    const MvOutcome &q = plan.outcomes[(size_t)sl];
                    if (j.ng > 0)
                        std::memcpy(h_refit.data() + jp.refit_off[(size_t)q.out], h_ws.data() + j.ws0, sizeof(double) * (size_t)j.ng * q.k);
                }
            }
        }
        CUSK_HIP(e, evs.record(1, s));
        CUSK_HIP(e, res.read_back(s));
        if (nex) CUSK_HIP(e, hipMemcpyAsync(h_jk.data(), jk.jk, sizeof(double) * 4 * nex, hipMemcpyDeviceToHost, s));
        if (nex) CUSK_HIP(e, hipMemcpyAsync(h_arg.data(), jk.jk_arg, sizeof(int) * nex, hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipMemcpyAsync(h_jkstats.data(), jk.jk_stats, sizeof(double) * 2 * na, hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipMemcpyAsync(h_jkstatus.data(), jk.jk_status, sizeof(int) * na, hipMemcpyDeviceToHost, s));
        if (pres)
        {
            h_pres.resize(std::max<size_t>(niv, 1));
            CUSK_HIP(e, hipMemcpyAsync(h_pres.data(), jk.pres, sizeof(double) * niv, hipMemcpyDeviceToHost, s));
        }
        CUSK_HIP(e, hipStreamSynchronize(s));
        float ms = 0.0f;
        CUSK_HIP(e, evs.elapsed(&ms, 0, 1));
        if (kernel_ms) *kernel_ms = ms;
    }
    mv_fill_unset(nout, plan.status, ex_off, theta, se, stats, status);
    for (int a = 0; a < nout; a++)
    {  // what holds where no refit is made for a reason the host knows
        jk_status[a] = jp.status[(size_t)a];
        jk_stats[(size_t)a * 2] = jk_stats[(size_t)a * 2 + 1] = kMvNaN;
        for (int c = ex_off[a]; c < ex_off[a + 1]; c++)
        {
            for (int i = 0; i < 4; i++) jk_out[(size_t)c * 4 + i] = kMvNaN;
            jk_arg[c] = -1;
        }
    }
    if (pres)
        for (long long i = iv_off[0]; i < iv_off[nout]; i++) pres[i] = kMvNaN;
    if (refit)
        for (long long i = 0; i < jp.refit_off[(size_t)nout]; i++) refit[i] = kMvNaN;
    for (size_t slot = 0; slot < na; slot++)
    {
        const MvOutcome &q = plan.outcomes[slot];
        status[q.out] = res.status[slot];
        for (int c = 0; c < 3; c++) stats[(size_t)q.out * 3 + c] = res.stats[slot * 3 + c];
        jk_status[q.out] = h_jkstatus[slot];
        for (int c = 0; c < 2; c++) jk_stats[(size_t)q.out * 2 + c] = h_jkstats[slot * 2 + c];
        for (int c = 0; c < q.k; c++)
        {
            theta[q.ex0 + c] = res.theta[(size_t)q.ex0 + c];
            se[q.ex0 + c] = res.se[(size_t)q.ex0 + c];
            for (int i = 0; i < 4; i++) jk_out[(size_t)(q.ex0 + c) * 4 + i] = h_jk[(size_t)(q.ex0 + c) * 4 + i];
            jk_arg[q.ex0 + c] = h_arg[(size_t)q.ex0 + c];
        }
        if (h_jkstatus[slot] != 0) continue;
        if (pres) std::memcpy(pres + q.iv0, h_pres.data() + q.iv0, sizeof(double) * (size_t)q.m);
        if (refit)
        {
            const size_t off = (size_t)jp.refit_off[(size_t)q.out], cnt = (size_t)jp.outcomes[slot].ng * q.k;
            std::memcpy(refit + off, h_refit.data() + off, sizeof(double) * cnt);
        }
    }
    return CUSK_OK;
}

}  // namespace

}  // namespace cusk

extern "C" int cusk_mvivw_jackknife(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout,
                                    const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex,
                                    const long long *grp_off, const int *grp, int model, double *theta, double *se, double *stats,
                                    int *status, double *jk, int *jk_arg, double *jk_stats, int *jk_status, double *pres,
                                    double *refit, float *kernel_ms)
{
    return cusk::mvivw_jackknife_impl(e, beta, weight, M, p, nout, outcome, iv_off, iv, ex_off, ex, grp_off, grp, model, theta, se,
                                      stats, status, jk, jk_arg, jk_stats, jk_status, pres, refit, kernel_ms);
}
