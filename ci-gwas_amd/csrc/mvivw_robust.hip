// mvivw_robust.hip -- outlier-resistant IVW regressions by iteratively reweighted least squares (cusk_mvivw_robust and
// cusk_abs_median of include/cusk_hip.h, where the rule is stated; `ci-gwas mvivw --robust`).
//
// The problems, their chunks and their plain start are those of mvivw.hip: the same plan, the same Gram, solve and tile
// code (mvivw_reg.h).  Around them an iteration per outcome, Huber weights first, then (psi = 2) bisquare weights, each
// update one weighted Gram pass.  Everything is IEEE double, every sum over rows is a sum of chunk sums in chunk order,
// and the scale is an exact order statistic found on integers: no floating-point atomics, two runs give the same bytes.
//
//   mv_rb_resid_kernel   one workgroup per (outcome, chunk), one row per thread: e_i = sqrt(w_i) (y_i - x_i theta)
//   mv_abs_select        (device function) the r-th smallest of |v_0| .. |v_{n-1}| by a radix select on the 63-bit
//                        patterns of the absolute values: eight passes of eight bits, a histogram of 256 integer counts in
//                        LDS per pass.  Counts are integers, so the answer does not depend on the order they are made in.
//   abs_median_kernel    one workgroup per segment: the median of |v| (cusk_abs_median)
//   mv_rb_step_kernel    one workgroup per outcome: the scale from the median of |e|, the convergence test, the stage and
//                        update counters, the statuses 5 and 6, and the freeze of an outcome that is done
//   mv_rb_weight_kernel  one workgroup per (outcome, chunk): rho_i from e_i and the scale; in its last call also the chunk
//                        sums of psi^2, psi', rho and e^2
//   mv_rb_finish_kernel  one workgroup per outcome: the chunk sums in chunk order, tau, the standard errors, the stats
// An update enqueues weight -> Gram (rho form) -> solve -> residual -> step and nothing waits for it: the host reads the
// count of outcomes still running once per kRbPoll updates.  The workgroups of a frozen outcome return at once, and a
// frozen outcome's values are never touched again, so they do not depend on what the other outcomes of the call do.
#include "mvivw_reg.h"

#include <cstring>
#include <string>

namespace cusk {

namespace {

constexpr int kRbMaxUpdates = 100;  // per stage
constexpr int kRbPoll = 8;          // updates enqueued between two reads of the live count
constexpr int kRbStats = 6;
constexpr double kRbMad = 1.4826, kRbHuber = 1.345, kRbBisq = 4.685, kRbTol = 1e-10;

struct MvRobust
{
    double *e;          // layout of iv: the standardised residuals at the outcome's current theta
    double *rho;        // layout of iv
    double *theta_cur;  // per active outcome: kMvVec doubles, theta before the update in flight
    double *v;          // per active outcome: kMvVec doubles, diag(G^-1) of the plain Gram
    double *d;          // per active outcome: kMvVec doubles, sqrt(G_jj) of the plain Gram
    double *scale;      // per active outcome
    double *csum;       // per chunk of the call: sum psi^2, sum psi', sum rho, sum e^2
    int *stage;         // per active outcome: 0 Huber, 1 bisquare
    int *updates;       // per active outcome: 2 ints, updates of the stage and of the outcome
    int *frozen;        // per active outcome
    int *nlive;         // outcomes of the group in flight that are not frozen
    int psi;
};

__device__ __forceinline__ unsigned long long mv_abs_bits(double v)
{
    return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
}

// The r-th smallest (r = 0 .. n - 1) of the absolute values of v[0 .. n), as its bit pattern.  Called by every thread of
// a workgroup of 256 with the same arguments; hist: 256 counts, pick: 2 words, both in LDS.
__device__ unsigned long long mv_abs_select(const double *__restrict__ v, unsigned n, unsigned r, unsigned *hist, unsigned *pick)
{
    const int tid = threadIdx.x;
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8)
    {
        hist[tid] = 0;
        __syncthreads();
        for (unsigned i = tid; i < n; i += 256)
        {
            const unsigned long long key = mv_abs_bits(v[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0)
        {
            unsigned below = 0, bin = 0;
            while (bin < 255 && below + hist[bin] <= r) below += hist[bin++];
            pick[0] = bin;
            pick[1] = r - below;
        }
        __syncthreads();
        prefix |= (unsigned long long)pick[0] << shift;
        mask |= 0xffull << shift;
        r = pick[1];
        __syncthreads();
    }
    return prefix;
}

// the median of |v[0 .. n)|, n >= 1: the middle value, or (a + b) * 0.5 of the two middle ones
__device__ double mv_abs_median(const double *__restrict__ v, unsigned n, unsigned *hist, unsigned *pick)
{
    const double hi = __longlong_as_double((long long)mv_abs_select(v, n, n / 2, hist, pick));
    if (n & 1u) return hi;
    const double lo = __longlong_as_double((long long)mv_abs_select(v, n, n / 2 - 1, hist, pick));
    return (lo + hi) * 0.5;
}

__global__ void __launch_bounds__(256) abs_median_kernel(const double *__restrict__ vals, const long long *__restrict__ seg_off,
                                                         double *__restrict__ out)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];
    const long long a = seg_off[blockIdx.x], n = seg_off[blockIdx.x + 1] - a;  // n < 2^31 by the host's check
    const double med = n > 0 ? mv_abs_median(vals + a, (unsigned)n, hist, pick) : NAN;
    if (threadIdx.x == 0) out[blockIdx.x] = med;
}

__global__ void __launch_bounds__(256) mv_rb_resid_kernel(MvBatch b, MvRobust rb, const MvChunk *__restrict__ chunks)
{
    __shared__ double th[kMvVec];
    __shared__ int cols[kMvVec];
    const int tid = threadIdx.x;
    const MvChunk ch = chunks[blockIdx.x];
    if (rb.frozen[ch.slot] || b.status[ch.slot] != 0) return;  // the same for the whole workgroup
    const MvOutcome q = b.outs[ch.slot];
    const int k = q.k, p = b.p;
    if (tid < k)
    {
        th[tid] = b.sol[(size_t)ch.slot * kMvSolLd + tid];
        cols[tid] = b.ex[q.ex0 + tid];
    }
    __syncthreads();
    const int pos = ch.chunk * kMvChunk + tid;
    if (pos < q.m)
    {
        const size_t base = (size_t)b.iv[q.iv0 + pos] * p;
        double fit = 0.0;
        for (int j = 0; j < k; j++) fit = fma(b.beta[base + cols[j]], th[j], fit);
        rb.e[q.iv0 + pos] = sqrt(b.weight[base + q.o]) * (b.beta[base + q.o] - fit);
    }
}

// rho of one row: Huber (stage 0) min(1, 1.345 s / |e|), bisquare (stage 1) (1 - u^2)^2 inside |u| < 1, u = e / (4.685 s)
__device__ __forceinline__ double mv_rb_rho(double e, double s, int stage, double *dpsi)
{
    if (stage == 0)
    {
        const double a = fabs(e), c = kRbHuber * s;
        *dpsi = a <= c ? 1.0 : 0.0;
        return a <= c ? 1.0 : c / a;
    }
    const double u = e / (kRbBisq * s), u2 = u * u;
    if (!(fabs(u) < 1.0))
    {
        *dpsi = 0.0;
        return 0.0;
    }
    *dpsi = (1.0 - u2) * (1.0 - 5.0 * u2);
    return (1.0 - u2) * (1.0 - u2);
}

// last: the call after the iteration, for every outcome of status 0, with the chunk sums
__global__ void __launch_bounds__(256) mv_rb_weight_kernel(MvBatch b, MvRobust rb, const MvChunk *__restrict__ chunks, int last)
{
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const MvChunk ch = chunks[blockIdx.x];
    if (last ? b.status[ch.slot] != 0 : rb.frozen[ch.slot] != 0) return;  // the same for the whole workgroup
    const MvOutcome q = b.outs[ch.slot];
    const int pos = ch.chunk * kMvChunk + tid;
    const double s = rb.scale[ch.slot];
    const int stage = rb.stage[ch.slot];
    double e = 0.0, rho = 0.0, dpsi = 0.0;
    if (pos < q.m)
    {
        e = rb.e[q.iv0 + pos];
        rho = mv_rb_rho(e, s, stage, &dpsi);
        rb.rho[q.iv0 + pos] = rho;
    }
    if (!last) return;
    const double psi = e * rho;
    double sums[4];
    sums[0] = mv_block_sum(psi * psi, sh);
    __syncthreads();
    sums[1] = mv_block_sum(dpsi, sh);
    __syncthreads();
    sums[2] = mv_block_sum(rho, sh);
    __syncthreads();
    sums[3] = mv_block_sum(e * e, sh);
    if (tid == 0)
        for (int c = 0; c < 4; c++) rb.csum[(size_t)(q.chunk0 + ch.chunk) * 4 + c] = sums[c];
}

// start: after the plain solve; keeps theta, v and the first scale and makes no update
__global__ void __launch_bounds__(256) mv_rb_step_kernel(MvBatch b, MvRobust rb, int first, int start)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    if (rb.frozen[slot]) return;
    const MvOutcome q = b.outs[slot];
    const int k = q.k;
    int st = b.status[slot];  // 2 or 3: the solve kernel's verdict
    const int stage = rb.stage[slot];
    double s = rb.scale[slot];
    if (st == 0 && (start || stage == 0))
    {
        s = kRbMad * mv_abs_median(rb.e + q.iv0, (unsigned)q.m, hist, pick);
        if (!(s > 0.0)) st = 6;
    }
    if (st != 0)
    {
        if (tid == 0)
        {
            b.status[slot] = st;
            rb.frozen[slot] = 1;
            atomicSub(rb.nlive, 1);
        }
        return;
    }
    const double *sol = b.sol + (size_t)slot * kMvSolLd;
    double *cur = rb.theta_cur + (size_t)slot * kMvVec;
    if (start)
    {
        if (tid < k)
        {
            cur[tid] = sol[tid];
            rb.v[(size_t)slot * kMvVec + tid] = sol[kMvVec + tid];
        }
        if (tid == 0) rb.scale[slot] = s;
        return;
    }
    const double tol = kRbTol * s * sqrt((double)q.m);
    int moved = 0;
    if (tid < k)
    {
        const double nw = sol[tid];
        moved = !(rb.d[(size_t)slot * kMvVec + tid] * fabs(nw - cur[tid]) <= tol);
        cur[tid] = nw;
    }
    moved = __syncthreads_or(moved);
    if (tid == 0)
    {
        rb.scale[slot] = s;
        const int done = rb.updates[2 * slot] + 1;
        rb.updates[2 * slot] = done;
        rb.updates[2 * slot + 1] += 1;
        bool freeze = false;
        if (!moved)
        {
            if (stage == 0 && rb.psi == 2)
            {
                rb.stage[slot] = 1;
                rb.updates[2 * slot] = 0;
            }
            else
                freeze = true;
        }
        else if (done >= kRbMaxUpdates)
        {
            b.status[slot] = 5;
            freeze = true;
        }
        if (freeze)
        {
            rb.frozen[slot] = 1;
            atomicSub(rb.nlive, 1);
        }
    }
}

__global__ void __launch_bounds__(128) mv_rb_finish_kernel(MvBatch b, MvRobust rb, int first)
{
    __shared__ double s_f;
    const int tid = threadIdx.x, slot = first + blockIdx.x;
    const MvOutcome q = b.outs[slot];
    const double *sol = b.sol + (size_t)slot * kMvSolLd;
    double *stats = b.stats + (size_t)slot * kRbStats;
    if (tid == 0)
    {
        int st = b.status[slot];
        double f = NAN;
        if (st == 0)
        {
            double sum[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < q.nchunks; c++)
                for (int i = 0; i < 4; i++) sum[i] += rb.csum[(size_t)(q.chunk0 + c) * 4 + i];
            const double s = rb.scale[slot];
            const double A = sum[0] / (double)(q.m - q.k), B = sum[1] / (double)q.m;
            if (B > 0.0)
            {
                const double tau = sqrt(A) / B;
                const bool random = b.model == 1 || (b.model == 0 && q.m >= 4);
                const double g = random ? tau : tau / s;
                f = g > 1.0 ? g : 1.0;
                stats[0] = sum[3];
                stats[1] = s;
                stats[2] = tau;
                stats[3] = sol[2 * kMvVec];
                stats[4] = (double)rb.updates[2 * slot + 1];
                stats[5] = sum[2];
            }
            else
                b.status[slot] = st = 5;
        }
        if (st != 0)
        {
            for (int c = 0; c < kRbStats; c++) stats[c] = NAN;
            if (st == 2) stats[3] = sol[2 * kMvVec];
        }
        s_f = f;
    }
    __syncthreads();
    if (tid < q.k)
    {
        const double f = s_f;  // NaN: no estimates
        b.theta[q.ex0 + tid] = f == f ? sol[tid] : NAN;
        b.se[q.ex0 + tid] = f == f ? sqrt(rb.v[(size_t)slot * kMvVec + tid]) * f : NAN;
    }
}

int mvivw_robust_impl(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, const int *outcome,
                      const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, int psi, double *theta,
                      double *se, double *stats, int *status, double *rho, float *kernel_ms)
{
    const std::string who = "cusk_mvivw_robust";
    if (!e) return CUSK_ERR_ARG;
    if (!beta || !weight || (nout > 0 && (!stats || !status))) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (psi < 1 || psi > 2) return fail(e, CUSK_ERR_ARG, who + ": psi " + std::to_string(psi) + " is not 1 (Huber) or 2 (bisquare)");
    MvPlan plan;
    std::string msg;
    if (mvivw_plan_build(M, p, nout, outcome, iv_off, iv, ex_off, ex, model, (size_t)e->opt_mvivw_part_bytes, plan, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (nout > 0 && ex_off[nout] > ex_off[0] && (!theta || !se)) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nout == 0) return CUSK_OK;
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout], niv = (size_t)iv_off[nout];
    MvResults res(na, nex, kRbStats);
    std::vector<double> h_rho;
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_iv, d_ex, d_outs, d_chunks, d_part, d_bad, d_rpart;
        ScopedDevBuf d_e, d_rho, d_cur, d_v, d_d, d_scale, d_csum, d_ints;
        ScopedEvents<2> evs;
        CUSK_HIP(e, upload_async(d_beta, beta, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_weight, weight, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_iv, iv, sizeof(int) * niv, s));
        CUSK_HIP(e, upload_async(d_ex, ex, sizeof(int) * nex, s));
        CUSK_HIP(e, upload_async(d_outs, plan.outcomes.data(), sizeof(MvOutcome) * na, s));
        CUSK_HIP(e, upload_async(d_chunks, plan.chunks.data(), sizeof(MvChunk) * plan.chunks.size(), s));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * plan.max_part_doubles));
        CUSK_HIP(e, d_bad.ensure(sizeof(int) * (size_t)plan.total_chunks));
        CUSK_HIP(e, d_e.ensure(sizeof(double) * niv));
        CUSK_HIP(e, d_rho.ensure(sizeof(double) * niv));
        CUSK_HIP(e, d_cur.ensure(sizeof(double) * na * kMvVec));
        CUSK_HIP(e, d_v.ensure(sizeof(double) * na * kMvVec));
        CUSK_HIP(e, d_d.ensure(sizeof(double) * na * kMvVec));
        CUSK_HIP(e, d_scale.ensure(sizeof(double) * na));
        CUSK_HIP(e, d_csum.ensure(sizeof(double) * 4 * (size_t)plan.total_chunks));
        const size_t nints = 4 * na + 1;  // stage, updates (2), frozen per outcome; the live count
        CUSK_HIP(e, d_ints.ensure(sizeof(int) * nints));
        CUSK_HIP(e, hipMemsetAsync(d_ints.p, 0, sizeof(int) * nints, s));
        CUSK_HIP(e, hipMemsetAsync(d_scale.p, 0, sizeof(double) * na, s));

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
        b.rpart = nullptr;  // of mv_resid_kernel, which is not launched here
        CUSK_HIP(e, res.alloc(b));
        MvRobust rb;
        rb.e = d_e.as<double>();
        rb.rho = d_rho.as<double>();
        rb.theta_cur = d_cur.as<double>();
        rb.v = d_v.as<double>();
        rb.d = d_d.as<double>();
        rb.scale = d_scale.as<double>();
        rb.csum = d_csum.as<double>();
        rb.stage = d_ints.as<int>();
        rb.updates = rb.stage + na;
        rb.frozen = rb.stage + 3 * na;
        rb.nlive = rb.stage + 4 * na;
        rb.psi = psi;
        b.frozen = rb.frozen;
        MvBatch b0 = b;  // the plain start: no rho, and the solve kernel keeps d
        b0.dsc = rb.d;
        b.rho = rb.rho;
        CUSK_HIP(e, mv_reg_prepare());
        CUSK_HIP(e, evs.record(0, s));
        const MvChunk *chunks = d_chunks.as<MvChunk>();
        for (const MvGroup &g : plan.groups)
        {  // one stream: a group's partials are read before the next Gram pass overwrites them
            const unsigned nslots = (unsigned)(g.last - g.first);
            const unsigned nchunks = (unsigned)(g.class_first[kMvClasses] - g.class_first[0]);
            const MvChunk *gch = chunks + g.class_first[0];
            int live = (int)nslots;
            CUSK_HIP(e, hipMemcpyAsync(rb.nlive, &live, sizeof(int), hipMemcpyHostToDevice, s));
            auto gram_solve = [&](const MvBatch &bb, bool with_rho) -> hipError_t {
                for (int c = 0; c < kMvClasses; c++)
                {
                    const size_t cnt = g.class_first[c + 1] - g.class_first[c];
                    if (cnt == 0) continue;
                    launch_mv_gram(s, bb, c, chunks + g.class_first[c], cnt, with_rho);
                    if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
                }
                launch_mv_solve(s, bb, g.first, nslots);
                if (hipError_t st = hipGetLastError(); st != hipSuccess) return st;
                hipLaunchKernelGGL(mv_rb_resid_kernel, dim3(nchunks), dim3(256), 0, s, bb, rb, gch);
                return hipGetLastError();
            };
            CUSK_HIP(e, gram_solve(b0, false));
            hipLaunchKernelGGL(mv_rb_step_kernel, dim3(nslots), dim3(256), 0, s, b, rb, g.first, 1);
            CUSK_HIP(e, hipGetLastError());
            // every outcome freezes within kRbMaxUpdates updates per stage, so the live count reaches 0 by then
            for (int done = 0; live > 0 && done < 2 * kRbMaxUpdates; done += kRbPoll)
            {
                for (int u = 0; u < kRbPoll; u++)
                {
                    hipLaunchKernelGGL(mv_rb_weight_kernel, dim3(nchunks), dim3(256), 0, s, b, rb, gch, 0);
                    CUSK_HIP(e, hipGetLastError());
                    CUSK_HIP(e, gram_solve(b, true));
                    hipLaunchKernelGGL(mv_rb_step_kernel, dim3(nslots), dim3(256), 0, s, b, rb, g.first, 0);
                    CUSK_HIP(e, hipGetLastError());
                }
                CUSK_HIP(e, hipMemcpyAsync(&live, rb.nlive, sizeof(int), hipMemcpyDeviceToHost, s));
                CUSK_HIP(e, hipStreamSynchronize(s));
            }
            if (live != 0) return fail(e, CUSK_ERR_HIP, who + ": outcomes still running after the last update");
            hipLaunchKernelGGL(mv_rb_weight_kernel, dim3(nchunks), dim3(256), 0, s, b, rb, gch, 1);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(mv_rb_finish_kernel, dim3(nslots), dim3(128), 0, s, b, rb, g.first);
            CUSK_HIP(e, hipGetLastError());
        }
        CUSK_HIP(e, evs.record(1, s));
        CUSK_HIP(e, res.read_back(s));
        if (rho)
        {
            h_rho.resize(niv);
            CUSK_HIP(e, hipMemcpyAsync(h_rho.data(), rb.rho, sizeof(double) * niv, hipMemcpyDeviceToHost, s));
        }
        CUSK_HIP(e, hipStreamSynchronize(s));
        float ms = 0.0f;
        CUSK_HIP(e, evs.elapsed(&ms, 0, 1));
        if (kernel_ms) *kernel_ms = ms;
    }
    mv_fill_unset(nout, plan.status, ex_off, theta, se, stats, status, kRbStats);
    if (rho)
        for (long long i = iv_off[0]; i < iv_off[nout]; i++) rho[i] = kMvNaN;
    for (size_t slot = 0; slot < na; slot++)
    {
        const MvOutcome &q = plan.outcomes[slot];
        status[q.out] = res.status[slot];
        for (int c = 0; c < kRbStats; c++) stats[(size_t)q.out * kRbStats + c] = res.stats[slot * kRbStats + c];
        for (int c = 0; c < q.k; c++)
        {
            theta[q.ex0 + c] = res.theta[(size_t)q.ex0 + c];
            se[q.ex0 + c] = res.se[(size_t)q.ex0 + c];
        }
        if (rho && res.status[slot] == 0) std::memcpy(rho + q.iv0, h_rho.data() + q.iv0, sizeof(double) * (size_t)q.m);
    }
    return CUSK_OK;
}

int abs_median_impl(cusk_engine *e, const double *vals, const long long *seg_off, int nseg, double *out)
{
    const std::string who = "cusk_abs_median";
    if (!e) return CUSK_ERR_ARG;
    if (nseg < 0 || (nseg > 0 && (!seg_off || !out))) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (nseg == 0) return CUSK_OK;
    if (seg_off[0] < 0) return fail(e, CUSK_ERR_ARG, who + ": bad offsets");
    for (int a = 0; a < nseg; a++)
        if (seg_off[a + 1] < seg_off[a] || seg_off[a + 1] - seg_off[a] > 0x7fffffffll)
            return fail(e, CUSK_ERR_ARG, who + ": segment " + std::to_string(a) + ": offsets are not monotone, or 2^31 values or more");
    if (seg_off[nseg] > 0 && !vals) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    ScopedDevBuf d_vals, d_off, d_out;
    CUSK_HIP(e, upload_async(d_vals, vals, sizeof(double) * (size_t)seg_off[nseg], s));
    CUSK_HIP(e, upload_async(d_off, seg_off, sizeof(long long) * ((size_t)nseg + 1), s));
    CUSK_HIP(e, d_out.ensure(sizeof(double) * (size_t)nseg));
    hipLaunchKernelGGL(abs_median_kernel, dim3((unsigned)nseg), dim3(256), 0, s, d_vals.as<double>(), d_off.as<long long>(),
                       d_out.as<double>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(out, d_out.p, sizeof(double) * (size_t)nseg, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

}  // namespace

}  // namespace cusk

extern "C" int cusk_mvivw_robust(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout,
                                 const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex,
                                 int model, int psi, double *theta, double *se, double *stats, int *status, double *rho,
                                 float *kernel_ms)
{
    return cusk::mvivw_robust_impl(e, beta, weight, M, p, nout, outcome, iv_off, iv, ex_off, ex, model, psi, theta, se, stats,
                                   status, rho, kernel_ms);
}

extern "C" int cusk_abs_median(cusk_engine *e, const double *vals, const long long *seg_off, int nseg, double *out)
{
    return cusk::abs_median_impl(e, vals, seg_off, nseg, out);
}
