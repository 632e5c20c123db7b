// mvivw_ld.hip -- multivariable IVW regressions with correlated instruments by generalised least squares (cusk_mvivw_ld
// of include/cusk_hip.h, where the rule is stated; `ci-gwas mvivw --ld`).
//
// Per outcome: R = the LD of its m instruments (unit diagonal, ridge), R = CC', the whitened table
// Zw = C^-1 diag(sqrt(w)) (X, y), and on Zw the rule of cusk_mvivw with every weight 1.  IEEE double throughout, no
// floating-point atomics; outcomes run one after another on the engine's stream and share one workspace.
//
// The workspace holds R row-major (leading dimension m, lower triangle and diagonal) and, as K = k + 1 further rows of
// length m, the table Zt = (diag(sqrt(w)) (X, y))'.  The blocked right-looking factorisation runs over the m columns of
// that (m + K) x m trapezoid (host/mvivw_ld_plan.h): what it leaves in the last K rows is Zw', so the forward substitution
// of the whitening is done by the panel solve and the trailing update and needs no kernel of its own.
//
//   ld_gather_kernel  one workgroup per list position a: row a of R from `ld` (strict lower triangle, times 1 - ridge), the
//                     unit diagonal, column a of Zt; a non-finite value read, or a weight <= 0, sets code 3
//   ld_factor_kernel  one workgroup per panel: the nb x nb diagonal block in LDS, unblocked right-looking Cholesky with the
//                     pivot test (code 4 and the failing pivot by plain vector stores), the factor written back and its
//                     inverse, computed in place in LDS, stored for the panel solve
//   ld_solve_kernel   32 rows below the diagonal block per workgroup: L21 = A21 L11^-T as a product with the stored inverse
//   ld_update_kernel  one 64 x 64 tile of the trailing rows per workgroup, A22 -= L21 L21' with a depth of one panel: this
//                     is where the m^3 / 3 lives.  FP64 vector pipe: thread t owns a 4 x 4 register tile and walks two LDS
//                     slabs (transposed, so that the four values of a thread are two ds_read_b128) with plain FMAs, k
//                     ascending.  Every element takes its updates in panel order.
//   ld_gram_kernel, ld_resid_kernel
//                     the Gram and residual steps of the regression for unit weights, identity lists and the transposed
//                     table Zw': chunks of CUSK_MVIVW_CHUNK rows in row order, added in chunk order.  Only their staging
//                     and their reads of Zw' are written here; the tile walk, the packed store and the ordered sum are
//                     those of mvivw_reg.h, and the solve and finish steps are mv_solve_kernel and mv_finish_kernel of
//                     mvivw.hip themselves, launched per outcome on its slot of the plan's MvOutcome table
// Every kernel after the gather returns at once when the outcome's code is set; the host reads the code after the last
// panel and launches nothing further for an outcome that failed.  The host (host/mvivw_ld_plan.h) checks every index and
// the workspace bound before anything is launched.
//
// Why the vector pipe and not v_mfma_f64_16x16x4_f64: on gfx950 the FP64 matrix rate equals the FP64 vector rate (the
// matrix instruction saves operand traffic, not cycles), the update's depth is one panel (64), and the plain FMA chain has
// one obvious summation order.  The matrix form is the follow-up once a wider panel makes LDS traffic the limit.
#include "host/mvivw_ld_plan.h"
#include "mvivw_reg.h"

#include <string>

namespace cusk {

namespace {

constexpr int kLdS = kLdPanel + 1;  // LDS row stride of the 64 x 64 blocks
static_assert(kLdPanel == 64 && kLdTile == 64 && kLdSolveRows == 32, "the kernels' thread maps are written for these");

struct LdState
{
    double minpiv;   // smallest squared pivot of R so far
    double failpiv;  // the pivot that failed (code 4)
    int code;        // 0, 3 or 4
    int pad;
};

struct LdProblem
{
    double *A;   // m x m, row-major, lower triangle
    double *zt;  // K x m
    LdState *st;
    int m, K;    // K = k + 1
};

__device__ __forceinline__ double *ld_row(const LdProblem &q, int r)
{
    return r < q.m ? q.A + (size_t)r * q.m : q.zt + (size_t)(r - q.m) * q.m;
}

__global__ void ld_init_kernel(LdState *st)
{
    st->minpiv = INFINITY;
    st->failpiv = NAN;
    st->code = 0;
    st->pad = 0;
}

__global__ void __launch_bounds__(256) ld_gather_kernel(LdProblem q, const double *__restrict__ ld, const double *__restrict__ beta,
                                                        const double *__restrict__ weight, long long M, int p, const int *__restrict__ iv,
                                                        const int *__restrict__ ex, int o, double ridge)
{
    const int tid = threadIdx.x, a = blockIdx.x, k = q.K - 1;
    const int ia = iv[a];
    const double *src = ld + (size_t)ia * (size_t)M;
    double *dst = q.A + (size_t)a * q.m;
    const double scale = 1.0 - ridge;
    int bad = 0;
    for (int b = tid; b < a; b += 256)
    {  // the list ascends: iv[b] < ia, the strict lower triangle of ld
        const double v = src[iv[b]];
        bad |= !mv_finite(v);
        dst[b] = v * scale;
    }
    if (tid == 0) dst[a] = 1.0;
    const double w = weight[(size_t)ia * p + o];
    const int wbad = !(w > 0.0 && w <= DBL_MAX);
    const double sw = sqrt(w);
    for (int c = tid; c < q.K; c += 256)
    {
        const double x = beta[(size_t)ia * p + (c < k ? ex[c] : o)];
        bad |= (!mv_finite(x)) | wbad;
        q.zt[(size_t)c * q.m + a] = x * sw;
    }
    if (__syncthreads_or(bad) && tid == 0) q.st->code = 3;
}

__global__ void __launch_bounds__(256) ld_factor_kernel(LdProblem q, int j0, int nb, double *__restrict__ dinv)
{
    __shared__ double S[kLdPanel * kLdS];
    const int tid = threadIdx.x;
    if (q.st->code != 0) return;
    for (int idx = tid; idx < nb * nb; idx += 256)
    {
        const int r = idx / nb, c = idx - r * nb;
        S[r * kLdS + c] = c <= r ? q.A[(size_t)(j0 + r) * q.m + j0 + c] : 0.0;
    }
    double minpiv = q.st->minpiv;
    __syncthreads();
    const int tr = tid >> 4, tc = tid & 15;
    for (int j = 0; j < nb; j++)
    {
        const double piv = S[j * kLdS + j];
        if (!(piv >= minpiv)) minpiv = piv;
        if (!(piv >= kMvPivotMin))
        {  // the same for every thread
            if (tid == 0)
            {
                q.st->failpiv = piv;
                q.st->code = 4;
            }
            return;
        }
        const double l = sqrt(piv);
        __syncthreads();
        if (tid == 0) S[j * kLdS + j] = l;
        for (int r = j + 1 + tid; r < nb; r += 256) S[r * kLdS + j] /= l;
        __syncthreads();
        for (int r = j + 1 + tr; r < nb; r += 16)
        {
            const double lrj = S[r * kLdS + j];
            for (int c = j + 1 + tc; c <= r; c += 16) S[r * kLdS + c] = fma(-lrj, S[c * kLdS + j], S[r * kLdS + c]);
        }
        __syncthreads();
    }
    for (int idx = tid; idx < nb * nb; idx += 256)
    {
        const int r = idx / nb, c = idx - r * nb;
        if (c <= r) q.A[(size_t)(j0 + r) * q.m + j0 + c] = S[r * kLdS + c];
    }
    if (tid == 0) q.st->minpiv = minpiv;
    // the inverse of the block's factor in place, last column first: X_jj = 1 / L_jj, X_ij = -(sum_{c = j+1..i} X_ic L_cj) / L_jj
    for (int j = nb - 1; j >= 0; j--)
    {
        const double ajj = 1.0 / S[j * kLdS + j];
        double s = 0.0;
        if (tid > j && tid < nb)
            for (int c = j + 1; c <= tid; c++) s = fma(S[tid * kLdS + c], S[c * kLdS + j], s);
        __syncthreads();
        if (tid > j && tid < nb) S[tid * kLdS + j] = -s * ajj;
        if (tid == j) S[j * kLdS + j] = ajj;
        __syncthreads();
    }
    for (int idx = tid; idx < kLdPanel * kLdPanel; idx += 256)
    {
        const int r = idx >> 6, c = idx & 63;
        dinv[idx] = (r < nb && c <= r) ? S[r * kLdS + c] : 0.0;
    }
}

__global__ void __launch_bounds__(256) ld_solve_kernel(LdProblem q, int j0, int nb, const double *__restrict__ dinv)
{
    __shared__ double Li[kLdPanel * kLdS];
    __shared__ double As[kLdSolveRows * kLdS];
    const int tid = threadIdx.x;
    if (q.st->code != 0) return;
    const int rows = q.m + q.K, r0 = j0 + nb + (int)blockIdx.x * kLdSolveRows;
    for (int idx = tid; idx < kLdPanel * kLdPanel; idx += 256) Li[(idx >> 6) * kLdS + (idx & 63)] = dinv[idx];
    for (int idx = tid; idx < kLdSolveRows * kLdPanel; idx += 256)
    {
        const int r = idx >> 6, c = idx & 63, gr = r0 + r;
        As[r * kLdS + c] = (gr < rows && c < nb) ? ld_row(q, gr)[j0 + c] : 0.0;
    }
    __syncthreads();
    const int r = tid >> 3, cg = tid & 7, gr = r0 + r;
    if (gr >= rows) return;
    double *dst = ld_row(q, gr) + j0;
    for (int i = 0; i < 8; i++)
    {  // L21[r][c] = sum_{j <= c} A21[r][j] Linv[c][j]
        const int c = cg + 8 * i;
        double s = 0.0;
        for (int j = 0; j <= c; j++) s = fma(As[r * kLdS + j], Li[c * kLdS + j], s);
        if (c < nb) dst[c] = s;
    }
}

constexpr int kLdUs = kLdTile + 2;  // slab stride: 16-byte aligned rows, the staging writes spread over the banks

__global__ void __launch_bounds__(256) ld_update_kernel(LdProblem q, int j0)
{
    __shared__ __attribute__((aligned(16))) double As[32 * kLdUs];
    __shared__ __attribute__((aligned(16))) double Bs[32 * kLdUs];
    const int tid = threadIdx.x, tj = blockIdx.x, ti = blockIdx.y;
    if (!ld_tile_active(ti, tj)) return;
    if (q.st->code != 0) return;
    const int rows = q.m + q.K, c0 = j0 + kLdPanel;
    const int rbase = c0 + ti * kLdTile, cbase = c0 + tj * kLdTile;
    const int ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (int kh = 0; kh < kLdPanel; kh += 32)
    {
        for (int idx = tid; idx < 32 * kLdTile; idx += 256)
        {
            const int kk = idx & 31, r = idx >> 5;
            const int gr = rbase + r, gc = cbase + r;
            As[kk * kLdUs + r] = gr < rows ? ld_row(q, gr)[j0 + kh + kk] : 0.0;
            Bs[kk * kLdUs + r] = gc < q.m ? q.A[(size_t)gc * q.m + j0 + kh + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 32; kk++)
        {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = As[kk * kLdUs + ty * 4 + i];
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = Bs[kk * kLdUs + tx * 4 + j];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const int gr = rbase + ty * 4 + i;
        if (gr >= rows) continue;
        double *dst = ld_row(q, gr);
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int gc = cbase + tx * 4 + j;
            if (gc < q.m && (gr >= q.m || gc <= gr)) dst[gc] -= acc[i][j];
        }
    }
}

// ---- the regression on the whitened table Zw' (zt: K x m, row c = column c of Zw): unit weights, identity lists ----
template <int TS, int LD, int SLAB>
__global__ void __launch_bounds__(256) ld_gram_kernel(const double *zt, int m, int K, double *part)
{
    __shared__ double zs[SLAB * LD];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const int T = (K + TS - 1) / TS, ntiles = T * (T + 1) / 2;
    const int t = min(tid, ntiles - 1), ti = mv_tile_row(t), tj = t - ti * (ti + 1) / 2;
    double acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.0;
    const int row0 = chunk * kMvChunk, rows = min(kMvChunk, m - row0);
    for (int s0 = 0; s0 < rows; s0 += SLAB)
    {
        for (int idx = tid; idx < SLAB * LD; idx += 256)
        {  // consecutive threads read consecutive rows of one column: consecutive addresses of zt
            const int r = idx % SLAB, c = idx / SLAB;
            zs[r * LD + c] = (s0 + r < rows && c < K) ? zt[(size_t)c * m + row0 + s0 + r] : 0.0;
        }
        __syncthreads();
        if (tid < ntiles) mv_slab_walk<TS, LD, SLAB>(zs + ti * TS, zs + tj * TS, acc);
        __syncthreads();
    }
    if (tid < ntiles) mv_store_tile<TS>(part + (size_t)chunk * (K * (K + 1) / 2), K, ti, tj, acc);
}

// `sol`, `status`: those of the outcome's slot
__global__ void __launch_bounds__(256) ld_resid_kernel(const double *zt, int m, int k, const double *sol, const int *status, double *rpart)
{
    __shared__ double th[kMvVec];
    __shared__ double sh[4];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (*status != 0) return;  // the same for the whole workgroup; its partial is never read
    if (tid < k) th[tid] = sol[tid];
    __syncthreads();
    const int pos = chunk * kMvChunk + tid;
    double term = 0.0;
    if (pos < m)
    {
        double fit = 0.0;
        for (int j = 0; j < k; j++) fit = fma(zt[(size_t)j * m + pos], th[j], fit);
        const double r = zt[(size_t)k * m + pos] - fit;
        term = r * r;
    }
    const double sum = mv_block_sum(term, sh);
    if (tid == 0) rpart[chunk] = sum;
}

int mvivw_ld_impl(cusk_engine *e, const double *beta, const double *weight, const double *ld, double ridge, long long M, int p,
                  int nout, const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model,
                  double *theta, double *se, double *stats, int *status, float *kernel_ms)
{
    const std::string who = "cusk_mvivw_ld";
    if (!e) return CUSK_ERR_ARG;
    if (!beta || !weight || !ld || (nout > 0 && (!stats || !status))) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    LdPlan plan;
    std::string msg;
    if (mvivw_ld_plan_build(M, p, nout, outcome, iv_off, iv, ex_off, ex, model, ridge, e->opt_mvivw_ld_bytes, plan, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (nout > 0 && ex_off[nout] > ex_off[0] && (!theta || !se)) return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nout == 0) return CUSK_OK;
    const double nan = kMvNaN;
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout];
    MvResults res(na, nex);
    std::vector<double> rpiv_h(na, nan);
    std::vector<int> code_h(na, 0);
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_ld, d_iv, d_ex, d_outs, d_ws, d_zt, d_dinv, d_state, d_part, d_rpart;
        ScopedEvents<2> evs;
        CUSK_HIP(e, upload_async(d_beta, beta, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_weight, weight, sizeof(double) * (size_t)M * p, s));
        CUSK_HIP(e, upload_async(d_ld, ld, sizeof(double) * (size_t)M * (size_t)M, s));
        CUSK_HIP(e, upload_async(d_iv, iv, sizeof(int) * (size_t)iv_off[nout], s));
        CUSK_HIP(e, upload_async(d_ex, ex, sizeof(int) * nex, s));
        CUSK_HIP(e, upload_async(d_outs, plan.outcomes.data(), sizeof(MvOutcome) * na, s));
        const size_t emax = (size_t)(kMvMaxExposures + 1) * (kMvMaxExposures + 2) / 2;
        CUSK_HIP(e, d_ws.ensure(sizeof(double) * plan.ws_doubles));
        CUSK_HIP(e, d_zt.ensure(sizeof(double) * plan.zt_doubles));
        CUSK_HIP(e, d_dinv.ensure(sizeof(double) * kLdPanel * kLdPanel));
        CUSK_HIP(e, d_state.ensure(sizeof(LdState)));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * (size_t)plan.max_chunks * emax));
        CUSK_HIP(e, d_rpart.ensure(sizeof(double) * (size_t)plan.max_chunks));
        MvBatch b;  // for the solve and finish kernels, which read no table
        b.beta = b.weight = nullptr;
        b.p = p;
        b.model = model;
        b.iv = b.ex = nullptr;
        b.outs = d_outs.as<MvOutcome>();
        b.part = d_part.as<double>();
        b.chunk_bad = nullptr;  // status 3 comes from the gather
        b.rpart = d_rpart.as<double>();
        CUSK_HIP(e, res.alloc(b));
        CUSK_HIP(e, mv_reg_prepare());
        CUSK_HIP(e, evs.record(0, s));
        for (size_t slot = 0; slot < na; slot++)
        {
            const MvOutcome &o = plan.outcomes[slot];
            LdProblem q;
            q.A = d_ws.as<double>();
            q.zt = d_zt.as<double>();
            q.st = d_state.as<LdState>();
            q.m = o.m;
            q.K = o.k + 1;
            hipLaunchKernelGGL(ld_init_kernel, dim3(1), dim3(1), 0, s, q.st);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(ld_gather_kernel, dim3((unsigned)o.m), dim3(256), 0, s, q, d_ld.as<double>(), d_beta.as<double>(),
                               d_weight.as<double>(), M, p, d_iv.as<int>() + o.iv0, d_ex.as<int>() + o.ex0, o.o, ridge);
            CUSK_HIP(e, hipGetLastError());
            for (const LdPanel &pn : ld_panels(o.m, q.K))
            {
                hipLaunchKernelGGL(ld_factor_kernel, dim3(1), dim3(256), 0, s, q, pn.j0, pn.nb, d_dinv.as<double>());
                CUSK_HIP(e, hipGetLastError());
                if (pn.solve_blocks > 0)
                {
                    hipLaunchKernelGGL(ld_solve_kernel, dim3((unsigned)pn.solve_blocks), dim3(256), 0, s, q, pn.j0, pn.nb,
                                       d_dinv.as<double>());
                    CUSK_HIP(e, hipGetLastError());
                }
                if (pn.tc > 0)
                {
                    hipLaunchKernelGGL(ld_update_kernel, dim3((unsigned)pn.tc, (unsigned)pn.tr), dim3(256), 0, s, q, pn.j0);
                    CUSK_HIP(e, hipGetLastError());
                }
            }
            LdState st_host;
            CUSK_HIP(e, hipMemcpyAsync(&st_host, d_state.p, sizeof(LdState), hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipStreamSynchronize(s));
            code_h[slot] = st_host.code;
            rpiv_h[slot] = st_host.code == 4 ? st_host.failpiv : st_host.code == 0 ? st_host.minpiv : nan;
            if (st_host.code != 0) continue;  // nothing further reads a factor that does not exist
            hipLaunchKernelGGL((ld_gram_kernel<8, 128, 16>), dim3((unsigned)o.nchunks), dim3(256), 0, s, q.zt, o.m, q.K, b.part);
            CUSK_HIP(e, hipGetLastError());
            launch_mv_solve(s, b, (int)slot, 1);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(ld_resid_kernel, dim3((unsigned)o.nchunks), dim3(256), 0, s, q.zt, o.m, o.k, b.sol + slot * kMvSolLd,
                               b.status + slot, b.rpart);
            CUSK_HIP(e, hipGetLastError());
            launch_mv_finish(s, b, (int)slot, 1);
            CUSK_HIP(e, hipGetLastError());
        }
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
        const MvOutcome &o = plan.outcomes[slot];
        if (code_h[slot] != 0)
        {  // 3 or 4: no estimates; stats[2] is the pivot of R that failed (4) or NaN (3)
            status[o.out] = code_h[slot];
            stats[(size_t)o.out * 3 + 2] = rpiv_h[slot];
            continue;
        }
        const int st = res.status[slot];
        status[o.out] = st;
        stats[(size_t)o.out * 3] = res.stats[slot * 3];
        stats[(size_t)o.out * 3 + 1] = res.stats[slot * 3 + 1];
        stats[(size_t)o.out * 3 + 2] = st == 0 ? rpiv_h[slot] : res.stats[slot * 3 + 2];
        if (st != 0) continue;
        for (int c = 0; c < o.k; c++)
        {
            theta[o.ex0 + c] = res.theta[(size_t)o.ex0 + c];
            se[o.ex0 + c] = res.se[(size_t)o.ex0 + c];
        }
    }
    return CUSK_OK;
}

}  // namespace

}  // namespace cusk

extern "C" int cusk_mvivw_ld(cusk_engine *e, const double *beta, const double *weight, const double *ld, double ridge, long long M,
                             int p, int nout, const int *outcome, const long long *iv_off, const int *iv, const int *ex_off,
                             const int *ex, int model, double *theta, double *se, double *stats, int *status, float *kernel_ms)
{
    return cusk::mvivw_ld_impl(e, beta, weight, ld, ridge, M, p, nout, outcome, iv_off, iv, ex_off, ex, model, theta, se, stats,
                               status, kernel_ms);
}
