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
//   ld_gram_kernel, ld_reg_solve_kernel, ld_resid_kernel, ld_finish_kernel
//                     the Gram, solve, residual and finish steps of mvivw.hip instantiated for unit weights, identity
//                     lists and the transposed table Zw' (mvivw.hip itself is not touched): chunks of CUSK_MVIVW_CHUNK
//                     rows in row order, added in chunk order
// Every kernel after the gather returns at once when the outcome's code is set; the host reads the code after the last
// panel and launches nothing further for an outcome that failed.  The host (host/mvivw_ld_plan.h) checks every index and
// the workspace bound before anything is launched.
//
// Why the vector pipe and not v_mfma_f64_16x16x4_f64: on gfx950 the FP64 matrix rate equals the FP64 vector rate (the
// matrix instruction saves operand traffic, not cycles), the update's depth is one panel (64), and the plain FMA chain has
// one obvious summation order.  The matrix form is the follow-up once a wider panel makes LDS traffic the limit.
#include "cusk_internal.h"
#include "host/mvivw_ld_plan.h"

#include <cfloat>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace cusk {

namespace {

constexpr int kLdVec = 128;
constexpr int kLdTriMax = kMvMaxExposures * (kMvMaxExposures + 1) / 2;
constexpr int kLdSolLd = 2 * kLdVec + 1;  // theta[128], v[128], the smallest squared pivot of the Gram
constexpr double kLdPivotMin = CUSK_PHEN_PIVOT_MIN;
constexpr int kLdS = kLdPanel + 1;  // LDS row stride of the 64 x 64 blocks
static_assert(kLdPanel == 64 && kLdTile == 64 && kLdSolveRows == 32, "the kernels' thread maps are written for these");
static_assert(kMvChunk == 256, "the residual kernel gives every thread of a workgroup one row of a chunk");

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

__device__ __forceinline__ bool ld_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN
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
        bad |= !ld_finite(v);
        dst[b] = v * scale;
    }
    if (tid == 0) dst[a] = 1.0;
    const double w = weight[(size_t)ia * p + o];
    const int wbad = !(w > 0.0 && w <= DBL_MAX);
    const double sw = sqrt(w);
    for (int c = tid; c < q.K; c += 256)
    {
        const double x = beta[(size_t)ia * p + (c < k ? ex[c] : o)];
        bad |= (!ld_finite(x)) | wbad;
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
        if (!(piv >= kLdPivotMin))
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

// ---- the regression on the whitened table: the steps of mvivw.hip for unit weights and identity lists ----
struct LdReg
{
    const double *zt;  // K x m: row c = column c of Zw
    int m, k;
    int model;
    int ex0, slot;
    double *part;   // nchunks x E
    double *rpart;  // nchunks
    double *sol;    // kLdSolLd
    int *status;    // per active outcome
    double *theta, *se, *stats;
};

template <int TS, int LD, int SLAB>
__global__ void __launch_bounds__(256) ld_gram_kernel(LdReg b)
{
    __shared__ double zs[SLAB * LD];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const int K = b.k + 1;
    const int T = (K + TS - 1) / TS, ntiles = T * (T + 1) / 2;
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
    const int row0 = chunk * kMvChunk, rows = min(kMvChunk, b.m - row0);
    for (int s0 = 0; s0 < rows; s0 += SLAB)
    {
        for (int idx = tid; idx < SLAB * LD; idx += 256)
        {
            const int r = idx % SLAB, c = idx / SLAB;
            zs[r * LD + c] = (s0 + r < rows && c < K) ? b.zt[(size_t)c * b.m + row0 + s0 + r] : 0.0;
        }
        __syncthreads();
        if (tid < ntiles)
        {
            const double *za = zs + ti * TS, *zb = zs + tj * TS;
#pragma unroll 2
            for (int kk = 0; kk < SLAB; kk++)
            {
                double a[TS], c[TS];
#pragma unroll
                for (int i = 0; i < TS; i++) a[i] = za[kk * LD + i];
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
    if (tid < ntiles)
    {
        const int E = K * (K + 1) / 2;
        double *dst = b.part + (size_t)chunk * E;
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

// LDS carve (doubles): L[kLdTriMax], d[128], bv[128], x[128]
constexpr size_t kLdRegSolveLds = sizeof(double) * ((size_t)kLdTriMax + 3 * kLdVec);

__global__ void __launch_bounds__(256) ld_reg_solve_kernel(LdReg b, int nchunks)
{
    extern __shared__ double s_mem[];
    const int tid = threadIdx.x;
    const int k = b.k, K = k + 1, E = K * (K + 1) / 2, EL = k * (k + 1) / 2;
    double *L = s_mem;
    double *d = L + kLdTriMax;
    double *bv = d + kLdVec;
    double *x = bv + kLdVec;
    double *sol = b.sol;
    for (int e = tid; e < E - 1; e += 256)
    {  // in chunk order; the last entry, y'y, is not used
        double s = 0.0;
        for (int c = 0; c < nchunks; c++) s += b.part[(size_t)c * E + e];
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
            b.status[b.slot] = 2;
            sol[2 * kLdVec] = 0.0;
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
        if (!(piv >= kLdPivotMin))
        {  // the same for every thread
            if (tid == 0)
            {
                b.status[b.slot] = 2;
                sol[2 * kLdVec] = piv;
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
    // the inverse of L in place, last column first
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
        sol[kLdVec + tid] = v / (d[tid] * d[tid]);
    }
    if (tid == 0)
    {
        sol[2 * kLdVec] = minpiv;
        b.status[b.slot] = 0;
    }
}

__global__ void __launch_bounds__(256) ld_resid_kernel(LdReg b)
{
    __shared__ double th[kLdVec];
    __shared__ double sh[4];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    if (b.status[b.slot] != 0) return;  // the same for the whole workgroup; its partial is never read
    const int k = b.k;
    if (tid < k) th[tid] = b.sol[tid];
    __syncthreads();
    const int pos = chunk * kMvChunk + tid;
    double term = 0.0;
    if (pos < b.m)
    {
        double fit = 0.0;
        for (int j = 0; j < k; j++) fit = fma(b.zt[(size_t)j * b.m + pos], th[j], fit);
        const double r = b.zt[(size_t)k * b.m + pos] - fit;
        term = r * r;
    }
    // one order: butterflies inside each wavefront, then wavefront 0 .. 3
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
    if ((tid & 63) == 0) sh[tid >> 6] = term;
    __syncthreads();
    if (tid == 0) b.rpart[chunk] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ void __launch_bounds__(128) ld_finish_kernel(LdReg b, int nchunks)
{
    __shared__ double s_sigma;
    const int tid = threadIdx.x;
    const int st = b.status[b.slot];
    double *stats = b.stats + (size_t)b.slot * 3;
    if (st != 0)
    {
        if (tid < b.k)
        {
            b.theta[b.ex0 + tid] = NAN;
            b.se[b.ex0 + tid] = NAN;
        }
        if (tid == 0)
        {
            stats[0] = NAN;
            stats[1] = NAN;
            stats[2] = b.sol[2 * kLdVec];
        }
        return;
    }
    if (tid == 0)
    {
        double rss = 0.0;
        for (int c = 0; c < nchunks; c++) rss += b.rpart[c];
        const double sigma = sqrt(rss / (double)(b.m - b.k));
        s_sigma = sigma;
        stats[0] = rss;
        stats[1] = sigma;
        stats[2] = b.sol[2 * kLdVec];
    }
    __syncthreads();
    if (tid < b.k)
    {
        const bool random = b.model == 1 || (b.model == 0 && b.m >= 4);
        const double sigma = s_sigma, f = (random && sigma > 1.0) ? sigma : 1.0;
        b.theta[b.ex0 + tid] = b.sol[tid];
        b.se[b.ex0 + tid] = sqrt(b.sol[kLdVec + tid]) * f;
    }
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
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t na = plan.outcomes.size(), nex = (size_t)ex_off[nout];
    std::vector<double> th_h(nex, nan), se_h(nex, nan), stats_h(na * 3, nan), rpiv_h(na, nan);
    std::vector<int> st_h(na, 0), code_h(na, 0);
    if (na > 0)
    {
        CUSK_HIP(e, hipSetDevice(e->device));
        hipStream_t s = e->stream;
        ScopedDevBuf d_beta, d_weight, d_ld, d_iv, d_ex, d_ws, d_zt, d_dinv, d_state, d_part, d_rpart, d_sol, d_status, d_theta, d_se,
            d_stats;
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
        CUSK_HIP(e, up(d_ld, ld, sizeof(double) * (size_t)M * (size_t)M));
        CUSK_HIP(e, up(d_iv, iv, sizeof(int) * (size_t)iv_off[nout]));
        CUSK_HIP(e, up(d_ex, ex, sizeof(int) * nex));
        const size_t emax = (size_t)(kMvMaxExposures + 1) * (kMvMaxExposures + 2) / 2;
        CUSK_HIP(e, d_ws.ensure(sizeof(double) * plan.ws_doubles));
        CUSK_HIP(e, d_zt.ensure(sizeof(double) * plan.zt_doubles));
        CUSK_HIP(e, d_dinv.ensure(sizeof(double) * kLdPanel * kLdPanel));
        CUSK_HIP(e, d_state.ensure(sizeof(LdState)));
        CUSK_HIP(e, d_part.ensure(sizeof(double) * (size_t)plan.max_chunks * emax));
        CUSK_HIP(e, d_rpart.ensure(sizeof(double) * (size_t)plan.max_chunks));
        CUSK_HIP(e, d_sol.ensure(sizeof(double) * kLdSolLd));
        CUSK_HIP(e, d_status.ensure(sizeof(int) * na));
        CUSK_HIP(e, d_theta.ensure(sizeof(double) * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_se.ensure(sizeof(double) * std::max<size_t>(nex, 1)));
        CUSK_HIP(e, d_stats.ensure(sizeof(double) * na * 3));
        CUSK_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(ld_reg_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kLdRegSolveLds));
        for (hipEvent_t &v : evs.ev) CUSK_HIP(e, hipEventCreate(&v));
        CUSK_HIP(e, hipEventRecord(evs.ev[0], s));
        for (size_t slot = 0; slot < na; slot++)
        {
            const LdOutcome &o = plan.outcomes[slot];
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
            LdReg b;
            b.zt = q.zt;
            b.m = o.m;
            b.k = o.k;
            b.model = model;
            b.ex0 = o.ex0;
            b.slot = (int)slot;
            b.part = d_part.as<double>();
            b.rpart = d_rpart.as<double>();
            b.sol = d_sol.as<double>();
            b.status = d_status.as<int>();
            b.theta = d_theta.as<double>();
            b.se = d_se.as<double>();
            b.stats = d_stats.as<double>();
            hipLaunchKernelGGL((ld_gram_kernel<8, 128, 16>), dim3((unsigned)o.nchunks), dim3(256), 0, s, b);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(ld_reg_solve_kernel, dim3(1), dim3(256), kLdRegSolveLds, s, b, o.nchunks);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(ld_resid_kernel, dim3((unsigned)o.nchunks), dim3(256), 0, s, b);
            CUSK_HIP(e, hipGetLastError());
            hipLaunchKernelGGL(ld_finish_kernel, dim3(1), dim3(128), 0, s, b, o.nchunks);
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
        const LdOutcome &o = plan.outcomes[slot];
        if (code_h[slot] != 0)
        {  // 3 or 4: no estimates; stats[2] is the pivot of R that failed (4) or NaN (3)
            status[o.out] = code_h[slot];
            stats[(size_t)o.out * 3 + 2] = rpiv_h[slot];
            continue;
        }
        status[o.out] = st_h[slot];
        stats[(size_t)o.out * 3] = stats_h[slot * 3];
        stats[(size_t)o.out * 3 + 1] = stats_h[slot * 3 + 1];
        stats[(size_t)o.out * 3 + 2] = st_h[slot] == 0 ? rpiv_h[slot] : stats_h[slot * 3 + 2];
        if (st_h[slot] != 0) continue;
        for (int c = 0; c < o.k; c++)
        {
            theta[o.ex0 + c] = th_h[(size_t)o.ex0 + c];
            se[o.ex0 + c] = se_h[(size_t)o.ex0 + c];
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
