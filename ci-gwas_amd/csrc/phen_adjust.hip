// phen_adjust.hip -- traits residualised on covariates and standardised (cusk_phen_adjust, cusk_phen_moments of
// include/cusk_hip.h, where the rule is stated; `mps prep-phen` / `mps check-phen`).
//
// Everything is IEEE double until the one float store per individual, and every sum over individuals has one order: a
// workgroup owns a chunk of CUSK_PHEN_CHUNK individuals and adds it in an order fixed by thread index, the chunk partials
// are stored with plain vector stores and a second small kernel adds them in chunk order.  No floating-point atomics.
//
//   covar_valid_kernel       one ballot per 64 individuals: the bit of individual i says "every covariate finite" (A)
//   covar_sum_kernel         grid (chunk, covariate): sum and count over A, then the centred sum of squares
//   covar_finish_kernel      mu_j, sigma_j
//   masked_gram_kernel       grid (chunk, adjusted trait): the lower triangle of Z'Z for Z = (1, xs_1 .. xs_c, y), which
//                            holds G, b and y'y.  A slab of 64 individuals of Z stands in LDS as doubles (zero columns for
//                            an individual outside U_t, so the trait's validity is the weight); every thread owns up to
//                            nine fixed entries in double registers and walks the slab with plain FMAs.
//   gram_reduce_kernel       the ordered sum of the chunk partials
//   chol_solve_kernel        one wavefront per adjusted trait: the Gram scaled to unit diagonal in LDS (64 x 65 doubles),
//                            right-looking Cholesky with the pivot test, both substitutions, beta in scaled and raw units
//   residual_moments_kernel  grid (chunk, trait), two passes: sum(e), sum(y), n; then sum((e - m)^2), sum((y - ybar)^2);
//                            e is recomputed from x and beta every time, there is no N x p array of residuals
//   moments_finish_kernel    m, s, r2, the status
//   standardise_kernel       out = (float)((e - m) / s), NaN outside U_t
// Individuals are 0 .. N-1: no load or store touches anything behind row ends.
#include <cmath>
#include <limits>
#include <vector>

#include "cusk_internal.h"

namespace cusk {

constexpr int kPhChunk = CUSK_PHEN_CHUNK;
constexpr int kPhSlab = 64;                         // individuals of Z in LDS at a time
constexpr int kPhCols = CUSK_PHEN_MAX_COVAR + 2;    // columns of Z: intercept, covariates, the trait
constexpr int kPhLd = kPhSlab + 1;                  // doubles per column in LDS: consecutive columns on consecutive banks
constexpr int kPhBetaLd = CUSK_PHEN_MAX_COVAR + 1;  // scaled coefficients per trait
static_assert(kPhChunk % 256 == 0 && kPhChunk % kPhSlab == 0, "a chunk is whole slabs and whole workgroup strides");

// per covariate: mu, sigma, |A|; per trait: n, m, ybar, centred sum of squares of e, of y, s, r2
constexpr int kCStat = 3, kTStat = 8;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum over the workgroup's 256 threads in one order: butterflies inside each wavefront, then wavefront 0 .. 3
template <int Q>
__device__ __forceinline__ void block_sum(double (&v)[Q], double *sh /* 4 * Q */)
{
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < Q; q++)
    {
        v[q] = wave_sum_d(v[q]);
        if (lane == 0) sh[w * Q + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) v[q] = ((sh[q] + sh[Q + q]) + sh[2 * Q + q]) + sh[3 * Q + q];
}

__device__ __forceinline__ bool valid_bit(const unsigned long long *valid, size_t i) { return (valid[i >> 6] >> (i & 63)) & 1ull; }

// valid[g]: bit l = every covariate of individual 64 g + l is finite; zero from individual N on.  One wavefront per word.
__global__ void __launch_bounds__(256) covar_valid_kernel(const float *__restrict__ X, size_t N, int c, size_t groups,
                                                          unsigned long long *__restrict__ valid)
{
    const size_t g = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (g >= groups) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const size_t i = g * 64 + lane;
    bool ok = i < N;
    if (ok)
        for (int j = 0; j < c; j++) ok = ok && finite_f(X[(size_t)j * N + i]);
    const unsigned long long b = __ballot(ok);
    if (lane == 0) valid[g] = b;
}

// PASS 0: part[(j * nchunks + chunk) * 2] = sum of x over A in the chunk, [.. + 1] = |A| in the chunk
// PASS 1: [..] = sum of (x - mu_j)^2
template <int PASS>
__global__ void __launch_bounds__(256) covar_sum_kernel(const float *__restrict__ X, size_t N, const unsigned long long *__restrict__ valid,
                                                        const double *__restrict__ cstat, size_t nchunks, double *__restrict__ part)
{
    __shared__ double sh[8];
    const size_t chunk = blockIdx.x, j = blockIdx.y, base = chunk * kPhChunk;
    const double mu = PASS ? cstat[j * kCStat] : 0.0;
    double v[2] = {0.0, 0.0};
    for (int u = 0; u < kPhChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        if (i < N && valid_bit(valid, i))
        {
            const double x = (double)X[j * N + i];
            if (PASS == 0)
            {
                v[0] += x;
                v[1] += 1.0;
            }
            else
            {
                const double d = x - mu;
                v[0] += d * d;
            }
        }
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0)
    {
        part[(j * nchunks + chunk) * 2] = v[0];
        if (PASS == 0) part[(j * nchunks + chunk) * 2 + 1] = v[1];
    }
}

template <int PASS>
__global__ void covar_finish_kernel(const double *__restrict__ part, size_t nchunks, int c, double *__restrict__ cstat)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c) return;
    double s = 0.0, n = 0.0;
    for (size_t k = 0; k < nchunks; k++)
    {
        s += part[((size_t)j * nchunks + k) * 2];
        if (PASS == 0) n += part[((size_t)j * nchunks + k) * 2 + 1];
    }
    if (PASS == 0)
    {
        cstat[j * kCStat] = s / n;
        cstat[j * kCStat + 2] = n;
    }
    else
        cstat[j * kCStat + 1] = sqrt(s / cstat[j * kCStat + 2]);
}

// part[(a * nchunks + chunk) * E + e], e = r (r + 1) / 2 + q for columns r >= q of Z = (1, xs, y): the sum of Z_r Z_q over the
// chunk's individuals of U_t, t = adj_ix[a].  Thread th owns the entries th + 256 u, u < NE.
template <int NE>
__global__ void __launch_bounds__(256) masked_gram_kernel(const float *__restrict__ Y, const float *__restrict__ X, size_t N, int c,
                                                          const unsigned long long *__restrict__ valid, const double *__restrict__ cstat,
                                                          const int *__restrict__ adj_ix, size_t nchunks, double *__restrict__ part)
{
    __shared__ double zs[kPhCols * kPhLd];
    const int K = c + 2, E = K * (K + 1) / 2;
    const size_t chunk = blockIdx.x, t = (size_t)adj_ix[blockIdx.y], base = chunk * kPhChunk;
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    int ro[NE], qo[NE];
    double acc[NE];
#pragma unroll
    for (int u = 0; u < NE; u++)
    {
        const int e = min((int)threadIdx.x + 256 * u, E - 1);  // past the last entry: computed again, never stored
        int r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
        while (r * (r + 1) / 2 > e) r--;
        while ((r + 1) * (r + 2) / 2 <= e) r++;
        ro[u] = r * kPhLd;
        qo[u] = (e - r * (r + 1) / 2) * kPhLd;
        acc[u] = 0.0;
    }
    for (int slab = 0; slab < kPhChunk / kPhSlab; slab++)
    {
        const size_t s0 = base + (size_t)slab * kPhSlab;
        if (s0 >= N) break;  // the same for the whole workgroup
        const size_t i = s0 + lane;
        float y = 0.0f;
        bool ok = i < N && valid_bit(valid, i);
        if (ok)
        {
            y = Y[t * N + i];
            ok = finite_f(y);
        }
        for (int col = (int)w; col < K; col += 4)
        {
            double z = 0.0;
            if (ok)
            {
                if (col == 0)
                    z = 1.0;
                else if (col == K - 1)
                    z = (double)y;
                else
                    z = ((double)X[(size_t)(col - 1) * N + i] - cstat[(col - 1) * kCStat]) / cstat[(col - 1) * kCStat + 1];
            }
            zs[col * kPhLd + lane] = z;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kPhSlab; k++)
        {
#pragma unroll
            for (int u = 0; u < NE; u++) acc[u] = fma(zs[ro[u] + k], zs[qo[u] + k], acc[u]);
        }
        __syncthreads();
    }
    double *dst = part + ((size_t)blockIdx.y * nchunks + chunk) * E;
#pragma unroll
    for (int u = 0; u < NE; u++)
    {
        const int e = (int)threadIdx.x + 256 * u;
        if (e < E) dst[e] = acc[u];
    }
}

// gram[a * E + e] = part[a][0][e] + part[a][1][e] + ... in chunk order
__global__ void __launch_bounds__(256) gram_reduce_kernel(const double *__restrict__ part, size_t nchunks, int E, double *__restrict__ gram)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const size_t a = blockIdx.y;
    double s = 0.0;
    for (size_t k = 0; k < nchunks; k++) s += part[(a * nchunks + k) * E + e];
    gram[a * E + e] = s;
}

// One wavefront per adjusted trait.  beta_s[t * kPhBetaLd + r]: the coefficients on (1, xs); beta_raw[t * (c + 1) + r]: on
// (1, x); status[t].
__global__ void __launch_bounds__(64) chol_solve_kernel(const double *__restrict__ gram, int c, const int *__restrict__ adj_ix,
                                                        const double *__restrict__ cstat, double *__restrict__ beta_s,
                                                        double *__restrict__ beta_raw, int *__restrict__ status)
{
    __shared__ double S[(CUSK_PHEN_MAX_COVAR + 1) * kPhLd];
    __shared__ double vec[CUSK_PHEN_MAX_COVAR + 1];
    const int k = c + 1, K = c + 2, E = K * (K + 1) / 2;
    const int a = blockIdx.x, t = adj_ix[a], r = threadIdx.x;
    const double *G = gram + (size_t)a * E;
    const double nt = G[0];  // the sum of 1 * 1: exact
    if (nt < (double)(c + 2))
    {
        if (r == 0) status[t] = CUSK_PHEN_TOO_FEW;
        return;
    }
    double d = 0.0;
    bool bad = false;
    if (r < k)
    {
        const double g = G[r * (r + 1) / 2 + r];
        bad = !(g > 0.0);
        d = 1.0 / sqrt(g);
    }
    vec[r] = d;
    __syncthreads();
    if (__ballot(bad))
    {
        if (r == 0) status[t] = CUSK_PHEN_SINGULAR;
        return;
    }
    if (r < k)
        for (int q = 0; q <= r; q++) S[r * kPhLd + q] = q == r ? 1.0 : G[r * (r + 1) / 2 + q] * d * vec[q];
    __syncthreads();
    for (int j = 0; j < k; j++)
    {
        const double piv = S[j * kPhLd + j];
        if (!(piv >= CUSK_PHEN_PIVOT_MIN))
        {
            if (r == 0) status[t] = CUSK_PHEN_SINGULAR;
            return;  // the same for every lane
        }
        const double l = sqrt(piv);
        __syncthreads();
        if (r == j) S[j * kPhLd + j] = l;
        if (r > j && r < k) S[r * kPhLd + j] /= l;
        __syncthreads();
        const double lrj = (r > j && r < k) ? S[r * kPhLd + j] : 0.0;
        for (int m = j + 1; m < k; m++)
            if (r >= m && r < k) S[r * kPhLd + m] -= lrj * S[m * kPhLd + j];
        __syncthreads();
    }
    // L w = D^-1/2 b
    double rhs = r < k ? G[k * (k + 1) / 2 + r] * d : 0.0;
    for (int j = 0; j < k; j++)
    {
        if (r == j) vec[j] = rhs / S[j * kPhLd + j];
        __syncthreads();
        if (r > j && r < k) rhs -= S[r * kPhLd + j] * vec[j];
        __syncthreads();
    }
    // L' v = w
    rhs = r < k ? vec[r] : 0.0;
    __syncthreads();
    for (int j = k - 1; j >= 0; j--)
    {
        if (r == j) vec[j] = rhs / S[j * kPhLd + j];
        __syncthreads();
        if (r < j) rhs -= S[j * kPhLd + r] * vec[j];
        __syncthreads();
    }
    const double bs = r < k ? vec[r] * d : 0.0;  // on the scaled design
    __syncthreads();
    if (r < k)
    {
        beta_s[(size_t)t * kPhBetaLd + r] = bs;
        vec[r] = r == 0 ? bs : bs / cstat[(r - 1) * kCStat + 1];
    }
    __syncthreads();
    if (r > 0 && r < k) beta_raw[(size_t)t * k + r] = vec[r];
    if (r == 0)
    {
        double b0 = vec[0];
        for (int j = 1; j < k; j++) b0 -= vec[j] * cstat[(j - 1) * kCStat];
        beta_raw[(size_t)t * k] = b0;
    }
}

// what a thread needs of trait t to recompute e: the scaled coefficients and the covariate scaling, in LDS
struct ResidualCtx
{
    double beta[kPhBetaLd], mu[CUSK_PHEN_MAX_COVAR], sigma[CUSK_PHEN_MAX_COVAR];
};

__device__ __forceinline__ void load_ctx(ResidualCtx &cx, bool fitted, int c, const double *beta_s, const double *cstat, size_t t)
{
    if (fitted)
        for (int j = threadIdx.x; j <= c; j += blockDim.x)
        {
            cx.beta[j] = beta_s[t * kPhBetaLd + j];
            if (j < c)
            {
                cx.mu[j] = cstat[j * kCStat];
                cx.sigma[j] = cstat[j * kCStat + 1];
            }
        }
    __syncthreads();
}

__device__ __forceinline__ double residual(const ResidualCtx &cx, bool fitted, int c, const float *__restrict__ X, size_t N, size_t i, double y)
{
    if (!fitted) return y;
    double dot = cx.beta[0];
    for (int j = 0; j < c; j++) dot = fma(cx.beta[j + 1], ((double)X[(size_t)j * N + i] - cx.mu[j]) / cx.sigma[j], dot);
    return y - dot;
}

// PASS 0: mpart[(t * nchunks + chunk) * 3 + ..] = sum(e), sum(y), n over the chunk's individuals of U_t (a trait whose fit
//         failed is counted with e = y: only its n is used)
// PASS 1: sum((e - m)^2), sum((y - ybar)^2); zeros for a trait whose fit failed
template <int PASS>
__global__ void __launch_bounds__(256) residual_moments_kernel(const float *__restrict__ Y, const float *__restrict__ X, size_t N, int c,
                                                               const unsigned long long *__restrict__ valid,
                                                               const double *__restrict__ cstat, const unsigned char *__restrict__ adjusted,
                                                               const double *__restrict__ beta_s, const int *__restrict__ status,
                                                               const double *__restrict__ tstat, size_t nchunks,
                                                               double *__restrict__ mpart)
{
    __shared__ ResidualCtx cx;
    __shared__ double sh[12];
    const size_t chunk = blockIdx.x, t = blockIdx.y, base = chunk * kPhChunk;
    const bool adj = adjusted[t] != 0, fitted = adj && status[t] == 0;
    double v[3] = {0.0, 0.0, 0.0};
    if (PASS == 0 || !adj || fitted)
    {
        load_ctx(cx, fitted, c, beta_s, cstat, t);
        const double m = PASS ? tstat[t * kTStat + 1] : 0.0, ybar = PASS ? tstat[t * kTStat + 2] : 0.0;
        for (int u = 0; u < kPhChunk / 256; u++)
        {
            const size_t i = base + (size_t)u * 256 + threadIdx.x;
            if (i >= N || (adj && !valid_bit(valid, i))) continue;
            const float yf = Y[t * N + i];
            if (!finite_f(yf)) continue;
            const double y = (double)yf, e = residual(cx, fitted, c, X, N, i, y);
            if (PASS == 0)
            {
                v[0] += e;
                v[1] += y;
                v[2] += 1.0;
            }
            else
            {
                const double de = e - m, dy = y - ybar;
                v[0] += de * de;
                v[1] += dy * dy;
            }
        }
    }
    block_sum<3>(v, sh);
    if (threadIdx.x < 3) mpart[(t * nchunks + chunk) * 3 + threadIdx.x] = v[threadIdx.x];
}

// tstat[t * kTStat + ..]: 0 n, 1 m, 2 ybar (PASS 0); 3 sum((e - m)^2), 4 sum((y - ybar)^2), 5 s, 6 r2 (PASS 1).  With
// `decide` the status of step 6 is completed: too few individuals (PASS 0), s == 0 (PASS 1).
template <int PASS>
__global__ void moments_finish_kernel(const double *__restrict__ mpart, size_t nchunks, int p, int c, const unsigned char *__restrict__ adjusted,
                                      int decide, double *__restrict__ tstat, int *__restrict__ status)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (size_t k = 0; k < nchunks; k++)
    {
        const double *q = mpart + ((size_t)t * nchunks + k) * 3;
        s0 += q[0];
        s1 += q[1];
        if (PASS == 0) s2 += q[2];
    }
    double *ts = tstat + (size_t)t * kTStat;
    if (PASS == 0)
    {
        ts[0] = s2;
        ts[1] = s0 / s2;
        ts[2] = s1 / s2;
        if (decide && status[t] == 0 && s2 < (adjusted[t] ? (double)(c + 2) : 2.0)) status[t] = CUSK_PHEN_TOO_FEW;
    }
    else
    {
        const double n = ts[0], m = ts[1];
        ts[3] = s0;
        ts[4] = s1;
        ts[5] = sqrt(s0 / n);
        ts[6] = 1.0 - (s0 + n * m * m) / s1;
        if (decide && status[t] == 0 && !(ts[5] > 0.0)) status[t] = CUSK_PHEN_TOO_FEW;
    }
}

__global__ void __launch_bounds__(256) standardise_kernel(const float *__restrict__ Y, const float *__restrict__ X, size_t N, int c,
                                                          const unsigned long long *__restrict__ valid, const double *__restrict__ cstat,
                                                          const unsigned char *__restrict__ adjusted, const double *__restrict__ beta_s,
                                                          const int *__restrict__ status, const double *__restrict__ tstat,
                                                          float *__restrict__ out)
{
    __shared__ ResidualCtx cx;
    const size_t chunk = blockIdx.x, t = blockIdx.y, base = chunk * kPhChunk;
    const bool adj = adjusted[t] != 0, good = status[t] == 0, fitted = adj && good;
    load_ctx(cx, fitted, c, beta_s, cstat, t);
    const double m = tstat[t * kTStat + 1], s = tstat[t * kTStat + 5];
    for (int u = 0; u < kPhChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        if (i >= N) break;
        float o = __builtin_nanf("");
        if (good && !(adj && !valid_bit(valid, i)))
        {
            const float yf = Y[t * N + i];
            if (finite_f(yf)) o = (float)((residual(cx, fitted, c, X, N, i, (double)yf) - m) / s);
        }
        out[t * N + i] = o;
    }
}

namespace {

template <int NE>
void launch_gram(dim3 grid, hipStream_t s, const float *Y, const float *X, size_t N, int c, const unsigned long long *valid,
                 const double *cstat, const int *adj_ix, size_t nchunks, double *part)
{
    hipLaunchKernelGGL(masked_gram_kernel<NE>, grid, dim3(256), 0, s, Y, X, N, c, valid, cstat, adj_ix, nchunks, part);
}

}  // namespace

// adjust == nullptr: the moments alone (cusk_phen_moments)
static int phen_adjust_impl(cusk_engine *e, const float *phen, const float *covar, size_t N, size_t p, size_t c_in,
                            const unsigned char *adjust, float *out_host, int *n_out, double *mean_out, double *sd_out,
                            double *beta_out, double *r2_out, int *status_out)
{
    const bool moments_only = adjust == nullptr;
    const char *name = moments_only ? "cusk_phen_moments" : "cusk_phen_adjust";
    if (!e) return CUSK_ERR_ARG;
    if (!phen || N == 0 || p == 0 || (!moments_only && !out_host)) return fail(e, CUSK_ERR_ARG, std::string(name) + ": bad arguments");
    if (c_in > CUSK_PHEN_MAX_COVAR)
        return fail(e, CUSK_ERR_ARG, std::string(name) + ": at most " + std::to_string(CUSK_PHEN_MAX_COVAR) + " covariates");
    if (c_in > 0 && !covar) return fail(e, CUSK_ERR_ARG, std::string(name) + ": covariates without their values");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, std::string(name) + ": counts are 32-bit: too many individuals");
    if (p > 65535) return fail(e, CUSK_ERR_ARG, std::string(name) + ": too many traits for one launch");
    const int c = (int)c_in, k = c + 1, K = c + 2, E = K * (K + 1) / 2;
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t groups = (N + 63) / 64, nchunks = (N + kPhChunk - 1) / kPhChunk;

    std::vector<unsigned char> adj_h(p, 0);
    std::vector<int> adj_ix;
    if (!moments_only && c > 0)
        for (size_t t = 0; t < p; t++)
            if (adjust[t])
            {
                adj_h[t] = 1;
                adj_ix.push_back((int)t);
            }
    const size_t na = adj_ix.size();

    ScopedEvents<6> pe;  // the marks of the five phases

    const float *Y = phen;
    if (!is_device_pointer(phen))
    {
        CUSK_HIP(e, e->phen_dev.ensure(sizeof(float) * p * N));
        CUSK_HIP(e, hipMemcpyAsync(e->phen_dev.p, phen, sizeof(float) * p * N, hipMemcpyHostToDevice, s));
        Y = e->phen_dev.as<float>();
    }
    ScopedDevBuf x_buf, out_buf, work;
    const float *X = covar;
    if (c > 0 && !is_device_pointer(covar))
    {
        CUSK_HIP(e, upload_async(x_buf, covar, sizeof(float) * c * N, s));
        X = x_buf.as<float>();
    }
    // one allocation, in doubles: covariate and trait statistics, scaled and raw coefficients, the Grams, the chunk
    // partials (the covariate sums, the Gram partials and the moment partials are never alive together), then the words
    // of A, the list of adjusted traits, the statuses and the flags
    const size_t part_d = std::max(std::max((size_t)c * nchunks * 2, na * nchunks * (size_t)E), p * nchunks * 3);
    const size_t d_cstat = 0, d_tstat = d_cstat + (size_t)std::max(c, 1) * kCStat, d_bs = d_tstat + p * kTStat,
                 d_braw = d_bs + p * kPhBetaLd, d_gram = d_braw + p * k, d_part = d_gram + std::max<size_t>(na, 1) * E,
                 d_valid = d_part + part_d, d_adjix = d_valid + groups, d_status = d_adjix + (p + 1) / 2,
                 d_flags = d_status + (p + 1) / 2, d_end = d_flags + (p + 7) / 8;
    CUSK_HIP(e, work.ensure(d_end * sizeof(double)));
    double *wd = work.as<double>();
    double *cstat = wd + d_cstat, *tstat = wd + d_tstat, *beta_s = wd + d_bs, *beta_raw = wd + d_braw, *gram = wd + d_gram,
           *part = wd + d_part;
    unsigned long long *valid = reinterpret_cast<unsigned long long *>(wd + d_valid);
    int *adj_ix_d = reinterpret_cast<int *>(wd + d_adjix), *status_d = reinterpret_cast<int *>(wd + d_status);
    unsigned char *flags_d = reinterpret_cast<unsigned char *>(wd + d_flags);
    CUSK_HIP(e, hipMemsetAsync(status_d, 0, sizeof(int) * p, s));
    CUSK_HIP(e, hipMemcpyAsync(flags_d, adj_h.data(), p, hipMemcpyHostToDevice, s));
    if (na) CUSK_HIP(e, hipMemcpyAsync(adj_ix_d, adj_ix.data(), sizeof(int) * na, hipMemcpyHostToDevice, s));
    if (!moments_only) CUSK_HIP(e, out_buf.ensure(sizeof(float) * p * N));

    CUSK_HIP(e, pe.record(0, s));
    if (c > 0)
    {
        hipLaunchKernelGGL(covar_valid_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, s, X, N, c, groups, valid);
        const dim3 cg((unsigned)nchunks, (unsigned)c);
        hipLaunchKernelGGL(covar_sum_kernel<0>, cg, dim3(256), 0, s, X, N, valid, cstat, nchunks, part);
        hipLaunchKernelGGL(covar_finish_kernel<0>, dim3(1), dim3(64), 0, s, part, nchunks, c, cstat);
        hipLaunchKernelGGL(covar_sum_kernel<1>, cg, dim3(256), 0, s, X, N, valid, cstat, nchunks, part);
        hipLaunchKernelGGL(covar_finish_kernel<1>, dim3(1), dim3(64), 0, s, part, nchunks, c, cstat);
        CUSK_HIP(e, hipGetLastError());
        std::vector<double> cs((size_t)c * kCStat);
        CUSK_HIP(e, hipMemcpyAsync(cs.data(), cstat, sizeof(double) * cs.size(), hipMemcpyDeviceToHost, s));
        CUSK_HIP(e, hipStreamSynchronize(s));
        for (int j = 0; j < c; j++)
            if (!(cs[j * kCStat + 1] > 0.0) || !std::isfinite(cs[j * kCStat + 1]))
                return fail(e, CUSK_ERR_ARG,
                            std::string(name) + ": covariate " + std::to_string(j) + " is constant on the " +
                                std::to_string((long long)cs[j * kCStat + 2]) + " individuals with every covariate observed");
    }
    CUSK_HIP(e, pe.record(1, s));
    if (na)
    {
        const dim3 gg((unsigned)nchunks, (unsigned)na);
        const int per_thread = (E + 255) / 256;
        if (per_thread <= 1)
            launch_gram<1>(gg, s, Y, X, N, c, valid, cstat, adj_ix_d, nchunks, part);
        else if (per_thread <= 2)
            launch_gram<2>(gg, s, Y, X, N, c, valid, cstat, adj_ix_d, nchunks, part);
        else if (per_thread <= 4)
            launch_gram<4>(gg, s, Y, X, N, c, valid, cstat, adj_ix_d, nchunks, part);
        else
            launch_gram<9>(gg, s, Y, X, N, c, valid, cstat, adj_ix_d, nchunks, part);
        CUSK_HIP(e, hipGetLastError());
    }
    CUSK_HIP(e, pe.record(2, s));
    if (na)
    {
        hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((E + 255) / 256), (unsigned)na), dim3(256), 0, s, part, nchunks, E, gram);
        hipLaunchKernelGGL(chol_solve_kernel, dim3((unsigned)na), dim3(64), 0, s, gram, c, adj_ix_d, cstat, beta_s, beta_raw, status_d);
        CUSK_HIP(e, hipGetLastError());
    }
    CUSK_HIP(e, pe.record(3, s));
    const dim3 mg((unsigned)nchunks, (unsigned)p), fg((unsigned)((p + 63) / 64));
    const int decide = moments_only ? 0 : 1;
    hipLaunchKernelGGL(residual_moments_kernel<0>, mg, dim3(256), 0, s, Y, X, N, c, valid, cstat, flags_d, beta_s, status_d, tstat, nchunks, part);
    hipLaunchKernelGGL(moments_finish_kernel<0>, fg, dim3(64), 0, s, part, nchunks, (int)p, c, flags_d, decide, tstat, status_d);
    hipLaunchKernelGGL(residual_moments_kernel<1>, mg, dim3(256), 0, s, Y, X, N, c, valid, cstat, flags_d, beta_s, status_d, tstat, nchunks, part);
    hipLaunchKernelGGL(moments_finish_kernel<1>, fg, dim3(64), 0, s, part, nchunks, (int)p, c, flags_d, decide, tstat, status_d);
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, pe.record(4, s));
    if (!moments_only)
    {
        hipLaunchKernelGGL(standardise_kernel, mg, dim3(256), 0, s, Y, X, N, c, valid, cstat, flags_d, beta_s, status_d, tstat, out_buf.as<float>());
        CUSK_HIP(e, hipGetLastError());
    }
    CUSK_HIP(e, pe.record(5, s));

    std::vector<double> ts(p * kTStat), braw(p * k);
    std::vector<int> st(p);
    CUSK_HIP(e, hipMemcpyAsync(ts.data(), tstat, sizeof(double) * ts.size(), hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(st.data(), status_d, sizeof(int) * p, hipMemcpyDeviceToHost, s));
    if (na) CUSK_HIP(e, hipMemcpyAsync(braw.data(), beta_raw, sizeof(double) * braw.size(), hipMemcpyDeviceToHost, s));
    if (!moments_only) CUSK_HIP(e, hipMemcpyAsync(out_host, out_buf.p, sizeof(float) * p * N, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    for (int q = 0; q < 5; q++) CUSK_HIP(e, pe.elapsed(&e->phen_ms[q], q, q + 1));

    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t t = 0; t < p; t++)
    {
        const bool good = st[t] == 0, fitted = good && adj_h[t];
        if (n_out) n_out[t] = (int)ts[t * kTStat];
        if (mean_out) mean_out[t] = good ? ts[t * kTStat + 1] : nan;
        if (sd_out) sd_out[t] = good ? ts[t * kTStat + 5] : nan;
        if (r2_out) r2_out[t] = fitted ? ts[t * kTStat + 6] : nan;
        if (status_out) status_out[t] = st[t];
        if (beta_out)
            for (int r = 0; r < k; r++) beta_out[t * k + r] = fitted ? braw[t * k + r] : nan;
    }
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_phen_adjust(cusk_engine *e, const float *phen, const float *covar, size_t N, size_t p, size_t c,
                                const unsigned char *adjust, float *out_host, int *n_out, double *mean_out, double *sd_out,
                                double *beta_out, double *r2_out, int *status_out)
{
    if (e && !adjust) return cusk::fail(e, CUSK_ERR_ARG, "cusk_phen_adjust: bad arguments");
    return cusk::phen_adjust_impl(e, phen, covar, N, p, c, adjust, out_host, n_out, mean_out, sd_out, beta_out, r2_out, status_out);
}

extern "C" int cusk_phen_moments(cusk_engine *e, const float *phen, size_t N, size_t p, int *n_out, double *mean_out, double *sd_out)
{
    return cusk::phen_adjust_impl(e, phen, nullptr, N, p, 0, nullptr, nullptr, n_out, mean_out, sd_out, nullptr, nullptr, nullptr);
}

extern "C" void cusk_phen_timing(cusk_engine *e, float *ms5)
{
    if (!e || !ms5) return;
    for (int q = 0; q < 5; q++) ms5[q] = e->phen_ms[q];
}
