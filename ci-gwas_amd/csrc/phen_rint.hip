// phen_rint.hip -- rank-based inverse normal transform of traits (cusk_phen_rint of include/cusk_hip.h, where the rule is
// stated; `mps prep-phen ... rint`).
//
// Ranks are integers from a keys-only sort: equal keys are indistinguishable, so the sort needs neither stability nor a
// payload, and an element finds its rank by two binary searches over the sorted keys of its trait.  The index arithmetic
// of the sort, the key map and the rank formula are in rint_math.h, shared with tools/rint_selftest.cpp.  The scores are
// IEEE double, recomputed from the stored integer rank wherever they are needed (one function of one integer: the same
// bits every time); their sums follow the chunk discipline of phen_adjust.hip: a workgroup adds a chunk of
// CUSK_PHEN_CHUNK individuals in an order fixed by thread index, a second small kernel adds the partials in chunk order.
// No floating-point atomics; the only atomic is the integer count of observed values.
//
//   rint_keys_kernel         grid (chunk, trait): the key of every individual into the trait's row of npad keys (padding and
//                            missing values: 0xFFFFFFFF), n from one ballot per wavefront and an integer add; for a trait
//                            that is not transformed the count alone
//   rint_tile_kernel         grid (tile, trait): kRtTile keys in LDS, the bitonic steps j < kRtTile of merge sizes
//                            k_lo .. k_hi: the whole sort of a tile (k = 2 .. kRtTile), or the tail of one larger merge
//   rint_global_step_kernel  grid (npad / 2048, trait): one compare-exchange step j >= kRtTile of merge size k on the rows
//                            in global memory, four pairs per thread as 16-byte loads and stores
//   rint_rank_kernel         grid (chunk, trait): lower and upper bound of the individual's key among the first n sorted
//                            keys of its trait, rank2 = lower + upper + 1 (0 for a missing value)
//   rint_moments_kernel      grid (chunk, trait), two passes: sum(q), then sum((q - m)^2)
//   rint_finish_kernel       m, s and the status
//   rint_standardise_kernel  out = (float)((q - m) / s), NaN for a missing value and for a trait with a status
// Individuals are 0 .. N-1 and keys 0 .. npad-1 of the trait's own row: no load or store touches anything else.
#include <cmath>
#include <limits>
#include <memory>
#include <vector>

#include "cusk_internal.h"
#include "ordinal_math.h"
#include "rint_math.h"

namespace cusk {

using namespace rintm;

constexpr int kRtChunk = CUSK_PHEN_CHUNK;
// 8192 keys = 32 KB of LDS per workgroup of 512 threads: four workgroups fill the 32 wavefront slots of a CU and take 128
// of its 160 KB.  A 64 KB tile would save one merge stage (one global pass per larger merge) and leave two workgroups =
// 16 wavefronts per CU to hide the barrier after every step.
constexpr unsigned kRtTile = 8192;
constexpr unsigned kRtThreads = 512;
constexpr unsigned kRtPairs = kRtTile / 2 / kRtThreads;  // compare-exchange pairs per thread and step
static_assert((kRtTile & (kRtTile - 1)) == 0 && kRtTile % kRtChunk == 0, "npad is whole tiles and whole chunks");
static_assert(kRtTile % (8 * 256) == 0, "a global step runs whole workgroups of four pairs per thread");

__device__ __forceinline__ double rt_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum over the workgroup's 256 threads in one order: butterflies inside each wavefront, then wavefront 0 .. 3
__device__ __forceinline__ double rt_block_sum(double v, double *sh /* 4 */)
{
    v = rt_wave_sum(v);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// q of step 4: the rank is rank2 / 2 exactly, denom = (n + 1) - 2 offset
__device__ __forceinline__ double rt_score(uint32_t rank2, double offset, double denom)
{
    return ord::ppnd16((0.5 * (double)rank2 - offset) / denom);
}

// Trait ix[blockIdx.y].  WRITE: grid.x = npad / kRtChunk, the keys of row blockIdx.y; otherwise grid.x = chunks of N.
template <bool WRITE>
__global__ void __launch_bounds__(256) rint_keys_kernel(const float *__restrict__ Y, size_t N, size_t npad, const int *__restrict__ ix,
                                                        uint32_t *__restrict__ keys, unsigned *__restrict__ n_d)
{
    const size_t t = (size_t)ix[blockIdx.y], base = (size_t)blockIdx.x * kRtChunk;
    unsigned cnt = 0;
    for (int u = 0; u < kRtChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        uint32_t key = kMissingKey;
        if (i < N) key = rint_key(__float_as_uint(Y[t * N + i]));
        cnt += (unsigned)__popcll(__ballot(key != kMissingKey));
        if (WRITE) keys[(size_t)blockIdx.y * npad + i] = key;  // i < npad: the grid covers npad exactly
    }
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&n_d[t], cnt);
}

__global__ void __launch_bounds__(kRtThreads) rint_tile_kernel(uint32_t *__restrict__ keys, size_t npad, size_t k_lo, size_t k_hi)
{
    __shared__ uint32_t s[kRtTile];
    const size_t base = (size_t)blockIdx.x * kRtTile;
    uint4 *row4 = reinterpret_cast<uint4 *>(keys + (size_t)blockIdx.y * npad + base);
    uint4 *s4 = reinterpret_cast<uint4 *>(s);
    for (unsigned v = threadIdx.x; v < kRtTile / 4; v += kRtThreads) s4[v] = row4[v];
    __syncthreads();
    for (size_t k = k_lo; k <= k_hi; k <<= 1)
        for (unsigned j = (unsigned)(k < kRtTile ? k : kRtTile) / 2; j > 0; j >>= 1)
        {
#pragma unroll
            for (unsigned u = 0; u < kRtPairs; u++)
            {
                const unsigned i = rint_pair_low(u * kRtThreads + threadIdx.x, j), q = rint_partner(i, j);
                const uint32_t a = s[i], b = s[q];
                if (rint_exchange(a, b, rint_ascending(base + i, k)))
                {
                    s[i] = b;
                    s[q] = a;
                }
            }
            __syncthreads();
        }
    for (unsigned v = threadIdx.x; v < kRtTile / 4; v += kRtThreads) row4[v] = s4[v];
}

__global__ void __launch_bounds__(256) rint_global_step_kernel(uint32_t *__restrict__ keys, size_t npad, size_t k, size_t j)
{
    uint32_t *row = keys + (size_t)blockIdx.y * npad;
    // four consecutive pairs: j >= kRtTile is a multiple of four, so they are contiguous and share their direction
    const size_t t = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t i = rint_pair_low(t, j), q = rint_partner(i, j);
    const bool asc = rint_ascending(i, k);
    uint4 a = *reinterpret_cast<const uint4 *>(row + i), b = *reinterpret_cast<const uint4 *>(row + q);
    uint32_t *av = reinterpret_cast<uint32_t *>(&a), *bv = reinterpret_cast<uint32_t *>(&b);
    bool any = false;
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (rint_exchange(av[c], bv[c], asc))
        {
            const uint32_t x = av[c];
            av[c] = bv[c];
            bv[c] = x;
            any = true;
        }
    if (any)
    {
        *reinterpret_cast<uint4 *>(row + i) = a;
        *reinterpret_cast<uint4 *>(row + q) = b;
    }
}

__global__ void __launch_bounds__(256) rint_rank_kernel(const float *__restrict__ Y, size_t N, size_t npad, const int *__restrict__ ix,
                                                        const uint32_t *__restrict__ keys, const unsigned *__restrict__ n_d,
                                                        uint32_t *__restrict__ rank2)
{
    const size_t t = (size_t)ix[blockIdx.y], base = (size_t)blockIdx.x * kRtChunk;
    const uint32_t *row = keys + (size_t)blockIdx.y * npad;
    const uint32_t n = n_d[t];
    for (int u = 0; u < kRtChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        if (i >= N) break;
        const uint32_t key = rint_key(__float_as_uint(Y[t * N + i]));
        uint32_t r = 0;
        if (key != kMissingKey)
        {
            const uint32_t lo = rint_lower(row, n, key);
            r = rint_rank2(lo, lo + rint_upper(row + lo, n - lo, key));
        }
        rank2[(size_t)blockIdx.y * N + i] = r;
    }
}

// tstat[t * 2]: m, [t * 2 + 1]: s.  PASS 0: part[slot * nchunks + chunk] = sum of q over the chunk; PASS 1: of (q - m)^2
template <int PASS>
__global__ void __launch_bounds__(256) rint_moments_kernel(const uint32_t *__restrict__ rank2, size_t N, const int *__restrict__ ix,
                                                           const unsigned *__restrict__ n_d, double offset,
                                                           const double *__restrict__ tstat, size_t nchunks, double *__restrict__ part)
{
    __shared__ double sh[4];
    const size_t t = (size_t)ix[blockIdx.y], base = (size_t)blockIdx.x * kRtChunk;
    const double denom = ((double)n_d[t] + 1.0) - 2.0 * offset, m = PASS ? tstat[t * 2] : 0.0;
    double v = 0.0;
    for (int u = 0; u < kRtChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        const uint32_t r = i < N ? rank2[(size_t)blockIdx.y * N + i] : 0u;
        if (r)
        {
            const double q = rt_score(r, offset, denom);
            if (PASS == 0)
                v += q;
            else
                v += (q - m) * (q - m);
        }
    }
    v = rt_block_sum(v, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * nchunks + blockIdx.x] = v;
}

template <int PASS>
__global__ void rint_finish_kernel(const double *__restrict__ part, size_t nchunks, int g, const int *__restrict__ ix,
                                   const unsigned *__restrict__ n_d, double *__restrict__ tstat, int *__restrict__ status)
{
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= g) return;
    const size_t t = (size_t)ix[slot];
    double s = 0.0;
    for (size_t k = 0; k < nchunks; k++) s += part[(size_t)slot * nchunks + k];
    const double n = (double)n_d[t];
    if (PASS == 0)
    {
        tstat[t * 2] = s / n;
        if (n < 2.0) status[t] = CUSK_PHEN_TOO_FEW;
    }
    else
    {
        const double sd = sqrt(s / n);
        tstat[t * 2 + 1] = sd;
        if (status[t] == 0 && !(sd > 0.0)) status[t] = CUSK_PHEN_TOO_FEW;
    }
}

__global__ void __launch_bounds__(256) rint_standardise_kernel(const uint32_t *__restrict__ rank2, size_t N, const int *__restrict__ ix,
                                                               const unsigned *__restrict__ n_d, double offset,
                                                               const double *__restrict__ tstat, const int *__restrict__ status,
                                                               float *__restrict__ out)
{
    const size_t t = (size_t)ix[blockIdx.y], base = (size_t)blockIdx.x * kRtChunk;
    const double denom = ((double)n_d[t] + 1.0) - 2.0 * offset, m = tstat[t * 2], s = tstat[t * 2 + 1];
    const bool good = status[t] == 0;
    for (int u = 0; u < kRtChunk / 256; u++)
    {
        const size_t i = base + (size_t)u * 256 + threadIdx.x;
        if (i >= N) break;
        const uint32_t r = rank2[(size_t)blockIdx.y * N + i];
        out[t * N + i] = good && r ? (float)((rt_score(r, offset, denom) - m) / s) : __builtin_nanf("");
    }
}

static int phen_rint_impl(cusk_engine *e, const float *vals, size_t N, size_t p, const unsigned char *select, double offset,
                          float *out_host, int *n_out, double *mean_out, double *sd_out, int *status_out, unsigned *rank2_out)
{
    if (!e) return CUSK_ERR_ARG;
    if (!vals || !out_host || N == 0 || p == 0) return fail(e, CUSK_ERR_ARG, "cusk_phen_rint: bad arguments");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_phen_rint: counts are 32-bit: too many individuals");
    if (p > 65535) return fail(e, CUSK_ERR_ARG, "cusk_phen_rint: too many traits for one launch");
    if (!(offset >= 0.0 && offset <= 0.5)) return fail(e, CUSK_ERR_ARG, "cusk_phen_rint: the offset is not in [0, 0.5]");
    std::vector<int> ix;  // the transformed traits, then the others
    for (size_t t = 0; t < p; t++)
        if (!select || select[t]) ix.push_back((int)t);
    const size_t nsel = ix.size();
    for (size_t t = 0; t < p; t++)
        if (select && !select[t]) ix.push_back((int)t);
    const size_t npad = rint_npad(N, kRtTile), trait_bytes = rint_trait_bytes(N, kRtTile), nchunks = (N + kRtChunk - 1) / kRtChunk;
    if (nsel && trait_bytes > (size_t)e->opt_phen_rint_bytes)
        return fail(e, CUSK_ERR_ARG,
                    "cusk_phen_rint: one trait of " + std::to_string(N) + " individuals needs " + std::to_string(trait_bytes) +
                        " bytes, more than phen_rint_bytes = " + std::to_string(e->opt_phen_rint_bytes));
    const size_t gmax = nsel ? std::min<size_t>((size_t)e->opt_phen_rint_bytes / trait_bytes, nsel) : 0;
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;

    const float *Y = vals;
    if (!is_device_pointer(vals))
    {
        CUSK_HIP(e, e->phen_dev.ensure(sizeof(float) * p * N));
        CUSK_HIP(e, hipMemcpyAsync(e->phen_dev.p, vals, sizeof(float) * p * N, hipMemcpyHostToDevice, s));
        Y = e->phen_dev.as<float>();
    }
    ScopedDevBuf out_buf;
    CUSK_HIP(e, out_buf.ensure(sizeof(float) * p * N));
    float *out_d = out_buf.as<float>();
    // scratch_a: the rows of keys of a group, then its rows of rank2.  scratch_b, in doubles: m and s per trait, the chunk
    // partials of a group, then n, the status and the trait lists.
    if (gmax) CUSK_HIP(e, e->scratch_a.ensure(gmax * trait_bytes));
    uint32_t *keys = e->scratch_a.as<uint32_t>(), *rank2 = keys + gmax * npad;
    const size_t d_tstat = 0, d_part = d_tstat + 2 * p, d_n = d_part + gmax * nchunks, d_status = d_n + (p + 1) / 2,
                 d_ix = d_status + (p + 1) / 2, d_end = d_ix + (p + 1) / 2;
    CUSK_HIP(e, e->scratch_b.ensure(d_end * sizeof(double)));
    double *wd = e->scratch_b.as<double>(), *tstat = wd + d_tstat, *part = wd + d_part;
    unsigned *n_d = reinterpret_cast<unsigned *>(wd + d_n);
    int *status_d = reinterpret_cast<int *>(wd + d_status), *ix_d = reinterpret_cast<int *>(wd + d_ix);
    CUSK_HIP(e, hipMemsetAsync(wd + d_n, 0, (d_ix - d_n) * sizeof(double), s));
    CUSK_HIP(e, hipMemcpyAsync(ix_d, ix.data(), sizeof(int) * p, hipMemcpyHostToDevice, s));
    if (rank2_out)
        for (size_t u = nsel; u < p; u++) std::fill_n(rank2_out + (size_t)ix[u] * N, N, 0u);

    // the traits that are not transformed: their count, and their values as they are
    if (nsel < p)
    {
        hipLaunchKernelGGL(rint_keys_kernel<false>, dim3((unsigned)nchunks, (unsigned)(p - nsel)), dim3(256), 0, s, Y, N, npad, ix_d + nsel,
                           (uint32_t *)nullptr, n_d);
        CUSK_HIP(e, hipGetLastError());
        for (size_t u = nsel; u < p; u++)
            CUSK_HIP(e, hipMemcpyAsync(out_d + (size_t)ix[u] * N, Y + (size_t)ix[u] * N, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    }

    std::vector<std::unique_ptr<ScopedEvents<5>>> marks;  // per group: the marks of the four phases
    for (size_t g0 = 0; g0 < nsel; g0 += gmax)
    {
        const unsigned g = (unsigned)std::min(gmax, nsel - g0);
        const int *gix = ix_d + g0;
        marks.emplace_back(new ScopedEvents<5>());
        ScopedEvents<5> &pe = *marks.back();
        const dim3 cg((unsigned)nchunks, g), fg((g + 63) / 64);
        CUSK_HIP(e, pe.record(0, s));
        hipLaunchKernelGGL(rint_keys_kernel<true>, dim3((unsigned)(npad / kRtChunk), g), dim3(256), 0, s, Y, N, npad, gix, keys, n_d);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, pe.record(1, s));
        const dim3 tg((unsigned)(npad / kRtTile), g), gg((unsigned)(npad / 2048), g);
        hipLaunchKernelGGL(rint_tile_kernel, tg, dim3(kRtThreads), 0, s, keys, npad, (size_t)2, (size_t)kRtTile);
        for (size_t k = 2 * (size_t)kRtTile; k <= npad; k <<= 1)
        {
            for (size_t j = k / 2; j >= kRtTile; j >>= 1) hipLaunchKernelGGL(rint_global_step_kernel, gg, dim3(256), 0, s, keys, npad, k, j);
            hipLaunchKernelGGL(rint_tile_kernel, tg, dim3(kRtThreads), 0, s, keys, npad, k, k);
        }
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, pe.record(2, s));
        hipLaunchKernelGGL(rint_rank_kernel, cg, dim3(256), 0, s, Y, N, npad, gix, keys, n_d, rank2);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, pe.record(3, s));
        hipLaunchKernelGGL(rint_moments_kernel<0>, cg, dim3(256), 0, s, rank2, N, gix, n_d, offset, tstat, nchunks, part);
        hipLaunchKernelGGL(rint_finish_kernel<0>, fg, dim3(64), 0, s, part, nchunks, (int)g, gix, n_d, tstat, status_d);
        hipLaunchKernelGGL(rint_moments_kernel<1>, cg, dim3(256), 0, s, rank2, N, gix, n_d, offset, tstat, nchunks, part);
        hipLaunchKernelGGL(rint_finish_kernel<1>, fg, dim3(64), 0, s, part, nchunks, (int)g, gix, n_d, tstat, status_d);
        hipLaunchKernelGGL(rint_standardise_kernel, cg, dim3(256), 0, s, rank2, N, gix, n_d, offset, tstat, status_d, out_d);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, pe.record(4, s));
        if (rank2_out)
            for (unsigned u = 0; u < g; u++)
                CUSK_HIP(e, hipMemcpyAsync(rank2_out + (size_t)ix[g0 + u] * N, rank2 + (size_t)u * N, sizeof(unsigned) * N, hipMemcpyDeviceToHost, s));
    }

    std::vector<double> ts(2 * p);
    std::vector<unsigned> nh(p);
    std::vector<int> st(p);
    CUSK_HIP(e, hipMemcpyAsync(ts.data(), tstat, sizeof(double) * ts.size(), hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(nh.data(), n_d, sizeof(unsigned) * p, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(st.data(), status_d, sizeof(int) * p, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(out_host, out_d, sizeof(float) * p * N, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    for (int q = 0; q < 4; q++) e->rint_ms[q] = 0.0f;
    for (const auto &pe : marks)
        for (int q = 0; q < 4; q++)
        {
            float ms = 0.0f;
            CUSK_HIP(e, pe->elapsed(&ms, q, q + 1));
            e->rint_ms[q] += ms;
        }

    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t u = 0; u < p; u++)
    {
        const size_t t = (size_t)ix[u];
        const bool good = u < nsel && st[t] == 0;
        if (n_out) n_out[t] = (int)nh[t];
        if (mean_out) mean_out[t] = good ? ts[t * 2] : nan;
        if (sd_out) sd_out[t] = good ? ts[t * 2 + 1] : nan;
        if (status_out) status_out[t] = st[t];
    }
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_phen_rint(cusk_engine *e, const float *vals, size_t N, size_t p, const unsigned char *select, double offset,
                              float *out_host, int *n_out, double *mean_out, double *sd_out, int *status_out, unsigned *rank2_out)
{
    return cusk::phen_rint_impl(e, vals, N, p, select, offset, out_host, n_out, mean_out, sd_out, status_out, rank2_out);
}

extern "C" void cusk_phen_rint_timing(cusk_engine *e, float *ms4)
{
    if (!e || !ms4) return;
    for (int q = 0; q < 4; q++) ms4[q] = e->rint_ms[q];
}

extern "C" size_t cusk_phen_rint_tile(void) { return cusk::kRtTile; }
