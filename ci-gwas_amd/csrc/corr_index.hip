// corr_index.hip -- correlation build over a marker index list, and the summary-statistic layouts of its result.
//
// `cuskss` on the union of the markers that all LD blocks selected (merged_blocks.ixs) wants the LD of those markers,
// which lie scattered over every chromosome of the .bed.  The build kernels of corr_mxm.hip / corr_mxp.hip read a CONTIGUOUS range
// of .bed rows, so the selected rows (and their means / standard deviations) are first packed into a contiguous HBM
// scratch by a row-gather kernel and the build kernels then run on that, unchanged: k * ceil(N/4) bytes of extra
// traffic beside a contraction of O(k^2 N).  The other two kernels of this file turn the square in-HBM matrix into what
// the summary-statistic route reads: the `mxm` file layout (lower triangle with diagonal, NaN -> 0;
// /root/reference/cusk/src/marker_summary_stats.cpp:8-24) and NaN -> 0 in place (what the mxp / pxp loaders do,
// marker_trait_summary_stats.cpp:40-299, trait_summary_stats.cpp:5-169).  All three are pure bandwidth: one aligned
// 16-byte store per lane, consecutive lanes on consecutive addresses.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cusk_internal.h"

namespace cusk {

// dst[r * clb + b] = bed[ix[r] * clb + b] for r < k, b < clb.  One thread per aligned 16-byte chunk of dst (dst is a
// fresh allocation: 16-byte aligned; `total` = k * clb bytes).  A chunk inside one row whose source bytes lie at least
// 4 bytes before the end of the .bed (`bed_bytes`) is fetched as aligned dwords and shifted into place -- rows of
// ceil(N/4) bytes start at any byte offset -- so that consecutive lanes read consecutive 16-byte spans; chunks that
// straddle two rows, the tail of dst and the last bytes of the .bed go byte by byte.
__global__ void __launch_bounds__(256) gather_bed_rows_kernel(const unsigned char *__restrict__ bed, const int *__restrict__ ix,
                                                              unsigned char *__restrict__ dst, size_t clb, size_t total,
                                                              size_t bed_bytes)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t d0 = c * 16;
    if (d0 >= total) return;
    const size_t r = d0 / clb, off = d0 - r * clb;
    if (off + 16 <= clb)
    {
        const size_t s0 = (size_t)ix[r] * clb + off;
        const unsigned sh = (unsigned)((reinterpret_cast<uintptr_t>(bed) + s0) & 3u);
        if (s0 >= sh && s0 - sh + 20 <= bed_bytes)
        {
            const unsigned *src = reinterpret_cast<const unsigned *>(bed + s0 - sh);  // dword aligned
            unsigned w[5];
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = src[j];
            w[4] = sh ? src[4] : 0u;
            uint4 o;
            o.x = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
            o.y = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
            o.z = __builtin_amdgcn_alignbyte(w[3], w[2], sh);
            o.w = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
            *reinterpret_cast<uint4 *>(dst + d0) = o;
            return;
        }
    }
    size_t row = r, b = off;
    for (size_t d = d0; d < d0 + 16 && d < total; d++)
    {
        dst[d] = bed[(size_t)ix[row] * clb + b];
        if (++b == clb)
        {
            b = 0;
            row++;
        }
    }
}

// mean / standard deviation of the selected markers
__global__ void gather_f32_kernel(const float *__restrict__ src, const int *__restrict__ ix, float *__restrict__ dst, size_t k)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) dst[i] = src[ix[i]];
}

// out[i (i + 1) / 2 + j] = C[i * n + j] for j <= i < k, NaN -> 0.  One thread per four consecutive elements of out (one
// aligned 16-byte store; 64-bit element offsets: k = 50,000 is 1.25e9 elements); the row of the first element comes from
// the inverse of the triangular numbers in double precision, corrected by integer comparison, and the four elements are
// walked from there, so a wave reads one contiguous kilobyte of a matrix row (two pieces where a row ends).
__global__ void __launch_bounds__(256) pack_lower_tri_kernel(const float *__restrict__ C, size_t n, size_t k, float *__restrict__ out,
                                                             size_t total)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= total) return;
    size_t i = (size_t)((sqrt(8.0 * (double)t0 + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= t0) i++;
    while (i * (i + 1) / 2 > t0) i--;
    size_t j = t0 - i * (i + 1) / 2;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int u = 0; u < 4; u++)
    {
        if (t0 + u < total)
        {
            const float x = C[i * n + j];
            v[u] = (x != x) ? 0.0f : x;
        }
        if (++j > i)
        {
            j = 0;
            i++;
        }
    }
    if (t0 + 4 <= total)
        *reinterpret_cast<float4 *>(out + t0) = make_float4(v[0], v[1], v[2], v[3]);
    else
        for (size_t u = 0; t0 + u < total; u++) out[t0 + u] = v[u];
}

// NaN -> 0 in place, four elements per thread (M is an allocation of its own: 16-byte aligned)
__global__ void __launch_bounds__(256) nan_to_zero_kernel(float *M, size_t count)
{
    const size_t t0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= count) return;
    if (t0 + 4 <= count)
    {
        float4 v = *reinterpret_cast<const float4 *>(M + t0);
        if (v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w)
        {
            v.x = (v.x != v.x) ? 0.0f : v.x;
            v.y = (v.y != v.y) ? 0.0f : v.y;
            v.z = (v.z != v.z) ? 0.0f : v.z;
            v.w = (v.w != v.w) ? 0.0f : v.w;
            *reinterpret_cast<float4 *>(M + t0) = v;
        }
    }
    else
        for (size_t t = t0; t < count; t++)
            if (M[t] != M[t]) M[t] = 0.0f;
}

// the index list of a build over scattered markers: ascending, distinct, inside the .bed
int check_marker_ix(cusk_engine *e, const int *marker_ix, size_t k, size_t m_total)
{
    if (m_total > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "marker indices are 32-bit: too many markers");
    for (size_t i = 0; i < k; i++)
        if (marker_ix[i] < 0 || (size_t)marker_ix[i] >= m_total || (i > 0 && marker_ix[i] <= marker_ix[i - 1]))
            return fail(e, CUSK_ERR_ARG, "marker indices must be ascending, distinct and below the number of markers (entry " +
                                             std::to_string(i) + ")");
    return CUSK_OK;
}

// The .bed rows marker_ix[0 .. k-1] made contiguous (bed_k): device-resident rows are gathered into e->bed_dev by the kernel
// above (ix_d: the index list on the device; uploaded to scratch_a here when the caller has not done so), host rows are
// packed into bed_h for the caller to upload.
int pack_bed_rows(cusk_engine *e, const unsigned char *bed, const int *marker_ix, const int *&ix_d, size_t k, size_t m_total,
                  size_t clb, std::vector<unsigned char> &bed_h, const unsigned char *&bed_k)
{
    hipStream_t s = e->stream;
    if (is_device_pointer(bed))
    {
        if (!ix_d)
        {
            CUSK_HIP(e, e->scratch_a.ensure(sizeof(int) * k));
            CUSK_HIP(e, hipMemcpyAsync(e->scratch_a.p, marker_ix, sizeof(int) * k, hipMemcpyHostToDevice, s));
            ix_d = e->scratch_a.as<int>();
        }
        const size_t total = k * clb;
        CUSK_HIP(e, e->bed_dev.ensure(total));
        hipLaunchKernelGGL(gather_bed_rows_kernel, dim3((unsigned)(((total + 15) / 16 + 255) / 256)), dim3(256), 0, s, bed, ix_d,
                           e->bed_dev.as<unsigned char>(), clb, total, m_total * clb);
        CUSK_HIP(e, hipGetLastError());
        bed_k = e->bed_dev.as<unsigned char>();
    }
    else
    {
        bed_h.resize(k * clb);
        for (size_t i = 0; i < k; i++) std::memcpy(&bed_h[i * clb], bed + (size_t)marker_ix[i] * clb, clb);
        bed_k = bed_h.data();
    }
    return CUSK_OK;
}

static int corr_build_indexed_impl(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                                   size_t m_total, size_t N, size_t p, const float *mean, const float *std, float *C_dev,
                                   float *mxp_host)
{
    if (!e || !bed || !phen || !marker_ix || !mean || !std || k == 0 || N == 0 || m_total == 0)
        return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (const int rc = check_marker_ix(e, marker_ix, k, m_total)) return rc;
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t clb = (N + 3) / 4;
    const bool bed_on_dev = is_device_pointer(bed), mean_on_dev = is_device_pointer(mean), std_on_dev = is_device_pointer(std);
    const auto t0 = std::chrono::steady_clock::now();
    // Device-resident inputs are gathered by the kernels above into the scratch corr_build_impl itself would copy host
    // inputs to; of host inputs only the selected rows are packed (and then uploaded by corr_build_impl).
    const int *ix_d = nullptr;
    if (bed_on_dev || mean_on_dev || std_on_dev)
    {
        CUSK_HIP(e, e->scratch_a.ensure(sizeof(int) * k));
        CUSK_HIP(e, hipMemcpyAsync(e->scratch_a.p, marker_ix, sizeof(int) * k, hipMemcpyHostToDevice, s));
        ix_d = e->scratch_a.as<int>();
    }
    std::vector<unsigned char> bed_h;
    std::vector<float> mean_h, std_h;
    const unsigned char *bed_k = nullptr;
    const float *mean_k = nullptr, *std_k = nullptr;
    if (const int rc = pack_bed_rows(e, bed, marker_ix, ix_d, k, m_total, clb, bed_h, bed_k)) return rc;
    auto gather_stat = [&](const float *src, bool on_dev, DevBuf &buf, std::vector<float> &host, const float *&out) -> hipError_t {
        if (on_dev)
        {
            const hipError_t st = buf.ensure(sizeof(float) * k);
            if (st != hipSuccess) return st;
            hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, src, ix_d, buf.as<float>(), k);
            out = buf.as<float>();
        }
        else
        {
            host.resize(k);
            for (size_t i = 0; i < k; i++) host[i] = src[marker_ix[i]];
            out = host.data();
        }
        return hipSuccess;
    };
    CUSK_HIP(e, gather_stat(mean, mean_on_dev, e->mean_dev, mean_h, mean_k));
    CUSK_HIP(e, gather_stat(std, std_on_dev, e->std_dev, std_h, std_k));
    CUSK_HIP(e, hipGetLastError());
    if (e->opt_hostprof)
    {
        CUSK_HIP(e, hipStreamSynchronize(s));
        std::fprintf(stderr, "[hostprof] corr_build_indexed: gather of %zu rows x %zu bytes (%s): %.3f ms\n", k, clb,
                     bed_on_dev ? "device" : "host",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    return corr_build_impl(e, bed_k, phen, k, N, p, mean_k, std_k, C_dev, mxp_host, nullptr, nullptr);
}

}  // namespace cusk

using namespace cusk;

extern "C" int cusk_corr_build_indexed(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                                       size_t m_total, size_t N, size_t p, const float *mean, const float *std, float *C_dev,
                                       float *mxp_host)
{
    return corr_build_indexed_impl(e, bed, phen, marker_ix, k, m_total, N, p, mean, std, C_dev, mxp_host);
}

extern "C" int cusk_pack_lower_tri(cusk_engine *e, const float *C_dev, size_t n, size_t k, float *out, int out_on_device)
{
    if (!e || !C_dev || !out || k == 0 || k > n) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t total = k * (k + 1) / 2;
    float *dst = out;
    if (!out_on_device)
    {
        CUSK_HIP(e, e->scratch_b.ensure(sizeof(float) * total));
        dst = e->scratch_b.as<float>();
    }
    else if (reinterpret_cast<uintptr_t>(out) & 15u)
        return fail(e, CUSK_ERR_ARG, "cusk_pack_lower_tri: the device output must be 16-byte aligned");
    const size_t groups = ((total + 3) / 4 + 255) / 256;
    if (groups > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_pack_lower_tri: k too large for one launch");
    hipLaunchKernelGGL(pack_lower_tri_kernel, dim3((unsigned)groups), dim3(256), 0, e->stream, C_dev, n, k, dst, total);
    CUSK_HIP(e, hipGetLastError());
    if (!out_on_device) CUSK_HIP(e, hipMemcpyAsync(out, dst, sizeof(float) * total, hipMemcpyDeviceToHost, e->stream));
    CUSK_HIP(e, hipStreamSynchronize(e->stream));
    return CUSK_OK;
}

extern "C" int cusk_nan_to_zero(cusk_engine *e, float *M_dev, size_t count)
{
    if (!e || !M_dev || (reinterpret_cast<uintptr_t>(M_dev) & 15u)) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (count == 0) return CUSK_OK;
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t groups = ((count + 3) / 4 + 255) / 256;
    if (groups > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_nan_to_zero: too many elements for one launch");
    hipLaunchKernelGGL(nan_to_zero_kernel, dim3((unsigned)groups), dim3(256), 0, e->stream, M_dev, count);
    CUSK_HIP(e, hipGetLastError());
    return CUSK_OK;
}
