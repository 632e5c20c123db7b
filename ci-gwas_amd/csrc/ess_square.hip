// ess_square.hip -- the sample-size matrix of one block, expanded on the device (cusk_ess_square of include/cusk_hip.h).
//
// A skeleton run at per-pair sample sizes (cusk_run_skeleton_het, cusk_run_hetcor) reads an n x n float32 matrix,
// n = m markers + p traits.  Only m p + p^2 of its values carry information -- a marker and a trait, two traits; the rest
// is one number, N between markers (make_square_cuskss_inputs, cli.cpp:89-173).  The host computes those values (the
// cusk_se_from_count -> cusk_ess_from_se chain, so that a pair gets the same size wherever it is looked at) and this
// kernel writes the 4 n^2 bytes: 400 MB at a 10k block, at the rate of HBM instead of a host fill and a PCIe copy.
//
//   out[i][j] = n_uniform          i, j < m
//               mxp[i * p + t]     i < m, j = m + t   and mirrored at (m + t, i)
//               pxp[a * p + b]     i = m + a, j = m + b, a != b
//               NaN                i = j >= m
//
// The matrix is a linear run of n^2 floats that may start at any element: the kernel cuts it into the 16-byte aligned
// chunks in between (one 16-byte store per lane) and at most three single elements at either end (one lane).  An
// element's row and column come from its linear index by a 64-bit division -- n^2 exceeds 2^31 from n = 46,341 on.
#include <algorithm>

#include "cusk_internal.h"

namespace cusk {

__device__ __forceinline__ float ess_square_value(const float *__restrict__ mxp, const float *__restrict__ pxp, size_t m,
                                                  size_t p, float n_uniform, size_t i, size_t j)
{
    if (i < m) return (j < m) ? n_uniform : mxp[i * p + (j - m)];
    if (j < m) return mxp[j * p + (i - m)];
    return (i == j) ? __uint_as_float(0x7fc00000u) : pxp[(i - m) * p + (j - m)];
}

// lane q < nvec: elements head + 4 q .. + 3 (out + head is 16-byte aligned); lane nvec: the `head` elements in front of
// the first chunk and the total - head - 4 nvec behind the last
__global__ void __launch_bounds__(256) ess_square_kernel(const float *__restrict__ mxp, const float *__restrict__ pxp, size_t m,
                                                         size_t p, float n_uniform, float *__restrict__ out, size_t head,
                                                         size_t nvec, size_t total)
{
    const size_t n = m + p;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < nvec)
    {
        const size_t e0 = head + 4 * q;
        size_t i = e0 / n, j = e0 - i * n;
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            v[u] = ess_square_value(mxp, pxp, m, p, n_uniform, i, j);
            if (++j == n)
            {
                j = 0;
                i++;
            }
        }
        *reinterpret_cast<float4 *>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    }
    else if (q == nvec)
    {
        for (size_t e = 0; e < head; e++) out[e] = ess_square_value(mxp, pxp, m, p, n_uniform, e / n, e % n);
        for (size_t e = head + 4 * nvec; e < total; e++) out[e] = ess_square_value(mxp, pxp, m, p, n_uniform, e / n, e % n);
    }
}

static int ess_square_impl(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, size_t m, size_t p, float n_uniform,
                           float *N_dev)
{
    const size_t n = m + p;
    if (!e || !N_dev || n == 0 || (p > 0 && !pxp_ess) || (m > 0 && p > 0 && !mxp_ess)) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (n > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ess_square: too many variables");
    if (reinterpret_cast<uintptr_t>(N_dev) & 3u) return fail(e, CUSK_ERR_ARG, "cusk_ess_square: the matrix must be 4-byte aligned");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // the m p + p^2 values: host arrays are uploaded to engine scratch, device-resident ones are read in place
    const float *mxp_d = mxp_ess, *pxp_d = pxp_ess;
    const size_t cm = m * p, cp = p * p;
    const bool up_m = cm > 0 && !is_device_pointer(mxp_ess), up_p = cp > 0 && !is_device_pointer(pxp_ess);
    if (up_m || up_p)
    {
        CUSK_HIP(e, e->scratch_a.ensure(sizeof(float) * (cm + cp)));
        float *d = e->scratch_a.as<float>();
        if (up_m)
        {
            CUSK_HIP(e, hipMemcpyAsync(d, mxp_ess, sizeof(float) * cm, hipMemcpyHostToDevice, s));
            mxp_d = d;
        }
        if (up_p)
        {
            CUSK_HIP(e, hipMemcpyAsync(d + cm, pxp_ess, sizeof(float) * cp, hipMemcpyHostToDevice, s));
            pxp_d = d + cm;
        }
    }
    const size_t total = n * n;
    const size_t head = std::min<size_t>(total, ((16u - (unsigned)(reinterpret_cast<uintptr_t>(N_dev) & 15u)) & 15u) / 4u);
    const size_t nvec = (total - head) / 4;
    const size_t blocks = (nvec + 1 + 255) / 256;  // one lane more than chunks: the ends
    if (blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ess_square: too many variables for one launch");
    hipLaunchKernelGGL(ess_square_kernel, dim3((unsigned)blocks), dim3(256), 0, s, mxp_d, pxp_d, m, p, n_uniform, N_dev, head, nvec,
                       total);
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipStreamSynchronize(s));  // the host arrays may go away; the scratch is reused by the next call
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_ess_square(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, size_t m, size_t p, float n_uniform,
                               float *N_dev)
{
    return cusk::ess_square_impl(e, mxp_ess, pxp_ess, m, p, n_uniform, N_dev);
}
