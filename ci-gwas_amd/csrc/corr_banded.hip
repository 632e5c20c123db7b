// corr_banded.hip -- the device side of `mps block`: banded SNP x SNP correlations of a chromosome with their forward row sums
// (cusk_corr_banded: the FP4 kernel of corr_mxm.hip in its banded layout) and the Hanning smoother of that profile (cusk_hanning_smooth).
#include "corr_kernels.h"

namespace cusk {

// forward row sums of |band|: one thread per row, float accumulation in column order (the reference's host loop,
// corr_host.cu:112-128, so the sums are bit-identical)
__global__ void band_row_abs_sums_kernel(const float *__restrict__ band, size_t m, size_t w, float *sums)
{
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    float acc = 0.0f;
    for (size_t c = 0; c < w; c++) acc += fabsf(band[row * w + c]);
    sums[row] = acc;
}

// cal_mcorrk_banded + marker_corr_banded_mat_row_abs_sums (corr_host.cu:65-128) for one chromosome
extern "C" int cusk_corr_banded(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, size_t width, float *rowsums_host, float *band_host)
{
    if (!e || !bed || !rowsums_host || m == 0 || N == 0 || width == 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t clb = (N + 3) / 4;
    CUSK_HIP(e, e->bed_dev.ensure(m * clb));
    ScopedDevBuf sums, band;  // released when the call ends, on its error returns too
    CUSK_HIP(e, band.ensure(sizeof(float) * m * width));
    CUSK_HIP(e, sums.ensure(sizeof(float) * m));
    CUSK_HIP(e, hipMemcpyAsync(e->bed_dev.p, bed, m * clb, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemsetAsync(band.p, 0, sizeof(float) * m * width, s));  // pairs past the last marker stay 0
    launch_mxm_fp4(s, MxmFp4Args{e->bed_dev.as<unsigned char>(), band.as<float>(), m, N, clb, m, width, nullptr, 0, nullptr});
    hipLaunchKernelGGL(band_row_abs_sums_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, band.as<float>(), m, width,
                       sums.as<float>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(rowsums_host, sums.p, sizeof(float) * m, hipMemcpyDeviceToHost, s));
    if (band_host) CUSK_HIP(e, hipMemcpyAsync(band_host, band.p, sizeof(float) * m * width, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

// Hanning smoothing of the row-sum profile (blocking.cpp:13-35): one thread per centre, the window walked in
// order with separate double multiply and add (this file is compiled -ffp-contract=off), so every value equals
// the reference's host loop bit for bit; the bisection of `mps block` calls it a dozen times per chromosome and
// the O(n * window) loop is the one host hot spot the reference has there.
__global__ void hanning_smooth_kernel(const float *__restrict__ v, const double *__restrict__ weight, long long n, int window,
                                      double *out)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const long long margin = window / 2;
    double acc = 0.0;
    if (c >= margin && c < n - margin)
    {
        const float *src = v + (c - margin);
        for (int i = 0; i < window; i++) acc += weight[i] * (double)src[i];
    }
    out[c] = acc;
}

extern "C" int cusk_hanning_smooth(cusk_engine *e, const float *v_host, size_t n, const double *weight_host, int window, double *out_host)
{
    if (!e || !v_host || !weight_host || !out_host || n == 0 || window <= 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    ScopedDevBuf dout, dw, dv;
    CUSK_HIP(e, dv.ensure(sizeof(float) * n));
    CUSK_HIP(e, dw.ensure(sizeof(double) * (size_t)window));
    CUSK_HIP(e, dout.ensure(sizeof(double) * n));
    CUSK_HIP(e, hipMemcpyAsync(dv.p, v_host, sizeof(float) * n, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(dw.p, weight_host, sizeof(double) * (size_t)window, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(hanning_smooth_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, dv.as<float>(), dw.as<double>(),
                       (long long)n, window, dout.as<double>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(out_host, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

}  // namespace cusk
