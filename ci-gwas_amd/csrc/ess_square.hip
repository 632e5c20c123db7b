// ess_square.hip -- the sample-size matrix of one block, expanded on the device (cusk_ess_square of include/cusk_hip.h), and
// of the blocks of a batch on the diagonal of one allocation (cusk_ess_square_batch).
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
#include <vector>

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

// The same values for MANY blocks on the diagonal of one n x n allocation (cusk_ess_square_batch): block b holds the
// variables base .. base + m + p, its m x p and p x p tables start at mxp_off / b p^2.  One wave per row of the
// allocation; the row's block comes from a per-row table (-1: padding, nothing is written), as row_range gives level 0 its
// columns.  Only the (m + p) values of the row inside its own block are written: nothing reads the rest.  Bases are
// multiples of 64 and the allocation is 16-byte aligned, so a block row starts on a 16-byte boundary whenever n is a
// multiple of 4: 16-byte stores then, single floats for the tail and for other n.
struct EssBlock
{
    long long mxp_off;
    int base, m;
};

__global__ void __launch_bounds__(256) ess_square_batch_kernel(const float *__restrict__ mxp, const float *__restrict__ pxp,
                                                               const EssBlock *__restrict__ blk, const int *__restrict__ row_blk,
                                                               size_t p, float n_uniform, int n, float *__restrict__ out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t lane = threadIdx.x & 63;
    if (row >= n) return;
    const int b = row_blk[row];
    if (b < 0) return;
    const EssBlock k = blk[b];
    const size_t m = (size_t)k.m, nb = m + p, i = (size_t)(row - k.base);
    const float *mx = mxp + k.mxp_off, *px = pxp + (size_t)b * p * p;
    const size_t e0 = (size_t)row * (size_t)n + (size_t)k.base;
    float *dst = out + e0;
    const size_t nvec = (e0 & 3u) == 0 ? nb / 4 : 0;
    for (size_t q = lane; q < nvec; q += 64)
    {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = ess_square_value(mx, px, m, p, n_uniform, i, 4 * q + u);
        *reinterpret_cast<float4 *>(dst + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    }
    for (size_t j = 4 * nvec + lane; j < nb; j += 64) dst[j] = ess_square_value(mx, px, m, p, n_uniform, i, j);
}

// Is the size matrix its own transpose, bit for bit?  One wave per row, the lanes over the columns right of the diagonal
// inside the row's block (the whole row without row_range); a difference stores 1 into *flag (pinned host memory, set to
// 0 by the host before the launch).  NaN payloads compare as bits, so a NaN diagonal or a mirrored NaN pair is symmetric.
// The union-major sweep at per-pair sample sizes (sweep_tmaj.hip, HET) is planned only when the flag stays 0.
__global__ void __launch_bounds__(256) ess_symmetry_kernel(const unsigned *__restrict__ N, int n, const int2 *__restrict__ row_range,
                                                           int *flag)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int2 rr = row_range ? row_range[row] : make_int2(0, n);
    bool bad = false;
    for (int j = max(rr.x, row + 1) + lane; j < rr.y; j += 64) bad |= N[(size_t)row * n + j] != N[(size_t)j * n + row];
    if (bad) *reinterpret_cast<volatile int *>(flag) = 1;
}

hipError_t launch_ess_symmetry(const float *N, int n, const int2 *row_range, int *flag, hipStream_t st)
{
    hipLaunchKernelGGL(ess_symmetry_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const unsigned *>(N), n,
                       row_range, flag);
    return hipGetLastError();
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

static int ess_square_batch_impl(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, int nblk, const int *m, const int *base,
                                 size_t p, float n_uniform, int n, float *N_dev)
{
    if (!e || !N_dev || !m || !base || nblk <= 0 || n <= 0 || (p > 0 && !pxp_ess)) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (reinterpret_cast<uintptr_t>(N_dev) & 15u) return fail(e, CUSK_ERR_ARG, "cusk_ess_square_batch: the matrix must be 16-byte aligned");
    std::vector<EssBlock> blk((size_t)nblk);
    std::vector<int> row_blk((size_t)n, -1);
    size_t cm = 0;
    long long prev = 0;
    for (int b = 0; b < nblk; b++)
    {
        if (m[b] < 0 || (base[b] & 63) != 0 || (long long)base[b] < prev)
            return fail(e, CUSK_ERR_ARG, "cusk_ess_square_batch: block bases must be ascending multiples of 64, the blocks disjoint");
        const long long end = (long long)base[b] + m[b] + (long long)p;
        if (end > (long long)n) return fail(e, CUSK_ERR_ARG, "cusk_ess_square_batch: a block reaches beyond the n x n allocation");
        blk[(size_t)b].mxp_off = (long long)cm;
        blk[(size_t)b].base = base[b];
        blk[(size_t)b].m = m[b];
        for (long long r = base[b]; r < end; r++) row_blk[(size_t)r] = b;
        cm += (size_t)m[b] * p;
        prev = end;
    }
    if (cm > 0 && !mxp_ess) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // engine scratch: [m x p tables | p x p tables] (host arrays only; device-resident ones are read in place), block
    // table, per-row table
    const size_t cp = (size_t)nblk * p * p;
    const bool up_m = cm > 0 && !is_device_pointer(mxp_ess), up_p = cp > 0 && !is_device_pointer(pxp_ess);
    const size_t o_blk = (sizeof(float) * (cm + cp) + 15) & ~(size_t)15, o_row = o_blk + sizeof(EssBlock) * (size_t)nblk;
    CUSK_HIP(e, e->scratch_a.ensure(o_row + sizeof(int) * (size_t)n));
    char *d = e->scratch_a.as<char>();
    const float *mxp_d = mxp_ess, *pxp_d = pxp_ess;
    if (up_m)
    {
        CUSK_HIP(e, hipMemcpyAsync(d, mxp_ess, sizeof(float) * cm, hipMemcpyHostToDevice, s));
        mxp_d = reinterpret_cast<const float *>(d);
    }
    if (up_p)
    {
        CUSK_HIP(e, hipMemcpyAsync(d + sizeof(float) * cm, pxp_ess, sizeof(float) * cp, hipMemcpyHostToDevice, s));
        pxp_d = reinterpret_cast<const float *>(d) + cm;
    }
    CUSK_HIP(e, hipMemcpyAsync(d + o_blk, blk.data(), sizeof(EssBlock) * (size_t)nblk, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(d + o_row, row_blk.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ess_square_batch_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, mxp_d, pxp_d,
                       reinterpret_cast<const EssBlock *>(d + o_blk), reinterpret_cast<const int *>(d + o_row), p, n_uniform, n, N_dev);
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

extern "C" int cusk_ess_square_batch(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, int nblk, const int *m, const int *base,
                                     size_t p, float n_uniform, int n, float *N_dev)
{
    return cusk::ess_square_batch_impl(e, mxp_ess, pxp_ess, nblk, m, base, p, n_uniform, n, N_dev);
}
