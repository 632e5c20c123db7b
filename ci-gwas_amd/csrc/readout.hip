// readout.hip -- result expansion into the reference's dense layouts, sub-matrix gathers, packed block bitmaps.
#include "ci_exact.h"
#include "sweep_common.h"

namespace cusk {

// ---------------------------------------------------------------------------
// result expansion into the reference's dense layouts
// ---------------------------------------------------------------------------

__global__ void expand_adj_kernel(const unsigned long long *__restrict__ adj, int *G, int n, int words)
{
    const int row = blockIdx.y;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n) return;
    const unsigned long long w = adj[(size_t)row * words + (col >> 6)];
    G[(size_t)row * n + col] = (int)((w >> (col & 63)) & 1ull);
}

hipError_t launch_expand_adj(const unsigned long long *adj, int *G, int n, int words, hipStream_t st)
{
    hipLaunchKernelGGL(expand_adj_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, adj, G, n, words);
    return hipGetLastError();
}

// pMax before the sparse records are applied (cuPC-S.cu:424-442 semantics): -100000 on
// surviving edges, 1 on the diagonal, level-0 z where level 0 removed the pair, else 0.
__global__ void expand_pmax_kernel(const unsigned long long *__restrict__ adj,
                                   const unsigned long long *__restrict__ adj0, const float *__restrict__ C,
                                   float *pmax, int n, int words)
{
    const int row = blockIdx.y;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n) return;
    const bool live = (adj[(size_t)row * words + (col >> 6)] >> (col & 63)) & 1ull;
    const bool live0 = (adj0[(size_t)row * words + (col >> 6)] >> (col & 63)) & 1ull;
    float v;
    if (row == col)
        v = 1.0f;
    else if (live)
        v = -100000.0f;
    else if (!live0)
    {
        const int i = min(row, col), j = max(row, col);
        v = fisher_z_ratio(C[(size_t)i * n + j]);
    }
    else
        v = 0.0f;
    pmax[(size_t)row * n + col] = v;
}

__global__ void scatter_pmax_kernel(const int *x, const int *y, const float *z, long long nrec, float *pmax, int n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    // a stored z is never NaN (NaN fails z < th) and never negative: integer order == float order
    const int zi = __float_as_int(z[i]);
    atomicMax(reinterpret_cast<int *>(&pmax[(size_t)x[i] * n + y[i]]), zi);
    atomicMax(reinterpret_cast<int *>(&pmax[(size_t)y[i] * n + x[i]]), zi);
}

hipError_t launch_expand_pmax(const unsigned long long *adj, const unsigned long long *adj0, const float *C, float *pmax,
                              int n, int words, const int *x, const int *y, const float *z, long long nrec, hipStream_t st)
{
    hipLaunchKernelGGL(expand_pmax_kernel, dim3((n + 255) / 256, n), dim3(256), 0, st, adj, adj0, C, pmax, n, words);
    if (nrec > 0)
        hipLaunchKernelGGL(scatter_pmax_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st, x, y, z, nrec, pmax,
                           n);
    return hipGetLastError();
}

// out[a * k + b] = M[idx[a] * n + idx[b]]
__global__ void gather_sub_kernel(const float *__restrict__ M, int n, const int *__restrict__ idx, int k, float *out)
{
    const int a = blockIdx.y;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < k) out[(size_t)a * k + b] = M[(size_t)idx[a] * n + idx[b]];
}

hipError_t launch_gather_sub(const float *M, int n, const int *idx, int k, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(gather_sub_kernel, dim3((k + 255) / 256, k), dim3(256), 0, st, M, n, idx, k, out);
    return hipGetLastError();
}

// many sub-matrices in one launch (cusk_gather_rows): one wave per output row
__global__ void __launch_bounds__(256) gather_rows_kernel(const float *__restrict__ M, int n, const int *__restrict__ idx,
                                                           const int *__restrict__ row_src, const int *__restrict__ row_k,
                                                           const long long *__restrict__ row_first,
                                                           const long long *__restrict__ row_out, long long nrows, float *out)
{
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= nrows) return;
    const float *src = M + (size_t)row_src[t] * n;
    const int k = row_k[t];
    const int *cols = idx + row_first[t];
    float *dst = out + row_out[t];
    for (int c = lane; c < k; c += 64) dst[c] = src[cols[c]];
}

hipError_t launch_gather_rows(const float *M, int n, const int *idx, const int *row_src, const int *row_k, const long long *row_first,
                              const long long *row_out, long long nrows, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, M, n, idx, row_src, row_k, row_first,
                       row_out, nrows, out);
    return hipGetLastError();
}

// batched runs: the bitmap rows of every block, cut to the block's own words, packed back to back
// tail > 0: only the last `tail` rows of every block (the traits: all the pruning of depth 1 looks at)
__global__ void __launch_bounds__(256) pack_block_bits_kernel(const unsigned long long *__restrict__ adj, int n, int words,
                                                               const int2 *__restrict__ row_range, const int *__restrict__ row_blk,
                                                               const long long *__restrict__ blk_woff, unsigned long long *out,
                                                               int tail)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int b = row_blk[row];
    if (b < 0) return;
    const int2 rg = row_range[row];
    const int first = (tail > 0) ? max(rg.x, rg.y - tail) : rg.x;
    if (row < first) return;
    const int wb = (rg.y - rg.x + 63) >> 6, w0 = rg.x >> 6;
    unsigned long long *dst = out + blk_woff[b] + (long long)(row - first) * wb;
    for (int w = lane; w < wb; w += 64) dst[w] = adj[(size_t)row * words + w0 + w];
}

hipError_t launch_pack_block_bits(const unsigned long long *adj, int n, int words, const int2 *row_range, const int *row_blk,
                                  const long long *blk_woff, unsigned long long *out, int tail, hipStream_t st)
{
    hipLaunchKernelGGL(pack_block_bits_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, adj, n, words, row_range, row_blk,
                       blk_woff, out, tail);
    return hipGetLastError();
}

}  // namespace cusk
