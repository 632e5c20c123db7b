// pair_counts.hip -- per-pair numbers of complete observations (cusk_pair_counts of include/cusk_hip.h).
//
// The Pearson blocks of the correlation build divide by the number of individuals for which both variables are
// observed and then drop it.  A skeleton run on phenotypes with gaps needs that number per pair (the sample-size matrix
// of cusk_run_hetcor), so it is computed here as a result of its own, exactly, in integers:
//   mxp_n[i][t] = #{individuals: marker i not missing (.bed code != 01) and trait t not NaN}
//   pxp_n[a][b] = #{individuals: traits a and b not NaN}
// Both are popcounts of ANDed bit vectors.  trait_mask_kernel first writes each trait's "not NaN" flags in the bit layout
// of a .bed row -- one bit per individual at the even bit of its 2-bit code, zero from individual N on, rows padded to 16
// bytes -- which is p * ceil(N / 64) * 16 bytes (2.5 MB for 20 traits x 500,000 individuals) and stays in cache.
// pair_count_kernel then gives a wavefront one piece of one marker row: a lane takes 16 bytes of the row, forms the
// "not missing" bits (~(lo & ~hi) on the even bits) and adds popcount(bits & mask) for eight traits held in registers;
// the counters are summed over the wavefront once per piece and added to the result with integer atomics (pieces of a
// row are spread over workgroups when there are too few rows to fill the chip; integer sums do not depend on the order).
// Nothing depends on the bits of a row beyond individual N or on what follows the row in memory: the mask is zero there.
//
// Rows of ceil(N / 4) bytes start at any byte offset.  All global loads are aligned 16-byte loads nevertheless: a lane
// reads the two aligned chunks its 16 row bytes lie in and shifts them into place (v_alignbyte), and an aligned chunk is
// only touched when it holds at least one byte of the row, so no load leaves the pages of the rows.
#include <algorithm>
#include <vector>

#include "cusk_internal.h"

namespace cusk {

constexpr int kPcTraits = 8;  // traits whose counters a lane holds at a time

// masks[t][g * 4 + j]: the flags of individuals 64 g + 16 j .. + 15 of trait t spread to the even bits.  One wavefront per
// 64 individuals of one trait (blockIdx.y): coalesced reads of phen, one ballot, lanes 0-3 write the 16 bytes.
__global__ void __launch_bounds__(256) trait_mask_kernel(const float *__restrict__ phen, size_t N, size_t groups,
                                                         unsigned *__restrict__ masks)
{
    const size_t g = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (g >= groups) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const size_t t = blockIdx.y, i = g * 64 + lane;
    bool seen = false;
    if (i < N)
    {
        const float v = phen[t * N + i];
        seen = v == v;
    }
    const unsigned long long b = __ballot(seen);
    if (lane < 4)
    {
        unsigned x = (unsigned)(b >> (16 * lane)) & 0xffffu;
        x = (x | (x << 8)) & 0x00ff00ffu;
        x = (x | (x << 4)) & 0x0f0f0f0fu;
        x = (x | (x << 2)) & 0x33333333u;
        x = (x | (x << 1)) & 0x55555555u;
        masks[(t * groups + g) * 4 + lane] = x;
    }
}

// bytes Q * 4 + b .. + 15 of the 32 bytes in W
template <int Q>
__device__ __forceinline__ void shifted_chunk(const unsigned (&W)[8], unsigned b, unsigned (&o)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_alignbyte(W[Q + j + 1], W[Q + j], b);
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// out[row * p + t] += count over the 16-byte chunks [sg * seg, (sg + 1) * seg) of row `row`, item = row * nseg + sg, one
// wavefront per item.  bed: k rows of clb bytes; masks: p rows of `groups` uint4; out: k * p, zeroed.
__global__ void __launch_bounds__(256) pair_count_kernel(const unsigned char *__restrict__ bed, size_t clb, size_t k,
                                                         const uint4 *__restrict__ masks, size_t groups, size_t p, size_t seg,
                                                         size_t nseg, int *__restrict__ out)
{
    const size_t item = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (item >= k * nseg) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const size_t row = item / nseg, sg = item - row * nseg;
    const size_t c_begin = sg * seg, c_end = min(c_begin + seg, groups);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(bed) + row * clb;
    const unsigned sh = (unsigned)(addr & 15u), q = sh >> 2, b = sh & 3u;
    const uint4 *al = reinterpret_cast<const uint4 *>(addr - sh);  // aligned chunk c holds row bytes 16 c - sh .. + 15
    const size_t nal = (sh + clb + 15) / 16;                       // aligned chunks with a byte of the row in them
    for (size_t t0 = 0; t0 < p; t0 += kPcTraits)
    {
        int cnt[kPcTraits];
#pragma unroll
        for (int u = 0; u < kPcTraits; u++) cnt[u] = 0;
        for (size_t c = c_begin + lane; c < c_end; c += 64)
        {
            // c < groups: row byte 16 c exists (16 (groups - 1) < N / 4) and lies in aligned chunk c
            const uint4 lo = al[c];
            uint4 hi = make_uint4(0u, 0u, 0u, 0u);
            if (sh && c + 1 < nal) hi = al[c + 1];
            const unsigned W[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned o[4];
            switch (q)  // the same for all lanes
            {
            case 0: shifted_chunk<0>(W, b, o); break;
            case 1: shifted_chunk<1>(W, b, o); break;
            case 2: shifted_chunk<2>(W, b, o); break;
            default: shifted_chunk<3>(W, b, o); break;
            }
            unsigned nm[4];
#pragma unroll
            for (int j = 0; j < 4; j++) nm[j] = (~o[j] | (o[j] >> 1)) & 0x55555555u;  // anything but 01 (missing)
#pragma unroll
            for (int u = 0; u < kPcTraits; u++)
            {
                const size_t t = min(t0 + u, p - 1);  // past the last trait: counted again, never written
                const uint4 mk = masks[t * groups + c];
                cnt[u] += __popc(nm[0] & mk.x) + __popc(nm[1] & mk.y) + __popc(nm[2] & mk.z) + __popc(nm[3] & mk.w);
            }
        }
#pragma unroll
        for (int u = 0; u < kPcTraits; u++)
        {
            const int total = wave_sum(cnt[u]);
            if (lane == (unsigned)u && t0 + u < p && total) atomicAdd(&out[row * p + t0 + u], total);
        }
    }
}

// out[a * p + b] = out[b * p + a] = popcount(mask a & mask b) for a <= b; one workgroup per (a, b), out zeroed
__global__ void __launch_bounds__(256) trait_pair_count_kernel(const uint4 *__restrict__ masks, size_t groups, size_t p,
                                                               int *__restrict__ out)
{
    const size_t a = blockIdx.x / p, b = blockIdx.x - a * p;
    if (b < a) return;
    int v = 0;
    for (size_t c = threadIdx.x; c < groups; c += 256)
    {
        const uint4 x = masks[a * groups + c], y = masks[b * groups + c];
        v += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
    }
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0 && v)
    {
        atomicAdd(&out[a * p + b], v);
        if (a != b) atomicAdd(&out[b * p + a], v);
    }
}

static int pair_counts_impl(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                            size_t m_total, size_t N, size_t p, int *mxp_n_host, int *pxp_n_host)
{
    if (!e || !bed || !phen || k == 0 || N == 0 || p == 0 || (!mxp_n_host && !pxp_n_host) || m_total < k)
        return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_pair_counts: counts are 32-bit: too many individuals");
    if (p > 65535) return fail(e, CUSK_ERR_ARG, "cusk_pair_counts: too many traits for one launch");
    if (marker_ix)
        if (const int rc = check_marker_ix(e, marker_ix, k, m_total)) return rc;
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t clb = (N + 3) / 4, groups = (N + 63) / 64;

    const float *phen_d = phen;
    if (!is_device_pointer(phen))
    {
        CUSK_HIP(e, e->phen_dev.ensure(sizeof(float) * p * N));
        CUSK_HIP(e, hipMemcpyAsync(e->phen_dev.p, phen, sizeof(float) * p * N, hipMemcpyHostToDevice, s));
        phen_d = e->phen_dev.as<float>();
    }
    CUSK_HIP(e, e->pc_masks.ensure(p * groups * 16));
    CUSK_HIP(e, e->pc_counts.ensure(sizeof(int) * (k * p + p * p)));
    int *mxp_n_d = e->pc_counts.as<int>(), *pxp_n_d = mxp_n_d + k * p;
    CUSK_HIP(e, hipMemsetAsync(mxp_n_d, 0, sizeof(int) * (k * p + p * p), s));
    const size_t mask_blocks = (groups + 3) / 4;
    if (mask_blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_pair_counts: too many individuals for one launch");
    hipLaunchKernelGGL(trait_mask_kernel, dim3((unsigned)mask_blocks, (unsigned)p), dim3(256), 0, s, phen_d, N, groups,
                       e->pc_masks.as<unsigned>());
    CUSK_HIP(e, hipGetLastError());

    if (mxp_n_host)
    {
        std::vector<unsigned char> bed_h;
        const unsigned char *bed_k = bed;  // k contiguous rows, host or device
        const int *ix_d = nullptr;
        if (marker_ix)
            if (const int rc = pack_bed_rows(e, bed, marker_ix, ix_d, k, m_total, clb, bed_h, bed_k)) return rc;
        if (!is_device_pointer(bed_k))
        {
            CUSK_HIP(e, e->bed_dev.ensure(k * clb));
            CUSK_HIP(e, hipMemcpyAsync(e->bed_dev.p, bed_k, k * clb, hipMemcpyHostToDevice, s));
            CUSK_HIP(e, hipStreamSynchronize(s));  // bed_h goes out of scope below
            bed_k = e->bed_dev.as<unsigned char>();
        }
        // about 8192 wavefronts keep the chip busy: rows are cut into pieces of whole kilobytes when there are fewer
        const size_t steps = (groups + 63) / 64;  // kilobytes (64 lanes x 16 bytes) of a row
        const size_t nseg = std::min(steps, std::max<size_t>(1, 8192 / k));
        const size_t seg = (steps + nseg - 1) / nseg * 64;
        const size_t nseg_used = (groups + seg - 1) / seg;
        const size_t blocks = (k * nseg_used + 3) / 4;
        if (blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_pair_counts: too many markers for one launch");
        hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bed_k, clb, k,
                           e->pc_masks.as<uint4>(), groups, p, seg, nseg_used, mxp_n_d);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, hipMemcpyAsync(mxp_n_host, mxp_n_d, sizeof(int) * k * p, hipMemcpyDeviceToHost, s));
    }
    if (pxp_n_host)
    {
        if (p * p > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_pair_counts: too many traits for one launch");
        hipLaunchKernelGGL(trait_pair_count_kernel, dim3((unsigned)(p * p)), dim3(256), 0, s, e->pc_masks.as<uint4>(), groups, p,
                           pxp_n_d);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, hipMemcpyAsync(pxp_n_host, pxp_n_d, sizeof(int) * p * p, hipMemcpyDeviceToHost, s));
    }
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_pair_counts(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                                size_t m_total, size_t N, size_t p, int *mxp_n_host, int *pxp_n_host)
{
    return cusk::pair_counts_impl(e, bed, phen, marker_ix, k, m_total, N, p, mxp_n_host, pxp_n_host);
}
