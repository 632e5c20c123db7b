// ld_prune.hip -- the device side of `mps prune`: per-marker genotype counts, the conflict bitmap of a banded
// correlation matrix and the greedy "first kept marker wins" pass over it (cusk_genotype_counts, cusk_ld_prune_scan,
// cusk_ld_prune of include/cusk_hip.h, where the rule is stated).
//
// The correlations are those of `mps block`: launch_mxm_fp4 in its banded layout, band[i * W + c] = r(i, i + 1 + c).
// Three kernels follow it.
//
// genotype_count_kernel: one wavefront per marker row of ceil(N / 4) bytes, which starts at any byte.  The 16-byte
// chunks that lie inside the row and are aligned in memory are read as uint4, coalesced; the at most 15 bytes in front
// of them and the at most 15 behind are read as bytes.  No load leaves the row.  Counts are popcounts on the even and
// odd bit planes under a mask of the codes that belong to individuals < N, so what the last byte holds past individual
// N does not matter; code 00 is N minus the other three.
//
// conflict_bits_kernel: one wavefront per row of the band.  Row i of the bitmap holds ceil(W / 64) 64-bit words, bit b
// of word k = |r(i, i + 1 + 64 k + b)| >= r_max.  One ballot over 64 consecutive columns forms a word, lane k keeps
// word k, and the row goes out in one coalesced store.  Columns >= W give 0.
//
// ld_prune_scan_kernel: ONE wavefront walks the markers in order.  The markers that an earlier kept marker blocks are
// bits of a ring of 64 * (ceil(W / 64) + 1) bits in LDS, marker t at bit t mod ring.  Deciding j reads and clears bit
// j.  When j is kept, lane k shifts word k of row j by (j + 1) mod 64 and ORs the two pieces into the two ring words
// they land in (the second may wrap to word 0).  Only markers j + 1 .. j + W ever have a bit set, W <= ring - 64 bits,
// so a position is never shared by two live markers.  Bits of columns >= W and of pairs that reach past the last
// marker are masked off before the OR: the scan makes no assumption about them.  The rows of the bitmap are read
// eight markers ahead (their addresses do not depend on the decisions), the constant flags 64 at a time, and the
// statuses go out 64 at a time.  One lane holds one word, hence kPruneMaxWindow = 64 * 64.
#include "corr_kernels.h"

namespace cusk {

constexpr size_t kPruneMaxWindow = CUSK_PRUNE_MAX_WINDOW;
constexpr int kScanAhead = 8;  // markers whose bitmap rows are in flight; divides 64
static_assert(kPruneMaxWindow == 64 * 64, "ld_prune_scan_kernel: one lane per word of a bitmap row");

__device__ __forceinline__ int prune_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// codes 01, 10, 11 among the 16 codes of x whose individuals first .. first + 15 are < N
__device__ __forceinline__ void count_codes(unsigned x, size_t first, size_t N, int &n1, int &n2, int &n3)
{
    unsigned valid = 0x55555555u;
    if (first + 16 > N) valid = first < N ? valid & ((1u << (2 * (unsigned)(N - first))) - 1u) : 0u;
    const unsigned lo = x & valid, hi = (x >> 1) & valid;
    n1 += __popc(lo & ~hi);
    n2 += __popc(hi & ~lo);
    n3 += __popc(lo & hi);
}

// counts[row * 4 + c] = individuals < N with code c; constant[row] (when not null) = at most one of the codes 00, 10, 11 occurs
__global__ void __launch_bounds__(256) genotype_count_kernel(const unsigned char *__restrict__ bed, size_t clb, size_t m, size_t N,
                                                             int4 *__restrict__ counts, unsigned char *__restrict__ constant)
{
    const size_t row = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (row >= m) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const unsigned char *r = bed + row * clb;
    const size_t head = min(clb, (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(r) & 15u)) & 15u));
    const size_t chunks = (clb - head) / 16, tail = clb - head - chunks * 16;
    int n1 = 0, n2 = 0, n3 = 0;
    const uint4 *body = reinterpret_cast<const uint4 *>(r + head);
    for (size_t c = lane; c < chunks; c += 64)
    {
        const uint4 v = body[c];
        const size_t first = (head + c * 16) * 4;
        count_codes(v.x, first, N, n1, n2, n3);
        count_codes(v.y, first + 16, N, n1, n2, n3);
        count_codes(v.z, first + 32, N, n1, n2, n3);
        count_codes(v.w, first + 48, N, n1, n2, n3);
    }
    if (lane < head + tail)  // head + tail <= 30
    {
        const size_t at = lane < head ? lane : head + chunks * 16 + (lane - head);
        count_codes(r[at], at * 4, N, n1, n2, n3);
    }
    n1 = prune_wave_sum(n1);
    n2 = prune_wave_sum(n2);
    n3 = prune_wave_sum(n3);
    if (lane == 0)
    {
        const int n0 = (int)N - n1 - n2 - n3;
        counts[row] = make_int4(n0, n1, n2, n3);
        if (constant) constant[row] = (unsigned char)((n0 > 0) + (n2 > 0) + (n3 > 0) <= 1);
    }
}

// bits[i * nw + k], nw = ceil(W / 64) <= 64
__global__ void __launch_bounds__(256) conflict_bits_kernel(const float *__restrict__ band, size_t m, size_t W, unsigned nw, float r_max,
                                                            unsigned long long *__restrict__ bits)
{
    const size_t i = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (i >= m) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const float *row = band + i * W;
    unsigned long long mine = 0;
    for (unsigned k = 0; k < nw; k++)
    {
        const size_t c = (size_t)k * 64 + lane;
        bool hit = false;
        if (c < W) hit = fabsf(row[c]) >= r_max;  // false for NaN
        const unsigned long long word = __ballot(hit);
        if (lane == k) mine = word;
    }
    if (lane < nw) bits[i * nw + lane] = mine;
}

// the low `count` bits (0 .. 64)
__device__ __forceinline__ unsigned long long low_bits(size_t count)
{
    return count >= 64 ? ~0ull : ((1ull << count) - 1ull);
}

__global__ void __launch_bounds__(64) ld_prune_scan_kernel(const unsigned long long *__restrict__ bits, const unsigned char *__restrict__ constant,
                                                           size_t m, size_t W, unsigned nw, unsigned char *__restrict__ status)
{
    __shared__ unsigned long long ring[kPruneMaxWindow / 64 + 1];
    const unsigned lane = threadIdx.x;
    const unsigned rw = nw + 1;  // ring words
    for (unsigned k = lane; k < rw; k += 64) ring[k] = 0;
    __syncthreads();

    auto load_row = [&](size_t j) -> unsigned long long { return (j < m && lane < nw) ? bits[j * nw + lane] : 0ull; };
    unsigned long long cur[kScanAhead], nxt[kScanAhead];
#pragma unroll
    for (int u = 0; u < kScanAhead; u++) cur[u] = load_row((size_t)u);

    unsigned word = 0, bit = 0;  // ring position of marker j: word * 64 + bit
    unsigned long long const_mask = 0;
    unsigned char mine = 0;  // status of marker (j & ~63) + lane
    for (size_t j0 = 0; j0 < m; j0 += kScanAhead)
    {
#pragma unroll
        for (int u = 0; u < kScanAhead; u++) nxt[u] = load_row(j0 + kScanAhead + u);
        if ((j0 & 63) == 0)
        {
            const size_t t = j0 + lane;
            const_mask = __ballot(t < m && constant[t] != 0);
        }
#pragma unroll
        for (int u = 0; u < kScanAhead; u++)
        {
            const size_t j = j0 + u;
            if (j >= m) break;  // the same for all lanes
            const unsigned long long here = ring[word];
            const bool blocked = (here >> bit) & 1ull;
            const bool is_const = (const_mask >> (j & 63)) & 1ull;
            if (lane == 0 && blocked) ring[word] = here & ~(1ull << bit);
            if (lane == (unsigned)(j & 63)) mine = is_const ? CUSK_PRUNE_CONSTANT : blocked ? CUSK_PRUNE_LD : CUSK_PRUNE_KEEP;
            // marker j + 1 is at the next ring position
            unsigned word1 = word, bit1 = bit + 1;
            if (bit1 == 64)
            {
                bit1 = 0;
                word1 = word + 1 == rw ? 0 : word + 1;
            }
            if (!is_const && !blocked)
            {
                // columns c < min(W, m - 1 - j): pairs inside the window whose second marker exists
                const size_t limit = min(W, m - 1 - j), c0 = (size_t)lane * 64;
                const unsigned long long src = c0 < limit ? cur[u] & low_bits(limit - c0) : 0ull;
                if (src)
                {
                    unsigned w0 = word1 + lane;  // < 2 * rw: word1 < rw, lane < nw < rw
                    if (w0 >= rw) w0 -= rw;
                    const unsigned w1 = w0 + 1 == rw ? 0 : w0 + 1;
                    atomicOr(&ring[w0], src << bit1);
                    if (bit1) atomicOr(&ring[w1], src >> (64 - bit1));
                }
            }
            __syncthreads();  // one wavefront: orders the LDS accesses of this marker before the next one's
            word = word1;
            bit = bit1;
            if ((j & 63) == 63 || j + 1 == m)
            {
                const size_t t = (j & ~(size_t)63) + lane;
                if (t < m) status[t] = mine;
            }
        }
#pragma unroll
        for (int u = 0; u < kScanAhead; u++) cur[u] = nxt[u];
    }
}

static unsigned prune_words(size_t W) { return (unsigned)((W + 63) / 64); }

static void launch_counts(hipStream_t s, const unsigned char *bed, size_t clb, size_t m, size_t N, int *counts, unsigned char *constant)
{
    hipLaunchKernelGGL(genotype_count_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, bed, clb, m, N, reinterpret_cast<int4 *>(counts),
                       constant);
}

static void launch_scan(hipStream_t s, const unsigned long long *bits, const unsigned char *constant, size_t m, size_t W, unsigned char *status)
{
    hipLaunchKernelGGL(ld_prune_scan_kernel, dim3(1), dim3(64), 0, s, bits, constant, m, W, prune_words(W), status);
}

// what every entry point refuses about the marker count (grids of four rows per workgroup)
static bool too_many_markers(size_t m) { return (m + 3) / 4 > (size_t)0x7fffffff; }

}  // namespace cusk

using namespace cusk;

extern "C" int cusk_genotype_counts(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, int *counts_out)
{
    if (!e || !bed || !counts_out || m == 0 || N == 0) return fail(e, CUSK_ERR_ARG, "cusk_genotype_counts: bad arguments");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_genotype_counts: counts are 32-bit: too many individuals");
    if (too_many_markers(m)) return fail(e, CUSK_ERR_ARG, "cusk_genotype_counts: too many markers for one launch");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t clb = (N + 3) / 4;
    ScopedDevBuf counts;
    CUSK_HIP(e, e->bed_dev.ensure(m * clb));
    CUSK_HIP(e, counts.ensure(sizeof(int) * 4 * m));
    CUSK_HIP(e, hipMemcpyAsync(e->bed_dev.p, bed, m * clb, hipMemcpyHostToDevice, s));
    launch_counts(s, e->bed_dev.as<unsigned char>(), clb, m, N, counts.as<int>(), nullptr);
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(counts_out, counts.p, sizeof(int) * 4 * m, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

extern "C" int cusk_ld_prune_scan(cusk_engine *e, const unsigned long long *conflict_bits, const unsigned char *constant_flags, size_t m,
                                  size_t W, unsigned char *status_out)
{
    if (!e || !conflict_bits || !constant_flags || !status_out || m == 0 || W == 0)
        return fail(e, CUSK_ERR_ARG, "cusk_ld_prune_scan: bad arguments");
    if (W > kPruneMaxWindow) return fail(e, CUSK_ERR_ARG, "cusk_ld_prune_scan: window above CUSK_PRUNE_MAX_WINDOW");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t nw = prune_words(W);
    ScopedDevBuf bits, flags, status;
    CUSK_HIP(e, bits.ensure(sizeof(unsigned long long) * m * nw));
    CUSK_HIP(e, flags.ensure(m));
    CUSK_HIP(e, status.ensure(m));
    CUSK_HIP(e, hipMemcpyAsync(bits.p, conflict_bits, sizeof(unsigned long long) * m * nw, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(flags.p, constant_flags, m, hipMemcpyHostToDevice, s));
    launch_scan(s, bits.as<unsigned long long>(), flags.as<unsigned char>(), m, W, status.as<unsigned char>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(status_out, status.p, m, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

extern "C" int cusk_ld_prune(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, size_t W, float r_max, unsigned char *status_out,
                             int *counts_out)
{
    if (!e || !bed || !status_out || m == 0 || N == 0 || W == 0 || !(r_max > 0.0f && r_max <= 1.0f))
        return fail(e, CUSK_ERR_ARG, "cusk_ld_prune: bad arguments");
    if (W > kPruneMaxWindow) return fail(e, CUSK_ERR_ARG, "cusk_ld_prune: window above CUSK_PRUNE_MAX_WINDOW");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ld_prune: counts are 32-bit: too many individuals");
    if (too_many_markers(m)) return fail(e, CUSK_ERR_ARG, "cusk_ld_prune: too many markers for one launch");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t clb = (N + 3) / 4, nw = prune_words(W);
    ScopedDevBuf band, counts, flags, bits, status;  // released when the call ends, on its error returns too
    CUSK_HIP(e, e->bed_dev.ensure(m * clb));
    CUSK_HIP(e, band.ensure(sizeof(float) * m * W));
    CUSK_HIP(e, counts.ensure(sizeof(int) * 4 * m));
    CUSK_HIP(e, flags.ensure(m));
    CUSK_HIP(e, bits.ensure(sizeof(unsigned long long) * m * nw));
    CUSK_HIP(e, status.ensure(m));
    // phase marks: upload | band | counts | bitmap | scan (cusk_ld_prune_timing); the events live in the engine
    for (hipEvent_t &v : e->ev_prune)
        if (!v) CUSK_HIP(e, hipEventCreate(&v));
    hipEvent_t *ev = e->ev_prune;
    CUSK_HIP(e, hipEventRecord(ev[0], s));
    CUSK_HIP(e, hipMemcpyAsync(e->bed_dev.p, bed, m * clb, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipEventRecord(ev[1], s));
    // the build of cusk_corr_banded: pairs past the last marker stay 0
    CUSK_HIP(e, hipMemsetAsync(band.p, 0, sizeof(float) * m * W, s));
    launch_mxm_fp4(s, MxmFp4Args{e->bed_dev.as<unsigned char>(), band.as<float>(), m, N, clb, m, W, nullptr, 0, nullptr});
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipEventRecord(ev[2], s));
    launch_counts(s, e->bed_dev.as<unsigned char>(), clb, m, N, counts.as<int>(), flags.as<unsigned char>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipEventRecord(ev[3], s));
    hipLaunchKernelGGL(conflict_bits_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, band.as<float>(), m, W, (unsigned)nw, r_max,
                       bits.as<unsigned long long>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipEventRecord(ev[4], s));
    launch_scan(s, bits.as<unsigned long long>(), flags.as<unsigned char>(), m, W, status.as<unsigned char>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipEventRecord(ev[5], s));
    CUSK_HIP(e, hipMemcpyAsync(status_out, status.p, m, hipMemcpyDeviceToHost, s));
    if (counts_out) CUSK_HIP(e, hipMemcpyAsync(counts_out, counts.p, sizeof(int) * 4 * m, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    for (int k = 0; k < 5; k++) CUSK_HIP(e, hipEventElapsedTime(&e->prune_ms[k], ev[k], ev[k + 1]));
    return CUSK_OK;
}

extern "C" void cusk_ld_prune_timing(const cusk_engine *e, float *ms5)
{
    if (!e || !ms5) return;
    for (int k = 0; k < 5; k++) ms5[k] = e->prune_ms[k];
}
