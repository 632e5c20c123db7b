// ordinal.hip -- polychoric / polyserial correlations of ordinal traits (cusk_ordinal_tables, cusk_polychoric_fit,
// cusk_polyserial_fit of include/cusk_hip.h).  A binary or graded trait has no Pearson correlation worth testing: the
// latent correlation is estimated from the contingency table of the pair (marker class x level, level x level) or, for
// a continuous partner, from the observations themselves.  Three kernels:
//
//   ordinal_table_kernel   the part that grows with N.  level_mask_kernel writes, per ordinal trait and level, one bit
//                          per individual in the .bed row layout (the layout and padding of trait_mask_kernel of
//                          pair_counts.hip: even bit of the 2-bit code, zero from individual N on, rows padded to 16
//                          bytes).  A wavefront then takes a piece of one marker row, as pair_count_kernel does, with
//                          the same aligned loads at any byte offset; it decodes the three genotype classes into
//                          bit-planes (ordered by dosage: code 11 -> 0, 10 -> 1, 00 -> 2; 01 is missing and in no plane)
//                          and adds popcount(plane & mask) into 3 x 8 counters held in registers, one trait at a time.
//                          Counters are summed over the wavefront and added with 32-bit integer atomics, so the tables
//                          are exact and do not depend on the order.  The masks are zero beyond individual N and for
//                          levels a trait does not have: nothing in the padding of a row or behind it reaches a count.
//   polychoric_fit_kernel  one table per lane.  A fit is a few dozen evaluations of the likelihood, each a walk over the
//                          cells with two bivariate-normal corners per cell (ordinal_math.h); tables are independent and
//                          there are k x q of them, so a lane per table fills the chip without any exchange between
//                          lanes, and a lane group per table would leave five lanes in eight idle on the 3 x K tables
//                          that make up all but q^2 of the work.  The table is read from global memory where it lies
//                          (cached; the arithmetic dominates), the thresholds sit in LDS at a stride of one workgroup, so
//                          no array is indexed in registers and nothing goes to scratch.
//   polyserial_fit_kernel  one workgroup per (continuous, ordinal) pair: mean, deviation, level counts and then every
//                          evaluation of the likelihood stream the N values and are reduced in a fixed order (a thread's
//                          own stride first, then a tree in LDS), so results are reproducible.  At most p^2 pairs: small.
#include <algorithm>
#include <cstring>
#include <vector>

#include "cusk_internal.h"
#include "ordinal_math.h"

namespace cusk {

constexpr int kOrdLevels = ord::kMaxLevels;

// masks[(t * 8 + u) * groups * 4 + g * 4 + j]: the individuals 64 g + 16 j .. + 15 whose value of ordinal trait t is its
// level u, spread to the even bits.  blockIdx.y = t * 8 + u; a level the trait does not have gets zeros.
__global__ void __launch_bounds__(256) level_mask_kernel(const float *__restrict__ phen, size_t N, size_t groups,
                                                         const int *__restrict__ ord_ix, const float *__restrict__ levels,
                                                         const int *__restrict__ nlev, unsigned *__restrict__ masks)
{
    const size_t g = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (g >= groups) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const size_t t = blockIdx.y / kOrdLevels, i = g * 64 + lane;
    const int u = blockIdx.y % kOrdLevels;
    bool is = false;
    if (i < N && u < nlev[t]) is = phen[(size_t)ord_ix[t] * N + i] == levels[t * kOrdLevels + u];  // false for NaN
    const unsigned long long b = __ballot(is);
    if (lane < 4)
    {
        unsigned x = (unsigned)(b >> (16 * lane)) & 0xffffu;
        x = (x | (x << 8)) & 0x00ff00ffu;
        x = (x | (x << 4)) & 0x0f0f0f0fu;
        x = (x | (x << 2)) & 0x33333333u;
        x = (x | (x << 1)) & 0x55555555u;
        masks[(blockIdx.y * groups + g) * 4 + lane] = x;
    }
}

template <int Q>
__device__ __forceinline__ void ord_shifted_chunk(const unsigned (&W)[8], unsigned b, unsigned (&o)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_alignbyte(W[Q + j + 1], W[Q + j], b);
}

__device__ __forceinline__ int ord_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int popc4(const unsigned (&x)[4], const uint4 &m)
{
    return __popc(x[0] & m.x) + __popc(x[1] & m.y) + __popc(x[2] & m.z) + __popc(x[3] & m.w);
}

// out[((row * q + t) * 3 + class) * 8 + level] += count over the 16-byte chunks [sg * seg, (sg + 1) * seg) of row `row`,
// item = row * nseg + sg, one wavefront per item.  bed: k rows of clb bytes at any byte offset; out zeroed.
__global__ void __launch_bounds__(256) ordinal_table_kernel(const unsigned char *__restrict__ bed, size_t clb, size_t k,
                                                            const uint4 *__restrict__ masks, size_t groups, size_t q,
                                                            const int *__restrict__ nlev, size_t seg, size_t nseg,
                                                            int *__restrict__ out)
{
    const size_t item = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (item >= k * nseg) return;  // whole wavefronts
    const unsigned lane = threadIdx.x & 63u;
    const size_t row = item / nseg, sg = item - row * nseg;
    const size_t c_begin = sg * seg, c_end = min(c_begin + seg, groups);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(bed) + row * clb;
    const unsigned sh = (unsigned)(addr & 15u), qq = sh >> 2, b = sh & 3u;
    const uint4 *al = reinterpret_cast<const uint4 *>(addr - sh);  // aligned chunk c holds row bytes 16 c - sh .. + 15
    const size_t nal = (sh + clb + 15) / 16;                       // aligned chunks with a byte of the row in them
    for (size_t t = 0; t < q; t++)
    {
        const int K = nlev[t];
        int cnt[3][kOrdLevels];
#pragma unroll
        for (int g = 0; g < 3; g++)
#pragma unroll
            for (int u = 0; u < kOrdLevels; u++) cnt[g][u] = 0;
        for (size_t c = c_begin + lane; c < c_end; c += 64)
        {
            // c < groups: row byte 16 c exists (16 (groups - 1) < N / 4) and lies in aligned chunk c
            const uint4 lo = al[c];
            uint4 hi = make_uint4(0u, 0u, 0u, 0u);
            if (sh && c + 1 < nal) hi = al[c + 1];
            const unsigned W[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned o[4];
            switch (qq)  // the same for all lanes
            {
            case 0: ord_shifted_chunk<0>(W, b, o); break;
            case 1: ord_shifted_chunk<1>(W, b, o); break;
            case 2: ord_shifted_chunk<2>(W, b, o); break;
            default: ord_shifted_chunk<3>(W, b, o); break;
            }
            unsigned g0[4], g1[4], g2[4];  // dosage 0 (code 11), 1 (10), 2 (00) on the even bits
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const unsigned l = o[j] & 0x55555555u, h = (o[j] >> 1) & 0x55555555u;
                g0[j] = l & h;
                g1[j] = h & ~l;
                g2[j] = ~(l | h) & 0x55555555u;
            }
#pragma unroll
            for (int u = 0; u < kOrdLevels; u++)
                if (u < K)  // the same for all lanes
                {
                    const uint4 mk = masks[(t * kOrdLevels + u) * groups + c];
                    cnt[0][u] += popc4(g0, mk);
                    cnt[1][u] += popc4(g1, mk);
                    cnt[2][u] += popc4(g2, mk);
                }
        }
#pragma unroll
        for (int g = 0; g < 3; g++)
#pragma unroll
            for (int u = 0; u < kOrdLevels; u++)
                if (u < K)
                {
                    const int total = ord_wave_sum(cnt[g][u]);
                    if (lane == (unsigned)(g * kOrdLevels + u) && total)
                        atomicAdd(&out[((row * q + t) * 3 + g) * kOrdLevels + u], total);
                }
    }
}

// out[((a * q + b) * 8 + la) * 8 + lb] = popcount(mask(a, la) & mask(b, lb)); one workgroup per (a, b, la), out zeroed
__global__ void __launch_bounds__(256) ordinal_trait_table_kernel(const uint4 *__restrict__ masks, size_t groups, size_t q,
                                                                  const int *__restrict__ nlev, int *__restrict__ out)
{
    const size_t a = blockIdx.x / (q * kOrdLevels), rem = blockIdx.x - a * q * kOrdLevels, b = rem / kOrdLevels,
                 la = rem - b * kOrdLevels;
    if ((int)la >= nlev[a]) return;
    int cnt[kOrdLevels];
#pragma unroll
    for (int u = 0; u < kOrdLevels; u++) cnt[u] = 0;
    for (size_t c = threadIdx.x; c < groups; c += 256)
    {
        const uint4 x = masks[(a * kOrdLevels + la) * groups + c];
        const unsigned xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int u = 0; u < kOrdLevels; u++) cnt[u] += popc4(xs, masks[(b * kOrdLevels + u) * groups + c]);
    }
#pragma unroll
    for (int u = 0; u < kOrdLevels; u++)
    {
        const int total = ord_wave_sum(cnt[u]);
        if ((threadIdx.x & 63u) == (unsigned)u && total) atomicAdd(&out[((a * q + b) * kOrdLevels + la) * kOrdLevels + u], total);
    }
}

struct TableCell
{
    const int *T;
    int kb;
    __device__ __forceinline__ int operator()(int a, int b) const { return T[a * kb + b]; }
};

// r, se, status of table `blockIdx.x * 256 + threadIdx.x`; tables: ntab x ka x kb counts, ka, kb <= 8
__global__ void __launch_bounds__(256) polychoric_fit_kernel(const int *__restrict__ tables, size_t ntab, int ka, int kb,
                                                             double *__restrict__ r_out, double *__restrict__ se_out,
                                                             int *__restrict__ status_out)
{
    __shared__ double th[2 * kOrdLevels][256];  // thresholds of this lane's table: rows, then columns
    const size_t tab = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (tab >= ntab) return;
    const TableCell cell{tables + tab * (size_t)(ka * kb), kb};
    double r, se;
    int status;
    ord::polychoric_fit(cell, ka, kb, &th[0][threadIdx.x], 256, &th[kOrdLevels][threadIdx.x], 256, r, se, status);
    r_out[tab] = r;
    se_out[tab] = se;
    status_out[tab] = status;
}

// sums over the workgroup in a fixed order, returned to every thread; red: 256 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double *red)
{
    __syncthreads();  // red may still be read from the call before
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1)
    {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

// the level of y among the K levels, or -1 when y is none of them (NaN included): the rule of level_mask_kernel
__device__ __forceinline__ int level_code(float y, const float *lev, int K)
{
    int code = -1;
#pragma unroll
    for (int u = 0; u < kOrdLevels; u++) code = (u < K && y == lev[u]) ? u : code;
    return code;
}

// pair blockIdx.x = c * q + o of continuous trait cont_ix[c] and ordinal trait ord_ix[o]
__global__ void __launch_bounds__(256) polyserial_fit_kernel(const float *__restrict__ phen, size_t N,
                                                             const int *__restrict__ cont_ix, const int *__restrict__ ord_ix,
                                                             size_t q, const float *__restrict__ levels,
                                                             const int *__restrict__ nlev, double *__restrict__ r_out,
                                                             double *__restrict__ se_out, int *__restrict__ status_out)
{
    __shared__ double red[256];
    __shared__ double tau[kOrdLevels + 1];  // tau[u]: lower threshold of level u; tau[u + 1]: its upper one
    __shared__ float lev[kOrdLevels];
    const size_t c = blockIdx.x / q, o = blockIdx.x - c * q;
    const float *x = phen + (size_t)cont_ix[c] * N, *y = phen + (size_t)ord_ix[o] * N;
    const int K = nlev[o];
    if (threadIdx.x < kOrdLevels) lev[threadIdx.x] = levels[o * kOrdLevels + threadIdx.x];
    __syncthreads();

    double sum = 0.0, cnt = 0.0;
    for (size_t i = threadIdx.x; i < N; i += 256)
    {
        const float xv = x[i];
        if (xv == xv && level_code(y[i], lev, K) >= 0)
        {
            sum += (double)xv;
            cnt += 1.0;
        }
    }
    const double n = block_sum(cnt, red);  // exact: integers below 2^53
    const double mean = block_sum(sum, red) / n;
    double ss = 0.0;
    for (size_t i = threadIdx.x; i < N; i += 256)
    {
        const float xv = x[i];
        if (xv == xv && level_code(y[i], lev, K) >= 0)
        {
            const double d = (double)xv - mean;
            ss += d * d;
        }
    }
    const double sd = sqrt(block_sum(ss, red) / (n - 1.0));
    int seen = 0;
    double cum = 0.0;
    if (threadIdx.x == 0) tau[0] = -INFINITY;
    for (int u = 0; u < K; u++)
    {
        double m = 0.0;
        for (size_t i = threadIdx.x; i < N; i += 256)
        {
            const float xv = x[i];
            if (xv == xv && level_code(y[i], lev, K) == u) m += 1.0;
        }
        m = block_sum(m, red);
        seen += m > 0.0;
        cum += m;
        if (threadIdx.x == 0) tau[u + 1] = ord::threshold_of((long long)cum, (long long)n);
    }
    __syncthreads();
    if (seen < 2 || !(n >= 2.0) || !(sd > 0.0))
    {
        if (threadIdx.x == 0)
        {
            r_out[blockIdx.x] = se_out[blockIdx.x] = NAN;
            status_out[blockIdx.x] = ord::kStatusDegenerate;
        }
        return;
    }
    ord::RootIter it;  // the same in every thread: it is fed the reduced values only
    it.start();
    double d2 = 0.0;
    while (!it.done())
    {
        const double rho = it.rho();
        double sc = 0.0, dsc = 0.0;
        bool barrier = false;
        for (size_t i = threadIdx.x; i < N; i += 256)
        {
            const float xv = x[i];
            const int code = level_code(y[i], lev, K);
            if (xv == xv && code >= 0) ord::polyserial_term(((double)xv - mean) / sd, tau[code], tau[code + 1], rho, sc, dsc, barrier);
        }
        const bool any_barrier = block_sum(barrier ? 1.0 : 0.0, red) > 0.0;
        sc = block_sum(sc, red);
        dsc = block_sum(dsc, red);
        d2 = any_barrier ? 0.0 : dsc;
        if (it.last())
            it.finish();
        else
            it.step(sc, dsc, any_barrier);
    }
    if (threadIdx.x == 0)
    {
        double r, se;
        int status;
        ord::conclude(it, d2, r, se, status);
        r_out[blockIdx.x] = r;
        se_out[blockIdx.x] = se;
        status_out[blockIdx.x] = status;
    }
}

// M[idx][j] = M[j][idx] = v[j]
__global__ void __launch_bounds__(256) set_cross_kernel(float *__restrict__ M, size_t n, size_t idx, const float *__restrict__ v)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    M[idx * n + j] = v[j];
    M[j * n + idx] = v[j];
}

namespace {

// kernel time between two events on the engine's stream, created and destroyed around one launch
struct LaunchTimer
{
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    explicit LaunchTimer(hipStream_t st) : s(st)
    {
        if (hipEventCreate(&a) != hipSuccess) a = nullptr;
        if (hipEventCreate(&b) != hipSuccess) b = nullptr;
    }
    void begin()
    {
        if (a) (void)hipEventRecord(a, s);
    }
    void end()
    {
        if (b) (void)hipEventRecord(b, s);
    }
    float ms()  // after the stream was synchronised
    {
        float v = 0.0f;
        if (a && b && hipEventElapsedTime(&v, a, b) != hipSuccess) v = 0.0f;
        return v;
    }
    ~LaunchTimer()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

int check_ordinal_spec(cusk_engine *e, const char *who, size_t p, const int *ord_ix, size_t q, const float *levels, const int *nlev)
{
    if (!ord_ix || !levels || !nlev || q == 0 || q > p) return fail(e, CUSK_ERR_ARG, std::string(who) + ": bad arguments");
    for (size_t t = 0; t < q; t++)
    {
        if (ord_ix[t] < 0 || (size_t)ord_ix[t] >= p) return fail(e, CUSK_ERR_ARG, std::string(who) + ": ordinal trait index out of range");
        if (nlev[t] < 1 || nlev[t] > kOrdLevels)
            return fail(e, CUSK_ERR_ARG, std::string(who) + ": an ordinal trait has between 1 and 8 levels");
        for (int u = 1; u < nlev[t]; u++)
            if (!(levels[t * kOrdLevels + u] > levels[t * kOrdLevels + u - 1]))
                return fail(e, CUSK_ERR_ARG, std::string(who) + ": levels must be ascending and distinct");
    }
    return CUSK_OK;
}

// ord_ix (q ints), nlev (q ints), levels (q * 8 floats) in one device buffer
struct SpecOnDevice
{
    ScopedDevBuf buf;
    const int *ord_ix = nullptr, *nlev = nullptr;
    const float *levels = nullptr;
    hipError_t upload(const int *ix, size_t q, const float *lv, const int *nl, hipStream_t s)
    {
        std::vector<int> h(q * (2 + kOrdLevels));
        std::copy(ix, ix + q, h.begin());
        std::copy(nl, nl + q, h.begin() + q);
        std::memcpy(&h[2 * q], lv, sizeof(float) * q * kOrdLevels);
        hipError_t st = buf.ensure(sizeof(int) * h.size());
        if (st != hipSuccess) return st;
        st = hipMemcpyAsync(buf.p, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, s);
        if (st != hipSuccess) return st;
        st = hipStreamSynchronize(s);  // h goes out of scope
        ord_ix = buf.as<int>();
        nlev = ord_ix + q;
        levels = reinterpret_cast<const float *>(nlev + q);
        return st;
    }
};

}  // namespace

static int ordinal_tables_impl(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                               size_t m_total, size_t N, size_t p, const int *ord_ix, size_t q, const float *levels,
                               const int *nlev, int *mxo_tab_host, int *oxo_tab_host)
{
    if (!e || !phen || N == 0 || p == 0 || (!mxo_tab_host && !oxo_tab_host)) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (mxo_tab_host && (!bed || k == 0 || m_total < k)) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (N > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ordinal_tables: counts are 32-bit: too many individuals");
    if (const int rc = check_ordinal_spec(e, "cusk_ordinal_tables", p, ord_ix, q, levels, nlev)) return rc;
    if (q * kOrdLevels > 65535) return fail(e, CUSK_ERR_ARG, "cusk_ordinal_tables: too many ordinal traits for one launch");
    if (mxo_tab_host && marker_ix)
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
    SpecOnDevice spec;
    CUSK_HIP(e, spec.upload(ord_ix, q, levels, nlev, s));
    const size_t mxo_cells = mxo_tab_host ? k * q * 3 * kOrdLevels : 0, oxo_cells = q * q * kOrdLevels * kOrdLevels;
    CUSK_HIP(e, e->pc_masks.ensure(q * kOrdLevels * groups * 16));
    CUSK_HIP(e, e->pc_counts.ensure(sizeof(int) * (mxo_cells + oxo_cells)));
    int *mxo_d = e->pc_counts.as<int>(), *oxo_d = mxo_d + mxo_cells;
    CUSK_HIP(e, hipMemsetAsync(mxo_d, 0, sizeof(int) * (mxo_cells + oxo_cells), s));
    const size_t mask_blocks = (groups + 3) / 4;
    if (mask_blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ordinal_tables: too many individuals for one launch");
    hipLaunchKernelGGL(level_mask_kernel, dim3((unsigned)mask_blocks, (unsigned)(q * kOrdLevels)), dim3(256), 0, s, phen_d, N, groups,
                       spec.ord_ix, spec.levels, spec.nlev, e->pc_masks.as<unsigned>());
    CUSK_HIP(e, hipGetLastError());

    LaunchTimer timer(s);
    if (mxo_tab_host)
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
        // the cut of pair_counts.hip: about 8192 wavefronts, rows in pieces of whole kilobytes when there are fewer
        const size_t steps = (groups + 63) / 64;
        const size_t nseg = std::min(steps, std::max<size_t>(1, 8192 / k));
        const size_t seg = (steps + nseg - 1) / nseg * 64;
        const size_t nseg_used = (groups + seg - 1) / seg;
        const size_t blocks = (k * nseg_used + 3) / 4;
        if (blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ordinal_tables: too many markers for one launch");
        timer.begin();
        hipLaunchKernelGGL(ordinal_table_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bed_k, clb, k, e->pc_masks.as<uint4>(),
                           groups, q, spec.nlev, seg, nseg_used, mxo_d);
        timer.end();
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, hipMemcpyAsync(mxo_tab_host, mxo_d, sizeof(int) * mxo_cells, hipMemcpyDeviceToHost, s));
    }
    if (oxo_tab_host)
    {
        if (q * q * kOrdLevels > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_ordinal_tables: too many ordinal traits for one launch");
        hipLaunchKernelGGL(ordinal_trait_table_kernel, dim3((unsigned)(q * q * kOrdLevels)), dim3(256), 0, s, e->pc_masks.as<uint4>(),
                           groups, q, spec.nlev, oxo_d);
        CUSK_HIP(e, hipGetLastError());
        CUSK_HIP(e, hipMemcpyAsync(oxo_tab_host, oxo_d, sizeof(int) * oxo_cells, hipMemcpyDeviceToHost, s));
    }
    CUSK_HIP(e, hipStreamSynchronize(s));
    if (mxo_tab_host) e->ord_ms[0] = timer.ms();
    return CUSK_OK;
}

static int polychoric_fit_impl(cusk_engine *e, const int *tables, size_t ntab, int ka, int kb, double *r_out, double *se_out,
                               int *status_out)
{
    if (!e || !tables || !r_out || !se_out || !status_out || ntab == 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (ka < 1 || kb < 1 || ka > kOrdLevels || kb > kOrdLevels)
        return fail(e, CUSK_ERR_ARG, "cusk_polychoric_fit: a table has between 1 and 8 rows and columns");
    const size_t blocks = (ntab + 255) / 256;
    if (blocks > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_polychoric_fit: too many tables for one launch");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const size_t cells = ntab * (size_t)(ka * kb);
    ScopedDevBuf tab_buf, out_buf;
    const int *tab_d = tables;
    if (!is_device_pointer(tables))
    {
        if (cells > 0)
            for (size_t i = 0; i < cells; i++)
                if (tables[i] < 0) return fail(e, CUSK_ERR_ARG, "cusk_polychoric_fit: negative count");
        CUSK_HIP(e, tab_buf.ensure(sizeof(int) * cells));
        CUSK_HIP(e, hipMemcpyAsync(tab_buf.p, tables, sizeof(int) * cells, hipMemcpyHostToDevice, s));
        tab_d = tab_buf.as<int>();
    }
    CUSK_HIP(e, out_buf.ensure((2 * sizeof(double) + sizeof(int)) * ntab));
    double *r_d = out_buf.as<double>(), *se_d = r_d + ntab;
    int *st_d = reinterpret_cast<int *>(se_d + ntab);
    LaunchTimer timer(s);
    timer.begin();
    hipLaunchKernelGGL(polychoric_fit_kernel, dim3((unsigned)blocks), dim3(256), 0, s, tab_d, ntab, ka, kb, r_d, se_d, st_d);
    timer.end();
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(r_out, r_d, sizeof(double) * ntab, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(se_out, se_d, sizeof(double) * ntab, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(status_out, st_d, sizeof(int) * ntab, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    e->ord_ms[1] = timer.ms();
    return CUSK_OK;
}

static int polyserial_fit_impl(cusk_engine *e, const float *phen, size_t N, size_t p, const int *cont_ix, size_t nc, const int *ord_ix,
                               size_t q, const float *levels, const int *nlev, double *r_out, double *se_out, int *status_out)
{
    if (!e || !phen || !cont_ix || !r_out || !se_out || !status_out || N == 0 || p == 0 || nc == 0)
        return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (const int rc = check_ordinal_spec(e, "cusk_polyserial_fit", p, ord_ix, q, levels, nlev)) return rc;
    for (size_t c = 0; c < nc; c++)
        if (cont_ix[c] < 0 || (size_t)cont_ix[c] >= p) return fail(e, CUSK_ERR_ARG, "cusk_polyserial_fit: trait index out of range");
    const size_t pairs = nc * q;
    if (pairs > (size_t)0x7fffffff) return fail(e, CUSK_ERR_ARG, "cusk_polyserial_fit: too many pairs for one launch");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const float *phen_d = phen;
    if (!is_device_pointer(phen))
    {
        CUSK_HIP(e, e->phen_dev.ensure(sizeof(float) * p * N));
        CUSK_HIP(e, hipMemcpyAsync(e->phen_dev.p, phen, sizeof(float) * p * N, hipMemcpyHostToDevice, s));
        phen_d = e->phen_dev.as<float>();
    }
    SpecOnDevice spec;
    CUSK_HIP(e, spec.upload(ord_ix, q, levels, nlev, s));
    ScopedDevBuf cont_buf, out_buf;
    CUSK_HIP(e, cont_buf.ensure(sizeof(int) * nc));
    CUSK_HIP(e, hipMemcpyAsync(cont_buf.p, cont_ix, sizeof(int) * nc, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, out_buf.ensure((2 * sizeof(double) + sizeof(int)) * pairs));
    double *r_d = out_buf.as<double>(), *se_d = r_d + pairs;
    int *st_d = reinterpret_cast<int *>(se_d + pairs);
    LaunchTimer timer(s);
    timer.begin();
    hipLaunchKernelGGL(polyserial_fit_kernel, dim3((unsigned)pairs), dim3(256), 0, s, phen_d, N, cont_buf.as<int>(), spec.ord_ix, q,
                       spec.levels, spec.nlev, r_d, se_d, st_d);
    timer.end();
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipMemcpyAsync(r_out, r_d, sizeof(double) * pairs, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(se_out, se_d, sizeof(double) * pairs, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(status_out, st_d, sizeof(int) * pairs, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    e->ord_ms[2] = timer.ms();
    return CUSK_OK;
}

static int matrix_set_cross_impl(cusk_engine *e, float *M_dev, size_t n, size_t idx, const float *vals_host)
{
    if (!e || !M_dev || !vals_host || n == 0 || idx >= n) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (!is_device_pointer(M_dev)) return fail(e, CUSK_ERR_ARG, "cusk_matrix_set_cross: the matrix must be device-resident");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    ScopedDevBuf v;
    CUSK_HIP(e, v.ensure(sizeof(float) * n));
    CUSK_HIP(e, hipMemcpyAsync(v.p, vals_host, sizeof(float) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(set_cross_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, M_dev, n, idx, v.as<float>());
    CUSK_HIP(e, hipGetLastError());
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_ordinal_tables(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                                   size_t m_total, size_t N, size_t p, const int *ord_ix, size_t q, const float *levels,
                                   const int *nlev, int *mxo_tab_host, int *oxo_tab_host)
{
    return cusk::ordinal_tables_impl(e, bed, phen, marker_ix, k, m_total, N, p, ord_ix, q, levels, nlev, mxo_tab_host, oxo_tab_host);
}

extern "C" int cusk_polychoric_fit(cusk_engine *e, const int *tables, size_t ntab, int ka, int kb, double *r_out, double *se_out,
                                   int *status_out)
{
    return cusk::polychoric_fit_impl(e, tables, ntab, ka, kb, r_out, se_out, status_out);
}

extern "C" int cusk_polyserial_fit(cusk_engine *e, const float *phen, size_t N, size_t p, const int *cont_ix, size_t nc,
                                   const int *ord_ix, size_t q, const float *levels, const int *nlev, double *r_out, double *se_out,
                                   int *status_out)
{
    return cusk::polyserial_fit_impl(e, phen, N, p, cont_ix, nc, ord_ix, q, levels, nlev, r_out, se_out, status_out);
}

extern "C" int cusk_matrix_set_cross(cusk_engine *e, float *M_dev, size_t n, size_t idx, const float *vals_host)
{
    return cusk::matrix_set_cross_impl(e, M_dev, n, idx, vals_host);
}

extern "C" void cusk_ordinal_timing(const cusk_engine *e, float *ms3)
{
    for (int i = 0; i < 3; i++) ms3[i] = e ? e->ord_ms[i] : 0.0f;
}
