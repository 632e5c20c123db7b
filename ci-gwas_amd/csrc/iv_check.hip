// iv_check.hip -- conditional-independence tests of the instrument filter (`check-ivs`) for a batch of items.
//
// Reference: cusk_postprocessing/check_mr_assumptions.py:14-26 (_indep).  A test of (x, y | S) inverts the correlation
// sub-matrix over [x, y] + S with np.linalg.inv, takes rho = -m01 / sqrt(|m00 m11|), z = |0.5 log|(1 + rho)/(1 - rho)||
// and calls the pair independent when z < norm.ppf(1 - alpha/2) / sqrt(N - |S| - 3).  check_ivs (:57-116) does that once
// per (outcome, candidate SNP) with S = every other valid trait: O(|S|^3) flops per SNP in Python.
//
// S is the same for every SNP of an outcome, so here the set is factored once: with W = C[S,S]^-1 the 2 x 2 Schur
// complement of S in [x, y] + S is
//     d_xx = 1 - c_xS' W c_xS      d_yy = 1 - c_yS' W c_yS      d_xy = c_xy - c_xS' W c_yS
// and rho = d_xy / sqrt(|d_xx d_yy|) is the reference's partial correlation up to the sign that its outer abs removes.
//   iv_setup_kernel   one workgroup per set that an item names, one launch per size class: Gauss-Jordan inverse of C[S,S] in LDS, in double, with partial pivoting
//                     (pairwise-complete trait correlations need not be positive definite; np.linalg.inv does not care
//                     either).  An exactly zero pivot column marks the set singular (status 2).  The symmetric part of
//                     W goes to a per-set packed lower triangle in global memory.
//   iv_item_kernel    one wavefront per tile of at most 64 items of one (set, y): W (packed) and the tile's rows c_xS
//                     (row stride odd) in LDS; w_y = W c_yS and d_yy once per workgroup; each lane owns one x.  W is read
//                     at a wave-uniform address (broadcast), the lane's row at stride `ld` doubles (conflict free).
// Everything is IEEE double, -ffp-contract=off like the rest of the library; a NaN z or threshold compares false:
// "dependent".
//
// HET (cusk_iv_check_het): the threshold of a test over V = {x, y} + S, |S| = l, is q / sqrt(mean - l - 3) with mean =
// (64-bit sum of the sizes of all (l + 2)(l + 1) / 2 unordered pairs of V) / that count -- het_thr of sepselect.hip.  The
// pairs inside S + {y} are summed once per workgroup, the lane adds its x's l + 1 sizes.
#include "cusk_internal.h"
#include "host/iv_plan.h"

#include <cmath>
#include <string>
#include <vector>

namespace cusk {

namespace {

struct IvBatch
{
    const double *tc;        // n x p: corr[v, t]
    int p;
    const int *set_off;      // nsets + 1
    const int *set;          // trait ids
    double *w;               // packed lower triangles of the W's
    const long long *w_off;  // nsets + 1
    int *set_status;         // 0 ok, 2 singular
    const int *setup_sets;   // the sets of this set-up launch
    const IvTile *tiles;
    const int *xs;           // x of the item at a sorted position
    const int *order;        // sorted position -> index into z / flags
    const double *thr;       // thr[l]; not read in HET mode
    const int *tn;           // HET: n x p sample sizes, layout of tc
    double q;                // HET: norm.ppf(1 - alpha / 2)
    double *z;
    int *flags;
};

__device__ __forceinline__ double iv_abs_fisher_z(double r) { return fabs(0.5 * log(fabs((1.0 + r) / (1.0 - r)))); }

// q / sqrt(mean - l - 3): the rule of het_thr in sepselect.hip, same arithmetic
__device__ __forceinline__ double iv_het_thr(double q, long long nsum, int l)
{
    const double mean = (double)nsum / (double)((l + 2) * (l + 1) / 2);
    return q / sqrt(mean - (double)l - 3.0);
}

// LDS carve (doubles): A[cap * (cap|1)], f[cap], rk[cap]; then ints perm[cap], ids[cap]
size_t iv_setup_bytes(int cap) { return sizeof(double) * ((size_t)cap * (cap | 1) + 2 * (size_t)cap) + sizeof(int) * 2 * (size_t)cap; }

__global__ void __launch_bounds__(256) iv_setup_kernel(IvBatch b, int cap)
{
    extern __shared__ double s_mem[];
    __shared__ int s_pick;
    const int tid = threadIdx.x, sid = b.setup_sets[blockIdx.x];
    const int o0 = b.set_off[sid];
    const int s = b.set_off[sid + 1] - o0;
    const int ld = cap | 1, p = b.p;  // the host launches non-empty sets only, s <= cap
    double *A = s_mem;
    double *f = A + (size_t)cap * ld;
    double *rk = f + cap;
    int *perm = reinterpret_cast<int *>(rk + cap);
    int *ids = perm + cap;
    for (int k = tid; k < s; k += 256) ids[k] = b.set[o0 + k];
    __syncthreads();
    for (int e = tid; e < s * s; e += 256)
    {
        const int a = e / s, c = e - a * s;
        A[a * ld + c] = b.tc[(size_t)ids[a] * p + ids[c]];
    }
    __syncthreads();
    int status = 0;
    for (int k = 0; k < s; k++)
    {
        if (tid < 64)
        {  // the largest |entry| of column k at or below the diagonal; a NaN never wins, all NaN keeps row k
            double best = -1.0;
            int r = k;
            for (int i = k + tid; i < s; i += 64)
            {
                const double v = fabs(A[i * ld + k]);
                if (v > best)
                {
                    best = v;
                    r = i;
                }
            }
            for (int o = 32; o > 0; o >>= 1)
            {
                const double ob = __shfl_xor(best, o);
                const int orow = __shfl_xor(r, o);
                if (ob > best || (ob == best && orow < r))
                {
                    best = ob;
                    r = orow;
                }
            }
            if (tid == 0) s_pick = (best == 0.0) ? -1 : r;
        }
        __syncthreads();
        const int r = s_pick;
        if (r < 0)
        {
            status = 2;
            break;
        }
        if (r != k)
            for (int j = tid; j < s; j += 256)
            {
                const double t = A[k * ld + j];
                A[k * ld + j] = A[r * ld + j];
                A[r * ld + j] = t;
            }
        if (tid == 0) perm[k] = r;
        __syncthreads();
        const double piv = A[k * ld + k];
        for (int i = tid; i < s; i += 256)
        {  // the factor is formed before the product, so a row equal to the pivot row cancels exactly
            f[i] = (i == k) ? 0.0 : A[i * ld + k] / piv;
            rk[i] = A[k * ld + i];
        }
        __syncthreads();
        for (int e = tid; e < s * s; e += 256)
        {
            const int i = e / s, j = e - i * s;
            double v;
            if (i != k)
                v = (j != k) ? A[i * ld + j] - f[i] * rk[j] : -f[i];
            else
                v = (j != k) ? rk[j] / piv : 1.0 / piv;
            A[i * ld + j] = v;
        }
        __syncthreads();
    }
    if (status == 0)
    {  // rows were exchanged, so the columns of the result are: undo in reverse
        for (int k = s - 1; k >= 0; k--)
        {
            const int c = perm[k];
            if (c != k)
            {
                for (int i = tid; i < s; i += 256)
                {
                    const double t = A[i * ld + k];
                    A[i * ld + k] = A[i * ld + c];
                    A[i * ld + c] = t;
                }
                __syncthreads();
            }
        }
        double *W = b.w + b.w_off[sid];
        for (int e = tid; e < s * s; e += 256)
        {
            const int i = e / s, j = e - i * s;
            if (j <= i) W[i * (i + 1) / 2 + j] = 0.5 * (A[i * ld + j] + A[j * ld + i]);
        }
    }
    if (tid == 0) b.set_status[sid] = status;
}

// LDS carve (doubles): W[cap (cap + 1) / 2], X[kIvTile * (cap|1)], cy[cap], wy[cap]; then ints ids[cap]
//   cap   8: 4.9 KB    16: 9.9 KB    32: 21.3 KB    64: 50.0 KB    127: 129.5 KB  (limit 160 KB per workgroup)
size_t iv_item_bytes(int cap)
{
    return sizeof(double) * ((size_t)cap * (cap + 1) / 2 + (size_t)kIvTile * (cap | 1) + 2 * (size_t)cap) + sizeof(int) * (size_t)cap;
}

template <bool HET>
__global__ void __launch_bounds__(kIvTile) iv_item_kernel(IvBatch b, int cap)
{
    extern __shared__ double s_mem[];
    const int lane = threadIdx.x;
    const IvTile t = b.tiles[blockIdx.x];
    const int ld = cap | 1, p = b.p;
    double *W = s_mem;
    double *X = W + (size_t)cap * (cap + 1) / 2;
    double *cy = X + (size_t)kIvTile * ld;
    double *wy = cy + cap;
    int *ids = reinterpret_cast<int *>(wy + cap);
    int s = 0, o0 = 0;
    if (t.set >= 0)
    {
        o0 = b.set_off[t.set];
        s = b.set_off[t.set + 1] - o0;
    }
    const bool active = lane < t.count;
    const int pos = t.start + (active ? lane : 0);  // idle lanes shadow the first item and store nothing
    const int x = b.xs[pos], y = t.y;
    const int out = b.order[pos];
    if (s > 0 && b.set_status[t.set] != 0)
    {
        if (active)
        {
            b.z[out] = NAN;
            b.flags[out] = b.set_status[t.set] << 8;
        }
        return;
    }
    if (s > 0)
    {
        for (int k = lane; k < s; k += kIvTile)
        {
            const int tk = b.set[o0 + k];
            ids[k] = tk;
            cy[k] = b.tc[(size_t)y * p + tk];
        }
        const double *Wg = b.w + b.w_off[t.set];
        for (int e = lane; e < s * (s + 1) / 2; e += kIvTile) W[e] = Wg[e];
        __syncthreads();
        if (s >= 32)
        {  // a row at a time, the lanes along the set: neighbouring addresses
            for (int l = 0; l < t.count; l++)
            {
                const size_t row = (size_t)b.xs[t.start + l] * p;
                for (int j = lane; j < s; j += kIvTile) X[l * ld + j] = b.tc[row + ids[j]];
            }
        }
        else
        {
            for (int j = 0; j < s; j++) X[lane * ld + j] = b.tc[(size_t)x * p + ids[j]];
        }
        // w_y = W c_yS
        for (int i = lane; i < s; i += kIvTile)
        {
            double acc = 0.0;
            const int ri = i * (i + 1) / 2;
            for (int j = 0; j <= i; j++) acc += W[ri + j] * cy[j];
            for (int j = i + 1; j < s; j++) acc += W[j * (j + 1) / 2 + i] * cy[j];
            wy[i] = acc;
        }
        __syncthreads();
    }
    double dyy = 0.0;
    for (int j = 0; j < s; j++) dyy += cy[j] * wy[j];
    dyy = 1.0 - dyy;
    const double *xr = X + lane * ld;
    double sxy = 0.0, quad = 0.0;
    for (int i = 0; i < s; i++)
    {
        const double ci = xr[i];
        const double *wr = W + i * (i + 1) / 2;
        double acc = 0.0;
        for (int j = 0; j < i; j++) acc += wr[j] * xr[j];
        sxy += ci * wy[i];
        quad += ci * (wr[i] * ci + 2.0 * acc);
    }
    const double cxy = (y < p) ? b.tc[(size_t)x * p + y] : b.tc[(size_t)y * p + x];
    const double dxy = cxy - sxy, dxx = 1.0 - quad;
    const double z = iv_abs_fisher_z(dxy / sqrt(fabs(dxx * dyy)));
    double thr;
    if constexpr (HET)
    {
        long long nsum = 0;  // sizes of the pairs inside S + {y}: the same for every lane
        for (int a = lane; a < s; a += kIvTile)
        {
            nsum += b.tn[(size_t)y * p + ids[a]];
            for (int c = 0; c < a; c++) nsum += b.tn[(size_t)ids[a] * p + ids[c]];
        }
        for (int o = 32; o > 0; o >>= 1) nsum += __shfl_xor(nsum, o);
        nsum += (y < p) ? b.tn[(size_t)x * p + y] : b.tn[(size_t)y * p + x];
        for (int a = 0; a < s; a++) nsum += b.tn[(size_t)x * p + ids[a]];
        thr = iv_het_thr(b.q, nsum, s);
    }
    else
        thr = b.thr[s];
    if (active)
    {
        b.z[out] = z;
        b.flags[out] = (z < thr) ? 1 : 0;
    }
}

}  // namespace

static int iv_check_impl(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off, const int *set,
                  long long nitems, const int *item_x, const int *item_y, const int *item_set, const double *thr, bool het,
                  const int *trait_n, double q, double *z, int *flags, float *kernel_ms)
{
    const std::string who = het ? "cusk_iv_check_het" : "cusk_iv_check";
    if (!e) return CUSK_ERR_ARG;
    if (!trait_corr || (het ? !trait_n : !thr) || (nitems > 0 && (!z || !flags)))
        return fail(e, CUSK_ERR_ARG, who + ": bad arguments");
    IvPlan plan;
    std::string msg;
    if (iv_plan_build(n, p, nsets, set_off, set, nitems, item_x, item_y, item_set, plan, msg))
        return fail(e, CUSK_ERR_ARG, who + ": " + msg);
    if (het)
        for (int a = 0; a < p; a++)
            for (int c = a + 1; c < p; c++)
                if (trait_n[(size_t)a * p + c] != trait_n[(size_t)c * p + a])
                    return fail(e, CUSK_ERR_ARG, who + ": trait_n is not symmetric on the trait x trait block");
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nitems == 0) return CUSK_OK;

    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = e->stream;
    // every return below, the error ones included, gives the buffers and events back
    ScopedDevBuf d_tc, d_off, d_set, d_w, d_woff, d_status, d_slist, d_tiles, d_xs, d_order, d_thr, d_tn, d_z, d_flags;
    ScopedEvents<2> evs;
    const int zero_off[1] = {0};
    const size_t nset_ids = nsets ? (size_t)set_off[nsets] : 0;
    CUSK_HIP(e, upload_async(d_tc, trait_corr, sizeof(double) * (size_t)n * p, s));
    CUSK_HIP(e, upload_async(d_off, nsets ? set_off : zero_off, sizeof(int) * ((size_t)nsets + 1), s));
    CUSK_HIP(e, upload_async(d_set, set, sizeof(int) * nset_ids, s));
    CUSK_HIP(e, upload_async(d_woff, plan.w_off.data(), sizeof(long long) * plan.w_off.size(), s));
    CUSK_HIP(e, upload_async(d_slist, plan.setup_sets.data(), sizeof(int) * plan.setup_sets.size(), s));
    CUSK_HIP(e, upload_async(d_tiles, plan.tiles.data(), sizeof(IvTile) * plan.tiles.size(), s));
    CUSK_HIP(e, upload_async(d_xs, plan.xs.data(), sizeof(int) * plan.xs.size(), s));
    CUSK_HIP(e, upload_async(d_order, plan.order.data(), sizeof(int) * plan.order.size(), s));
    if (het)
        CUSK_HIP(e, upload_async(d_tn, trait_n, sizeof(int) * (size_t)n * p, s));
    else  // thr[l] is read for l = a set's length, and a set an item uses leaves out the item's trait: l <= p - 1
        CUSK_HIP(e, upload_async(d_thr, thr, sizeof(double) * (size_t)std::min(plan.max_len + 1, p), s));
    CUSK_HIP(e, d_w.ensure(std::max<size_t>(sizeof(double) * (size_t)plan.w_off.back(), 8)));
    CUSK_HIP(e, d_status.ensure(sizeof(int) * ((size_t)nsets + 1)));
    CUSK_HIP(e, d_z.ensure(sizeof(double) * (size_t)nitems));
    CUSK_HIP(e, d_flags.ensure(sizeof(int) * (size_t)nitems));

    IvBatch b;
    b.tc = d_tc.as<double>();
    b.p = p;
    b.set_off = d_off.as<int>();
    b.set = d_set.as<int>();
    b.w = d_w.as<double>();
    b.w_off = d_woff.as<long long>();
    b.set_status = d_status.as<int>();
    b.tiles = d_tiles.as<IvTile>();
    b.xs = d_xs.as<int>();
    b.order = d_order.as<int>();
    b.thr = d_thr.as<double>();
    b.tn = d_tn.as<int>();
    b.q = q;
    b.z = d_z.as<double>();
    b.flags = d_flags.as<int>();
    void (*const k_item)(IvBatch, int) = het ? iv_item_kernel<true> : iv_item_kernel<false>;
    CUSK_HIP(e, evs.record(0, s));
    for (int c = 0; c < kIvClasses; c++)
    {  // LDS sized to the class (127: 129.0 KB), so a one-trait set never takes the carve of the longest one
        const size_t cnt = plan.setup_first[c + 1] - plan.setup_first[c];
        if (cnt == 0) continue;
        const size_t lds = iv_setup_bytes(kIvCaps[c]);
        if (lds > 48 * 1024)
            CUSK_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(iv_setup_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        b.setup_sets = d_slist.as<int>() + plan.setup_first[c];
        hipLaunchKernelGGL(iv_setup_kernel, dim3((unsigned)cnt), dim3(256), lds, s, b, kIvCaps[c]);
        CUSK_HIP(e, hipGetLastError());
    }
    for (int c = 0; c < kIvClasses; c++)
    {
        const size_t cnt = plan.class_first[c + 1] - plan.class_first[c];
        if (cnt == 0) continue;
        const size_t lds = iv_item_bytes(kIvCaps[c]);
        if (lds > 48 * 1024)
            CUSK_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void *>(k_item), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds));
        b.tiles = d_tiles.as<IvTile>() + plan.class_first[c];
        hipLaunchKernelGGL(k_item, dim3((unsigned)cnt), dim3(kIvTile), lds, s, b, kIvCaps[c]);
        CUSK_HIP(e, hipGetLastError());
    }
    CUSK_HIP(e, evs.record(1, s));
    CUSK_HIP(e, hipMemcpyAsync(z, d_z.p, sizeof(double) * (size_t)nitems, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipMemcpyAsync(flags, d_flags.p, sizeof(int) * (size_t)nitems, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    float ms = 0.0f;
    CUSK_HIP(e, evs.elapsed(&ms, 0, 1));
    if (kernel_ms) *kernel_ms = ms;
    return CUSK_OK;
}

}  // namespace cusk

extern "C" int cusk_iv_check(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off,
                             const int *set, long long nitems, const int *item_x, const int *item_y, const int *item_set,
                             const double *thr, double *z, int *flags, float *kernel_ms)
{
    return cusk::iv_check_impl(e, trait_corr, n, p, nsets, set_off, set, nitems, item_x, item_y, item_set, thr, false, nullptr,
                               0.0, z, flags, kernel_ms);
}

extern "C" int cusk_iv_check_het(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off,
                                 const int *set, long long nitems, const int *item_x, const int *item_y, const int *item_set,
                                 const int *trait_n, double q, double *z, int *flags, float *kernel_ms)
{
    return cusk::iv_check_impl(e, trait_corr, n, p, nsets, set_off, set, nitems, item_x, item_y, item_set, nullptr, true, trait_n,
                               q, z, flags, kernel_ms);
}
