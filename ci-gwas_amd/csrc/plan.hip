// plan.hip -- bitmap -> CSR compaction (degrees, neighbour lists) and the level's work plan.
// Replaces the reference's scan_compact (cusk/src/cuPC-S.cu:6355-6432).
#include "sweep_common.h"

namespace cusk {

// ---------------------------------------------------------------------------
// compaction: bitmap -> CSR neighbour lists + work list
// ---------------------------------------------------------------------------

// degrees after level 0; the same pass leaves the level-0 copy of the bitmap (adj0: record slots, pMax) when asked to
__global__ void degree_kernel(const unsigned long long *__restrict__ adj, int *deg, int n, int words, unsigned long long *adj0)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    int d = 0;
    for (int w = lane; w < words; w += 64)
    {
        const unsigned long long v = adj[(size_t)row * words + w];
        if (adj0) adj0[(size_t)row * words + w] = v;
        d += __popcll(v);
    }
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (lane == 0) deg[row] = d;
}

hipError_t launch_degree(const unsigned long long *adj, int *deg, int n, int words, unsigned long long *adj0, hipStream_t st)
{
    hipLaunchKernelGGL(degree_kernel, dim3((n + 3) / 4), dim3(256), 0, st, adj, deg, n, words, adj0);
    return hipGetLastError();
}

// one wave per row: ascending neighbour indices, reset of the row's selection state
__global__ void fill_nbr_kernel(const unsigned long long *__restrict__ adj, const int *__restrict__ off, int *nbr,
                                unsigned long long *best, int n, int words, int *wpre, const LevelCounters *cnt,
                                const int2 *__restrict__ row_range)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n || !cnt->active) return;
    const int o0 = off[row];
    int run = 0;
    // batched runs: only the words of the row's own block can hold neighbours
    int w_begin = 0, w_end = words;
    if (row_range)
    {
        const int2 rg = row_range[row];
        w_begin = rg.x >> 6;
        w_end = (rg.y > rg.x) ? ((rg.y + 63) >> 6) : w_begin;
    }
    for (int w0 = w_begin; w0 < w_end; w0 += 64)
    {
        const int w = w0 + lane;
        unsigned long long bits = (w < w_end) ? adj[(size_t)row * words + w] : 0ull;
        const int c = __popcll(bits);
        int incl = c;
        for (int o = 1; o < 64; o <<= 1)
        {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        int pos = o0 + run + incl - c;
        // list position of the word's first neighbour: lets anyone turn (row, column) into a list position with
        // one more popcount (level1_prep_kernel)
        if (wpre && w < w_end) wpre[(size_t)row * words + w] = run + incl - c;
        while (bits)
        {
            const int b = __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            if (best) best[pos] = kNone;
            nbr[pos++] = w * 64 + b;
        }
        run += __shfl(incl, 63);
    }
}

hipError_t launch_fill_nbr(const unsigned long long *adj, const int *off, int *nbr, unsigned long long *best, int n, int words,
                           int *wpre, const LevelCounters *cnt, const int2 *row_range, hipStream_t st)
{
    hipLaunchKernelGGL(fill_nbr_kernel, dim3((n + 3) / 4), dim3(256), 0, st, adj, off, nbr, best, n, words, wpre, cnt, row_range);
    return hipGetLastError();
}

// Exclusive prefix of in[0..n) for the 256 rows of this workgroup, without a second kernel and without atomics:
// the workgroup first sums everything that lies before its block (redundantly with its peers: block b reads 256 b
// values, 40 loads per thread at 10k rows), then scans its own 256 values.  Returns the thread's exclusive prefix;
// *block_total receives the sum over the workgroup's own rows.  s_red: 8 long longs of LDS.
__device__ __forceinline__ long long prefix_256(const int *__restrict__ in, int n, int v, long long *s_red, long long *block_total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = blockIdx.x * 256;
    long long before = 0;
    for (int i0 = 0; i0 < first; i0 += 256 * 16)
    {  // sixteen independent loads in flight per thread
        int t[16];
#pragma unroll
        for (int u = 0; u < 16; u++)
        {
            const int i = i0 + u * 256 + tid;
            t[u] = (i < first) ? in[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 16; u++) before += t[u];
    }
    int incl = v;
    for (int o = 1; o < 64; o <<= 1)
    {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 63) s_red[wave] = incl;
    if (lane == 0) s_red[4 + wave] = before;
    __syncthreads();
    long long pre = s_red[4] + s_red[5] + s_red[6] + s_red[7];
    for (int w = 0; w < wave; w++) pre += s_red[w];
    *block_total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    (void)n;
    return pre + incl - v;
}

// The level's work plan, from the degrees alone (so it runs before the neighbour lists are even written): CSR offsets,
// class and work-item count of every row, the work items themselves, level totals, and the level's gate.  256 rows per
// workgroup.
//
// Round 2, second form: no same-address atomics.  The first form placed a workgroup's items with one returning atomicAdd
// per class, took the maximum degree with an atomicMax and found the last workgroup with a ticket counter: three to seven
// device-scope atomics on the same few addresses from every workgroup, which serialise at ~0.3-0.5 us each across the
// XCDs -- 18-23 us per level for a kernel that moves 40 KB.  Now every workgroup PUBLISHES its block totals (degree sum,
// items per class, maximum degree) as self-validating 64-bit words, (sequence number << 40) | value, written with
// agent-scope stores, and reads the words of the blocks before it (spinning on a word until it carries this launch's
// sequence number: no fence, no flag).  Exclusive sums over the earlier blocks give the CSR offsets and the placement
// of the items -- in row order, so the item lists are deterministic -- and the LAST block, which has seen every other
// block's totals, closes or opens the gate.  Forward progress: a workgroup only waits for workgroups with a smaller
// index, which the dispatcher starts first and which never wait for a larger one.
constexpr int kPlanWords = 8;  // per block: [0] degree sum, [1 .. kNumClasses] items per class, [6] maximum degree, [7] overflow
static_assert(kNumClasses + 1 < 7, "plan words");
constexpr unsigned long long kPlanMask = (1ull << 40) - 1ull;

__global__ void __launch_bounds__(256) plan_kernel(PlanArgs a)
{
    __shared__ long long s_wave[kNumClasses][4];  // (64-bit: 64 hub rows of a deep level can hold more than 2^31 items together)
    __shared__ int s_wdeg[4], s_wmax[4];
    __shared__ long long s_part[4][kPlanWords];
    __shared__ long long s_base[kNumClasses];
    __shared__ int s_cls[256], s_nch[256], s_pos[256];
    __shared__ unsigned long long s_big[4];
    LevelCounters *cnt = a.cnt;
    const int n = a.n, L = a.L;
    // the previous level did not run to completion (the loop ended there, or its recheck queue overflowed and it is
    // going to be redone): nothing of this level may touch the working sets; the gate stays closed (counters are zeroed
    // at run start)
    if (a.prev != nullptr && !level_complete(a.prev, a.prev_qcap))
    {
        if (blockIdx.x == 0 && threadIdx.x == 0)
        {
            HostGate *g = a.gate;
            g->active = 0;
            g->maxdeg = 0;
            g->overflow = 0;
            g->item_overflow = 0;
            g->sym = 0;
            g->total_edges = 0;
            for (int c = 0; c < kNumClasses; c++) g->class_items[c] = 0;
            __threadfence_system();
            *(volatile int *)&g->seq = a.seq;
        }
        return;
    }
    const int tid = threadIdx.x;
    const int row = blockIdx.x * 256 + tid;
    const int lane = tid & 63, wave = tid >> 6;
    int cls = -1, nchunks = 0;
    const int d = (row < n) ? a.deg[row] : 0;
    bool ovf = false;
    if (d > L)
    {
        // work units of the row: conditioning sets, or unordered neighbour pairs for the pair kernel
        const unsigned long long nc = a.pair_mode ? (unsigned long long)d * (d - 1) / 2
                                                  : (L == 1 ? (unsigned long long)d : a.binom[(size_t)d * kBinomStride + a.Lsets]);
        if (nc >= (1ull << 62))
            ovf = true;
        else
        {
            cls = 0;
            while (d > kClassCap[cls]) cls++;
            if (cls >= a.staged_classes) cls = kNumClasses - 1;
            const unsigned long long ch = (cls == 0) ? a.chunk0 : a.chunk;
            if (a.Lsets == L + 1 && L >= 2)
            {  // union-major level (sweep_tmaj.hip): items per end position s of the prefix
                const int np = L - 2;
                long long tot = 0;
                for (int s = np; s <= d - 3; s++)
                {
                    const unsigned long long nP = (np == 0) ? 1ull : a.binom[(size_t)s * kBinomStride + np];
                    const unsigned long long per = (unsigned long long)kThreads * tmaj_prefixes_per_lane(d, s, ch);
                    tot += (long long)((nP + per - 1ull) / per);
                }
                if (tot > (long long)0x7fffffff)
                    ovf = true;  // more work items than a row may have: reported like a binomial overflow
                else
                    nchunks = (int)tot;
            }
            else
            {
                const unsigned long long units = (nc + ch - 1) / ch;
                if (units > 0x7fffffffull)
                    ovf = true;
                else
                    nchunks = (int)units;
            }
            // row-sharded runs: only the owner of a row enumerates it (offsets, totals and the overflow checks are global)
            if (ovf || !(a.shard_world == 1 || row % a.shard_world == a.shard_rank))
            {
                cls = -1;
                nchunks = 0;
            }
        }
    }
    const bool wave_ovf = __ballot(ovf) != 0ull;
    // ---- scans inside the workgroup: degrees, items per class, maximum degree ----
    int dincl = d, dmax = d;
    for (int o = 1; o < 64; o <<= 1)
    {
        const int t = __shfl_up(dincl, o);
        if (lane >= o) dincl += t;
    }
    for (int o = 32; o > 0; o >>= 1) dmax = max(dmax, __shfl_xor(dmax, o));
    if (lane == 63) s_wdeg[wave] = dincl;
    if (lane == 0) s_wmax[wave] = dmax | (wave_ovf ? (1 << 30) : 0);  // bit 30: a row's C(d, l) does not fit 62 bits
    long long excl[kNumClasses];
#pragma unroll
    for (int c = 0; c < kNumClasses; c++)
    {
        const long long mine = (cls == c) ? nchunks : 0;
        long long v = mine;
        for (int o = 1; o < 64; o <<= 1)
        {
            const long long t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        excl[c] = v - mine;
        if (lane == 63) s_wave[c][wave] = v;
    }
    __syncthreads();
    // ---- publish this block's totals ----
    unsigned long long *blk = a.blocks + (size_t)blockIdx.x * kPlanWords;
    const unsigned long long tag = (unsigned long long)a.blk_seq << 40;
    if (tid < kPlanWords)
    {
        unsigned long long v = 0;
        if (tid == 0)
            v = (unsigned long long)((long long)s_wdeg[0] + s_wdeg[1] + s_wdeg[2] + s_wdeg[3]);
        else if (tid <= kNumClasses)
            v = (unsigned long long)(s_wave[tid - 1][0] + s_wave[tid - 1][1] + s_wave[tid - 1][2] + s_wave[tid - 1][3]);
        else if (tid == 6)
            v = (unsigned long long)(max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])) & ~(1 << 30));
        else if (tid == 7)
            v = (unsigned long long)(((s_wmax[0] | s_wmax[1] | s_wmax[2] | s_wmax[3]) >> 30) & 1);
        __hip_atomic_store(&blk[tid], tag | (v & kPlanMask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- totals of the blocks before this one: thread <-> (block j, word w), 32 blocks per round ----
    long long acc = 0;
    {
        const int w = tid & 7;
        for (int j = tid >> 3; j < (int)blockIdx.x; j += 32)
        {
            const unsigned long long *src = a.blocks + (size_t)j * kPlanWords + w;
            unsigned long long x;
            while (((x = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 40) != (unsigned long long)a.blk_seq)
                __builtin_amdgcn_s_sleep(1);
            const long long v = (long long)(x & kPlanMask);
            acc = (w >= 6) ? max(acc, v) : acc + v;
        }
        for (int o = 8; o < 64; o <<= 1)
        {
            const long long t = __shfl_xor(acc, o);
            acc = (w >= 6) ? max(acc, t) : acc + t;
        }
        if (lane < kPlanWords) s_part[wave][lane] = acc;
    }
    __syncthreads();
    long long before[kPlanWords];
#pragma unroll
    for (int w = 0; w < kPlanWords; w++)
    {
        const long long p0 = s_part[0][w], p1 = s_part[1][w], p2 = s_part[2][w], p3 = s_part[3][w];
        before[w] = (w >= 6) ? max(max(p0, p1), max(p2, p3)) : p0 + p1 + p2 + p3;
    }
    // CSR offsets of the level (exclusive prefix of the degrees)
    {
        long long o0 = before[0] + dincl - d;
        for (int w = 0; w < wave; w++) o0 += s_wdeg[w];
        if (row < n) a.off[row] = (int)o0;
    }
    const bool last = (blockIdx.x == gridDim.x - 1);
    long long tot_items[kNumClasses];
#pragma unroll
    for (int c = 0; c < kNumClasses; c++)
    {
        const long long mine = s_wave[c][0] + s_wave[c][1] + s_wave[c][2] + s_wave[c][3];
        tot_items[c] = before[1 + c] + mine;  // through this block (the last block: the level's total)
        if (tid == c) s_base[c] = (tot_items[c] > a.item_cap) ? -1 : before[1 + c];  // would not fit: the host grows the buffers
    }
    __syncthreads();
    // the work items of the workgroup's rows, written cooperatively (a hub row has hundreds of them)
    {
        int pos = -1;
        if (cls >= 0 && s_base[cls] >= 0)
        {  // (the class total fits the buffer here, so every position does)
            long long add = 0;
            for (int w = 0; w < wave; w++) add += s_wave[cls][w];
            long long e = 0;
#pragma unroll
            for (int c = 0; c < kNumClasses; c++)
                if (cls == c) e = excl[c];
            pos = (int)(s_base[cls] + add + e);
        }
        // rows with a single item write it themselves; the few rows with several (hubs: hundreds) are handled by the
        // whole workgroup, found through ballots instead of a walk over all 256 rows
        const bool big = (pos >= 0 && nchunks > 1);
        if (pos >= 0 && nchunks == 1) a.items[cls][pos] = make_int2(row, 0);
        const unsigned long long bm = __ballot(big);
        if (lane == 0) s_big[wave] = bm;
        if (big)
        {
            s_cls[tid] = cls;
            s_nch[tid] = nchunks;
            s_pos[tid] = pos;
        }
        __syncthreads();
        const int row0 = blockIdx.x * 256;
        for (int w = 0; w < 4; w++)
        {
            unsigned long long m = s_big[w];
            while (m)
            {
                const int r = w * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const int nch = s_nch[r];
                int2 *dst = a.items[s_cls[r]] + s_pos[r];
                for (int c = tid; c < nch; c += 256) dst[c] = make_int2(row0 + r, c);
            }
        }
    }
    // ---- the level's totals and gate: the last block has seen every block's words ----
    if (last && tid == 0)
    {
        const long long edges = before[0] + s_wdeg[0] + s_wdeg[1] + s_wdeg[2] + s_wdeg[3];
        const int maxdeg = (int)max(before[6], (long long)(max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])) & ~(1 << 30)));
        a.off[n] = (int)edges;
        const int ovf_all = (before[7] != 0 || (((s_wmax[0] | s_wmax[1] | s_wmax[2] | s_wmax[3]) >> 30) & 1)) ? 1 : 0;
        cnt->overflow = ovf_all;
        bool fits = true;
        HostGate *g = a.gate;
        for (int c = 0; c < kNumClasses; c++)
        {
            fits = fits && (tot_items[c] <= a.item_cap);
            cnt->class_items[c] = tot_items[c];
            g->class_items[c] = tot_items[c];
        }
        const int active = (maxdeg - 1 >= L && ovf_all == 0 && fits) ? 1 : 0;
        cnt->maxdeg = maxdeg;
        cnt->total_edges = edges;
        cnt->item_overflow = fits ? 0 : 1;
        cnt->active = active;
        g->active = active;
        g->maxdeg = maxdeg;
        g->overflow = ovf_all;
        g->item_overflow = fits ? 0 : 1;
        g->sym = a.sym ? *a.sym : 0;
        g->total_edges = edges;
        __threadfence_system();
        *(volatile int *)&g->seq = a.seq;
    }
}

hipError_t launch_plan(const PlanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(plan_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace cusk
