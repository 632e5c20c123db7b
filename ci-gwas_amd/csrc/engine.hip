// engine.hip -- the cusk_* C ABI of the engine: create / destroy, options, the run entry points (each ends in run_levels,
// level_loop.hip), result accessors and gathers.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sweep_common.h"

using namespace cusk;

// ---------------------------------------------------------------------------
// C ABI: engine
// ---------------------------------------------------------------------------

extern "C" int cusk_engine_create(cusk_engine **out, int device, void *stream)
{
    if (!out) return CUSK_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
        std::fprintf(stderr, "libcusk_hip: no HIP device available (this library has no CPU fallback)\n");
        return CUSK_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return CUSK_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return CUSK_ERR_HIP;
    cusk_engine *e = new cusk_engine();
    e->device = device;
    for (int l = 0; l < kLevels; l++) e->ev_k0[l] = e->ev_k1[l] = e->ev_l0[l] = e->ev_l1[l] = nullptr;
    bool ok = true;
    if (stream)
    {
        e->stream = reinterpret_cast<hipStream_t>(stream);
        e->own_stream = false;
    }
    else
    {
        ok = ok && hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess;
        e->own_stream = ok;
    }
    ok = ok && hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&e->stream3, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&e->ev_z, hipEventDisableTiming) == hipSuccess;
    {
        char *hctl = nullptr;
        ok = ok && hipHostMalloc(reinterpret_cast<void **>(&hctl), kCtlBytes) == hipSuccess;
        if (ok)
        {
            e->hcnt = reinterpret_cast<LevelCounters *>(hctl + kCtlCnt);
            e->hslots = reinterpret_cast<unsigned long long *>(hctl + kCtlSlots);
            e->hrec_base = reinterpret_cast<long long *>(hctl + kCtlRecBase);
            e->hcanon = reinterpret_cast<unsigned long long *>(hctl + kCtlCanon);
        }
    }
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&e->hflag), sizeof(int)) == hipSuccess;
    // gate records: the plan kernels store into this pinned, coherent host memory directly
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&e->hgate), sizeof(HostGate) * kLevels, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok)
    {
        std::memset(e->hgate, 0, sizeof(HostGate) * kLevels);
        ok = hipHostGetDevicePointer(reinterpret_cast<void **>(&e->hgate_dev), e->hgate, 0) == hipSuccess;
    }
    for (auto &ev : e->ev_run) ok = ok && hipEventCreate(&ev) == hipSuccess;
    for (auto &ev : e->ev_main) ok = ok && hipEventCreate(&ev) == hipSuccess;
    for (auto &ev : e->ev_corr) ok = ok && hipEventCreate(&ev) == hipSuccess;
    for (int l = 0; l < kLevels; l++)
    {
        ok = ok && hipEventCreate(&e->ev_k0[l]) == hipSuccess && hipEventCreate(&e->ev_k1[l]) == hipSuccess;
        ok = ok && hipEventCreate(&e->ev_l0[l]) == hipSuccess && hipEventCreate(&e->ev_l1[l]) == hipSuccess;
    }
    if (!ok)
    {
        cusk_engine_destroy(e);
        return CUSK_ERR_HIP;
    }
    *out = e;
    // kernel experiments without touching the caller: CUSK_OPTIONS="key=value,key=value" (cusk_engine_set_option pairs)
    if (const char *env = std::getenv("CUSK_OPTIONS"))
    {
        std::string all(env);
        size_t pos = 0;
        while (pos < all.size())
        {
            const size_t end = std::min(all.find(',', pos), all.size());
            const std::string kv = all.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos)
                (void)cusk_engine_set_option(e, kv.substr(0, eq).c_str(), std::atoll(kv.c_str() + eq + 1));
            pos = end + 1;
        }
    }
    return CUSK_OK;
}

extern "C" void cusk_engine_destroy(cusk_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    // every stream is idle before anything they may still use is released (an ahead correlation build on stream3 reads the
    // planes / mxp buffers and writes the pinned landing buffer)
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    if (e->stream3) (void)hipStreamSynchronize(e->stream3);
    for (DevBuf *b : {&e->row_range, &e->row_blk, &e->blk_woff, &e->pxp_dev, &e->corr_tab[0], &e->corr_tab[1], &e->pc_masks, &e->pc_counts, &e->mp_bits})
        b->release();
    for (PinnedBuf *b : {&e->res_pinned, &e->corr_tab_pinned[0], &e->corr_tab_pinned[1], &e->batch_pinned, &e->shard_host}) b->release();
    for (DevBuf *b : {&e->adj, &e->adj0, &e->deg, &e->binom, &e->counters, &e->ti, &e->queue,
                      &e->rv, &e->nv, &e->rpos, &e->sel, &e->wpre, &e->rec_x, &e->rec_y, &e->rec_l, &e->rec_s, &e->den_x, &e->den_y, &e->den_l,
                      &e->den_z, &e->den_s, &e->den_counts, &e->den_off, &e->off1, &e->planblk, &e->scratch_a, &e->scratch_b, &e->bed_dev, &e->phen_dev,
                      &e->mean_dev, &e->std_dev, &e->planes, &e->mxp_dev, &e->mxp_bq})
        b->release();
    for (int k = 0; k < 2; k++)
    {
        for (DevBuf *b : {&e->off[k], &e->nbr[k], &e->best[k]}) b->release();
        for (auto &b : e->items[k]) b.release();
    }
    if (e->hcnt) (void)hipHostFree(e->hcnt);
    if (e->hflag) (void)hipHostFree(e->hflag);
    if (e->hgate) (void)hipHostFree(e->hgate);
    for (hipEvent_t ev : {e->ev_run[0], e->ev_run[1], e->ev_main[0], e->ev_main[1], e->ev_corr[0], e->ev_corr[1], e->ev_corr[2], e->ev_corr[3], e->ev_corr[4]})
        if (ev) (void)hipEventDestroy(ev);
    for (int l = 0; l < kLevels; l++)
        for (hipEvent_t ev : {e->ev_k0[l], e->ev_k1[l], e->ev_l0[l], e->ev_l1[l]})
            if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {e->ev_fork, e->ev_join, e->ev_z, e->ev_mxp})
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev_prune)
        if (ev) (void)hipEventDestroy(ev);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->stream3) (void)hipStreamDestroy(e->stream3);
    e->mxp_pinned.release();
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" int cusk_engine_set_option(cusk_engine *e, const char *key, long long value)
{
    if (!e || !key) return CUSK_ERR_ARG;
    const std::string k(key);
    if (k == "fast")
        e->opt_fast = (int)value;
    else if (k == "validate")
        e->opt_validate = (int)value;
    else if (k == "het_filter")
        e->opt_het_filter = (int)value;
    else if (k == "het_rows" && (value == 0 || value == 1))
        e->opt_het_rows = (int)value;
    else if (k == "corr_fp4")
        e->opt_corr_fp4 = (int)value;
    else if (k == "pair")
        e->opt_pair = (int)value;
    else if (k == "rows")
        e->opt_rows = (int)value;
    else if (k == "vec")
        e->opt_vec = (int)value;
    else if (k == "overlap")
        e->opt_overlap = (int)value;
    else if (k == "corr_popcount")
        e->opt_corr_popcount = (int)value;
    else if (k == "corr_mxp_f32")
        e->opt_corr_mxp_f32 = (int)value;
    else if (k == "assume_symmetric")
        e->opt_assume_symmetric = (int)value;
    else if (k == "queue_capacity" && value > 0)
        e->opt_queue_cap = value;
    else if (k == "chunk" && value >= 256)
        e->opt_chunk = value;
    else if (k == "max_staged_classes")
        e->opt_max_staged_classes = (int)value;
    else if (k == "tmaj_validate_stride" && value >= 1 && (value & (value - 1)) == 0)
        e->opt_tmaj_validate_stride = (int)value;
    else if (k == "tmaj_min_level")
        e->opt_tmaj_min_level = (int)value;
    else if (k == "hostprof")
        e->opt_hostprof = (int)value;
    else if (k == "chunk0_low" && value >= 64)
        e->opt_chunk0_low = value;
    else if (k == "chunk0" && value >= 64)
        e->opt_chunk0 = value;
    else if (k == "vec_threads" && (value == 64 || value == 128 || value == 256))
        e->opt_vec_threads = (int)value;
    else if (k == "item_capacity" && value > 0)
    {
        e->opt_item_cap = value;
        e->item_cap_cur = 0;  // takes effect with the next run (buffers only ever grow)
    }
    else if (k == "lookahead" && value >= 0)
        e->opt_lookahead = (int)value;
    else if (k == "timing")
        e->opt_timing = (int)value;
    else if (k == "l1_threads" && (value == 0 || value == 256 || value == 512))
        e->opt_l1_threads = (int)value;
    else if (k == "l1_lds_row" && (value == 0 || value == 1))
        e->opt_l1_lds_row = (int)value;
    else if (k == "sync2")
        e->opt_sync2 = (int)value;
    else if (k == "sepselect_ws_bytes" && value > 0)
        e->opt_sep_ws_budget = value;
    else if (k == "mvivw_part_bytes" && value > 0)
        e->opt_mvivw_part_bytes = value;
    else if (k == "mvivw_ld_bytes" && value > 0)
        e->opt_mvivw_ld_bytes = value;
    else if (k == "mvivw_jk_bytes" && value > 0)
        e->opt_mvivw_jk_bytes = value;
    else if (k == "phen_rint_bytes" && value > 0)
        e->opt_phen_rint_bytes = value;
    else
        return fail(e, CUSK_ERR_ARG, "unknown option " + k);
    return CUSK_OK;
}

extern "C" int cusk_engine_set_row_shard(cusk_engine *e, int rank, int world, cusk_exchange_fn fn, void *user, int host_staging)
{
    if (!e) return CUSK_ERR_ARG;
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !fn))
        return fail(e, CUSK_ERR_ARG, "cusk_engine_set_row_shard: need 0 <= rank < world and an exchange function");
    e->shard_rank = rank;
    e->shard_world = world;
    e->shard_fn = fn;
    e->shard_user = user;
    e->shard_host_staging = host_staging ? 1 : 0;
    return CUSK_OK;
}

extern "C" const char *cusk_last_error(const cusk_engine *e) { return e ? e->err.c_str() : "no engine"; }
extern "C" void *cusk_engine_stream(const cusk_engine *e) { return e ? (void *)e->stream : nullptr; }
extern "C" int cusk_engine_device(const cusk_engine *e) { return e ? e->device : -1; }
extern "C" int cusk_engine_level1_form(const cusk_engine *e) { return e ? e->level1_form : -1; }
extern "C" int cusk_engine_bind_thread(cusk_engine *e)
{
    if (!e) return CUSK_ERR_ARG;
    CUSK_HIP(e, hipSetDevice(e->device));
    return CUSK_OK;
}

// the arguments of a Skeleton run (mode 0); Ness != nullptr: at per-pair sample sizes, Th[0] = alpha/2 quantile
static RunArgs skeleton_args(const float *C_dev, const float *N_dev, const float *Th, int n, int maxlevel)
{
    RunArgs a{};
    a.C = C_dev;
    a.Ness = N_dev;
    a.Th = Th;
    a.n = n;
    a.maxlevel = maxlevel;
    return a;
}

extern "C" int cusk_run_skeleton(cusk_engine *e, const float *C_dev, int n, const float *Th, int maxlevel,
                                 cusk_stats *stats)
{
    if (!e) return CUSK_ERR_ARG;
    e->batch_lo.clear();
    return run_levels(e, skeleton_args(C_dev, nullptr, Th, n, maxlevel), stats);
}

// what the runs at per-pair sample sizes ask of their arguments and of the engine (`who`: the entry point, for the message)
static int check_het_args(cusk_engine *e, const std::string &who, const float *N_dev)
{
    if (!N_dev) return fail(e, CUSK_ERR_ARG, who + ": needs the sample-size matrix");
    if (e->shard_world > 1)
        return fail(e, CUSK_ERR_ARG, who + ": a row-sharded engine is not supported (per-pair sample sizes run on one engine)");
    if (e->opt_validate && !e->opt_het_filter)
        return fail(e, CUSK_ERR_ARG, who + ": option validate is not supported (every test already runs on the exact path)");
    return CUSK_OK;
}

// the tables of a batched run (checked layout, per-row column range and block number, packed-bitmap offsets: uploaded on the
// engine's stream) and the RunArgs fields that describe the blocks; shared by the batched entry points
static int batch_setup(cusk_engine *e, const char *who, int n, int nblk, const int *lo, const int *hi, RunArgs &a)
{
    int prev = 0, span = 0;
    long long pairs0 = 0;
    for (int b = 0; b < nblk; b++)
    {
        if ((lo[b] & 63) != 0 || lo[b] < prev || hi[b] < lo[b] || hi[b] > n)
            return fail(e, CUSK_ERR_ARG, std::string(who) + ": block bases must be ascending multiples of 64 inside the matrix");
        prev = hi[b];
        span = std::max(span, hi[b] - lo[b]);
        pairs0 += (long long)(hi[b] - lo[b]) * (hi[b] - lo[b] - 1) / 2;
    }
    CUSK_HIP(e, hipSetDevice(e->device));
    // per-row tables: column range of the row's block, block number (-1: padding), and per block the offset of its packed
    // bitmap (cusk_result_adj_bits_blocks)
    const size_t bytes_rr = sizeof(int2) * (size_t)n, bytes_rb = sizeof(int) * (size_t)n, bytes_wo = sizeof(long long) * (size_t)nblk;
    const size_t need = bytes_rr + bytes_rb + bytes_wo;
    CUSK_HIP(e, e->batch_pinned.ensure(need, need + need / 2));
    // the previous run's copies out of this staging buffer have completed: every run ends with a stream synchronisation
    int2 *rr = e->batch_pinned.as<int2>();
    int *rb = reinterpret_cast<int *>(e->batch_pinned.as<char>() + bytes_rr);
    long long *wo = reinterpret_cast<long long *>(e->batch_pinned.as<char>() + bytes_rr + bytes_rb);
    for (int r = 0; r < n; r++)
    {
        rr[r] = make_int2(0, 0);
        rb[r] = -1;
    }
    long long woff = 0;
    for (int b = 0; b < nblk; b++)
    {
        for (int r = lo[b]; r < hi[b]; r++)
        {
            rr[r] = make_int2(lo[b], hi[b]);
            rb[r] = b;
        }
        wo[b] = woff;
        woff += (long long)(hi[b] - lo[b]) * ((hi[b] - lo[b] + 63) / 64);
    }
    CUSK_HIP(e, e->row_range.ensure(bytes_rr));
    CUSK_HIP(e, e->row_blk.ensure(bytes_rb));
    CUSK_HIP(e, e->blk_woff.ensure(bytes_wo));
    CUSK_HIP(e, hipMemcpyAsync(e->row_range.p, rr, bytes_rr, hipMemcpyHostToDevice, e->stream));
    CUSK_HIP(e, hipMemcpyAsync(e->row_blk.p, rb, bytes_rb, hipMemcpyHostToDevice, e->stream));
    CUSK_HIP(e, hipMemcpyAsync(e->blk_woff.p, wo, bytes_wo, hipMemcpyHostToDevice, e->stream));
    e->batch_lo.assign(lo, lo + nblk);
    e->batch_hi.assign(hi, hi + nblk);
    a.row_range = e->row_range.as<int2>();
    a.max_span = span;
    a.level0_pairs = pairs0;
    return CUSK_OK;
}

// Batched Skeleton run: `nblk` independent blocks laid out along the diagonal of one n x n allocation (include/cusk_hip.h).
// One plan / fill / sweep / finalise chain per level serves every block: after level 0 the engine only works on CSR rows,
// and a row never meets a column outside its block, so nothing but level 0 and the level-1 row staging knows about blocks.
extern "C" int cusk_run_skeleton_batch(cusk_engine *e, const float *C_dev, int n, int nblk, const int *lo, const int *hi,
                                       const float *Th, int maxlevel, cusk_stats *stats)
{
    if (!e) return CUSK_ERR_ARG;
    if (!C_dev || !lo || !hi || !Th || n <= 0 || nblk <= 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (e->shard_world > 1) return fail(e, CUSK_ERR_ARG, "batched runs are not row-sharded");
    RunArgs a = skeleton_args(C_dev, nullptr, Th, n, maxlevel);
    int rc = batch_setup(e, "cusk_run_skeleton_batch", n, nblk, lo, hi, a);
    if (rc != CUSK_OK) return rc;
    rc = run_levels(e, a, stats);
    if (rc != CUSK_OK) e->batch_lo.clear();
    return rc;
}

// The batched run at per-pair sample sizes: the het0 plan of run_levels (no vectorised or union-major sweep, no level-1
// row / pair kernels; exact path only unless option het_filter is set) with row_range set -- level 0 by level0_batch_kernel<true>, which
// also writes the level-0 copy and the degrees; from level 1 on the engine works on CSR rows, and the exact sweep reads
// C[a * n + b] and N[a * n + b] at the stride of the allocation, inside the row's own block only.
extern "C" int cusk_run_skeleton_batch_het(cusk_engine *e, const float *C_dev, const float *N_dev, int n, int nblk, const int *lo,
                                           const int *hi, float th, int maxlevel, cusk_stats *stats)
{
    if (!e) return CUSK_ERR_ARG;
    if (!C_dev || !lo || !hi || n <= 0 || nblk <= 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (const int rc = check_het_args(e, "cusk_run_skeleton_batch_het", N_dev)) return rc;
    RunArgs a = skeleton_args(C_dev, N_dev, &th, n, maxlevel);
    int rc = batch_setup(e, "cusk_run_skeleton_batch_het", n, nblk, lo, hi, a);
    if (rc != CUSK_OK) return rc;
    rc = run_levels(e, a, stats);
    if (rc != CUSK_OK) e->batch_lo.clear();
    return rc;
}

// the adjacency of the last batched run, block by block: rows lo..hi-1 of block b, each as the (hi - lo + 63) / 64 words of
// the block's own columns (bit j = local variable j; bases are multiples of 64), blocks back to back
static int pack_blocks(cusk_engine *e, uint64_t *out_host, int tail)
{
    if (!e || !e->have_result || e->batch_lo.empty() || !out_host || tail < 0) return fail(e, CUSK_ERR_STATE, "no batched result");
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t nblk = e->batch_lo.size();
    std::vector<long long> woff(nblk);
    long long total = 0;
    for (size_t b = 0; b < nblk; b++)
    {
        const int k = e->batch_hi[b] - e->batch_lo[b];
        woff[b] = total;
        total += (long long)(tail > 0 ? std::min(tail, k) : k) * ((k + 63) / 64);
    }
    if (total == 0) return CUSK_OK;
    CUSK_HIP(e, e->scratch_b.ensure(sizeof(unsigned long long) * (size_t)total));
    const long long *woff_d = e->blk_woff.as<long long>();  // the full packing's offsets were uploaded with the run
    if (tail > 0)
    {
        CUSK_HIP(e, e->scratch_a.ensure(sizeof(long long) * nblk));
        CUSK_HIP(e, hipMemcpyAsync(e->scratch_a.p, woff.data(), sizeof(long long) * nblk, hipMemcpyHostToDevice, e->stream));
        woff_d = e->scratch_a.as<long long>();
    }
    CUSK_HIP(e, launch_pack_block_bits(e->adj.as<unsigned long long>(), e->n, e->words, e->row_range.as<int2>(), e->row_blk.as<int>(),
                                       woff_d, e->scratch_b.as<unsigned long long>(), tail, e->stream));
    CUSK_HIP(e, hipMemcpyAsync(out_host, e->scratch_b.p, sizeof(unsigned long long) * (size_t)total, hipMemcpyDeviceToHost, e->stream));
    CUSK_HIP(e, hipStreamSynchronize(e->stream));  // (also covers the copy out of `woff`)
    return CUSK_OK;
}

extern "C" int cusk_result_adj_bits_blocks(cusk_engine *e, uint64_t *out_host) { return pack_blocks(e, out_host, 0); }
extern "C" int cusk_result_adj_bits_blocks_tail(cusk_engine *e, int tail_rows, uint64_t *out_host)
{
    if (tail_rows <= 0) return fail(e, CUSK_ERR_ARG, "tail_rows must be positive");
    return pack_blocks(e, out_host, tail_rows);
}

// rows [row0, row0 + nrows) of the last run's adjacency bitmap (cusk_result_words() words each): what the pruning of depth 1
// needs of a 10k-variable block are its trait rows, 25 KB instead of the 12.6 MB bitmap
extern "C" int cusk_result_adj_rows(cusk_engine *e, int row0, int nrows, uint64_t *out_host)
{
    if (!e || !e->have_result || !out_host || row0 < 0 || nrows < 0 || row0 + nrows > e->n) return fail(e, CUSK_ERR_ARG, "bad rows");
    if (nrows == 0) return CUSK_OK;
    CUSK_HIP(e, hipSetDevice(e->device));
    CUSK_HIP(e, hipMemcpyAsync(out_host, e->adj.as<unsigned long long>() + (size_t)row0 * e->words,
                               sizeof(unsigned long long) * (size_t)nrows * e->words, hipMemcpyDeviceToHost, e->stream));
    CUSK_HIP(e, hipStreamSynchronize(e->stream));
    return CUSK_OK;
}

// out[row_out[t] + c] = M[row_src[t] * n + idx[row_first[t] + c]], c < row_k[t], for nrows rows t: the sub-matrices of many
// blocks in one launch (stage-two matrices on the diagonal of a batch allocation: out on the device; the retained
// sub-matrices of the results: out on the host).  All index arrays are host memory.
extern "C" int cusk_gather_rows(cusk_engine *e, const float *M_dev, int n, const int *idx_host, long long nidx, const int *row_src,
                                const int *row_k, const long long *row_first, const long long *row_out, long long nrows,
                                float *out, long long out_count, int out_on_device)
{
    if (!e || !M_dev || !idx_host || !row_src || !row_k || !row_first || !row_out || !out || nrows < 0 || nidx < 0)
        return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (nrows == 0) return CUSK_OK;
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t b_idx = sizeof(int) * (size_t)nidx, b_src = sizeof(int) * (size_t)nrows, b_ll = sizeof(long long) * (size_t)nrows;
    const size_t o_src = (b_idx + 15) & ~(size_t)15, o_k = o_src + ((b_src + 15) & ~(size_t)15), o_first = o_k + ((b_src + 15) & ~(size_t)15),
                 o_out = o_first + b_ll, total = o_out + b_ll;
    CUSK_HIP(e, e->scratch_a.ensure(total));
    char *d = e->scratch_a.as<char>();
    hipStream_t s = e->stream;
    CUSK_HIP(e, hipMemcpyAsync(d, idx_host, b_idx, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(d + o_src, row_src, b_src, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(d + o_k, row_k, b_src, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(d + o_first, row_first, b_ll, hipMemcpyHostToDevice, s));
    CUSK_HIP(e, hipMemcpyAsync(d + o_out, row_out, b_ll, hipMemcpyHostToDevice, s));
    float *dst = out;
    if (!out_on_device)
    {
        CUSK_HIP(e, e->scratch_b.ensure(sizeof(float) * (size_t)out_count));
        dst = e->scratch_b.as<float>();
    }
    CUSK_HIP(e, launch_gather_rows(M_dev, n, reinterpret_cast<const int *>(d), reinterpret_cast<const int *>(d + o_src),
                                   reinterpret_cast<const int *>(d + o_k), reinterpret_cast<const long long *>(d + o_first),
                                   reinterpret_cast<const long long *>(d + o_out), nrows, dst, s));
    if (!out_on_device) CUSK_HIP(e, hipMemcpyAsync(out, dst, sizeof(float) * (size_t)out_count, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));  // the host arrays may go away; the scratch is reused by the next call
    return CUSK_OK;
}

extern "C" int cusk_run_hetcor(cusk_engine *e, const float *C_dev, const float *N_dev, float ess_uniform,
                               const int *G_init_dev, int n, float th, int maxlevel, const int *time_index,
                               cusk_stats *stats)
{
    if (!e) return CUSK_ERR_ARG;
    e->batch_lo.clear();
    RunArgs a{};
    a.mode = 1;
    a.C = C_dev;
    a.Ness = N_dev;
    a.ess_uniform = ess_uniform;
    a.Ginit = G_init_dev;
    float thv[1] = {th};
    a.Th = thv;
    a.time_index = time_index;
    a.n = n;
    a.maxlevel = maxlevel;
    return run_levels(e, a, stats);
}

// Skeleton's outputs (lowest passing rank per slot, separating-set records, pMax) decided at hetcor's per-test thresholds.
// The level loop is Skeleton's; every level runs on the exact path (sweep_exact.hip, MODE 0 / HET).  With option
// het_filter levels >= 2 go through the filter at the per-test threshold (sweep_fast.hip, MODE 0 / HET) and the tests it
// cannot certify through the recheck queue, as in the other modes; levels 0 and 1, the records and pMax are unchanged.
extern "C" int cusk_run_skeleton_het(cusk_engine *e, const float *C_dev, const float *N_dev, int n, float th, int maxlevel,
                                     cusk_stats *stats)
{
    if (!e) return CUSK_ERR_ARG;
    if (const int rc = check_het_args(e, "cusk_run_skeleton_het", N_dev)) return rc;
    e->batch_lo.clear();
    return run_levels(e, skeleton_args(C_dev, N_dev, &th, n, maxlevel), stats);
}

extern "C" int cusk_result_n(const cusk_engine *e) { return (e && e->have_result) ? e->n : 0; }
extern "C" int cusk_result_words(const cusk_engine *e) { return (e && e->have_result) ? e->words : 0; }
extern "C" const uint64_t *cusk_result_adj_bits_dev(const cusk_engine *e)
{
    return (e && e->have_result) ? reinterpret_cast<const uint64_t *>(e->adj.p) : nullptr;
}

extern "C" int cusk_result_adj_i32_dev(cusk_engine *e, int *G_dev)
{
    if (!e || !e->have_result) return fail(e, CUSK_ERR_STATE, "no result");
    CUSK_HIP(e, hipSetDevice(e->device));
    CUSK_HIP(e, launch_expand_adj(e->adj.as<unsigned long long>(), G_dev, e->n, e->words, e->stream));
    CUSK_HIP(e, hipStreamSynchronize(e->stream));
    return CUSK_OK;
}

extern "C" int cusk_result_adj_i32(cusk_engine *e, int *G_host)
{
    if (!e || !e->have_result) return fail(e, CUSK_ERR_STATE, "no result");
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t bytes = sizeof(int) * (size_t)e->n * e->n;
    int *tmp = nullptr;
    CUSK_HIP(e, hipMalloc(reinterpret_cast<void **>(&tmp), bytes));
    int rc = cusk_result_adj_i32_dev(e, tmp);
    if (rc == CUSK_OK)
    {
        hipError_t st = hipMemcpy(G_host, tmp, bytes, hipMemcpyDeviceToHost);
        if (st != hipSuccess) rc = fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
    }
    (void)hipFree(tmp);
    return rc;
}

// Result read-out, off the hot path: the sparse record store (level-1 slots) becomes a dense list ordered by slot,
// i.e. by (x, y); then, when asked for, the winners' exact Fisher z level by level.
static int materialize_records(cusk_engine *e, bool want_z)
{
    hipStream_t s = e->stream;
    if (!e->records_ready)
    {
        e->nrec = 0;
        const long long slots = e->rec_slots;
        if (slots > 0)
        {
            const long long nb = (slots + kRecBlock - 1) / kRecBlock;
            CUSK_HIP(e, e->den_counts.ensure(sizeof(int) * (size_t)nb));
            CUSK_HIP(e, e->den_off.ensure(sizeof(long long) * (size_t)nb));
            CUSK_HIP(e, launch_rec_count(e->rec_l.as<int>(), slots, e->den_counts.as<int>(), s));
            std::vector<int> counts((size_t)nb);
            CUSK_HIP(e, hipMemcpyAsync(counts.data(), e->den_counts.p, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipStreamSynchronize(s));
            std::vector<long long> off((size_t)nb);
            long long tot = 0;
            for (long long b = 0; b < nb; b++)
            {
                off[(size_t)b] = tot;
                tot += counts[(size_t)b];
            }
            e->nrec = tot;
            if (tot > 0)
            {
                CUSK_HIP(e, e->den_x.ensure(sizeof(int) * (size_t)tot));
                CUSK_HIP(e, e->den_y.ensure(sizeof(int) * (size_t)tot));
                CUSK_HIP(e, e->den_l.ensure(sizeof(int) * (size_t)tot));
                CUSK_HIP(e, e->den_z.ensure(sizeof(float) * (size_t)tot));
                CUSK_HIP(e, e->den_s.ensure(sizeof(int) * kML * (size_t)tot));
                e->den_stride = tot;
                CUSK_HIP(e, hipMemcpyAsync(e->den_off.p, off.data(), sizeof(long long) * (size_t)nb, hipMemcpyHostToDevice, s));
                CUSK_HIP(e, launch_rec_compact(e->rec_l.as<int>(), e->rec_x.as<int>(), e->rec_y.as<int>(), e->rec_s.as<int>(),
                                               e->rec_cap, slots, e->den_off.as<long long>(), e->den_x.as<int>(), e->den_y.as<int>(),
                                               e->den_l.as<int>(), e->den_s.as<int>(), e->den_stride, s));
                CUSK_HIP(e, hipStreamSynchronize(s));  // `off` lives on this stack frame
            }
        }
        e->records_ready = true;
        e->z_ready = false;
    }
    if (want_z && !e->z_ready)
    {
        if (e->nrec > 0)
        {
            if (!e->last_C) return fail(e, CUSK_ERR_STATE, "the matrix of the last run is needed for the separating sets' z");
            for (int l = 1; l <= e->last_levels; l++)
                CUSK_HIP(e, launch_record_z(l, e->last_C, e->n, e->den_x.as<int>(), e->den_y.as<int>(), e->den_l.as<int>(),
                                            e->den_s.as<int>(), e->den_stride, e->nrec, e->den_z.as<float>(), s));
            CUSK_HIP(e, hipStreamSynchronize(s));
        }
        e->z_ready = true;
    }
    return CUSK_OK;
}

extern "C" int cusk_result_pmax(cusk_engine *e, const float *C_dev, float *pMax_host)
{
    if (!e || !e->have_result || e->mode != 0) return fail(e, CUSK_ERR_STATE, "no Skeleton result");
    CUSK_HIP(e, hipSetDevice(e->device));
    if (C_dev) e->last_C = C_dev;
    int rc = materialize_records(e, true);
    if (rc != CUSK_OK) return rc;
    const size_t bytes = sizeof(float) * (size_t)e->n * e->n;
    float *tmp = nullptr;
    CUSK_HIP(e, hipMalloc(reinterpret_cast<void **>(&tmp), bytes));
    hipError_t st = launch_expand_pmax(e->adj.as<unsigned long long>(), e->adj0.as<unsigned long long>(), C_dev, tmp, e->n,
                                       e->words, e->den_x.as<int>(), e->den_y.as<int>(), e->den_z.as<float>(), e->nrec,
                                       e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(pMax_host, tmp, bytes, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    (void)hipFree(tmp);
    if (st != hipSuccess) return fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
    return CUSK_OK;
}

// separating sets of all records in the ABI's [nrec x 14] layout
static int records_to_host(cusk_engine *e, int *S_host)
{
    // engine-owned scratch: hipMalloc / hipFree per call would synchronise the whole device (several engines share it)
    const size_t bytes = sizeof(int) * kML * (size_t)e->nrec;
    CUSK_HIP(e, e->scratch_a.ensure(bytes));
    int *tmp = e->scratch_a.as<int>();
    hipError_t st = launch_expand_records(e->den_s.as<int>(), e->den_l.as<int>(), e->den_stride, e->nrec, tmp, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(S_host, tmp, bytes, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    if (st != hipSuccess) return fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
    return CUSK_OK;
}

// device -> host on the engine's stream (waits for that stream only)
static hipError_t fetch(cusk_engine *e, void *dst, const void *src, size_t bytes)
{
    hipError_t st = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    return st;
}

extern "C" int cusk_result_sepset_dense(cusk_engine *e, int *SepSet_host)
{
    if (!e || !e->have_result || e->mode != 0) return fail(e, CUSK_ERR_STATE, "no Skeleton result");
    CUSK_HIP(e, hipSetDevice(e->device));
    int rc = materialize_records(e, false);
    if (rc != CUSK_OK) return rc;
    const size_t count = (size_t)e->n * e->n * kML;
    // the dense n*n*14 array exists only for the reference's ABI; it is filled on the host
    std::fill(SepSet_host, SepSet_host + count, -1);
    if (e->nrec > 0)
    {
        std::vector<int> x(e->nrec), y(e->nrec), S((size_t)e->nrec * kML);
        CUSK_HIP(e, fetch(e, x.data(), e->den_x.p, sizeof(int) * e->nrec));
        CUSK_HIP(e, fetch(e, y.data(), e->den_y.p, sizeof(int) * e->nrec));
        rc = records_to_host(e, S.data());
        if (rc != CUSK_OK) return rc;
        for (long long r = 0; r < e->nrec; r++)
            std::memcpy(SepSet_host + ((size_t)x[r] * e->n + y[r]) * kML, S.data() + (size_t)r * kML, sizeof(int) * kML);
    }
    return CUSK_OK;
}

extern "C" long long cusk_result_sepsets(cusk_engine *e, int *x, int *y, int *level, float *z, int *S)
{
    if (!e || !e->have_result || e->mode != 0) return -1;
    if (hipSetDevice(e->device) != hipSuccess) return -1;
    if (materialize_records(e, z != nullptr) != CUSK_OK) return -1;
    const long long c = e->nrec;
    if (c > 0)
    {
        if (x && fetch(e, x, e->den_x.p, sizeof(int) * c) != hipSuccess) return -1;
        if (y && fetch(e, y, e->den_y.p, sizeof(int) * c) != hipSuccess) return -1;
        if (level && fetch(e, level, e->den_l.p, sizeof(int) * c) != hipSuccess) return -1;
        if (z && fetch(e, z, e->den_z.p, sizeof(float) * c) != hipSuccess) return -1;
        if (S && records_to_host(e, S) != CUSK_OK) return -1;
    }
    return c;
}

// x, y and the members of every record in ENGINE-OWNED PINNED host memory: one expand kernel, three copies, one
// synchronisation (cusk_result_sepsets copies into the caller's pageable arrays, each copy staged and synchronised by the
// runtime); valid until the next run or result call on this engine
extern "C" long long cusk_result_sepsets_view(cusk_engine *e, const int **x, const int **y, const int **S)
{
    if (!e || !e->have_result || e->mode != 0 || !x || !y || !S) return -1;
    if (hipSetDevice(e->device) != hipSuccess) return -1;
    if (materialize_records(e, false) != CUSK_OK) return -1;
    const long long c = e->nrec;
    *x = *y = *S = nullptr;
    if (c <= 0) return c;
    const size_t bx = sizeof(int) * (size_t)c, bs = sizeof(int) * kML * (size_t)c, need = 2 * bx + bs;
    if (e->res_pinned.ensure(need, need + need / 2) != hipSuccess) return -1;
    if (e->scratch_a.ensure(bs) != hipSuccess) return -1;
    int *hx = e->res_pinned.as<int>(), *hy = hx + c, *hs = hy + c;
    hipError_t st = launch_expand_records(e->den_s.as<int>(), e->den_l.as<int>(), e->den_stride, c, e->scratch_a.as<int>(), e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(hx, e->den_x.p, bx, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(hy, e->den_y.p, bx, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(hs, e->scratch_a.p, bs, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    if (st != hipSuccess)
    {
        (void)fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
        return -1;
    }
    *x = hx;
    *y = hy;
    *S = hs;
    return c;
}

extern "C" int cusk_gather_submatrix(cusk_engine *e, const float *M_dev, int n, const int *idx_host, int k, float *out_host)
{
    if (!e || !M_dev || !idx_host || !out_host || k <= 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    CUSK_HIP(e, e->scratch_a.ensure(sizeof(int) * (size_t)k));
    CUSK_HIP(e, e->scratch_b.ensure(sizeof(float) * (size_t)k * k));
    int *idx_d = e->scratch_a.as<int>();
    float *out_d = e->scratch_b.as<float>();
    hipError_t st = hipMemcpyAsync(idx_d, idx_host, sizeof(int) * (size_t)k, hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = launch_gather_sub(M_dev, n, idx_d, k, out_d, e->stream);
    if (st == hipSuccess)
        st = hipMemcpyAsync(out_host, out_d, sizeof(float) * (size_t)k * k, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    if (st != hipSuccess) return fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
    return CUSK_OK;
}

extern "C" int cusk_gather_submatrix_dev(cusk_engine *e, const float *M_dev, int n, const int *idx_host, int k, float *out_dev)
{
    if (!e || !M_dev || !idx_host || !out_dev || k <= 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    CUSK_HIP(e, e->scratch_a.ensure(sizeof(int) * (size_t)k));
    int *idx_d = e->scratch_a.as<int>();
    hipError_t st = hipMemcpyAsync(idx_d, idx_host, sizeof(int) * (size_t)k, hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = launch_gather_sub(M_dev, n, idx_d, k, out_dev, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);  // idx_host may go away; the next run reuses the scratch
    if (st != hipSuccess) return fail(e, CUSK_ERR_HIP, hipGetErrorString(st));
    return CUSK_OK;
}

// device -> host copy ordered after the engine's work and waiting for the engine's stream only (cusk_dev_download is a
// device-wide blocking copy: with several engines on one GPU it serialises them)
extern "C" int cusk_engine_download(cusk_engine *e, void *dst_host, const void *src_dev, size_t bytes)
{
    if (!e || !dst_host || !src_dev) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    CUSK_HIP(e, fetch(e, dst_host, src_dev, bytes));
    return CUSK_OK;
}

extern "C" void *cusk_dev_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return p;
}
extern "C" void cusk_dev_free(void *p)
{
    if (p) (void)hipFree(p);
}
extern "C" int cusk_dev_upload(void *dst, const void *src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? CUSK_OK : CUSK_ERR_HIP;
}
extern "C" int cusk_dev_download(void *dst, const void *src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? CUSK_OK : CUSK_ERR_HIP;
}
