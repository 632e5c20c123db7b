// corr_build.hip -- host drivers of the correlation build (the reference's cu_marker_phen_corr_pearson / cu_corr_pearson_npn,
// cusk/src/corr_host.cu:1023-1197): the n x n square matrix of src/cli.cpp:597-649 (markers first, traits last, unit diagonal,
// symmetric) is written straight into HBM, so that the level sweep starts without a host round trip.  Kernels: corr_kernels.h.
#include <algorithm>
#include <cstring>

#include "corr_kernels.h"

namespace cusk {

// true when p is a HIP device allocation (hipPointerGetAttributes fails for plain host memory: not an error here)
bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    return false;
}

// An input that already lives in HBM (a whole .bed staged once per GPU by the block driver, cusk_blockset_stage) is used
// where it is; a host input of `count` elements is copied to the engine scratch `buf` (>= `reserve` elements) and `ptr` moved there.
template <typename T>
static int stage(cusk_engine *e, DevBuf &buf, const T *&ptr, size_t count, size_t reserve, hipStream_t s)
{
    if (is_device_pointer(ptr)) return CUSK_OK;
    CUSK_HIP(e, buf.ensure(sizeof(T) * reserve));
    if (count) CUSK_HIP(e, hipMemcpyAsync(buf.p, ptr, sizeof(T) * count, hipMemcpyHostToDevice, s));
    ptr = buf.as<T>();
    return CUSK_OK;
}

// `ahead`: the build of the NEXT block, enqueued on the engine's third stream while the current block is swept
// (cusk_corr_build_begin): device-resident inputs only, no events, no synchronisation; the marker x trait correlations
// land in `mxp_host` (pinned) when the stream gets there.
int corr_build_impl(cusk_engine *e, const unsigned char *bed, const float *phen, size_t m, size_t N, size_t p, const float *mean,
                    const float *std, float *C_dev, float *mxp_host, float *mxm_tri_host, float *pxp_tri_host, bool ahead)
{
    if (!e || !bed || !phen || !mean || !std || m == 0 || N == 0) return fail(e, CUSK_ERR_ARG, "bad arguments");
    CUSK_HIP(e, hipSetDevice(e->device));
    hipStream_t s = ahead ? e->stream3 : e->stream;
    if (ahead && !(is_device_pointer(bed) && is_device_pointer(phen) && is_device_pointer(mean) && is_device_pointer(std)))
        return fail(e, CUSK_ERR_ARG, "cusk_corr_build_begin needs device-resident inputs");
    const size_t clb = (N + 3) / 4, n = m + p;
    hipEvent_t *ev = e->ev_corr;  // [0] start, [1] inputs staged, [2] SNP x SNP tiles, [3] SNP x trait, [4] done
    if (!ahead) CUSK_HIP(e, hipEventRecord(ev[0], s));
    if (int rc = stage(e, e->bed_dev, bed, m * clb, m * clb, s)) return rc;  // from here on bed, phen, mean, std are device pointers
    if (int rc = stage(e, e->phen_dev, phen, p * N, std::max<size_t>(p * N, 1), s)) return rc;
    if (int rc = stage(e, e->mean_dev, mean, m, m, s)) return rc;
    if (int rc = stage(e, e->std_dev, std, m, m, s)) return rc;
    if (mxp_host && p) CUSK_HIP(e, e->mxp_dev.ensure(sizeof(float) * m * p));
    float *mxp_d = (mxp_host && p) ? e->mxp_dev.as<float>() : nullptr;
    if (!ahead) CUSK_HIP(e, hipEventRecord(ev[1], s));
    if (C_dev && e->opt_corr_popcount)
    {
        // cross-check path: bit planes + AND/popcount (no matrix cores); the tiles are timed without the decode
        if (int rc = launch_mxm_popcount(e, s, bed, C_dev, m, N, clb, n, ahead ? nullptr : ev[2])) return rc;
    }
    else
    {
        if (!ahead) CUSK_HIP(e, hipEventRecord(ev[2], s));
        if (C_dev && e->opt_corr_fp4)
            launch_mxm_fp4(s, MxmFp4Args{bed, C_dev, m, N, clb, n, 0, nullptr, 0, nullptr});
        else if (C_dev)
            launch_mxm_int8(s, bed, C_dev, m, N, clb, n);
    }
    if (C_dev) launch_unit_diag(s, C_dev, n);
    if (!ahead) CUSK_HIP(e, hipEventRecord(ev[3], s));
    // the single build's choice of SNP x trait form (corr_kernels.h: the batch chooses differently)
    const MxpForm form = e->opt_corr_popcount ? MxpForm::Scalar : (e->opt_corr_mxp_f32 ? MxpForm::F32 : MxpForm::Bf16);
    if (int rc = launch_mxp(e, s, MxpArgs{form, bed, phen, mean, std, C_dev, mxp_d, m, N, p, clb, n, (int)((m + 31) / 32), nullptr, nullptr}))
        return rc;
    if (C_dev) launch_pxp(s, phen, C_dev, m, N, p, n);
    CUSK_HIP(e, hipGetLastError());
    if (!ahead) CUSK_HIP(e, hipEventRecord(ev[4], s));
    if (mxp_d) CUSK_HIP(e, hipMemcpyAsync(mxp_host, mxp_d, sizeof(float) * m * p, hipMemcpyDeviceToHost, s));
    if (ahead) return CUSK_OK;  // cusk_corr_build_end waits for the stream
    if (C_dev && (mxm_tri_host || pxp_tri_host))
    {
        ScopedDevBuf tri;
        const size_t cm = m * (m - 1) / 2, cp = p ? p * (p - 1) / 2 : 0;
        CUSK_HIP(e, tri.ensure(sizeof(float) * std::max<size_t>(std::max(cm, cp), 1)));
        const struct { float *host; size_t lo, k, count; } part[2] = {{mxm_tri_host, 0, m, cm}, {pxp_tri_host, m, p, cp}};
        for (const auto &t : part)
        {
            if (!t.host || !t.count) continue;
            launch_extract_tri(s, C_dev, tri.as<float>(), t.lo, t.k, n);
            CUSK_HIP(e, hipMemcpyAsync(t.host, tri.p, sizeof(float) * t.count, hipMemcpyDeviceToHost, s));
            CUSK_HIP(e, hipStreamSynchronize(s));
        }
    }
    CUSK_HIP(e, hipStreamSynchronize(s));
    static const int span[4][2] = {{1, 2}, {2, 3}, {3, 4}, {0, 4}};  // cusk_corr_timing: staged -> tiles -> SNP x trait -> done, start -> done
    for (int i = 0; i < 4; i++) CUSK_HIP(e, hipEventElapsedTime(&e->corr_ms[i], ev[span[i][0]], ev[span[i][1]]));
    return CUSK_OK;
}

// ---- batched build: the correlation matrices of many LD blocks in one set of launches (cusk_corr_build_batch_*) ----
struct BatchIn  // what both phases are given (cusk_corr_build_batch_mxp / _mxm in include/cusk_hip.h)
{
    const unsigned char *bed;
    const float *phen, *mean, *std;
    size_t N, p;
    int nblk;
    const long long *first_marker;
    const int *markers, *base;
    size_t n;
    float *C;
};

// Both phases: argument checks, the tables of the phase (host/corr_plan.h) and their upload through the phase's own pinned staging area
// (phase one waits for its stream, phase two is followed by a run that does).  -> `d`: the tables on the device; nullptr: phase two keeps no block.
static int batch_tables(cusk_engine *e, int phase, const BatchIn &in, const unsigned char *keep, CorrBatchPlan &pl, const char *&d)
{
    d = nullptr;
    if (!e || !in.bed || !in.phen || !in.mean || !in.std || !in.first_marker || !in.markers || !in.base || !in.C || in.nblk <= 0 || in.N == 0)
        return fail(e, CUSK_ERR_ARG, "bad arguments");
    if (!(is_device_pointer(in.bed) && is_device_pointer(in.phen) && is_device_pointer(in.mean) && is_device_pointer(in.std)))
        return fail(e, CUSK_ERR_ARG, "cusk_corr_build_batch needs device-resident inputs (cusk_blockset_stage)");
    CUSK_HIP(e, hipSetDevice(e->device));
    if (!corr_batch_plan(phase, in.nblk, in.first_marker, in.markers, in.base, keep, in.p, in.n, pl))
        return fail(e, CUSK_ERR_ARG, "cusk_corr_build_batch: block outside the batch allocation");
    if (phase == 2 && pl.kept.empty()) return CUSK_OK;  // no wait for a phase one still in flight here: ADVICE.md
    const int slot = phase - 1;
    CUSK_HIP(e, e->corr_tab_pinned[slot].ensure(pl.total, pl.total * 2));
    pl.write(e->corr_tab_pinned[slot].as<char>());
    CUSK_HIP(e, e->corr_tab[slot].ensure(pl.total));
    CUSK_HIP(e, hipMemcpyAsync(e->corr_tab[slot].p, e->corr_tab_pinned[slot].p, pl.total, hipMemcpyHostToDevice, e->stream));
    d = e->corr_tab[slot].as<char>();
    return CUSK_OK;
}

// Phase one: marker x trait correlations of every block (into the batch allocation and into a compact host array, block
// after block: the prefilter of cli.cpp:561-576 is the caller's).  Waits for the result, unless async_mxp
// (cusk_corr_build_batch): then the correlations land in pinned memory, an event marks their arrival, nobody waits here.
static int batch_mxp(cusk_engine *e, const BatchIn &in, float *mxp_host, bool async_mxp)
{
    CorrBatchPlan pl;
    const char *d;
    if (int rc = batch_tables(e, 1, in, nullptr, pl, d)) return rc;
    hipStream_t s = e->stream;
    const size_t p = in.p, cnt = (size_t)pl.markers * p;
    if (p == 0) return CUSK_OK;
    if (mxp_host) CUSK_HIP(e, e->mxp_dev.ensure(sizeof(float) * cnt));
    float *mxp_d = mxp_host ? e->mxp_dev.as<float>() : nullptr;
    // the batch's choice of SNP x trait form (corr_kernels.h): corr_mxp_f32 alone, never the scalar kernel
    const MxpForm form = e->opt_corr_mxp_f32 ? MxpForm::F32 : MxpForm::Bf16;
    if (int rc = launch_mxp(e, s, MxpArgs{form, in.bed, in.phen, in.mean, in.std, in.C, mxp_d, 0, in.N, p, (in.N + 3) / 4, in.n,
                                           (int)pl.tiles2.size(), reinterpret_cast<const CorrTile2 *>(d + pl.o_tiles),
                                           reinterpret_cast<const CorrBatchBlock *>(d)}))
        return rc;
    CUSK_HIP(e, hipGetLastError());
    if (async_mxp)
    {
        if (sizeof(float) * cnt > e->mxp_pinned.cap && e->mxp_pending) return fail(e, CUSK_ERR_STATE, "a correlation build is in flight");
        CUSK_HIP(e, e->mxp_pinned.ensure(sizeof(float) * cnt, sizeof(float) * (cnt + cnt / 4 + 64)));
        if (mxp_d) CUSK_HIP(e, hipMemcpyAsync(e->mxp_pinned.p, mxp_d, sizeof(float) * cnt, hipMemcpyDeviceToHost, s));
        if (!e->ev_mxp) CUSK_HIP(e, hipEventCreateWithFlags(&e->ev_mxp, hipEventDisableTiming));
        CUSK_HIP(e, hipEventRecord(e->ev_mxp, s));
        return CUSK_OK;
    }
    if (mxp_d) CUSK_HIP(e, hipMemcpyAsync(mxp_host, mxp_d, sizeof(float) * cnt, hipMemcpyDeviceToHost, s));
    CUSK_HIP(e, hipStreamSynchronize(s));
    return CUSK_OK;
}

// Phase two: marker x marker tiles (always the FP4 kernel: corr_popcount and corr_fp4 do not reach the batch), trait x trait and
// diagonal of the blocks the caller keeps; asynchronous on the engine's stream (the sweep that follows is ordered behind it).
static int batch_mxm(cusk_engine *e, const BatchIn &in, const unsigned char *keep)
{
    CorrBatchPlan pl;
    const char *d;
    if (int rc = batch_tables(e, 2, in, keep, pl, d)) return rc;
    if (!d) return CUSK_OK;
    const CorrBatchBlock *blk_d = reinterpret_cast<const CorrBatchBlock *>(d);
    launch_mxm_fp4(e->stream, MxmFp4Args{in.bed, in.C, 0, in.N, (in.N + 3) / 4, in.n, 0, reinterpret_cast<const CorrTile4 *>(d + pl.o_tiles),
                                 pl.tiles4.size(), blk_d});
    // trait x trait once (a p x p matrix of its own: m = 0, leading dimension p), then into every kept block with the diagonal
    CUSK_HIP(e, e->pxp_dev.ensure(sizeof(float) * std::max<size_t>(in.p * in.p, 1)));
    launch_pxp(e->stream, in.phen, e->pxp_dev.as<float>(), 0, in.N, in.p, in.p);
    launch_batch_finish(e->stream, in.C, in.n, blk_d, reinterpret_cast<const int *>(d + pl.o_kept), pl.kept.size(), e->pxp_dev.as<float>(), in.p);
    CUSK_HIP(e, hipGetLastError());
    return CUSK_OK;
}

// The reference-named correlation entry points (host buffers in and out, an engine per call; `square`: the n x n matrix and its
// triangles too); exported with C linkage by compat_api.hip and with the reference's own C++ linkage by compat_cxx.cpp.
static void compat_build(const char *name, const unsigned char *bed, const float *phen, size_t m, size_t N, size_t p, const float *mean,
                         const float *std, bool square, float *mxm_tri, float *mxp, float *pxp_tri)
{
    cusk_engine *e = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (cusk_engine_create(&e, dev, nullptr) != CUSK_OK)
    {
        std::fprintf(stderr, "libcusk_hip: cannot create engine (no HIP device?)\n");
        std::exit(EXIT_FAILURE);
    }
    float *Cd = square ? static_cast<float *>(cusk_dev_alloc(sizeof(float) * (m + p) * (m + p))) : nullptr;
    if ((square && !Cd) || corr_build_impl(e, bed, phen, m, N, p, mean, std, Cd, mxp, mxm_tri, pxp_tri) != CUSK_OK)
    {
        std::fprintf(stderr, "libcusk_hip: %s: %s\n", name, cusk_last_error(e));
        std::exit(EXIT_FAILURE);
    }
    if (square) cusk_dev_free(Cd);
    cusk_engine_destroy(e);
}

void compat_marker_phen_corr_pearson(const unsigned char *marker_vals, const float *phen_vals, const size_t num_markers, const size_t num_individuals,
                                     const size_t num_phen, const float *marker_mean, const float *marker_std, float *marker_phen_corrs)
{
    compat_build("cu_marker_phen_corr_pearson", marker_vals, phen_vals, num_markers, num_individuals, num_phen, marker_mean, marker_std, false,
                 nullptr, marker_phen_corrs, nullptr);
}

void compat_corr_pearson_npn(const unsigned char *marker_vals, const float *phen_vals, const size_t num_markers, const size_t num_individuals,
                             const size_t num_phen, const float *marker_mean, const float *marker_std, float *marker_corrs,
                             float *marker_phen_corrs, float *phen_corrs)
{
    compat_build("cu_corr_pearson_npn", marker_vals, phen_vals, num_markers, num_individuals, num_phen, marker_mean, marker_std, true, marker_corrs,
                 marker_phen_corrs, phen_corrs);
}

}  // namespace cusk

using namespace cusk;

extern "C" int cusk_corr_build(cusk_engine *e, const unsigned char *bed, const float *phen, size_t m, size_t N, size_t p,
                               const float *mean, const float *std, float *C_dev, float *mxp_host)
{
    return corr_build_impl(e, bed, phen, m, N, p, mean, std, C_dev, mxp_host, nullptr, nullptr);
}

extern "C" int cusk_corr_build_batch_mxp(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev, const float *std_dev,
                                         size_t N, size_t p, int nblk, const long long *first_marker, const int *markers, const int *base, int n, float *C_dev, float *mxp_host)
{
    return batch_mxp(e, BatchIn{bed_dev, phen_dev, mean_dev, std_dev, N, p, nblk, first_marker, markers, base, (size_t)n, C_dev}, mxp_host, false);
}

extern "C" int cusk_corr_build_batch_mxm(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev, const float *std_dev,
                                         size_t N, size_t p, int nblk, const long long *first_marker, const int *markers, const int *base, const unsigned char *keep, int n, float *C_dev)
{
    return batch_mxm(e, BatchIn{bed_dev, phen_dev, mean_dev, std_dev, N, p, nblk, first_marker, markers, base, (size_t)n, C_dev}, keep);
}

// Everything in one call, the marker x marker part speculatively for EVERY block: the host's prefilter (cli.cpp:561-576)
// then runs beside the contingency GEMMs instead of between two synchronisations (a block that is skipped after all had
// its matrix built for nothing: rare -- one false positive among its m x p marginal tests is enough to keep it)
extern "C" int cusk_corr_build_batch(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev, const float *std_dev,
                                     size_t N, size_t p, int nblk, const long long *first_marker, const int *markers, const int *base, int n, float *C_dev,
                                     float *mxp_host)
{
    if (!e || !mxp_host) return e ? fail(e, CUSK_ERR_ARG, "bad arguments") : CUSK_ERR_ARG;
    const BatchIn in{bed_dev, phen_dev, mean_dev, std_dev, N, p, nblk, first_marker, markers, base, (size_t)n, C_dev};
    if (int rc = batch_mxp(e, in, mxp_host, true)) return rc;
    if (int rc = batch_mxm(e, in, nullptr)) return rc;
    if (p == 0) return CUSK_OK;
    CUSK_HIP(e, hipEventSynchronize(e->ev_mxp));
    size_t cnt = 0;
    for (int b = 0; b < nblk; b++) cnt += (size_t)markers[b] * p;
    std::memcpy(mxp_host, e->mxp_pinned.p, sizeof(float) * cnt);
    return CUSK_OK;
}

// The build of the next block while the current one is swept: begin enqueues everything on the engine's third stream and
// returns; end waits for it and hands over the marker x trait correlations.  One build in flight per engine.
extern "C" int cusk_corr_build_begin(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, size_t m, size_t N,
                                     size_t p, const float *mean_dev, const float *std_dev, float *C_dev)
{
    if (!e || !C_dev || p == 0) return e ? fail(e, CUSK_ERR_ARG, "bad arguments") : CUSK_ERR_ARG;
    if (e->mxp_pending) return fail(e, CUSK_ERR_ARG, "a correlation build is already in flight");
    CUSK_HIP(e, e->mxp_pinned.ensure(sizeof(float) * m * p, sizeof(float) * (m * p + m * p / 4 + 64)));
    const int rc = corr_build_impl(e, bed_dev, phen_dev, m, N, p, mean_dev, std_dev, C_dev, e->mxp_pinned.as<float>(), nullptr, nullptr, true);
    if (rc == CUSK_OK) e->mxp_pending = m * p;
    return rc;
}

extern "C" int cusk_corr_build_pending(const cusk_engine *e) { return (e && e->mxp_pending) ? 1 : 0; }

extern "C" int cusk_corr_build_end(cusk_engine *e, float *mxp_host)
{
    if (!e) return CUSK_ERR_ARG;
    if (!e->mxp_pending) return fail(e, CUSK_ERR_ARG, "no correlation build in flight");
    CUSK_HIP(e, hipSetDevice(e->device));
    const size_t count = e->mxp_pending;
    e->mxp_pending = 0;
    CUSK_HIP(e, hipStreamSynchronize(e->stream3));
    if (mxp_host) std::memcpy(mxp_host, e->mxp_pinned.p, sizeof(float) * count);
    return CUSK_OK;
}

extern "C" void cusk_corr_timing(const cusk_engine *e, float *ms4) { for (int i = 0; i < 4; i++) ms4[i] = e ? e->corr_ms[i] : 0.0f; }
