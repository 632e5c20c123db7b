/*
 * cusk_hip.h -- C ABI of libcusk_hip.so, the MI355X-native `cusk` PC-skeleton engine.
 *
 * Plain pointers and sizes only.  Two groups of entry points:
 *
 *  (1) the reference's own operator interface for this path, with identical
 *      names, argument order and argument meaning, so that the reference's
 *      callers (cusk/src/cli.cpp:45,72,550,581,670) link against this library
 *      unchanged -- host buffers in, host buffers out, blocking;
 *  (2) a device-resident engine API (cusk_*) that the `mps` host program and
 *      bench.py use: matrices stay in HBM between the correlation build and
 *      the level sweep, adjacency is a bitmap, separation sets are sparse.
 *
 * Citations are to /root/reference/cusk.
 */
#ifndef CUSK_HIP_H_
#define CUSK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUSK_ML 14 /* include/mps/cuPC-S.h:49 (ML) */

/* ---------------------------------------------------------------------------
 * (1) reference-compatible entry points
 * ------------------------------------------------------------------------ */

/* Replaces `extern "C" void Skeleton(...)`, include/mps/cuPC-S.h:196-198,
 * src/cuPC-S.cu:61-450.  All pointers are caller-owned HOST memory.
 *   C        in   n*n fp32 row-major correlation matrix
 *   P        in   *P = n
 *   G        out  n*n int32 adjacency (fully overwritten)
 *   Th       in   thresholds Th[0..min(14,*maxlevel)]
 *   l        out  level counter as the reference leaves it
 *   maxlevel in   maximal conditioning-set size (<= 14)
 *   pMax     out  n*n fp32: -100000 on surviving edges, max Fisher z of the
 *                 two directions on removed ones, 1 on the diagonal
 *   SepSet   out  n*n*14 int32, -1 padded
 * Errors (HIP failure, combinatorial overflow): message on stderr, exit(EXIT_FAILURE),
 * as include/mps/gpuerrors.h:6-15 does. */
void Skeleton(float *C, int *P, int *G, float *Th, int *l, const int *maxlevel, float *pMax,
              int *SepSet);

/* Replaces `extern "C" void hetcor_skeleton(...)`, include/mps/hetcor-cuPC-S.h:46,
 * src/hetcor-cuPC-S.cu:75-341.  G is IN/OUT (zeros are respected, level 0 only
 * removes), N is the n*n effective-sample-size matrix, *Th the single
 * alpha/2 quantile, time_index has n entries (markers 0). */
void hetcor_skeleton(float *C, int *P, int *G, float *N, float *Th, int *l, const int *maxlevel,
                     const int *time_index);

/* Replaces threshold_array / hetcor_threshold, include/mps/cuPC_call_prep.h:7-15,
 * src/cuPC_call_prep.cpp:13-27 (the reference returns std::vector<float>; here
 * the caller passes room for 15 floats). */
void cusk_threshold_array(int n, float alpha, float *thr15);
float cusk_hetcor_threshold(float alpha);

/* Replace cu_marker_phen_corr_pearson / cu_corr_pearson_npn,
 * include/mps/corr_host.h:38-47,92-103, src/corr_host.cu:1023-1197.  Host
 * buffers; marker_vals is SNP-major packed .bed without the 3 magic bytes,
 * phen_vals column-major with NaN = missing.  Outputs: marker_corrs upper
 * triangle without diagonal (row-major linear), marker_phen_corrs m*p
 * row-major, phen_corrs upper triangle without diagonal. */
void cu_marker_phen_corr_pearson(const unsigned char *marker_vals, const float *phen_vals,
                                 const size_t num_markers, const size_t num_individuals,
                                 const size_t num_phen, const float *marker_mean,
                                 const float *marker_std, float *marker_phen_corrs);
void cu_corr_pearson_npn(const unsigned char *marker_vals, const float *phen_vals,
                         const size_t num_markers, const size_t num_individuals,
                         const size_t num_phen, const float *marker_mean, const float *marker_std,
                         float *marker_corrs, float *marker_phen_corrs, float *phen_corrs);

/* ---------------------------------------------------------------------------
 * (2) device-resident engine
 * ------------------------------------------------------------------------ */

typedef struct cusk_engine cusk_engine;

enum {
    CUSK_OK = 0,
    CUSK_ERR_HIP = 1,      /* a HIP runtime call failed */
    CUSK_ERR_ARG = 2,      /* bad argument */
    CUSK_ERR_OVERFLOW = 3, /* C(degree, level) does not fit 62 bits */
    CUSK_ERR_STATE = 4     /* call order (no result to fetch, ...) */
};

/* per-run counters; index = level */
typedef struct cusk_stats {
    int level;                        /* what the reference leaves in *l */
    int levels_run;                   /* number of levels that launched tests (incl. level 0) */
    int max_degree[CUSK_ML + 1];      /* max degree at the start of the level (level 0: n-1) */
    long long edges[CUSK_ML + 1];     /* directed edges at the start of the level */
    long long tests[CUSK_ML + 1];     /* CI tests evaluated (SURVEY.md 8d definition) */
    long long subsets[CUSK_ML + 1];   /* conditioning sets whose inverse was formed */
    long long removed[CUSK_ML + 1];   /* ordered pairs (X,Y) for which a separating set was found */
    float kernel_ms[CUSK_ML + 1];     /* HIP-event time of the level's sweep kernels */
    float level_ms[CUSK_ML + 1];      /* HIP-event time of the whole level (compaction + sweep + finalise) */
    float total_ms;                   /* whole run, events on the engine stream */
    long long rechecks[CUSK_ML + 1];  /* tests the fast filter could not certify (re-evaluated on the exact path); level 1: 0,
                                         except with option "het_rows", where it counts the tests the row kernel's
                                         filter sent to the exact form (and subsets[1] is 0 as for every row-kernel run) */
    long long violations;             /* validate mode only: certified verdicts contradicted by the exact path */
    long long exact_fallbacks;        /* levels redone entirely on the exact path (recheck queue overflow) */
    float main_kernel_ms[CUSK_ML + 1]; /* HIP-event time of the level's dominant kernel alone (level 1: the rows
                                         kernel without its prep / count passes; other levels = kernel_ms) */
    long long canonical_tests[CUSK_ML + 1]; /* cusk_run_skeleton: CI tests of the CANONICAL schedule -- the reference
                                         algorithm run sequentially per row: a neighbour is tested with every conditioning
                                         set up to its lowest passing one -- computed on the device from
                                         the selected ranks; `tests` counts what the parallel sweep executed (more: lanes
                                         cannot see each other's fresh verdicts).  cusk_run_hetcor: level 0 and -- on a
                                         symmetric matrix with one sample size and no time index (the row-streaming
                                         kernel) -- level 1; 0 at the other levels. */
} cusk_stats;

/* device = HIP device ordinal; stream = a hipStream_t to run on, or NULL for a
 * private non-blocking stream.  Returns CUSK_OK or an error code. */
int cusk_engine_create(cusk_engine **out, int device, void *stream);
void cusk_engine_destroy(cusk_engine *e);
const char *cusk_last_error(const cusk_engine *e);
/* options: "fast" (default 1: register-Cholesky filter + exact recheck for levels >= 2; 0: exact
 * arithmetic for every test), "validate" (default 0; 1: also run the exact path on every certified
 * verdict and count contradictions in cusk_stats.violations), "pair" (default 1: level-1 kernels that exploit a
 * symmetric matrix; 0: generic staged kernel), "rows" (default 1: the row-streaming level-1 kernel that reads C
 * exactly once; 0: the pair-gather kernel), "vec" (default 1: vectorised
 * four-tests-per-ds_read_b128 sweep kernel; 0: scalar fast kernel), "overlap" (default 1: independent degree
 * classes and the winners' exact z run on an auxiliary stream), "corr_fp4" (default 1: the SNP x SNP contingency GEMMs of
 * cusk_corr_build on the FP4 matrix pipe; 0: the int8 MFMA form), "corr_popcount" (default 0; 1: bit-plane AND/popcount
 * cross-check kernels instead of the matrix cores), "corr_mxp_f32" (default 0: SNP x trait sums on the bf16 matrix pipe with every
 * trait value split exactly into three bf16 pieces; 1: the f32 matrix instructions of rounds 1-2), "assume_symmetric" (default 0: level 0 verifies C == C^T bitwise;
 * 1: the caller guarantees it, e.g. a matrix written by cusk_corr_build), "queue_capacity" (recheck queue entries, default 4Mi), "chunk" (combination ranks per work item, default 2048), "timing" (HIP events for cusk_stats: 0 total_ms only; 1, the default, around every level's sweep: kernel_ms, and level_ms = end of the previous level's sweep to the end of this one's; 2 also level start / end: level_ms = plan to finaliser; 3 only the pair around the level-1 row kernel: main_kernel_ms[1] -- every event costs a few microseconds of device time), "chunk0" (conditioning sets per work item of the first degree class, default 512), "tmaj_min_level" (first level swept by unions T = S + Y, one inverse per l + 1 tests: default 6, 99 = never; single threshold and symmetric matrix only), "tmaj_validate_stride" (with "validate": the union-major sweep checks the unions whose per-lane count is a multiple of this power of two against double precision; default 1 = all), "hostprof" (1: host-side phase marks of every run on stderr), "max_staged_classes" (test hook: at most this many degree classes keep their sub-matrix in LDS; 0 sends every row through the kernels of the unstaged class), "chunk0_low" (work-item size of the first degree class at levels 2-4, default 256), "vec_threads" (workgroup size of the vectorised sweep for the first degree class: 64, 128 or 256; default 64), "lookahead" (levels the host enqueues ahead of the level counters it has seen, default 2; every kernel checks its level's gate on the device), "sync2" (default 1: the host reads level 2's gate record -- class counts, maximum degree -- before it enqueues that level's sweeps, so that degree classes that turn out empty are not launched at levels >= 2; 0: enqueue ahead on the level-1 degree bound), "item_capacity" (work items per degree class and level the buffers hold before the engine grows them and takes the level up again, default 1Mi), "het_filter" (default 0: cusk_run_skeleton_het / cusk_run_skeleton_batch_het run every level on the exact path; 1: their levels >= 2 go through the filter at the per-test threshold and the recheck queue like the other modes, "fast" = 0 still selects the exact path, and "validate" is accepted), "het_rows" (0 or 1, default 0: level 1 of cusk_run_skeleton_het / cusk_run_skeleton_batch_het runs on the exact sweep; 1: on the row-streaming level-1 kernel at per-pair sample sizes when "fast", "pair" and "rows" are non-zero and both C and N_dev are symmetric, N_dev bit for bit -- otherwise as with 0; same results; cusk_engine_level1_form tells which kernel ran), "sepselect_ws_bytes" (HBM work space of
 * cusk_sepselect_greedy for candidate lists too long for LDS, default 4 GiB; such pairs run in batches of what fits), "mvivw_part_bytes" (HBM of cusk_mvivw's chunk partials alive at
 * once, default 256 MiB; outcomes run in groups of what fits, an outcome that alone exceeds it as a group of its own; the
 * results do not depend on it), "mvivw_ld_bytes" (HBM of cusk_mvivw_ld's m x m workspace, default 8 GiB; an outcome that
 * needs more is an argument error), "mvivw_jk_bytes" (HBM of cusk_mvivw_jackknife's refitted estimates alive at once, default
 * 1 GiB; outcomes run in batches of what fits, an outcome that alone exceeds it as a batch of its own; the results do not
 * depend on it), "phen_rint_bytes" (HBM of cusk_phen_rint's sorted keys and ranks alive at once, default
 * 1 GiB; traits run in groups of what fits, the results do not depend on it, and a single trait that needs more is an
 * argument error). */
int cusk_engine_set_option(cusk_engine *e, const char *key, long long value);
/* Host only, no device needed: the workgroup size level 1's row-streaming kernel runs with when a row of C takes
 * row_bytes of LDS (4 (n + 8) for a single n x n matrix), or 0 when it gathers the row through the caches instead.
 * mode 0 Skeleton / 1 hetcor; forced_threads as the test options "l1_threads" (0 / 256 / 512; "l1_lds_row" = 0 and a
 * matrix that is not 16-byte aligned always give the gather form).  -1 for arguments out of range.  mode 2: the
 * forms at per-pair sample sizes (Skeleton mode with option "het_rows"), which keep the row of N behind the row of C:
 * row_bytes = 2 * 4 (n + 8), rounded up by at most 12 bytes so that the second row starts on a 16-byte boundary. */
int cusk_level1_rows_threads(long long row_bytes, int mode, int validate, int forced_threads);
void *cusk_engine_stream(const cusk_engine *e);
/* Makes the engine's device the calling thread's current HIP device, so that the cusk_dev_* helpers below act on it.
 * Needed on multi-GPU nodes by threads other than the one that created the engine (HIP's current device is per thread
 * and starts at 0). */
int cusk_engine_bind_thread(cusk_engine *e);
int cusk_engine_device(const cusk_engine *e); /* the HIP device ordinal the engine was created on */

/* Row-sharded sweep of ONE block over several engines, normally one per GPU (a single matrix too
 * large or too slow for one device; the reference has no counterpart, its Skeleton is single-GPU, cuPC-S.cu:42-190).
 * Every engine of the group holds the whole matrix and calls cusk_run_skeleton with identical arguments; engine
 * `rank` of `world` runs the conditional-independence tests of the rows X with X % world == rank only.  After each
 * level's sweep the engines join their per-edge selection state -- the lowest passing conditioning-set rank of every
 * ordered pair, "none" = all ones -- through `fn`, which must perform an element-wise UNSIGNED MIN all-reduce of
 * `count` elements of `elem_bytes` (4 at level 1, 8 beyond) across the group, in place, and return 0 once the
 * result is in the buffer.  Removal of edges, separating-set records and the next level's neighbour lists are then
 * derived identically on every engine, so all of them finish with the complete result (bit-identical to a
 * single-engine run).  host_staging = 1: `buf` is a pinned HOST copy (on_device = 0; for CPU collectives such as
 * gloo); 0: `buf` is the DEVICE buffer itself (on_device = 1; RCCL), the engine's stream is idle during the call and
 * the callee must have finished with the buffer when it returns.  world = 1 switches sharding off.  cusk_run_hetcor
 * shards the same way: what its engines join is one 32-bit mark per directed edge, 0 = removed at this level (elem_bytes
 * 4 at every level), and the removal of the marked edges is then applied identically on every engine. */
typedef int (*cusk_exchange_fn)(void *user, int level, void *buf, size_t count, int elem_bytes, int on_device, void *stream);
int cusk_engine_set_row_shard(cusk_engine *e, int rank, int world, cusk_exchange_fn fn, void *user, int host_staging);

/* Level sweep on a matrix already resident in HBM (C_dev: n*n fp32 row-major).
 * cusk_run_skeleton   : `Skeleton` semantics (fixed per-level thresholds Th[0..14] on
 *                       the host, sepsets + pMax recorded sparsely).
 * cusk_run_hetcor     : `hetcor_skeleton` semantics.  N_dev may be NULL when every
 *                       pair has the same effective sample size `ess_uniform`;
 *                       G_init_dev (n*n int32, device) may be NULL for the
 *                       complete graph; time_index is a HOST array of n ints or
 *                       NULL (all zero).
 * Both are asynchronous with respect to other streams but return after the
 * level loop has finished (the loop needs the max degree on the host each level). */
int cusk_run_skeleton(cusk_engine *e, const float *C_dev, int n, const float *Th, int maxlevel,
                      cusk_stats *stats);
int cusk_run_hetcor(cusk_engine *e, const float *C_dev, const float *N_dev, float ess_uniform,
                    const int *G_init_dev, int n, float th, int maxlevel, const int *time_index,
                    cusk_stats *stats);

/* `Skeleton` semantics at per-pair sample sizes: the outputs of cusk_run_skeleton (lowest passing conditioning set per
 * ordered pair in Skeleton's enumeration -- neighbours ascending, combinations lexicographic --, separating-set records,
 * pMax; read through cusk_result_adj_*, cusk_result_sepsets, cusk_result_sepset_dense, cusk_result_pmax) with every test
 * decided at the threshold of cusk_run_hetcor.  N_dev: the n*n fp32 sample-size matrix as cusk_run_hetcor takes it (e.g.
 * from cusk_ess_square); th = cusk_hetcor_threshold(alpha).  Level 0 removes the pair (i, j) when its Fisher z lies below
 * th / sqrt(N[i,j] - 3) and records the empty set and that z; a test of X, Y given S, |S| = l >= 1, compares with
 * th / sqrt(mean - l - 3), mean = the float sum of the (l + 2)(l + 1) / 2 sizes among {X, Y} + S, each truncated to int,
 * divided by their number (mean_ess, hetcor-cuPC-S.cu:3068-3088).  A NaN or negative radicand gives a NaN threshold: the
 * comparison is false and the edge stays.  There is no time index and no starting graph.  With every size equal to N the
 * result is that of cusk_run_skeleton with Th[l] = th / sqrt(N - l - 3) formed in that arithmetic.
 * Every level runs on the exact path.  Not supported, each an error with a message in cusk_last_error: an engine that is
 * row-sharded (cusk_engine_set_row_shard with world > 1), option "validate".  Batched form: cusk_run_skeleton_batch_het.
 * Option "het_filter" = 1: levels >= 2 run through the register-Cholesky filter at a float estimate of the per-test
 * threshold; what it cannot certify (guard band, conditioning guard, NaN threshold) is queued and decided on the exact
 * path, a queue overflow redoes the level there (exact_fallbacks), and "validate" counts certified verdicts the exact
 * per-test threshold contradicts.  Levels >= "tmaj_min_level" are swept by unions with one threshold per union when N_dev
 * is bitwise symmetric (checked on the device, inside the blocks of a batch), else by conditioning set.  Adjacency,
 * records and pMax are those of the exact path either way. */
int cusk_run_skeleton_het(cusk_engine *e, const float *C_dev, const float *N_dev, int n, float th, int maxlevel,
                          cusk_stats *stats);
/* Which kernel ran level 1 in the engine's last run (any mode): 0 the generic sweep, 1 the pair kernel, 2 / 3 the
 * row-streaming kernel with the row in LDS at 256 / 512 threads, 4 the row-streaming kernel in its gather form, -1 no level 1
 * ran (or no run yet).  With option "het_rows" it tells a row-kernel run at per-pair sample sizes from the fall-back to the
 * exact sweep (asymmetric N_dev or C, "fast" / "pair" / "rows" = 0). */
int cusk_engine_level1_form(const cusk_engine *e);

/* Batched Skeleton run: `nblk` independent blocks (the LD blocks of one GPU's share of a chromosome job, or their reduced
 * stage-two sets) swept in ONE run.  The reference has no counterpart: it runs one block per process (src/cli.cpp:507-512,
 * README.md:62); per block the result is that of cusk_run_skeleton on the block alone (adjacency, separating sets).
 * Layout: the blocks lie along the diagonal of one n x n allocation C_dev (leading dimension n): block b holds the
 * variables [lo[b], hi[b]), its matrix at C_dev[i * n + j] for i, j in that range, each bitwise symmetric (what
 * cusk_corr_build_batch and cusk_gather_rows write); lo[b] are ascending multiples of 64, the ranges disjoint; variables
 * outside every range are padding and elements outside the diagonal blocks are never read (they need not be initialised).
 * Th / maxlevel as cusk_run_skeleton (one threshold array: the blocks share the sample size).  stats are those of the
 * whole batch; `level` is the last level at which ANY block still had a row with more neighbours than the level (a block
 * that ends earlier has no test left at the later levels, so its result does not depend on the others).  Results:
 * cusk_result_adj_bits_blocks, cusk_result_sepsets (x, y and set members are variable indices of the batch). */
int cusk_run_skeleton_batch(cusk_engine *e, const float *C_dev, int n, int nblk, const int *lo, const int *hi,
                            const float *Th, int maxlevel, cusk_stats *stats);
/* The batched run at per-pair sample sizes: the layout rules and result accessors of cusk_run_skeleton_batch
 * (cusk_result_adj_bits_blocks[_tail], cusk_result_sepsets[_view]) with the decision rule of cusk_run_skeleton_het.  N_dev
 * is an n x n allocation like C_dev (same leading dimension) that holds every block's sample-size matrix on the diagonal,
 * bitwise symmetric inside the blocks (cusk_ess_square_batch, cusk_gather_rows); elements outside the diagonal blocks are
 * never read.  th = cusk_hetcor_threshold(alpha).  Per block the result is that of cusk_run_skeleton_het on the block
 * alone: level 0 takes the same verdict per pair, every later level runs on the same exact path.  Errors as
 * cusk_run_skeleton_het: a row-sharded engine, option "validate" (without "het_filter"), N_dev = NULL.  Option
 * "het_filter" as for cusk_run_skeleton_het. */
int cusk_run_skeleton_batch_het(cusk_engine *e, const float *C_dev, const float *N_dev, int n, int nblk, const int *lo,
                                const int *hi, float th, int maxlevel, cusk_stats *stats);
/* adjacency of the last batched run, block by block: rows lo..hi-1 of block b, each cut to the (hi - lo + 63) / 64
 * words of the block's own columns (bit j of a row = local variable j), blocks back to back.  out_host: room for
 * sum_b (hi[b] - lo[b]) * ((hi[b] - lo[b] + 63) / 64) words. */
int cusk_result_adj_bits_blocks(cusk_engine *e, uint64_t *out_host);
/* the same for the LAST tail_rows rows of every block only (the traits: parent_set.cpp:8-53 at depth 1 looks at nothing
 * else); a block with fewer rows gives all of them */
int cusk_result_adj_bits_blocks_tail(cusk_engine *e, int tail_rows, uint64_t *out_host);
/* rows [row0, row0 + nrows) of the last run's bitmap, cusk_result_words() words each, to host memory */
int cusk_result_adj_rows(cusk_engine *e, int row0, int nrows, uint64_t *out_host);
/* Many sub-matrices in one launch: out[row_out[t] + c] = M_dev[row_src[t] * n + idx[row_first[t] + c]] for c < row_k[t],
 * t < nrows (parent_set.cpp:84-238 for a batch: the stage-two matrices straight onto the diagonal of the next batch
 * allocation, out_on_device = 1; the retained sub-matrices of the results, out_on_device = 0, out_count floats).  Index
 * arrays are host memory. */
int cusk_gather_rows(cusk_engine *e, const float *M_dev, int n, const int *idx_host, long long nidx, const int *row_src,
                     const int *row_k, const long long *row_first, const long long *row_out, long long nrows, float *out,
                     long long out_count, int out_on_device);

/* Results of the last run (valid until the next run / destroy). */
int cusk_result_n(const cusk_engine *e);
/* adjacency bitmap on the device: n rows of cusk_result_words() uint64 words, bit j of row i */
const uint64_t *cusk_result_adj_bits_dev(const cusk_engine *e);
int cusk_result_words(const cusk_engine *e);
/* expand into the reference's layouts; dst is HOST memory unless the name says _dev */
int cusk_result_adj_i32(cusk_engine *e, int *G_host);
int cusk_result_adj_i32_dev(cusk_engine *e, int *G_dev);
int cusk_result_pmax(cusk_engine *e, const float *C_dev, float *pMax_host);
int cusk_result_sepset_dense(cusk_engine *e, int *SepSet_host /* n*n*14 */);
/* sparse separation sets: one record per ordered pair with a non-empty set, ordered by (x, y).
 * Returns the count; arrays may be NULL to query it.  x,y: count ints;
 * level: count ints; z: count floats; S: count*14 ints (-1 padded).  The winners' Fisher z is computed on the first
 * request that asks for it (z != NULL, or cusk_result_pmax) from the matrix of the run, which must still be resident. */
long long cusk_result_sepsets(cusk_engine *e, int *x, int *y, int *level, float *z, int *S);
/* the same records (x, y, S[count * 14]) in engine-owned PINNED host memory -- one synchronisation, no staging through
 * pageable memory; the pointers stay valid until the next run or result call on this engine.  Returns the count. */
long long cusk_result_sepsets_view(cusk_engine *e, const int **x, const int **y, const int **S);

/* Correlation build on the device (a2-a5).  bed/phen/mean/std
 * are HOST buffers as in cu_corr_pearson_npn; the n*n (n = m + p) square
 * matrix (markers first, then traits, unit diagonal, symmetric;
 * src/cli.cpp:597-649) is written to C_dev.  If mxp_host is not NULL it also
 * receives the m*p marker-trait correlations (for the prefilter, cli.cpp:561-576). */
int cusk_corr_build(cusk_engine *e, const unsigned char *bed, const float *phen, size_t m,
                    size_t N, size_t p, const float *mean, const float *std, float *C_dev,
                    float *mxp_host);
/* The same build for the NEXT block of a job while the current one is swept: begin enqueues it on a stream of its own
 * (device-resident inputs only: cusk_blockset_stage) and returns at once, end waits for it and copies the marker x trait
 * correlations out.  One build in flight per engine; the matrix must not be read before end returns. */
int cusk_corr_build_begin(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, size_t m, size_t N, size_t p,
                          const float *mean_dev, const float *std_dev, float *C_dev);
int cusk_corr_build_end(cusk_engine *e, float *mxp_host);
int cusk_corr_build_pending(const cusk_engine *e); /* 1 while a cusk_corr_build_begin has not been ended */
/* The correlation matrices of MANY LD blocks in one set of launches, written onto the diagonal of the n x n batch
 * allocation C_dev that cusk_run_skeleton_batch sweeps (cli.cpp:543-649 once per block in the reference).  Inputs are the
 * device-resident arrays of cusk_blockset_stage: bed_dev = marker 0 of the file set (ceil(N/4) bytes per marker),
 * mean_dev / std_dev indexed by global marker, phen_dev column-major p x N.  Block b = markers first_marker[b] ..
 * first_marker[b] + markers[b] - 1, variables base[b] .. base[b] + markers[b] + p - 1 of the allocation (markers, then the
 * p traits; base[b] a multiple of 64).  Host arrays of nblk entries.
 *   _mxp : marker x trait correlations of every block, into C_dev (both triangles) and, block after block, into the host
 *          array mxp_host (sum markers[b] x p floats, row-major) for the prefilter (cli.cpp:561-576); returns when they
 *          are there.
 *   _mxm : marker x marker (Kendall-npn on the FP4 matrix pipe), trait x trait and the unit diagonal of the blocks with
 *          keep[b] != 0 (keep = NULL: all); asynchronous on the engine's stream. */
/* both in one call, _mxm speculatively for EVERY block: returns when the marker x trait correlations are in mxp_host,
 * with the marker x marker part still running on the engine's stream (the caller's prefilter overlaps it) */
int cusk_corr_build_batch(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev,
                          const float *std_dev, size_t N, size_t p, int nblk, const long long *first_marker,
                          const int *markers, const int *base, int n, float *C_dev, float *mxp_host);
int cusk_corr_build_batch_mxp(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev,
                              const float *std_dev, size_t N, size_t p, int nblk, const long long *first_marker,
                              const int *markers, const int *base, int n, float *C_dev, float *mxp_host);
int cusk_corr_build_batch_mxm(cusk_engine *e, const unsigned char *bed_dev, const float *phen_dev, const float *mean_dev,
                              const float *std_dev, size_t N, size_t p, int nblk, const long long *first_marker,
                              const int *markers, const int *base, const unsigned char *keep, int n, float *C_dev);
/* cusk_corr_build for k markers that are NOT contiguous in the .bed: the markers of the build are the rows
 * marker_ix[0 .. k-1] (HOST array; ascending, distinct, < m_total) of a .bed of m_total markers -- the union of the markers
 * all LD blocks selected (merged_blocks.ixs), scattered over every chromosome; the reference has no counterpart, its
 * `cuskss` takes their LD from a file (cli.cpp:294-338).  mean / std are indexed by GLOBAL marker (m_total entries).  bed,
 * mean and std may each be host memory or device-resident (cusk_blockset_stage's copies, any cusk_dev_alloc): resident
 * rows are packed into contiguous engine scratch by a row-gather kernel, of host arrays only the selected rows are
 * uploaded; the kernels of cusk_corr_build then run on the packed rows, so the n x n matrix (n = k + p, selected markers in
 * index order, then traits) and mxp_host (k x p, may be NULL) are bit for bit those of cusk_corr_build on the k rows made
 * contiguous by the caller.  C_dev = NULL: marker x trait correlations only. */
int cusk_corr_build_indexed(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                            size_t m_total, size_t N, size_t p, const float *mean, const float *std, float *C_dev,
                            float *mxp_host);
/* The leading k x k block of the n x n device matrix C_dev in the layout of the `mxm` file of `cuskss`
 * (marker_summary_stats.cpp:8-24): lower triangle INCLUDING the diagonal, row-major, k (k + 1) / 2 floats, NaN (a marker
 * without variance) written as 0 -- what the readers of that file make of it.  out: host memory (out_on_device = 0) or a
 * 16-byte aligned device buffer (1).  Returns when the result is there. */
int cusk_pack_lower_tri(cusk_engine *e, const float *C_dev, size_t n, size_t k, float *out, int out_on_device);
/* NaN -> 0 in place on `count` floats of a device allocation (M_dev 16-byte aligned): what the mxm / mxp / pxp loaders of
 * `cuskss` do to the correlations they read, for a matrix that goes from cusk_corr_build* to cusk_run_hetcor without
 * visiting a file.  Asynchronous on the engine's stream. */
int cusk_nan_to_zero(cusk_engine *e, float *M_dev, size_t count);
/* Host only (no device, no engine): writes the three summary-statistic files of `cuskss` from arrays --
 *   <outdir>/mxm.bin  mxm_tri as it is, k (k + 1) / 2 floats (the layout of cusk_pack_lower_tri), NaN -> 0;
 *   <outdir>/mxp.txt  header "chr snp ref <trait names>", then m_total rows "chr[i] snp[i] ref[i] v1 .. vp" from mxp
 *                     (m_total x p row-major), one per marker of the whole .bim so that marker indices select rows;
 *                     NaN is written as NA;
 *   <outdir>/pxp.txt  header = trait names, then p rows "name v1 .. vp" from pxp_square (p x p row-major); NaN as nan
 * with nine significant digits (%.9g), which the loaders (marker_trait_summary_stats.cpp:40-299,
 * trait_summary_stats.cpp:5-169: text -> float32) read back bit for bit.  Every write and close is checked; on failure
 * the message goes to err (may be NULL) and an error code is returned. */
int cusk_sumstats_write(const char *outdir, const float *mxm_tri, size_t k, const float *mxp, size_t m_total, size_t p,
                        const float *pxp_square, const char *const *chr, const char *const *snp, const char *const *ref,
                        const char *const *trait_names, char *err, size_t err_len);
/* Complete-observation counts of the Pearson blocks of cusk_corr_build / cusk_corr_build_indexed, for phenotype tables
 * with gaps (NaN): the correlation kernels divide by these numbers and drop them, a skeleton run with per-pair sample
 * sizes (cusk_run_hetcor with N_dev) needs them.
 *   mxp_n_host[i * p + t]  individuals for which marker i is not missing (.bed code != 01) and trait t is not NaN
 *   pxp_n_host[a * p + b]  individuals for which neither trait a nor trait b is NaN (symmetric; diagonal: the trait's own)
 * The markers are rows marker_ix[0 .. k-1] of a .bed of m_total rows (HOST array; ascending, distinct), or rows 0 .. k-1 when
 * marker_ix is NULL.  bed and phen (p x N, trait-major) may each be host memory or device-resident; scattered resident
 * rows go through the row-gather scratch of cusk_corr_build_indexed.  Counts are exact 32-bit integers; individuals are
 * 0 .. N-1 whatever the last byte of a row or the memory behind it holds.  Either output may be NULL.  Returns when the
 * counts are there. */
int cusk_pair_counts(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                     size_t m_total, size_t N, size_t p, int *mxp_n_host, int *pxp_n_host);
/* The square sample-size matrix of a block of m markers and p traits, written on the device: N_dev (n x n float32, n =
 * m + p, row-major, a device pointer that may start at any float) receives n_uniform between two markers,
 * mxp_ess[i * p + t] at (i, m + t) and (m + t, i), pxp_ess[a * p + b] at (m + a, m + b) for a != b and NaN on the trait
 * diagonal -- what make_square_cuskss_inputs (cli.cpp:89-173) assembles on the host for `cuskss`.  mxp_ess (m x p) and
 * pxp_ess (p x p) are host arrays (device-resident ones are read in place); either may be NULL when it is empty.
 * Returns when the matrix is written. */
int cusk_ess_square(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, size_t m, size_t p, float n_uniform,
                    float *N_dev);
/* cusk_ess_square for the blocks of a batch, in one launch: block b holds the variables base[b] .. base[b] + m[b] + p of
 * the n x n allocation N_dev (leading dimension n) and receives the (m[b] + p)^2 values of cusk_ess_square in its diagonal
 * block.  mxp_ess: the blocks' m[b] x p tables back to back; pxp_ess: one p x p table per block, back to back (the blocks
 * share the phenotypes, but a size is formed from the correlation it comes with, which is the block's own).  Cells
 * outside the diagonal blocks are NOT written: no kernel reads them.  Errors, each with a message: bases that are not
 * ascending multiples of 64 (or blocks that overlap), a block that reaches beyond n, N_dev not 16-byte aligned.  Returns
 * when the matrix is written. */
int cusk_ess_square_batch(cusk_engine *e, const float *mxp_ess, const float *pxp_ess, int nblk, const int *m, const int *base,
                          size_t p, float n_uniform, int n, float *N_dev);
/* The marker x marker part of a sample-size matrix from the genotypes: for the rows marker_ix[0 .. k-1] of a .bed of m_total
 * rows (HOST array; ascending, distinct; NULL = rows 0 .. k-1; bed host or device-resident, as cusk_pair_counts takes them)
 * N_dev[i * ld + j] = (float)count(i, j) for all i, j < k, where count(i, j) is the number of individuals 0 .. N-1 for which
 * neither marker has the missing code 01 -- the individuals the Pearson correlation of the pair was formed on.  The diagonal
 * receives the marker's own count (nothing reads it).  Cells outside the k x k corner are not touched, so the call goes
 * AFTER cusk_ess_square on the same allocation (ld = m + p), which wrote n_uniform there.  Counts are exact integers and
 * N < 2^24 (an argument error otherwise), so the floats are exact; no standard-error chain is applied (the reference has no
 * file route for marker x marker sizes, and the sweep truncates a size to int).  The corner is bitwise symmetric by
 * construction: a tile and its mirror image are stored from the same integers.  Bits of a row beyond individual N and the
 * memory behind a row do not matter.  Returns when the corner is written. */
int cusk_marker_pair_sizes(cusk_engine *e, const unsigned char *bed, const int *marker_ix, size_t k, size_t m_total, size_t N,
                           float *N_dev, size_t ld);
/* cusk_marker_pair_sizes for the blocks of a batch, in one launch: block b holds its m[b] markers at the variables base[b] ..
 * base[b] + m[b] of the n x n allocation N_dev (leading dimension n; bases as cusk_ess_square_batch takes them) and receives
 * its m[b] x m[b] counts there; nothing outside these corners is written, so the call goes after cusk_ess_square_batch.
 * marker_ix: the .bed rows of all blocks in ONE list, block after block (sum of m[b] entries, each below m_total; a row may
 * occur more than once, since a batch may name a block twice; NULL = rows 0 .. sum - 1). */
int cusk_marker_pair_sizes_batch(cusk_engine *e, const unsigned char *bed, const int *marker_ix, size_t m_total, size_t N, int nblk,
                                 const int *m, const int *base, int n, float *N_dev);
/* Host only.  The sample size the mxp / pxp loaders of `cuskss` make of a correlation and its standard error:
 * ((1 - r^2) / se)^2 with their float / double mix (marker_trait_summary_stats.cpp:161-164). */
float cusk_ess_from_se(float r, float se);
/* Host only.  The standard error to write for a Pearson correlation r estimated on `count` observations:
 * (float)((1 - r^2) / sqrt(count)), moved by at most one ulp so that (int)cusk_ess_from_se(r, se) == count -- the sweep
 * truncates sample sizes to int (mean_ess), and the plain value gives count - 1 for about three pairs in ten.  That
 * holds for every count up to 2,000,000; at 8 million about 9 % of pairs and at 16 million about a third have no such
 * neighbour and get the plain value.  NaN when r is NaN, count <= 0 or r^2 >= 1. */
float cusk_se_from_count(float r, int count);
/* Host only.  <outdir>/mxp_se.txt and <outdir>/pxp_se.txt beside the files of cusk_sumstats_write, in the formats of
 * mxp.txt / pxp.txt (same header and label columns, %.9g): se = cusk_se_from_count(correlation, count) with the counts of
 * cusk_pair_counts (mxp_n m_total x p, pxp_n p x p), NaN where the correlation is NaN (the loaders do not read it there);
 * a NaN goes out as NA in mxp_se and nan in pxp_se.  The diagonal of pxp_se is nan: the pxp loader reads it, and any se
 * beside r = 1 is a sample size of 0 or NaN; NaN it is, on this route and in `mps cuskss-bed ... het` alike (a literal 0
 * would mean 0 / 0 to the loader, which not every reader of these files survives).  Errors as cusk_sumstats_write. */
int cusk_sumstats_write_se(const char *outdir, const float *mxp, const int *mxp_n, size_t m_total, size_t p,
                           const float *pxp_square, const int *pxp_n, const char *const *chr, const char *const *snp,
                           const char *const *ref, const char *const *trait_names, char *err, size_t err_len);
/* Host only.  mxp_se.txt / pxp_se.txt as cusk_sumstats_write_se writes them, from finished standard errors (mxp_se m_total x
 * p, pxp_se p x p) instead of counts: the polychoric / polyserial standard errors of ordinal traits do not come from a
 * count.  NaN goes out as NA in mxp_se and nan in pxp_se; the caller puts NaN on the diagonal of pxp_se. */
int cusk_sumstats_write_se_values(const char *outdir, const float *mxp_se, size_t m_total, size_t p, const float *pxp_se,
                                  const char *const *chr, const char *const *snp, const char *const *ref,
                                  const char *const *trait_names, char *err, size_t err_len);
/* Contingency tables of ordinal traits, counted on the device: the input of cusk_polychoric_fit.  The q ordinal traits are
 * the rows ord_ix[0 .. q-1] (0-based, HOST) of phen (p x N, trait-major, host or device-resident); trait t has the nlev[t]
 * (1 .. 8) levels levels[t * 8 + 0 .. nlev[t] - 1] (HOST, ascending), which must hold every distinct non-NaN value of the
 * trait: an individual whose value is none of them is in no table.  A marker has the three genotype classes of its
 * non-missing .bed codes in the order of the dosage the Pearson build gives them (code 11 -> class 0, 10 -> 1, 00 -> 2).
 *   mxo_tab_host[((i * q + t) * 3 + c) * 8 + u]   individuals with class c of marker i and level u of ordinal trait t
 *   oxo_tab_host[((a * q + b) * 8 + u) * 8 + v]   individuals with level u of ordinal trait a and level v of ordinal trait b
 * k * q * 3 * 8 and q * q * 8 * 8 int32; cells of levels a trait does not have are 0.  Markers, bed, marker_ix, k, m_total
 * and N as cusk_pair_counts takes them, with its guarantees: rows start at any byte, individuals are 0 .. N-1 whatever the
 * last byte of a row or the memory behind it holds, counts are exact.  Either output may be NULL (bed may then be NULL
 * when mxo_tab_host is).  Returns when the tables are there. */
int cusk_ordinal_tables(cusk_engine *e, const unsigned char *bed, const float *phen, const int *marker_ix, size_t k,
                        size_t m_total, size_t N, size_t p, const int *ord_ix, size_t q, const float *levels, const int *nlev,
                        int *mxo_tab_host, int *oxo_tab_host);
/* Polychoric correlations (polycor's two-step form) of ntab contingency tables of ka x kb int32 counts each (ka, kb <= 8;
 * host memory, or device-resident and read in place), one fit per table on the device, in IEEE double: rows and columns
 * without observations are left out; thresholds are the normal quantiles of the cumulative shares; rho maximises
 * sum n_ab log pi_ab(rho) over [-0.9999, 0.9999] with the thresholds held fixed (bivariate normal rectangle probabilities by
 * Genz's algorithm); se = 1 / sqrt(-l''(rho)).  status_out: 0 fitted; 1 boundary -- rho is +-0.9999, or the information is
 * not positive: r is set, se is NaN; 2 degenerate -- a side has fewer than two levels with observations: r and se are NaN.
 * r_out, se_out (double) and status_out (int): ntab values each, HOST.  Returns when they are there. */
int cusk_polychoric_fit(cusk_engine *e, const int *tables, size_t ntab, int ka, int kb, double *r_out, double *se_out,
                        int *status_out);
/* Polyserial correlations (two-step) of the continuous traits cont_ix[0 .. nc-1] with the ordinal traits ord_ix[0 .. q-1]
 * (trait indices into phen, p x N, host or device-resident; levels / nlev as cusk_ordinal_tables takes them), each pair on
 * the individuals for which neither value is NaN: z = (x - mean) / sd (n - 1), thresholds from the ordinal trait's
 * cumulative shares, rho maximises sum_i log[Phi((tau_hi - rho z_i) / sqrt(1 - rho^2)) - Phi((tau_lo - rho z_i) / sqrt(1 -
 * rho^2))]; an individual whose ordinal value is none of the listed levels is left out, as in cusk_ordinal_tables;
 * interval, se and status as cusk_polychoric_fit (degenerate also: fewer than two observations, or a constant
 * x).  Outputs: nc * q values each, pair (c, o) at c * q + o, HOST.  Sums over individuals are formed in a fixed order.
 * Returns when they are there. */
int cusk_polyserial_fit(cusk_engine *e, const float *phen, size_t N, size_t p, const int *cont_ix, size_t nc, const int *ord_ix,
                        size_t q, const float *levels, const int *nlev, double *r_out, double *se_out, int *status_out);
/* M_dev[idx * n + j] = M_dev[j * n + idx] = vals_host[j] for j < n: one variable's row and column of a device-resident n x n
 * matrix replaced from a host vector (the ordinal traits' correlations and sample sizes in `mps cuskss-bed ... het
 * ordinal=`).  Returns when the matrix is written. */
int cusk_matrix_set_cross(cusk_engine *e, float *M_dev, size_t n, size_t idx, const float *vals_host);
/* kernel times of the last calls (ms): [0] table kernel of cusk_ordinal_tables, [1] cusk_polychoric_fit, [2] cusk_polyserial_fit */
void cusk_ordinal_timing(const cusk_engine *e, float *ms3);
/* timing of the last cusk_corr_build: [0] decode, [1] count GEMM, [2] mxp/pxp, [3] total (ms) */
void cusk_corr_timing(const cusk_engine *e, float *ms4);

/* `mps block` (cli.cpp:362-411): cal_mcorrk_banded + marker_corr_banded_mat_row_abs_sums, corr_host.cu:65-128.
 * bed: packed genotypes of the m markers of ONE chromosome, SNP-major, ceil(N/4) bytes each (host).  Computes the
 * banded Kendall-npn correlations band[row * width + col] = corr(row, row + 1 + col) (0 where row + 1 + col >= m) on
 * the device and their forward row sums of absolute values (float accumulation in column order, as the reference's
 * host loop).  rowsums_host: m floats out.  band_host: m * width floats out, or NULL. */
int cusk_corr_banded(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, size_t width, float *rowsums_host,
                     float *band_host);
/* hanning_smoothing, blocking.cpp:13-35: out[c] = sum_i weight[i] * v[c - window/2 + i] for window/2 <= c < n - window/2,
 * 0 elsewhere; double accumulation in window order on the device (bit-identical to the host loop).  The caller supplies
 * the window weights (0.5 - 0.5 cosf(2 pi i / (window - 1)), blocking.cpp:8-11).  All pointers are host memory. */
int cusk_hanning_smooth(cusk_engine *e, const float *v_host, size_t n, const double *weight_host, int window,
                        double *out_host);
/* Host only.  The window weights `mps block` hands to cusk_hanning_smooth: out[i] = 0.5 - 0.5 cosf(2 pi i / (window - 1)),
 * single-precision cosine (blocking.cpp:8-11), i = 0 .. window-1.  window = 1 gives NaN (0 / 0), as in the reference.
 * CUSK_ERR_ARG for window <= 0 or a null pointer. */
int cusk_hanning_weights(int window, double *out);
/* block_chr, blocking.cpp:102-136: forward row sums of ONE chromosome (cusk_corr_banded) to its LD blocks -- the odd
 * smoothing window is bisected between 3 and n until the largest block is within 100 of, and not above, max_block_size
 * or the window stops moving; each step smooths on the device (cusk_hanning_smooth with cusk_hanning_weights) and cuts at
 * the strict local minima on the host.  This is the code `mps block` runs.  first / last (host, cap entries each)
 * receive the chromosome-local marker indices of the blocks, inclusive, in order; *count their number.  n blocks are
 * always enough.  CUSK_ERR_ARG with *count = the number needed when cap is smaller (nothing is written then), and for
 * n = 0 or a null pointer; an error of the smoothing is passed on (message in cusk_last_error). */
int cusk_block_chr(cusk_engine *e, const float *row_sums, size_t n, int max_block_size, long long *first, long long *last,
                   size_t cap, size_t *count);

/* `mps prune`: the two things the workflow asks of a fileset before `prep-bed` -- no marker without recorded variation
 * and no pair of markers with a correlation of 1 -- decided on the correlation the skeleton tests (the banded Kendall-npn
 * values of cusk_corr_banded), per chromosome, markers in .bim order, j local to the chromosome:
 *   counts(j)      individuals < N with .bed code 00, 01, 10, 11 (dosage 2, missing, dosage 1, dosage 0); the padding
 *                  codes of the last byte when N % 4 != 0 are not individuals
 *   constant(j)    at most one of the three non-missing counts is non-zero (an all-missing marker is constant)
 *   r(i, j)        for 0 < j - i <= W: band[i * W + (j - i - 1)] of cusk_corr_banded(.., width = W, ..), the same bits
 *   conflict(i, j) fabsf(r(i, j)) >= r_max as floats; NaN gives no conflict
 *   keep(j)        !constant(j) and no i in [max(0, j - W), j) with keep(i) and conflict(i, j)
 *   status(j)      CUSK_PRUNE_CONSTANT if constant, else CUSK_PRUNE_LD if not kept, else CUSK_PRUNE_KEEP
 * A dropped or constant marker never blocks another: the first kept marker wins.  (PLINK's --indep-pairwise prunes on the
 * Pearson r^2 of the dosages and keeps the marker with the higher minor allele frequency; this is neither.)
 * All pointers are host memory.  Argument errors (CUSK_ERR_ARG, message in cusk_last_error, nothing launched): a null
 * pointer, m == 0, N == 0, W == 0, W > CUSK_PRUNE_MAX_WINDOW, r_max not in (0, 1]. */
enum
{
    CUSK_PRUNE_KEEP = 0,
    CUSK_PRUNE_CONSTANT = 1,
    CUSK_PRUNE_LD = 2
};
#define CUSK_PRUNE_MAX_WINDOW 4096 /* largest W of cusk_ld_prune and cusk_ld_prune_scan */
/* counts_out[j * 4 + c] (int32) = counts(j) for code c = 00, 01, 10, 11, for the m rows of ceil(N / 4) bytes at bed. */
int cusk_genotype_counts(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, int *counts_out);
/* The greedy pass alone, on a caller's conflict bitmap: row i holds ceil(W / 64) little-endian 64-bit words, bit b of
 * word k stands for the pair (i, i + 1 + 64 k + b); constant_flags: one byte per marker (non-zero = constant);
 * status_out: m bytes.  Bits of columns >= W and of pairs with i + 1 + 64 k + b >= m are ignored, whatever they hold. */
int cusk_ld_prune_scan(cusk_engine *e, const unsigned long long *conflict_bits, const unsigned char *constant_flags, size_t m,
                       size_t W, unsigned char *status_out);
/* One chromosome: upload, the banded build of cusk_corr_banded, counts, bitmap, scan, download of the m status bytes (and
 * of the m x 4 counts when counts_out is not NULL).  The float band (m * W * 4 bytes) stays on the device. */
int cusk_ld_prune(cusk_engine *e, const unsigned char *bed, size_t m, size_t N, size_t W, float r_max, unsigned char *status_out,
                  int *counts_out);
/* device time of the phases of the last cusk_ld_prune: [0] upload, [1] band, [2] counts, [3] bitmap, [4] scan (ms) */
void cusk_ld_prune_timing(const cusk_engine *e, float *ms5);
/* Host only.  The fileset <bfiles> without the markers whose status (m_total bytes, one per line of <bfiles>.bim, as
 * cusk_ld_prune gives them chromosome after chromosome) is not CUSK_PRUNE_KEEP:
 *   <out_stem>.bed        the magic bytes, then the kept rows byte for byte
 *   <out_stem>.bim        the kept lines unchanged
 *   <out_stem>.fam        a copy
 *   <out_stem>.prune.in   the kept SNP ids (column 2 of the .bim), one per line, in order
 *   <out_stem>.prune.out  "id<TAB>constant" or "id<TAB>ld" per dropped marker, in order
 * CUSK_ERR_ARG for a null pointer, m_total == 0, out_stem equal to bfiles or an output path that names one of the input
 * files (another spelling, a link), a fileset that cannot be read or whose .bim does not have m_total lines or whose .bed
 * is shorter than they need; CUSK_ERR_STATE when a file cannot be written in full.  A call that fails leaves none of the
 * five files it would have created (files of these names from an earlier call may have been replaced by then, the input
 * never).  The reason goes to stderr. */
int cusk_prune_write(const char *bfiles, const char *out_stem, const unsigned char *status, size_t m_total);

/* `prep-phen`: traits residualised on covariates and standardised, on the device (phen_adjust.hip).  The third precondition
 * the reference's README leaves to the user ("make sure that the trait values are standardized"; its
 * cusk/scripts/phen_prep.py only checks it): the Pearson kernels form sum(y_a * y_b) / #jointly valid and so assume mean 0
 * and POPULATION standard deviation 1 (divisor n, not n - 1) of every trait over its observed values -- the quantity
 * pxp_kernel and the .stds of `mps prep` assume, hence the one used here.
 * Inputs: Y p x N float32 trait-major, X c x N float32 covariate-major, NaN (or +-Inf) = missing; adjust[t] per trait;
 * 0 <= c <= CUSK_PHEN_MAX_COVAR (64 columns with the intercept).  All arithmetic is IEEE double; only out is rounded.
 *   1. A = { i : every X[j, i] is finite }                                     (c == 0: everybody)
 *   2. per covariate mu_j = mean and sigma_j = population sd over A (two passes), xs = (x - mu_j) / sigma_j.  Residuals do
 *      not depend on this map in exact arithmetic; it is there so that the normal equations are formed on a well-scaled
 *      design.  sigma_j == 0 (or A empty): CUSK_ERR_ARG with a message that names j, nothing is written.
 *   3. adjusted traits (adjust[t] != 0 and c > 0): U_t = A and Y[t, i] finite, n_t = |U_t|, z_i = (1, xs_i),
 *      G_t = sum_{U_t} z z', b_t = sum_{U_t} z y; beta_t solves G_t beta = b_t by Cholesky on D^-1/2 G_t D^-1/2
 *      (D = diag G_t, unit diagonal); e_i = y_i - z_i' beta_t, computed from the data, not from G
 *   4. other traits: U_t = { i : Y[t, i] finite }, e = y
 *   5. every trait: m = sum(e) / n_t, s = sqrt(sum((e - m)^2) / n_t) (two passes, the second over the centred values);
 *      out[t, i] = (float)((e_i - m) / s) for i in U_t, NaN elsewhere
 *   6. status[t]: CUSK_PHEN_OK; CUSK_PHEN_SINGULAR when a pivot of the unit-diagonal factorisation is below
 *      CUSK_PHEN_PIVOT_MIN (a pivot is 1 - R^2 of a covariate on the earlier ones over U_t: "explained to eight digits by
 *      the others"; far above the rounding floor c n 2^-53 of a double Gram and far below any design a person would call
 *      non-collinear; part of the rule, not a knob); CUSK_PHEN_TOO_FEW when n_t < c + 2 (not adjusted: n_t < 2) or s == 0.
 *      A trait with status != 0 is all NaN in out, and NaN in mean, sd, beta and r2.
 *   7. every sum over individuals runs over chunks of CUSK_PHEN_CHUNK individuals, in a fixed order inside the chunk; the
 *      chunk partials are added in chunk order.  No floating-point atomics: two calls on the same input give the same bytes.
 * Outputs (HOST; out_host p x N, the others per trait; any of n/mean/sd/beta/r2/status may be NULL): n_out = n_t;
 * mean_out, sd_out = m and s of step 5; beta_out (c + 1) per trait in the units of the RAW covariates, intercept first
 * (NaN for traits that are not adjusted); r2_out = 1 - sum(e^2) / sum((y - ybar)^2) over U_t (NaN when not adjusted).
 * phen and covar may each be host memory or device-resident, as cusk_pair_counts takes phen.  Individuals are 0 .. N-1;
 * nothing behind the arrays is read or written.  CUSK_ERR_ARG (message in cusk_last_error, nothing launched): a null
 * engine, phen, adjust or out_host, N == 0, p == 0, c > CUSK_PHEN_MAX_COVAR, covar NULL with c > 0, N >= 2^31. */
#define CUSK_PHEN_MAX_COVAR 63
#define CUSK_PHEN_CHUNK 4096
#define CUSK_PHEN_PIVOT_MIN 1e-8
enum
{
    CUSK_PHEN_OK = 0,
    CUSK_PHEN_SINGULAR = 1,
    CUSK_PHEN_TOO_FEW = 2
};
int cusk_phen_adjust(cusk_engine *e, const float *phen, const float *covar, size_t N, size_t p, size_t c,
                     const unsigned char *adjust, float *out_host, int *n_out, double *mean_out, double *sd_out,
                     double *beta_out, double *r2_out, int *status_out);
/* The moments of step 5 alone on the values as they are (`check-phen`): n, m and s of every trait over its finite values,
 * with the same chunks and order; n == 0 gives NaN, NaN. */
int cusk_phen_moments(cusk_engine *e, const float *phen, size_t N, size_t p, int *n_out, double *mean_out, double *sd_out);
/* HIP-event times of the last cusk_phen_adjust on e: covariate mask and scaling, Gram partials, their ordered sum and the
 * Cholesky solves, residual moments (both passes), standardise.  ms5: 5 floats. */
void cusk_phen_timing(cusk_engine *e, float *ms5);

/* `prep-phen ... rint`: the rank-based inverse normal transform of traits, on the device (phen_rint.hip).  Every test
 * downstream is a Fisher-z test on Pearson correlations of the traits; a skewed trait or one with a few extreme values
 * biases them, and standardising does not repair that.  vals p x N float32 trait-major, host memory or device-resident as
 * cusk_phen_adjust takes phen; NaN or +-Inf = missing.  For a trait t with select[t] != 0 (select == NULL: every trait):
 *   1. U = { i : vals[t, i] finite }, n = |U|
 *   2. values are ordered as floats, -0.0 equal to +0.0: the key of a value is the usual order-preserving uint32 image of
 *      its bits (sign bit set for a non-negative value, all bits flipped for a negative one) with -0.0 on the image of
 *      +0.0; a missing value has the key 0xFFFFFFFF, which no finite float has, so missing values sort last
 *   3. lo_i = #{ j in U : v_j < v_i }, eq_i = #{ j in U : v_j = v_i }; the average rank r_i = lo_i + (eq_i + 1) / 2 is
 *      carried as the integer rank2_i = 2 lo_i + eq_i + 1 <= 2 N, which fits 32 bits because N < 2^31
 *   4. q_i = ppnd16((r_i - offset) / ((n + 1) - 2 offset)) in IEEE double: Wichura's AS 241 as csrc/ordinal_math.h has it,
 *      without a Newton step; 0 <= offset <= 0.5, 0.375 is Blom's
 *   5. m = sum(q) / n, s = sqrt(sum((q - m)^2) / n), two passes, summed as step 7 of cusk_phen_adjust sums: over chunks of
 *      CUSK_PHEN_CHUNK individuals in a fixed order, the partials added in chunk order, no floating-point atomics;
 *      out[t, i] = (float)((q_i - m) / s) for i in U, NaN elsewhere
 *   6. status[t]: CUSK_PHEN_OK, or CUSK_PHEN_TOO_FEW when n < 2 or s == 0 (every value equal: every score is then
 *      ppnd16(1/2) = 0); then the row of out is all NaN and mean / sd are NaN
 * A trait that is not selected: its row of out_host receives the input row's bytes, n = its count of finite values, mean /
 * sd NaN, status OK, rank2 0.
 * Consequences: equal inputs give bitwise-equal outputs (q is a function of the integer rank2 and n alone); the output is
 * non-decreasing in the input; two calls give the same bytes; nothing depends on how traits are grouped.
 * Outputs (HOST; out_host p x N; n / mean / sd / status per trait; rank2_out p x N: rank2_i, 0 for a missing value; any of
 * n / mean / sd / status / rank2 may be NULL).  Workspace: 4 (Npad + N) bytes per selected trait, Npad = the next power of
 * two >= max(N, cusk_phen_rint_tile()), from the engine's scratch; traits run in groups that keep it within engine option
 * "phen_rint_bytes".  CUSK_ERR_ARG (message in cusk_last_error, nothing launched, no output written): a null engine, vals
 * or out_host, N == 0, p == 0, N >= 2^31, an offset outside [0, 0.5] or NaN, a selected trait whose workspace alone
 * exceeds "phen_rint_bytes". */
int cusk_phen_rint(cusk_engine *e, const float *vals, size_t N, size_t p, const unsigned char *select, double offset,
                   float *out_host, int *n_out, double *mean_out, double *sd_out, int *status_out, unsigned *rank2_out);
/* HIP-event times of the last cusk_phen_rint on e, summed over its groups: keys, sort, ranks, moments + standardise.
 * ms4: 4 floats. */
void cusk_phen_rint_timing(cusk_engine *e, float *ms4);
/* Host only: the keys one workgroup sorts in LDS (a power of two). */
size_t cusk_phen_rint_tile(void);

/* Host only.  A trait or covariate table read and aligned to a .fam (host/phen_table.h).  Whitespace-separated text; the
 * header names two id columns, FID and IID in either order (IID may be called EID), then the value columns; NA tokens are
 * NA, NaN, nan, NAN; any other token that is not a number is an error with its line and column, as are a row of another
 * width, a duplicate IID, a header without the id columns and an empty file.  CRLF line ends are accepted; a header alone
 * is a table without rows.  With fam_path the rows are matched to the .fam (FID IID ...) by IID: the result has one row
 * per line of the .fam, in its order, individuals of the .fam that the table does not list are NaN in every column, rows of
 * the table that the .fam does not list are dropped and counted.  Without it (NULL) the rows stand as they come.
 * On failure: an error code, *out = NULL and the message in err (may be NULL). */
typedef struct cusk_phen_table cusk_phen_table;
int cusk_phen_table_load(cusk_phen_table **out, const char *table_path, const char *fam_path, char *err, size_t err_len);
size_t cusk_phen_table_rows(const cusk_phen_table *t);          /* N: lines of the .fam (rows of the table without one) */
size_t cusk_phen_table_cols(const cusk_phen_table *t);          /* value columns */
const char *cusk_phen_table_name(const cusk_phen_table *t, size_t col);
const float *cusk_phen_table_data(const cusk_phen_table *t);    /* cols x N, column-major (trait-major), NaN = NA */
size_t cusk_phen_table_matched(const cusk_phen_table *t);       /* individuals of the .fam found in the table */
size_t cusk_phen_table_dropped(const cusk_phen_table *t);       /* rows of the table the .fam does not list */
int cusk_phen_table_in_order(const cusk_phen_table *t);         /* 1: as many rows as the .fam and the same IID line by line */
void cusk_phen_table_free(cusk_phen_table *t);
/* Host only.  A .phen for the individuals of fam_path, in its order: header "FID\tIID\t<names>", the .fam's own FID and IID,
 * values %.9g (round-trips float32 through the loader of `mps cusk`), NaN as NA.  data: p x N trait-major, N = lines of the
 * .fam.  CUSK_ERR_ARG for null pointers, p == 0, a .fam that cannot be read or does not have N lines, a path that names the
 * .fam; CUSK_ERR_STATE when the file cannot be written in full (it is removed). */
int cusk_phen_write(const char *path, const char *fam_path, const char *const *names, size_t p, const float *data, size_t N,
                    char *err, size_t err_len);

/* `sepselect` / `orient-v-structs` hot loop: cusk_postprocessing/sepselect.py:262-329
 * (MergedCuskResults.find_maximal_and_min_pcorr_sepsets_incr) for a batch of outer pairs, one wavefront per pair.
 * All pointers are HOST memory.
 *   trait_corr  n x p doubles, row-major: corr[v, t] of every variable v with every trait t (merged layout: the
 *               traits are variables 0 .. p-1); the matrix must be symmetric on these entries
 *   pair_i/j    the outer pairs (variable indices), pair_corr[k] = corr[pair_i[k], pair_j[k]]
 *   cand_off    npairs + 1 offsets into cand; cand = the trait neighbours of pair_i[k] in the order the
 *               reference's loop visits them (iteration order of its Python set); ties of the minimum go to the
 *               LAST candidate in that order, as `<=` does at sepselect.py:286
 *   thr         thr[l] = norm.ppf(1 - alpha/2) / sqrt(num_samples - l - 3) (sepselect.py:25-26), l = 0 .. nthr-1,
 *               nthr > longest candidate list
 * Out: sel (cand_off layout) = the accepted traits of pair k in order, sel_len[k] of them (the maximal separating
 * set, :311); flags[k] bit 0 = the round-wise minimum of the partial correlation was passed (:292-294: the pair
 * gets an entry in min_pcorr_sepsets), flags[k] >> 8 = 0 ok, 1 = no candidate had a comparable z (the reference
 * fails on remove(None) there), 2 = a sub-matrix was exactly singular (the reference exits, :12-18).
 * kernel_ms (may be NULL): device time of the selection kernels alone. */
int cusk_sepselect_greedy(cusk_engine *e, const double *trait_corr, long long n, int p, long long npairs,
                          const int *pair_i, const int *pair_j, const double *pair_corr, const long long *cand_off,
                          const int *cand, const double *thr, int nthr, int *sel, int *sel_len, int *flags,
                          float *kernel_ms);
/* The same selection with every decision taken at the sample size of the variables it is about (a merged skeleton
 * found at per-pair sample sizes: `cuskss` with se files, `cuskss-merged --het`).  Arguments and results as above, with
 * the threshold table replaced by
 *   trait_n     n x p int32, row-major, layout of trait_corr: the number of individuals variable v and trait t were both
 *               observed on; must be symmetric on the trait x trait block (rows 0 .. p-1)
 *   pair_n      pair_n[k] = that number for (pair_i[k], pair_j[k])
 *   q           norm.ppf(1 - alpha/2)
 * A decision over the variables V = {i, j} + S + {t}, |S + {t}| = l, is taken against q / sqrt(mean - l - 3), where
 * mean = (sum of the sizes of all (l + 2)(l + 1) / 2 unordered pairs of V) / that count -- the mean_ess of the hetcor
 * sweep, with a 64-bit integer sum and IEEE double division and square root.  A negative or NaN radicand gives a NaN
 * threshold, against which the comparison is false: "not independent" (plain IEEE, nothing is special-cased).  Which
 * candidate a round picks does not depend on the threshold.  A marker's row of trait_n is read only where the marker
 * is i or j.  With every size equal to N the mean is exactly N and the results equal those of cusk_sepselect_greedy
 * with the table built from N. */
int cusk_sepselect_greedy_het(cusk_engine *e, const double *trait_corr, long long n, int p, long long npairs,
                              const int *pair_i, const int *pair_j, const double *pair_corr, const long long *cand_off,
                              const int *cand, const int *trait_n, const int *pair_n, double q, int *sel, int *sel_len,
                              int *flags, float *kernel_ms);

/* `check-ivs` hot loop: the conditional-independence tests of cusk_postprocessing/check_mr_assumptions.py:14-26 (_indep)
 * for a batch of items (x, y | S), with the conditioning sets given once and shared by the items that name them.  All
 * pointers are HOST memory.
 *   trait_corr  n x p doubles, row-major, as for cusk_sepselect_greedy (n >= p, symmetric on the trait rows)
 *   set_off     nsets + 1 offsets into set, set_off[0] = 0; set = trait ids.  At most 127 per set, no duplicate
 *   item_x/y    the tested pair (variable indices, distinct, at least one of them a trait: trait_corr holds no
 *               marker x marker entry); neither may lie in the item's own set
 *   item_set    the item's set, or -1 for the empty set (z of the raw correlation)
 *   thr         thr[l] = norm.ppf(1 - alpha/2) / sqrt(num_samples - l - 3), l = 0 .. p-1: one call serves one alpha
 * Out, in the caller's item order: z[k] = |0.5 log|(1 + rho)/(1 - rho)|| with rho the partial correlation of x and y given
 * S, from the 2 x 2 Schur complement of S (W = C[S,S]^-1 by Gauss-Jordan with partial pivoting, once per set):
 * rho = (c_xy - c_xS' W c_yS) / sqrt(|(1 - c_xS' W c_xS)(1 - c_yS' W c_yS)|) -- the reference's value from the inverse
 * over [x, y] + S up to rounding.  flags[k] bit 0 = independent (z < thr[|S|]; a NaN on either side compares false:
 * dependent, nothing is special-cased); flags[k] >> 8 = 0 ok, 2 = the set's sub-matrix is exactly singular (z is NaN
 * then; items of other sets are not affected).
 * Argument errors (CUSK_ERR_ARG, message in cusk_last_error, nothing launched): a set longer than 127, a duplicate or
 * an id outside [0, p) in a set, an item whose x or y lies in its set or outside [0, n), x equal to y, x and y both
 * markers, a set index outside [-1, nsets).
 * kernel_ms (may be NULL): device time of the set-up and item kernels alone. */
int cusk_iv_check(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off, const int *set,
                  long long nitems, const int *item_x, const int *item_y, const int *item_set, const double *thr, double *z,
                  int *flags, float *kernel_ms);
/* The same tests, each decided at the sample sizes of the variables it is about: thr is replaced by trait_n (n x p int32,
 * layout of trait_corr, symmetric on the trait x trait block) and q = norm.ppf(1 - alpha/2).  A test over V = {x, y} + S,
 * |S| = l, is decided against q / sqrt(mean - l - 3), mean = (64-bit sum of the sizes of all (l + 2)(l + 1) / 2 unordered
 * pairs of V) / that count: the rule of cusk_sepselect_greedy_het.  z does not depend on the sizes; with every size equal
 * to N the mean is exactly N and flags equal those of cusk_iv_check with the table built from N. */
int cusk_iv_check_het(cusk_engine *e, const double *trait_corr, long long n, int p, int nsets, const int *set_off,
                      const int *set, long long nitems, const int *item_x, const int *item_y, const int *item_set,
                      const int *trait_n, double q, double *z, int *flags, float *kernel_ms);

/* `mvivw`: multivariable inverse-variance-weighted regression of every outcome trait of a merged skeleton on its exposures
 * (the step of mvivw/cig_mvivw.R and cig_mvivw_filtered.R), many independent problems in one call.  All pointers are HOST
 * memory.
 * NOT the reference's estimator: the reference calls mr_mvivw(..., robust = TRUE) of the R package MendelianRandomization,
 * which uses robustbase::lmrob, an MM-estimator with random subsampling.  Neither R nor that package is on our machines
 * and its program text is not in the reference tree: it can be neither run nor restated, so nothing here claims to equal
 * it.  What is computed is the plain IVW estimator with multiplicative random effects: weighted least squares through the
 * origin with a standard-error inflation.  To our knowledge that is what the package computes with robust = FALSE; nobody
 * has checked this against R.
 *   beta        M x p doubles, row-major: corr[p + r, t] of marker row r (variable p + r) with trait t
 *   weight      M x p doubles, layout of beta: the weight of marker row r in the regression of outcome t; from Python
 *               1 / byse^2 with byse = (1 - beta^2) / sqrt(N - 2), the reference's SE
 *   outcome     nout outcome traits o, each in [0, p)
 *   iv_off/iv   nout + 1 offsets into iv; iv = the instrument rows I of an outcome, in [0, M), strictly ascending; m = |I|
 *   ex_off/ex   nout + 1 offsets into ex; ex = the exposure traits E of an outcome, in [0, p), strictly ascending, without
 *               o; k = |E| <= 127
 *   model       0 default, 1 random, 2 fixed (below)
 * The rule per outcome, IEEE double throughout.  X = beta[I, E], y = beta[I, o], w = weight[I, o].
 *   1. G = X'WX and b = X'Wy, summed over chunks of CUSK_MVIVW_CHUNK consecutive list positions in row order; the chunks
 *      are added in chunk order.  No floating-point atomics: two runs give the same bytes.
 *   2. d_j = sqrt(G_jj), Gs = G / (d d') with a unit diagonal; Cholesky of Gs; a squared pivot below CUSK_PHEN_PIVOT_MIN
 *      (the bound of cusk_phen_adjust: a pivot is 1 - R^2 of an exposure on the earlier ones), or a G_jj that is not
 *      positive, is status 2.
 *   3. theta = D^-1 Gs^-1 D^-1 b; v_j = (Gs^-1)_jj / d_j^2.
 *   4. rss = sum w (y - X theta)^2 in a second pass over the residuals with the same chunks (never y'Wy - theta'b, which
 *      cancels); sigma = sqrt(rss / (m - k)).
 *   5. se_j by model: 1 (random) sqrt(v_j) max(sigma, 1); 2 (fixed) sqrt(v_j); 0 (default) random when m >= 4, else fixed.
 * status[a]: 0 ok; 1 k = 0 or m <= k (the reference's "sufficient_ivs" fails; nothing is computed); 2 rank deficient by
 * the pivot rule; 3 a weight or a value of X or y among the problem's rows is NaN or infinite, or a weight is <= 0.  For
 * status != 0 theta and se of that outcome are NaN; other outcomes of the call are not affected.
 * Out: theta, se at the positions of ex (only [ex_off[a], ex_off[a + 1]) of every outcome is written); stats nout x 3:
 * rss, sigma, the smallest squared pivot (status 1 and 3: NaN, NaN, NaN; status 2: NaN, NaN, the pivot that failed, 0 for
 * a G_jj that is not positive); status nout ints.
 * Argument errors (CUSK_ERR_ARG, message in cusk_last_error, nothing launched, nothing written): an outcome outside
 * [0, p); an instrument outside [0, M) or an instrument list that is not strictly ascending; an exposure list that is not
 * strictly ascending, names the outcome or names a trait outside [0, p); more than 127 exposures; offsets that are not
 * monotone; model outside 0 .. 2; a null pointer.
 * The chunk partials (chunks x (k + 1)(k + 2) / 2 doubles per outcome) are sized from the call; outcomes are processed in
 * groups of at most 256 MB of partials (engine option "mvivw_part_bytes").  kernel_ms (may be NULL): device time of the kernels alone. */
#define CUSK_MVIVW_CHUNK 256
#define CUSK_MVIVW_MAX_EXPOSURES 127
int cusk_mvivw(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, const int *outcome,
               const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, double *theta, double *se,
               double *stats, int *status, float *kernel_ms);

/* `mvivw --ld`: the regressions of cusk_mvivw with CORRELATED instruments, by generalised least squares.  The reference
 * foresaw it (`use_ld` of mvivw/cig_mvivw.R hands the markers' correlation block to mr_mvinput(..., correlation = ...))
 * and hard-codes the switch off.
 * NOT the R package: as above, MendelianRandomization can be neither run nor restated here, and nobody has checked what
 * follows against R.  What is computed is the plain generalised-least-squares estimator
 *   theta = (X' Om^-1 X)^-1 X' Om^-1 y,  Om = diag(s) R diag(s),  s_i = 1 / sqrt(w_i),
 * through a Cholesky factor of R and the rule of cusk_mvivw on the whitened table.  All pointers are HOST memory; beta,
 * weight, outcome, iv_off/iv, ex_off/ex, model and the outputs are those of cusk_mvivw.
 *   ld     M x M doubles, row-major: the LD (correlation) of marker rows.  Only the STRICT LOWER triangle is read, and
 *          of it only the entries ld[I_a, I_b], a > b, of an outcome's instruments; the diagonal is taken as 1
 *   ridge  lambda in [0, 1): every off-diagonal entry read is multiplied by (1 - lambda), i.e. R_l = (1 - l) R + l I
 * The rule per outcome, IEEE double throughout.  I = the instrument list (m rows, in list order), K = k + 1.
 *   1. R is m x m with R_aa = 1 and R_ab = (1 - ridge) ld[max(I_a, I_b), min(I_a, I_b)] (the list ascends, so this is
 *      ld[I_a, I_b] for a > b).
 *   2. R = CC', C lower, right-looking.  A squared pivot that is not >= CUSK_PHEN_PIVOT_MIN (1e-8: the marker is
 *      explained to eight digits by the earlier ones of the list) is status 4.
 *   3. Zw = C^-1 diag(sqrt(w)) (X, y), m x K, by forward substitution.
 *   4. On Zw the rule of cusk_mvivw, steps 1 - 5, with every weight 1: Gram sums over chunks of CUSK_MVIVW_CHUNK list
 *      positions in row order, chunks added in chunk order; Cholesky of the unit-diagonal Gram with the 1e-8 rule (status
 *      2); theta and v; rss = sum r^2 over r = yw - Xw theta in a second pass; sigma = sqrt(rss / (m - k)); se by model.
 *   5. No floating-point atomics; every element of the trailing matrix of step 2 takes its updates in panel order (panels
 *      of 64 columns, each a sum over the panel's columns in ascending order): two runs give the same bytes.
 * status[a], in this order of precedence: 1 k = 0 or m <= k (decided on the host, nothing is computed); 3 a weight or a
 * value of X or y among the problem's rows, or an entry of ld that step 1 reads, is NaN or infinite, or a weight is <= 0;
 * 4 R fails the pivot rule; 2 the Gram of the whitened exposures fails it; 0 ok.  For status != 0 theta and se of the
 * outcome are NaN; other outcomes are not affected.
 * stats nout x 3: rss, sigma, and the smallest squared pivot of R (status 0); NaN, NaN, the pivot of R that failed
 * (status 4); NaN, NaN, the Gram pivot that failed (status 2); NaN, NaN, NaN (status 1 and 3).
 * Argument errors (CUSK_ERR_ARG, nothing launched, nothing written): those of cusk_mvivw; ld null; ridge outside [0, 1)
 * or NaN; an outcome whose m * m * 8 bytes exceed engine option "mvivw_ld_bytes" (default 8 GiB), named in the message.
 * Outcomes run one after another and share one m x m workspace; ld is copied to the device whole (M * M * 8 bytes).
 * Cost: m^3 / 3 multiply-adds per outcome.  kernel_ms (may be NULL): device time from the first to the last kernel. */
int cusk_mvivw_ld(cusk_engine *e, const double *beta, const double *weight, const double *ld, double ridge, long long M, int p,
                  int nout, const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model,
                  double *theta, double *se, double *stats, int *status, float *kernel_ms);

/* `mvivw --robust`: the regressions of cusk_mvivw made resistant to vertical outliers (instruments with a direct effect
 * on the outcome) by iteratively reweighted least squares: Huber weights, then optionally Tukey bisquare weights.
 * NOT the reference's estimator either, and not lmrob, MASS::rlm or the MendelianRandomization package: the reference's
 * robust = TRUE is an MM-estimator with random subsampling that can be neither run nor restated here.  This is a fully
 * stated, deterministic M-estimator of the same family, started from the plain fit and not from an S-estimate, so it has
 * no breakdown guarantee against leverage points.  Nobody has compared it with R.
 * All pointers are HOST memory.  beta, weight, M, p, outcome, iv_off/iv, ex_off/ex, model, the selections X = beta[I, E],
 * y = beta[I, o], w = weight[I, o], m = |I|, k = |E|, the argument rules, the chunks of CUSK_MVIVW_CHUNK list positions
 * and the pivot rule are those of cusk_mvivw.  psi: 1 Huber; 2 Huber, then bisquare from the Huber solution.
 * The rule per outcome, IEEE double throughout.  The standardised residual of row i at theta is
 * e_i = sqrt(w_i) (y_i - x_i theta), x_i theta summed over the exposures in list order.
 *   0. Start: steps 1 - 3 of cusk_mvivw give theta^0, d_j = sqrt(G_jj) and v_j = (G^-1)_jj of the plain weighted Gram;
 *      statuses 1, 2 and 3 as there.  d and v are kept.
 *   1. Scale: s = 1.4826 med_i |e_i|, about zero because the regression goes through the origin.  med is the exact
 *      median of the m absolute values: the middle order statistic, for even m (a + b) * 0.5 of the two middle ones.  It
 *      is selected on the bit patterns of |e_i|, so it does not depend on any order.  s not > 0: status 6 (more than half
 *      the rows are fitted exactly).
 *   2. Huber stage.  With c = 1.345 s, rho_i = 1 where |e_i| <= c, else c / |e_i|.  G_rho = X' diag(w rho) X and
 *      b_rho = X' diag(w rho) y (each weight is the product w_i rho_i, rounded once) over the same chunks in the same
 *      order as step 0, solved by step 2 - 3 of cusk_mvivw (its own unit-diagonal scaling and the 1e-8 pivot rule; a
 *      failure is status 2 and its pivot is reported).  Then e at the new theta and s by step 1 (status 6 applies).
 *      That is one update t -> t + 1.  The outcome has converged after it when
 *        max_j d_j |theta_j^{t+1} - theta_j^t| <= 1e-10 s^{t+1} sqrt(m),  d of step 0.
 *      At most 100 updates; an outcome that has not converged after the 100th is status 5.
 *   3. Bisquare stage (psi = 2 only), from the Huber solution and its e, with s fixed at the Huber stage's last value:
 *      u_i = e_i / (4.685 s), rho_i = (1 - u_i^2)^2 where |u_i| < 1, else 0.  The same update, the same stopping rule
 *      (with the fixed s), its own cap of 100 updates; statuses 2 and 5 as in step 2.
 *   4. Standard errors, Huber's classical form on the plain Gram.  At the last theta, with its e, the last s and the rho
 *      of the last stage evaluated at that e (the "final rho"): psi_i = e_i rho_i; psi'_i = 1 where |e_i| <= 1.345 s, else
 *      0 (Huber); (1 - u_i^2)(1 - 5 u_i^2) where |u_i| < 1, else 0 (bisquare).  A = sum psi_i^2 / (m - k),
 *      B = sum psi'_i / m, both sums over the chunks in chunk order; tau = sqrt(A) / B; B not > 0: status 5.
 *      se_j = sqrt(v_j) f with f by model: 1 (random) max(tau, 1); 2 (fixed) max(tau / s, 1); 0 (default) random when
 *      m >= 4, else fixed.
 * A converged or failed outcome is frozen: no kernel touches its values again, so they depend neither on the other
 * outcomes of the call nor on how the outcomes are grouped ("mvivw_part_bytes").  No floating-point atomics: two runs
 * give the same bytes.
 * status[a]: 0, 1, 2, 3 as cusk_mvivw; 5 not converged (or B not > 0); 6 the scale is not positive.
 * Out: theta, se at the positions of ex.  stats nout x 6: the plain rss = sum e_i^2 at the last theta; s; tau; the
 * smallest squared pivot of the last G_rho; the number of updates of both stages together; sum rho_i (final rho).  rho
 * (may be NULL; layout of iv, only [iv_off[0], iv_off[nout]) is written): the final rho_i of every row; 0 marks an
 * instrument the fit rejected.  For a status other than 0 theta, se, the outcome's rho and its stats are NaN, but
 * stats[3] of status 2 is the pivot that failed (0 for a G_jj that is not positive).
 * Argument errors (CUSK_ERR_ARG, nothing launched, nothing written): those of cusk_mvivw; psi outside 1 .. 2.
 * kernel_ms (may be NULL): device time from the first to the last kernel, the reads of the live count included. */
int cusk_mvivw_robust(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout, const int *outcome,
                      const long long *iv_off, const int *iv, const int *ex_off, const int *ex, int model, int psi, double *theta,
                      double *se, double *stats, int *status, double *rho, float *kernel_ms);
/* The selection of step 1 on its own: out[g] = the median of |vals[seg_off[g] .. seg_off[g + 1])|, g = 0 .. nseg - 1, exact
 * (for an even count (a + b) * 0.5 of the two middle absolute values); NaN for an empty segment.  Host pointers.  The
 * values are ordered by the bit patterns of their absolute values: -0.0 counts as 0, a NaN lies above every number.
 * Argument errors: a null pointer, offsets that are negative or not monotone, a segment of 2^31 values or more. */
int cusk_abs_median(cusk_engine *e, const double *vals, const long long *seg_off, int nseg, double *out);

/* `mvivw --jackknife`: the regressions of cusk_mvivw refitted without each group of an outcome's instruments.  With groups
 * of one instrument that is the leave-one-out table and its prediction residual sum of squares (PRESS); with contiguous
 * blocks of markers it is the delete-one-block jackknife, whose standard error needs no LD matrix.
 * Nothing in the reference computes this and nothing here was compared with R, MR-PRESSO or LDSC.  PRESS is what MR-PRESSO
 * calls the observed global residual sum of squares; the p-value of its global test needs a simulated null and is not
 * computed.  The block jackknife assumes groups wider than the LD range.
 * All pointers are HOST memory.  beta, weight, M, p, outcome, iv_off/iv, ex_off/ex, model, X = beta[I, E], y = beta[I, o],
 * w = weight[I, o], m = |I|, k = |E| are those of cusk_mvivw.
 *   grp_off/grp  nout + 1 offsets into grp; grp = for outcome a its ng + 1 group boundaries, list positions of the outcome's
 *                instrument list, strictly ascending, the first 0 and the last m.  Group g is the run of list positions
 *                [grp[g], grp[g + 1]) and has m_g rows.  An outcome with m = 0 has no boundary, or the single boundary 0.
 * The rule per outcome, IEEE double throughout, no floating-point atomics, every sum in the one order stated: two runs
 * give the same bytes, and an outcome's result depends neither on the other outcomes of the call nor on the engine
 * options "mvivw_part_bytes" and "mvivw_jk_bytes".
 *   0. The plain fit: steps 1 - 5 of cusk_mvivw give theta, se, stats and status, bit for bit what cusk_mvivw returns for
 *      the same call; G and b are the chunk-ordered sums of its step 1.  status != 0: jk_status is that status and nothing
 *      more is computed.
 *   1. Precondition: ng < 2, or a group with m - m_g <= k: jk_status 1, nothing more is computed.
 *   2. Per group g: G_g = sum_{i in g} (w_i x_i) x_i' and b_g = sum_{i in g} (w_i x_i) y_i, each entry one chain of fused
 *      multiply-adds from +0 over the group's rows in ascending order, w_i x_ij rounded first.  A = G - G_g, c = b - b_g,
 *      entry by entry.
 *   3. d_j = sqrt(A_jj), As = A / (d d') with a unit diagonal, Cholesky of As with the pivot rule and both substitutions
 *      exactly as steps 2 - 3 of cusk_mvivw (v is not formed): theta_-g = D^-1 As^-1 D^-1 c.  A squared pivot below
 *      CUSK_PHEN_PIVOT_MIN or an A_jj that is not positive in any group: jk_status 2; the pivot reported is that of the
 *      first such group in group order (0 for an A_jj that is not positive), and every other jackknife output of the
 *      outcome is NaN.
 *   4. Prediction residuals: for i in g, r_i = sqrt(w_i) (y_i - x_i theta_-g), x_i theta_-g one chain of fused multiply-adds
 *      from +0 over the exposures in list order.  The r_i^2 of a group are summed in runs of 256 consecutive rows from the
 *      group's first row, each run in the order of cusk_mvivw's chunk sums, the runs added in run order; PRESS is the sum
 *      of the group sums in the order of step 5.
 *   5. The weighted delete-group jackknife (Busing, Meijer, van der Leeden 1999) for unequal groups, per exposure j.  With
 *      h_g = m / m_g, every sum over groups taken in chunks of 256 consecutive groups, inside a chunk in ascending order
 *      from +0, the chunk sums added in chunk order:
 *        theta_J = theta + sum_g (1 - m_g / m) (theta - theta_-g)          (= ng theta - sum_g (1 - m_g / m) theta_-g)
 *        var_J   = (1 / ng) sum_g ((h_g - 1) (theta - theta_-g) - (theta_J - theta))^2 / (h_g - 1)
 *                                       (= (1 / ng) sum_g (tau_g - theta_J)^2 / (h_g - 1), tau_g = h_g theta - (h_g - 1) theta_-g)
 *        se_J    = sqrt(var_J)
 *      evaluated in the first forms, which do not cancel; h_g - 1 is m / m_g - 1.  With equal groups se_J is the textbook
 *      sqrt((ng - 1) / ng sum (theta_-g - mean)^2).  Also min_g and max_g of theta_-g,j, and the group with the largest
 *      |theta_-g,j - theta_j|, the first such group on ties.  model does not enter steps 1 - 5.
 * Out: theta, se, stats, status as cusk_mvivw (step 0).  jk nex x 4 at the positions of ex: theta_J, se_J, min, max.  jk_arg
 * at the positions of ex: the most influential group, -1 where jk_status != 0.  jk_stats nout x 2: PRESS; the smallest
 * squared pivot over all groups (jk_status 0) or the one that failed (jk_status 2), else NaN.  jk_status nout ints: 0; 1
 * (step 1, or the plain status 1); 2 (step 3, or the plain status 2); 3 (the plain status).  pres (may be NULL; layout of
 * iv, only [iv_off[0], iv_off[nout]) is written): r_i.  refit (may be NULL): sum_a ng_a k_a doubles, outcome-major, then
 * group, then exposure: theta_-g; an outcome with m = 0 and no boundary has ng = 0.  For jk_status != 0 the outcome's jk,
 * PRESS, pres and refit are NaN.
 * Argument errors (CUSK_ERR_ARG, nothing launched, nothing written): those of cusk_mvivw; grp_off null; boundaries that are
 * not strictly ascending from 0 to m; an outcome with m > 0 and no groups (fewer than two boundaries).
 * One workgroup refits one (outcome, group): the cost is ng (k^3 / 3 + m_g k^2 / 2) multiply-adds per outcome.  The
 * refitted estimates (ng k doubles per outcome) stay on the device in batches of at most 1 GiB (engine option
 * "mvivw_jk_bytes").  kernel_ms (may be NULL): device time from the first to the last kernel, with refit the copies of
 * the batches included. */
int cusk_mvivw_jackknife(cusk_engine *e, const double *beta, const double *weight, long long M, int p, int nout,
                         const int *outcome, const long long *iv_off, const int *iv, const int *ex_off, const int *ex,
                         const long long *grp_off, const int *grp, int model, double *theta, double *se, double *stats,
                         int *status, double *jk, int *jk_arg, double *jk_stats, int *jk_status, double *pres, double *refit,
                         float *kernel_ms);

/* out_host[a*k + b] = M_dev[idx[a]*n + idx[b]]: the retained sub-matrix of parent_set.cpp:84-238
 * (reduce_gc / reduce_gcs) without copying the n*n matrix to the host; idx_host has k entries. */
int cusk_gather_submatrix(cusk_engine *e, const float *M_dev, int n, const int *idx_host, int k, float *out_host);
/* the same with the k*k result left on the device (the stage-two matrix of reduced_gcs_cusk, cli.cpp:62-87, never
 * visits the host) */
int cusk_gather_submatrix_dev(cusk_engine *e, const float *M_dev, int n, const int *idx_host, int k, float *out_dev);

/* ---------------------------------------------------------------------------
 * (3) block driver: many LD blocks from one process
 * ------------------------------------------------------------------------ */

/* The reference processes one LD block per `mps cusk` invocation (src/cli.cpp:507-512, README.md:62) and leaves the
 * loop over blocks to the job scheduler.  A block set holds what every such invocation loads again -- .phen, the
 * <bfiles>.dim/.bim/.means/.stds, the .blocks file, the thresholds (cli.cpp:458-497) -- once, maps the .bed, and runs
 * any of its blocks through exactly the code `mps cusk` runs for that block (host/block_pipeline.h), on whichever
 * engine (= GPU) the caller hands in.  This is what the multi-GPU driver (ci-gwas_amd/run_blocks.py: one process per
 * GPU, longest-processing-time assignment of blocks to ranks, one gather of the per-block results) is built on.
 * A block set is read-only after open: several threads may run different blocks at once, each with its own engine. */
typedef struct cusk_blockset cusk_blockset;
typedef struct cusk_block_result cusk_block_result;

typedef struct cusk_block_stats {
    int skipped;            /* 1: no marginally significant marker-trait correlation (cli.cpp:561-576), no result */
    int num_sig;            /* marker-trait correlations at or above Th[0] */
    long long markers;      /* markers of the block */
    long long retained;     /* markers in the result */
    long long tests[2];     /* CI tests of stage one / stage two */
    double ms_inputs, ms_corr, ms_stage1, ms_prune, ms_stage2, ms_reduce; /* wall-clock phases of this block */
    cusk_stats stage[2];    /* engine counters of both stages */
} cusk_block_stats;

/* Same arguments as `mps cusk` without outdir and block index (cli.cpp:432-456).  On failure returns an error code
 * and writes the message (what `mps cusk` would have printed before exit(1)) to err (may be NULL). */
int cusk_blockset_open(cusk_blockset **out, const char *phen_path, const char *bfiles, const char *blocks_path,
                       float alpha, int max_level, int max_level_two, int depth, char *err, size_t err_len);
void cusk_blockset_close(cusk_blockset *bs);
int cusk_blockset_num_blocks(const cusk_blockset *bs);
long long cusk_blockset_num_samples(const cusk_blockset *bs);
int cusk_blockset_num_phen(const cusk_blockset *bs);
/* markers of block i and its output file stem "<chr>_<first>_<last>" (marker_block.h:36-60) */
long long cusk_blockset_block_markers(const cusk_blockset *bs, int block_index);
int cusk_blockset_block_stem(const cusk_blockset *bs, int block_index, char *stem, size_t stem_len);
/* Copies the inputs every block reads -- the packed genotypes of the whole .bed, the phenotypes, the marker means and
 * standard deviations -- to e's device once (288 GB of HBM hold a whole-genome .bed); blocks run on any engine of that
 * device then build their correlations straight from HBM (cusk_corr_build accepts device pointers) instead of copying
 * their slice over PCIe every time.  Optional: without it every block uploads its own slice.  Returns
 * CUSK_ERR_HIP (and stages nothing) when the device memory is not there.  Call before running blocks on that device. */
int cusk_blockset_stage(cusk_blockset *bs, cusk_engine *e);
/* cli.cpp:521-677 for one block on e's device.  *out receives the result (NULL when the block is skipped);
 * stats may be NULL.  Error text: cusk_blockset_last_error (per calling thread). */
int cusk_blockset_run_block(cusk_blockset *bs, cusk_engine *e, int block_index, cusk_block_result **out,
                            cusk_block_stats *stats);
/* the same, naming the block this engine runs next: its correlation build (cusk_corr_build_begin) runs beside this block's
 * sweeps when the inputs are staged in HBM; next_index = -1: none */
int cusk_blockset_run_block_next(cusk_blockset *bs, cusk_engine *e, int block_index, int next_index,
                                 cusk_block_result **out, cusk_block_stats *stats);
const char *cusk_blockset_last_error(void);
/* het = 1: cusk_blockset_run_block / _run_block_next run every block at per-pair sample sizes (`mps cusk ... het`: counts of
 * complete observations from the genotypes and the .phen, cusk_run_skeleton_het for both stages, the prefilter at the
 * marker x trait sizes); cusk_blockset_run_batch then returns an error (batches at per-pair sample sizes have an entry point
 * of their own, cusk_blockset_run_batch_het).  Set it before running blocks; not while other threads run blocks of the set. */
int cusk_blockset_set_het(cusk_blockset *bs, int het);
/* on = 1: the runs of this set at per-pair sample sizes (cusk_blockset_run_block with cusk_blockset_set_het(1),
 * cusk_blockset_run_batch_het) set engine option "het_filter" = 1 on the engine they are given, for both stages
 * (`mps cusk ... het filter`).  Same files; 0 (default) leaves the engine's option as it is.  Set it before running blocks. */
int cusk_blockset_set_het_filter(cusk_blockset *bs, int on);
/* on = 1: the same runs set engine option "het_rows" = 1 on the engine they are given, for both stages (`mps cusk ... het
 * rows`): level 1 on the row-streaming kernel at per-pair sample sizes.  Same files; 0 (default) leaves the engine's option
 * as it is.  Set it before running blocks. */
int cusk_blockset_set_het_rows(cusk_blockset *bs, int on);
/* on = 1: the same runs give every pair of markers of a block the number of individuals both were observed on
 * (cusk_marker_pair_sizes / _batch after cusk_ess_square / _batch) instead of the number of individuals (`mps cusk ... het
 * markers`).  The files CHANGE where markers have missing calls; the stage-two sizes follow through the gather.  An error
 * (with a message in cusk_blockset_last_error) unless cusk_blockset_set_het(bs, 1) came first; on = 0 is always accepted.
 * Set it before running blocks. */
int cusk_blockset_set_het_markers(cusk_blockset *bs, int on);
/* Forgets what the block set keeps for engine e -- its device scratch (block matrices) and the state of a correlation
 * build started ahead -- and releases that memory.  Call before destroying an engine that ran blocks of this set when the
 * set outlives it (cusk_blockset_close releases everything anyway). */
void cusk_blockset_release_engine(cusk_blockset *bs, cusk_engine *e);

/* MANY blocks in one set of device runs (host/batch_pipeline.h): the correlation matrices of all `nblocks` blocks are built
 * by one set of launches, both skeleton stages sweep them in one level loop each (cusk_run_skeleton_batch), one read-out
 * brings the reduced results back.  The reference runs one block per process (cli.cpp:507-512, README.md:62); per block
 * the result -- and every file written from it -- is the one of cusk_blockset_run_block (= `mps cusk` on that block).
 * Needs the inputs on e's device (cusk_blockset_stage; done here when it has not been).  The padded variable count of
 * the batch, sum over blocks of (markers + traits) rounded up to 64, squared, times 4 bytes is the device memory of its
 * matrix: the caller chooses the batches (ci-gwas_amd/run_blocks.py: --batch-vars).  stats may be NULL. */
typedef struct cusk_batch_result cusk_batch_result;
typedef struct cusk_batch_stats {
    int blocks, skipped;                 /* blocks asked for / skipped by the prefilter (cli.cpp:561-576) */
    long long markers, retained;         /* markers of all blocks / markers in the results */
    long long vars_stage1, vars_stage2;  /* padded variable counts of the two batch allocations */
    long long tests[2], canonical[2];    /* executed / canonical CI tests of stage one and two */
    double ms_corr, ms_stage1, ms_prune, ms_stage2, ms_reduce; /* wall-clock phases of the batch */
    cusk_stats stage[2];                 /* engine counters of both stages (whole batch) */
} cusk_batch_stats;
int cusk_blockset_run_batch(cusk_blockset *bs, cusk_engine *e, const int *block_indices, int nblocks,
                            cusk_batch_result **out, cusk_batch_stats *stats);
/* The same at per-pair sample sizes: per block the result -- and every file -- of cusk_blockset_run_block on a set with
 * cusk_blockset_set_het(1).  One count pass (cusk_pair_counts) serves the batch's markers, the sizes of every block go
 * through the cusk_se_from_count -> cusk_ess_from_se chain, the prefilter is the het one, both stages run through
 * cusk_run_skeleton_batch_het with the sizes on the diagonal of a second allocation (cusk_ess_square_batch; stage two:
 * gathered by the index tables that gather the correlations).  Works on any block set, whatever cusk_blockset_set_het
 * says.  Device memory: correlations and sizes, 2 x 4 x (padded variable count)^2 bytes for stage one.  The count and size
 * phases are part of ms_corr. */
int cusk_blockset_run_batch_het(cusk_blockset *bs, cusk_engine *e, const int *block_indices, int nblocks,
                                cusk_batch_result **out, cusk_batch_stats *stats);
int cusk_batch_result_count(const cusk_batch_result *r);                       /* blocks with a result */
int cusk_batch_result_block_index(const cusk_batch_result *r, int i);          /* index of result i in the .blocks file */
const cusk_block_result *cusk_batch_result_block(const cusk_batch_result *r, int i); /* borrowed; accessors below */
int cusk_batch_result_write(const cusk_batch_result *r, const char *outdir);   /* every block's five files */
/* the results as one byte string (the multi-GPU job gathers these to rank 0): per block six int32 {block index, num_var,
 * num_phen, max_level, 1, length of the stem} + stem + .ixs + .adj + .corr + .sep contents */
size_t cusk_batch_result_packed_bytes(const cusk_batch_result *r);
int cusk_batch_result_pack(const cusk_batch_result *r, void *buf, size_t bytes);
int cusk_packed_results_write(const void *buf, size_t bytes, const char *outdir, int *blocks_written);
/* the same byte string without the .sep arrays (nine tenths of the bytes; with_sep = 0): what the merge below needs.
 * with_sep = 2: the separating sets as a list instead of the dense num_var^2 x max_level array -- head word 4 = 2, then an int32
 * count and count records {int32 row, column, length, int32 members[14]} in ascending (row, column) order; understood by
 * cusk_packed_results_write and cusk_merge_packed (not by the reference-side Python unpacker: use it between library calls). */
size_t cusk_batch_result_packed_bytes_ex(const cusk_batch_result *r, int with_sep);
int cusk_batch_result_pack_ex(const cusk_batch_result *r, void *buf, size_t bytes, int with_sep);
/* host only: how many of the count marker-trait correlations pass the reference's pre-filter |atanh(c)| >= th0 (cli.cpp:561-565,
 * in that expression's float arithmetic) -- the num_sig of cusk_block_stats, 0 skips a block; -1 if mxp is NULL */
int cusk_count_significant(const float *mxp, size_t count, float th0);
/* `merge-block-outputs` (cusk_postprocessing/merge_blocks.py:361-395 + write_mm :298-325) on the packed results of a whole
 * job, in memory: writes <basepath>_sam.mtx, <basepath>_scm.mtx, <basepath>.mdim, <basepath>.ixs -- the files the
 * reference's merge writes from the per-block files, byte for byte.  blockfile = the job's .blocks file (order of the
 * blocks; a listed block without a result counts as skipped, as a block without files does there). */
int cusk_merge_packed(const char *blockfile, const void *buf, size_t bytes, const char *basepath);
void cusk_batch_result_free(cusk_batch_result *r);
/* the reduced result of one block: what ReducedGCS::to_file writes (include/mps/parent_set.h:42-52) */
void cusk_block_result_dims(const cusk_block_result *r, long long *num_var, long long *num_phen, long long *max_level);
const char *cusk_block_result_stem(const cusk_block_result *r);
const int *cusk_block_result_ixs(const cusk_block_result *r);    /* num_var */
const int *cusk_block_result_adj(const cusk_block_result *r);    /* num_var^2 */
const float *cusk_block_result_corr(const cusk_block_result *r); /* num_var^2 */
const int *cusk_block_result_sep(const cusk_block_result *r);    /* num_var^2 * max_level */
/* <outdir>/<stem>.mdim .ixs .adj .corr .sep */
int cusk_block_result_write(const cusk_block_result *r, const char *outdir);
void cusk_block_result_free(cusk_block_result *r);

/* device -> host copy ordered after the engine's work; waits for the engine's stream only */
int cusk_engine_download(cusk_engine *e, void *dst_host, const void *src_dev, size_t bytes);

/* device memory helpers so that C hosts need no HIP headers */
void *cusk_dev_alloc(size_t bytes);
void cusk_dev_free(void *p);
int cusk_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int cusk_dev_download(void *dst_host, const void *src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* CUSK_HIP_H_ */
