// corr_kernels.h -- the kernels of the correlation build behind host launchers.  A kernel is launched only from the file that defines
// it (corr_mxm.hip: SNP x SNP, corr_mxp.hip: SNP x trait, trait x trait); the drivers (corr_build.hip, corr_banded.hip) call these
// functions.  A launcher builds the grid and picks the template argument from its own alignment predicate; single, batched and banded
// callers pass the same arguments, null tables where they have none.  .bed 2-bit codes, low bits first: 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0.
#pragma once
#include "cusk_internal.h"
#include "host/corr_plan.h"  // CorrBatchBlock, CorrTile2 / CorrTile4, kMT

namespace cusk {

typedef float v16f __attribute__((ext_vector_type(16)));
// tile constants the launchers and drivers need (kMT: host/corr_plan.h)
constexpr int kTile = 32;         // marker pairs per tile side of mxm_popcount_kernel
constexpr int kMaxPhenRegs = 32;  // traits per launch of mxp_kernel and mxp_mfma_kernel
constexpr int kMxpWaves = 8;      // waves of mxp_mfma_kernel
constexpr int kMxbTraits = 21;    // traits per launch of mxp_bf16_kernel: 3 x 21 piece columns <= 64, 21 flags + the ones column <= 32
constexpr int kMxbCols = 96;
constexpr int kMxbWaves = 4;  // one wave per SIMD: two marker tiles x five products = 160 accumulator registers per wave

// every row of the .bed block starts on a 16-byte boundary: the FAST forms of mxm_fp4_kernel and mxp_bf16_kernel
inline bool bed_rows16(const unsigned char *bed, size_t clb) { return (clb % 16 == 0) && ((reinterpret_cast<uintptr_t>(bed) & 15u) == 0); }

// ---- corr_mxm.hip ----
// mxm_fp4_kernel: square output (band_w = 0, no table), banded output (band_w > 0) or the ntab tiles of a batch (m = 0)
struct MxmFp4Args
{
    const unsigned char *bed;
    float *C;
    size_t m, N, clb, n, band_w;
    const CorrTile4 *btile;
    size_t ntab;
    const CorrBatchBlock *bblk;
};
void launch_mxm_fp4(hipStream_t s, const MxmFp4Args &a);
void launch_mxm_int8(hipStream_t s, const unsigned char *bed, float *C, size_t m, size_t N, size_t clb, size_t n);
int launch_mxm_popcount(cusk_engine *e, hipStream_t s, const unsigned char *bed, float *C, size_t m, size_t N, size_t clb, size_t n,
                        hipEvent_t between);  // bit planes (engine scratch), `between` recorded when not null, then the popcount tiles
void launch_unit_diag(hipStream_t s, float *C, size_t n);
void launch_extract_tri(hipStream_t s, const float *C, float *out, size_t lo, size_t cnt, size_t n);  // rows / columns [lo, lo + cnt) of C
void launch_batch_finish(hipStream_t s, float *C, size_t n, const CorrBatchBlock *bblk, const int *kept, size_t nkept, const float *pxp, size_t p);

// ---- corr_mxp.hip ----
// The whole SNP x trait sequence.  The CALLER decides the form, and the two callers decide differently:
//   single build (corr_build_impl):  corr_popcount -> Scalar;  corr_mxp_f32 -> F32;  else Bf16
//   batch (batch_mxp):               corr_mxp_f32 -> F32;  else Bf16;  never Scalar
// (the SNP x SNP part of a batch always runs FP4: corr_popcount and corr_fp4 do not reach it).
enum class MxpForm { Scalar, F32, Bf16 };
struct MxpArgs
{
    MxpForm form;
    const unsigned char *bed;
    const float *phen, *mean, *sd;
    float *C, *mxp;            // either may be null
    size_t m, N, p, clb, n;    // m = 0 with a tile table
    int ntiles;                // 32-marker tiles: (m + 31) / 32, or the entries of mtile
    const CorrTile2 *mtile;
    const CorrBatchBlock *bblk;
};
int launch_mxp(cusk_engine *e, hipStream_t s, const MxpArgs &a);
void launch_pxp(hipStream_t s, const float *phen, float *C, size_t m, size_t N, size_t p, size_t n);  // nothing when p < 2

}  // namespace cusk
