// square_inputs.h -- the two rules that decide what a pair of variables is tested with, each written once: the sample size
// of a pair from its count of complete observations, and which cells the estimates of an ordinal trait replace.  Every
// command that looks at a pair (`mps cusk ... het`, the batched block runs, `mps sumstats ... se`, `mps cuskss-bed ... het`)
// goes through these functions, so a pair gets the same size and the same correlation wherever it is looked at.
//
// Pure host code: no engine calls, no I/O (cusk_se_from_count / cusk_ess_from_se are host arithmetic, sumstats_api.cpp).
// tools/square_inputs_selftest.cpp restates both rules per cell and compares bit patterns.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../../include/cusk_hip.h"
#include "ordinal_host.h"

namespace host {

// The sample sizes of a block at per-pair sample sizes, as `cuskss` would load them from the files of `mps sumstats ... se`
// and as `mps cuskss-bed ... het` forms them: the count of complete observations through the standard error such a file
// would hold (cusk_se_from_count -> cusk_ess_from_se), NaN where the correlation is NaN and on the trait diagonal.  pxp
// (p x p correlations) and pxp_n are read as the pxp loader reads them: the upper triangle, mirrored.
inline void block_sample_sizes(const float *mxp, const int *mxp_n, const float *pxp, const int *pxp_n, size_t m, size_t p,
                               std::vector<float> &mxp_ess, std::vector<float> &pxp_ess)
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    auto ess_of = [&](float r, int count) { return std::isnan(r) ? nan : cusk_ess_from_se(r, cusk_se_from_count(r, count)); };
    mxp_ess.resize(m * p);
    pxp_ess.assign(p * p, nan);
    for (size_t i = 0; i < m * p; i++) mxp_ess[i] = ess_of(mxp[i], mxp_n[i]);
    for (size_t a = 0; a < p; a++)
        for (size_t b = a + 1; b < p; b++) pxp_ess[a * p + b] = pxp_ess[b * p + a] = ess_of(pxp[a * p + b], pxp_n[a * p + b]);
}

// The n x n host matrix of sample sizes (k markers, then p traits) from the tables of block_sample_sizes: `uniform` between
// markers, or the k x k table `corner` (jointly genotyped individuals per pair of markers) when there is one; mxp_ess in
// both marker x trait parts; pxp_ess as it stands.  The layout cusk_ess_square gives the same tables on the device.
inline std::vector<float> square_sample_sizes(const std::vector<float> &mxp_ess, const std::vector<float> &pxp_ess, size_t k, size_t p,
                                              float uniform, const float *corner = nullptr)
{
    const size_t n = k + p;
    std::vector<float> ess(n * n, uniform);
    for (size_t i = 0; i < k; i++)
    {
        if (corner) std::copy_n(corner + i * k, k, &ess[i * n]);
        for (size_t t = 0; t < p; t++) ess[i * n + k + t] = ess[(k + t) * n + i] = mxp_ess[i * p + t];
    }
    for (size_t a = 0; a < p; a++) std::copy_n(&pxp_ess[a * p], p, &ess[(k + a) * n + k]);
    return ess;
}

// the sample size the loaders make of an estimate and its standard error; no correlation, no size
inline float size_from_se(float r, float se) { return std::isnan(r) ? std::numeric_limits<float>::quiet_NaN() : cusk_ess_from_se(r, se); }

// The ordinal overlay (`ordinal=`): every pair of a variable with an ordinal trait gets that trait's polychoric / polyserial
// estimate and its standard error instead of the Pearson value and the count's.  ix: the ordinal traits (0-based, q of
// them); mr / mse: rows x q estimates of `rows` markers (ordinal_marker_estimates); te: the p x q estimates between traits
// (NULL: markers only -- a later chunk of markers).  The sink is told each cell once: marker_trait(i, o, r, se) for marker
// row i and trait o, trait_trait(a, b, r, se) for both orientations of a pair of traits; a trait with itself is skipped.
template <class Sink>
void visit_ordinal_pairs(const std::vector<int> &ix, size_t rows, const float *mr, const float *mse, size_t p, const OrdinalTraitEstimates *te,
                         Sink &&sink)
{
    const size_t q = ix.size();
    for (size_t t = 0; t < q; t++)
    {
        const size_t o = (size_t)ix[t];
        for (size_t i = 0; i < rows; i++) sink.marker_trait(i, o, mr[i * q + t], mse[i * q + t]);
        for (size_t a = 0; te && a < p; a++)
        {
            if (a == o) continue;
            sink.trait_trait(a, o, te->r[a * q + t], te->se[a * q + t]);
            sink.trait_trait(o, a, te->r[a * q + t], te->se[a * q + t]);
        }
    }
}

// the file layout of `mps sumstats`: mxp / mxp_se (rows x p, the rows the estimates belong to), pxp / pxp_se (p x p)
struct OrdinalFileSink
{
    float *mxp, *mxp_se, *pxp, *pxp_se;
    size_t p;
    void marker_trait(size_t i, size_t o, float r, float se) { mxp[i * p + o] = r, mxp_se[i * p + o] = se; }
    void trait_trait(size_t a, size_t b, float r, float se) { pxp[a * p + b] = r, pxp_se[a * p + b] = se; }
};

// the square layout of `mps cuskss-bed` (k markers, then p traits; n = k + p): the sizes go into the n x n matrix `ess`, the
// correlations into `cross` (q x n), row t = what column k + ix[t] of the correlation matrix becomes (1 on its diagonal)
struct OrdinalSquareSink
{
    float *cross, *ess;
    size_t k, n;
    std::vector<int> t_of;  // trait -> its place in ix, -1 for a continuous trait
    OrdinalSquareSink(const std::vector<int> &ix, size_t k_, size_t p, float *cross_, float *ess_) : cross(cross_), ess(ess_), k(k_), n(k_ + p), t_of(p, -1)
    {
        for (size_t t = 0; t < ix.size(); t++)
        {
            t_of[(size_t)ix[t]] = (int)t;
            cross[t * n + k + (size_t)ix[t]] = 1.0f;
        }
    }
    void marker_trait(size_t i, size_t o, float r, float se)
    {
        cross[(size_t)t_of[o] * n + i] = r;
        ess[i * n + k + o] = ess[(k + o) * n + i] = size_from_se(r, se);
    }
    void trait_trait(size_t a, size_t b, float r, float se)
    {
        if (t_of[b] >= 0) cross[(size_t)t_of[b] * n + k + a] = r;
        ess[(k + a) * n + k + b] = size_from_se(r, se);
    }
};

}  // namespace host
