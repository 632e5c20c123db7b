// prefilter.h -- does a block have a marker-trait correlation worth a skeleton run?  The two counts behind "No significant
// correlations found. Skipping block.": at one sample size for all pairs, and at per-pair sample sizes.  Plain host
// arithmetic, no engine.
#pragma once
#include <cmath>
#include <cstddef>

namespace host {

// cli.cpp:561-565: how many marker-trait correlations have |atanh c| >= th0.  That is a comparison of |c| with t = tanh(th0):
// only the elements near t, NaN and |c| >= 1 go through the reference's expression -- its two logs per element cost 0.7 ms
// on the 200,000 correlations of a 10k-SNP x 20-trait block.  The expression works in float (<math.h> gives the float
// overloads): rounding 1 + c and 1 - c (2^-24 relative each) moves z = 0.5 (log - log) by up to 2^-24, the float logs and
// their difference add a few ulp of z, and |dc| = (1 - c^2) |dz| stays below 2^-22 + 1e-6 |c|.  That is absolute, not
// relative to t: at th0 = 0.0055 (N = 500k) it is 1e-5 of t, ten times the 1e-6 band this used to have.  The band is
// 2^-20 + 1e-5 t, four times both terms.
inline int count_significant(const float *mxp, size_t count, float th0)
{
    const double t = std::tanh((double)th0), band = 0x1p-20 + 1e-5 * t;
    const double c_lo = t - band, c_hi = t + band;
    int num_sig = 0;
    for (size_t i = 0; i < count; i++)
    {
        const float c = mxp[i];
        const double ac = std::fabs((double)c);
        if (ac < c_lo) continue;
        if (ac > c_hi && ac < 1.0)
        {
            num_sig++;
            continue;
        }
        num_sig += (std::fabs(0.5 * (std::log(std::fabs((1 + c))) - std::log(std::fabs(1 - c)))) >= th0);
    }
    return num_sig;
}

// The prefilter of a run at per-pair sample sizes (`mps cusk ... het`): a marker-trait pair counts when its correlation is
// not NaN and level 0 of cusk_run_skeleton_het keeps its edge.  This is the expression that kernel's verdicts are
// certified against (level0.hip: its single-precision estimate settles an element only outside a 1e-3 band around the
// threshold and hands everything else to this arithmetic; ci_exact.h: z_below / fisher_z_ratio), evaluated for every
// element, so the count cannot disagree with the sweep the way a second formula with its own rounding could: a block is
// skipped exactly when level 0 would leave no marker-trait edge with a defined correlation.  A NaN size, or one of 3 or
// less, gives a NaN threshold or a NaN comparison: false, the edge stays, the pair counts.
inline int count_significant_het(const float *mxp, const float *mxp_ess, size_t count, float th)
{
    int num_sig = 0;
    for (size_t i = 0; i < count; i++)
    {
        const float c = mxp[i];
        if (c != c) continue;
        const float lth = (float)((double)th / std::sqrt((double)mxp_ess[i] - 3.0));
        const float q = (1.0f + c) / (1.0f - c);
        const float z = std::fabs(0.5f * (float)std::log((double)std::fabs(q)));
        num_sig += !(z < lth);
    }
    return num_sig;
}

}  // namespace host
