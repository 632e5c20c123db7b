// level_policy.h -- the decisions of the level loop (level_loop.hip) as functions of plain values: no HIP, no engine
// state, so that the stand-alone program tools/level_policy_selftest.cpp tabulates them under the host sanitizers.
#pragma once
#include <cmath>

namespace cusk {

inline unsigned long long binom_sat(int n, int k)
{
    if (k < 0 || k > n) return 0;
    if (k > n - k) k = n - k;
    unsigned long long r = 1;
    const unsigned long long cap = 1ull << 62;
    for (int i = 1; i <= k; i++)
    {
        unsigned long long f = (unsigned long long)(n - k + i);
        if (r > cap / f) return cap;
        r = r * f / (unsigned long long)i;
    }
    return r;
}

// loc_th of the hetcor engine when every pair has the same effective sample size:
// the float running sum of (int)ess over (l+2)(l+1)/2 pairs, as mean_ess forms it
// (hetcor-cuPC-S.cu:3068-3088), then th / sqrt(mean_ess - l - 3) in double (:471,:612).
inline float uniform_ess_threshold(float th, float ess, int l)
{
    int t;
    if (ess != ess)
        t = 0;
    else if (ess >= 2147483648.0f)
        t = 2147483647;
    else if (ess <= -2147483648.0f)
        t = (-2147483647 - 1);
    else
        t = (int)ess;
    const int pairs = (l + 2) * (l + 1) / 2;
    float s = 0.0f;
    for (int i = 0; i < pairs; i++) s += (float)t;
    const float me = s / (float)pairs;
    return (float)((double)th / std::sqrt((double)me - (double)l - 3.0));
}

// The kernel that sweeps degree class c of level l.  use_pair / tmaj / use_fast: the level's plan; exact_only: the level is redone
// after a recheck-queue overflow; vec / validate: the options; vec_lds_fits: the one-wavefront kernel's LDS carve of the class fits.
enum class SweepKind { Pair, Tmaj, Vec, Fast, Exact };
inline SweepKind sweep_kind(int l, int c, bool het, bool use_pair, bool tmaj, bool use_fast, bool exact_only, bool vec, bool validate,
                            bool vec_lds_fits, int num_classes, int vec_max_level)
{
    if (exact_only) return SweepKind::Exact;
    if (use_pair) return SweepKind::Pair;
    if (!use_fast) return SweepKind::Exact;
    if (tmaj) return SweepKind::Tmaj;
    if (!het && vec && !validate && c < num_classes - 1 && vec_lds_fits && l < vec_max_level) return SweepKind::Vec;
    return SweepKind::Fast;
}

// Classes that can hold work at a level: a row of degree d belongs to the first class with d <= cap, no degree exceeds
// maxdeg_bound, rows too large to stage all go to the last class.  known_items: nitems[] holds the real counts.  -> their number
inline int classes_with_work(bool known_items, const long long *nitems, int staged_classes, int maxdeg_bound, const int *caps,
                             int num_classes, bool *may)
{
    int nonempty = 0;
    for (int c = 0; c < num_classes; c++)
    {
        if (known_items)
            may[c] = nitems[c] > 0;
        else if (c < staged_classes)
            may[c] = (c == 0 ? 0 : caps[c - 1] + 1) <= maxdeg_bound;
        else
            may[c] = (c == num_classes - 1) && (staged_classes == 0 || maxdeg_bound > caps[staged_classes - 1]);
        nonempty += may[c];
    }
    return nonempty;
}

// What follows the read-back of the control block.  ended: first level whose gate stayed closed (0: none); last_ran: the
// level before it, or the last one enqueued; fast_pending / tmaj: last_ran went through the filter and was not redone yet /
// was swept by unions; queue_overflow: its recheck queue overflowed; binom_overflow, item_overflow: flags of level `ended`.
enum class AfterReadBack
{
    Done,           // levels 1..level ran to completion
    RedoExact,      // sweep `level` again on the exact path, resume behind it (everything the fast pass recorded stays valid)
    ReplanTmaj,     // its work items count unions, not conditioning sets: plan `level` again for the exact kernels
    GrowItems,      // more work items at `level` than the buffers hold: grow them and take the level up again
    BinomOverflow,  // C(degree, level) exceeds 2^62: the run fails
};
struct ReadBack { AfterReadBack what; int level; };
inline ReadBack after_read_back(int ended, int last_ran, bool sharded, bool fast_pending, bool tmaj, bool queue_overflow,
                                bool binom_overflow, bool item_overflow)
{
    // an overflowed queue: that level was not finalised, nothing after it ran (a sharded run finishes it before its exchange)
    if (!sharded && last_ran >= 2 && fast_pending && queue_overflow)
        return {tmaj ? AfterReadBack::ReplanTmaj : AfterReadBack::RedoExact, last_ran};
    if (ended && binom_overflow) return {AfterReadBack::BinomOverflow, ended};
    if (ended && item_overflow) return {AfterReadBack::GrowItems, ended};
    return {AfterReadBack::Done, last_ran};
}

}  // namespace cusk
