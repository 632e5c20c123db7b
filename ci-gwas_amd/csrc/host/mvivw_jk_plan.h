// mvivw_jk_plan.h -- host side of cusk_mvivw_jackknife (csrc/mvivw_jackknife.hip): the checks of the group boundaries, the
// work items of the refit kernel and the batches of outcomes.  Plain C++, no HIP: the stand-alone program
// tools/mvivw_jk_plan_selftest.cpp drives it under the host sanitizers.
//
// On top of the plan of the plain regressions (mvivw_plan.h): every active outcome of that plan keeps its slot.  An
// outcome whose groups fail the precondition (fewer than two groups, or a group that leaves m - m_g <= k rows) gets
// jk_status 1 here and has no work items.  A work item is one (outcome slot, group): one workgroup of the refit kernel,
// which stores theta_-g (k doubles) into the workspace of the batch.  The outcomes are processed in batches of consecutive
// slots whose theta_-g fit `ws_bound` bytes (an outcome that alone exceeds it forms a batch of its own), and inside a batch
// the items are listed by the tile class of their outcome: one launch per class.
#pragma once

#include "mvivw_plan.h"

namespace cusk {

constexpr size_t kMvJkBytes = (size_t)1 << 30;  // bytes of theta_-g alive at once
constexpr int kMvJkChunk = 256;                 // groups per chunk of the ordered sums over groups

struct MvJkOutcome
{
    long long grp0;  // first boundary of the outcome in grp
    long long ws0;   // offset (doubles) of theta_-0 inside the batch's workspace; group g at ws0 + g k
    long long gi0;   // index of group 0 among the groups of the batch (press partials, pivots, flags)
    int ng;
    int active;      // 0: the precondition fails, jk_status 1
};

struct MvJkItem
{
    int slot;   // index into the active outcomes of the plain plan
    int group;  // 0 .. ng - 1 of that outcome
};

struct MvJkBatch
{
    int first, last;                     // slots first .. last - 1
    size_t class_first[kMvClasses + 1];  // items of class c: jk.items[class_first[c] .. class_first[c + 1])
    size_t ws_doubles;
    long long ngroups;
};

struct MvJkPlan
{
    std::vector<int> status;             // per caller's outcome: 1 where no refit is made for a reason known here, else 0
    std::vector<long long> refit_off;    // nout + 1: where the caller's `refit` keeps outcome a, ng_a k_a doubles each
    std::vector<MvJkOutcome> outcomes;   // per slot of the plain plan
    std::vector<MvJkItem> items;         // grouped by (batch, class), in slot and group order inside
    std::vector<MvJkBatch> batches;
    size_t max_ws_doubles = 0;
    long long max_groups = 0;
};

// 0, or 1 with `msg` set.  `plan`: what mvivw_plan_build made of the same call (its argument checks have passed).
inline int mvivw_jk_plan_build(const MvPlan &plan, int nout, const long long *iv_off, const int *ex_off, const long long *grp_off,
                               const int *grp, size_t ws_bound, MvJkPlan &jk, std::string &msg)
{
    jk = MvJkPlan();
    if (nout == 0) return 0;
    if (!grp_off)
    {
        msg = "bad arguments";
        return 1;
    }
    if (grp_off[0] < 0)
    {
        msg = "bad offsets";
        return 1;
    }
    for (int a = 0; a < nout; a++)
        if (grp_off[a + 1] < grp_off[a])
        {
            msg = "outcome " + std::to_string(a) + ": group offsets are not monotone";
            return 1;
        }
    if (grp_off[nout] > grp_off[0] && !grp)
    {
        msg = "bad arguments";
        return 1;
    }
    jk.status.assign((size_t)nout, 0);
    jk.refit_off.assign((size_t)nout + 1, 0);
    std::vector<int> ngs((size_t)nout, 0);
    for (int a = 0; a < nout; a++)
    {
        const std::string who = "outcome " + std::to_string(a);
        const long long m = iv_off[a + 1] - iv_off[a], nb = grp_off[a + 1] - grp_off[a];
        const int k = ex_off[a + 1] - ex_off[a];
        if (m > 0 && nb < 2)
        {
            msg = who + ": instruments and no groups";
            return 1;
        }
        if (nb > m + 1)
        {
            msg = who + ": the group boundaries are not strictly ascending from 0 to m";
            return 1;
        }
        for (long long q = grp_off[a]; q < grp_off[a + 1]; q++)
        {
            const bool first = q == grp_off[a], last = q + 1 == grp_off[a + 1];
            if ((first && grp[q] != 0) || (!first && grp[q] <= grp[q - 1]) || (last && grp[q] != m) || grp[q] > m)
            {
                msg = who + ": the group boundaries are not strictly ascending from 0 to m";
                return 1;
            }
        }
        const int ng = nb > 0 ? (int)(nb - 1) : 0;
        ngs[(size_t)a] = ng;
        jk.refit_off[(size_t)a + 1] = jk.refit_off[(size_t)a] + (long long)ng * k;
        bool ok = plan.status[(size_t)a] == 0 && ng >= 2;
        for (long long q = grp_off[a]; ok && q + 1 < grp_off[a + 1]; q++) ok = m - (grp[q + 1] - grp[q]) > k;
        if (!ok) jk.status[(size_t)a] = 1;
    }
    const int na = (int)plan.outcomes.size();
    jk.outcomes.resize((size_t)na);
    for (int s = 0; s < na; s++)
    {
        const MvOutcome &q = plan.outcomes[(size_t)s];
        MvJkOutcome &j = jk.outcomes[(size_t)s];
        j.grp0 = grp_off[q.out];
        j.ws0 = j.gi0 = 0;
        j.active = jk.status[(size_t)q.out] == 0;
        j.ng = j.active ? ngs[(size_t)q.out] : 0;  // an outcome without refits takes no workspace
    }
    const size_t bound_doubles = std::max<size_t>(ws_bound / sizeof(double), 1);
    for (int first = 0; first < na;)
    {
        MvJkBatch bt;
        bt.first = first;
        bt.ws_doubles = 0;
        bt.ngroups = 0;
        int last = first;
        while (last < na)
        {
            MvJkOutcome &j = jk.outcomes[(size_t)last];
            const size_t need = (size_t)j.ng * (size_t)plan.outcomes[(size_t)last].k;
            if (last > first && bt.ws_doubles + need > bound_doubles) break;
            j.ws0 = (long long)bt.ws_doubles;
            j.gi0 = bt.ngroups;
            bt.ws_doubles += need;
            bt.ngroups += j.ng;
            last++;
        }
        bt.last = last;
        for (int c = 0; c < kMvClasses; c++)
        {
            bt.class_first[c] = jk.items.size();
            for (int s = first; s < last; s++)
                if (mv_class_of(plan.outcomes[(size_t)s].k) == c)
                    for (int g = 0; g < jk.outcomes[(size_t)s].ng; g++) jk.items.push_back(MvJkItem{s, g});
            if (jk.items.size() - bt.class_first[c] > (size_t)INT_MAX)
            {
                msg = "more than 2^31 - 1 refits of one tile class in one batch: lower mvivw_jk_bytes";
                return 1;
            }
        }
        bt.class_first[kMvClasses] = jk.items.size();
        jk.max_ws_doubles = std::max(jk.max_ws_doubles, bt.ws_doubles);
        jk.max_groups = std::max(jk.max_groups, bt.ngroups);
        jk.batches.push_back(bt);
        first = last;
    }
    return 0;
}

}  // namespace cusk
