// mvivw_plan.h -- host side of cusk_mvivw (csrc/mvivw.hip): argument checks and the chunk plan.  Plain C++, no HIP: the
// stand-alone program tools/mvivw_plan_selftest.cpp drives it under the host sanitizers.
//
// One problem per outcome: m instrument rows, k exposures.  An outcome with k = 0 or m <= k gets status 1 here and never
// reaches the device.  Every other outcome is cut into chunks of kMvChunk consecutive list positions; a workgroup of the
// Gram kernel owns one chunk and stores one partial, the lower triangle of Z'WZ for Z = (X, y): E = (k + 1)(k + 2) / 2
// doubles.  The outcomes are processed in groups of consecutive active outcomes whose partials fit `part_bound` bytes (an
// outcome that alone exceeds it forms a group of its own), and inside a group the chunks are listed by the tile class of
// their outcome: one launch per class.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

namespace cusk {

constexpr int kMvChunk = 256;      // list positions per chunk: the unit of the ordered sums
constexpr int kMvMaxExposures = 127;
constexpr int kMvClasses = 3;
constexpr int kMvTile[kMvClasses] = {2, 4, 8};      // a thread of the Gram kernel owns a TS x TS tile of the triangle
constexpr int kMvCols[kMvClasses] = {44, 88, 128};  // columns of Z (k + 1) a class takes: at most 253 / 253 / 136 tiles
constexpr size_t kMvPartBound = (size_t)256 << 20;  // bytes of chunk partials alive at once

inline int mv_class_of(int k)
{
    int c = 0;
    while (c < kMvClasses - 1 && k + 1 > kMvCols[c]) c++;
    return c;
}

struct MvOutcome
{
    long long iv0;    // first position of the instrument list in iv
    long long part0;  // offset (doubles) of the first chunk partial inside the group's buffer
    int chunk0;       // index of the first chunk among all chunks of the call (flags, residual partials)
    int nchunks;
    int m, k;
    int ex0;  // first position of the exposure list in ex
    int o;    // the outcome trait
    int out;  // index in the caller's outcome list
    int pad;
};

struct MvChunk
{
    int slot;   // index into the active outcomes
    int chunk;  // 0 .. nchunks - 1 of that outcome
};

struct MvGroup
{
    int first, last;                       // active outcomes first .. last - 1
    size_t class_first[kMvClasses + 1];    // chunks of class c: plan.chunks[class_first[c] .. class_first[c + 1])
    size_t part_doubles;
};

struct MvPlan
{
    std::vector<int> status;          // per caller's outcome: 1 where nothing is computed, else 0
    std::vector<MvOutcome> outcomes;  // the active ones, in the caller's order
    std::vector<MvChunk> chunks;      // grouped by (group, class), in outcome and chunk order inside
    std::vector<MvGroup> groups;
    size_t max_part_doubles = 0;
    long long total_chunks = 0;
};

// 0, or 1 with `msg` set: an argument the kernels must never see.  Every index they form is checked here.
inline int mvivw_plan_build(long long M, int p, int nout, const int *outcome, const long long *iv_off, const int *iv,
                            const int *ex_off, const int *ex, int model, size_t part_bound, MvPlan &plan, std::string &msg)
{
    plan = MvPlan();
    if (M <= 0 || p <= 0 || nout < 0 || (nout > 0 && (!outcome || !iv_off || !ex_off)))
    {
        msg = "bad arguments";
        return 1;
    }
    if (model < 0 || model > 2)
    {
        msg = "model " + std::to_string(model) + " is not 0 (default), 1 (random) or 2 (fixed)";
        return 1;
    }
    if (nout == 0) return 0;
    if (iv_off[0] < 0 || ex_off[0] < 0)
    {
        msg = "bad offsets";
        return 1;
    }
    for (int a = 0; a < nout; a++)  // before any list is read: the last offset is the length the caller vouches for
        if (iv_off[a + 1] < iv_off[a] || ex_off[a + 1] < ex_off[a])
        {
            msg = "outcome " + std::to_string(a) + ": offsets are not monotone";
            return 1;
        }
    for (int a = 0; a < nout; a++)
    {
        const std::string who = "outcome " + std::to_string(a);
        const int o = outcome[a];
        if (o < 0 || o >= p)
        {
            msg = who + ": " + std::to_string(o) + " is not a trait index";
            return 1;
        }
        const long long m = iv_off[a + 1] - iv_off[a];
        const int k = ex_off[a + 1] - ex_off[a];
        if (m > M)
        {
            msg = who + ": more instruments than marker rows";
            return 1;
        }
        if (k > kMvMaxExposures)
        {
            msg = who + ": more than " + std::to_string(kMvMaxExposures) + " exposures";
            return 1;
        }
        if ((m > 0 && !iv) || (k > 0 && !ex))
        {
            msg = "bad arguments";
            return 1;
        }
        for (long long q = iv_off[a]; q < iv_off[a + 1]; q++)
        {
            const int r = iv[q];
            if (r < 0 || r >= M)
            {
                msg = who + ": instrument " + std::to_string(r) + " is not a marker row";
                return 1;
            }
            if (q > iv_off[a] && iv[q - 1] >= r)
            {
                msg = who + ": the instrument list is not strictly ascending";
                return 1;
            }
        }
        for (int q = ex_off[a]; q < ex_off[a + 1]; q++)
        {
            const int t = ex[q];
            if (t < 0 || t >= p)
            {
                msg = who + ": exposure " + std::to_string(t) + " is not a trait index";
                return 1;
            }
            if (t == o)
            {
                msg = who + ": the outcome is among its own exposures";
                return 1;
            }
            if (q > ex_off[a] && ex[q - 1] >= t)
            {
                msg = who + ": the exposure list is not strictly ascending";
                return 1;
            }
        }
    }
    plan.status.assign((size_t)nout, 0);
    for (int a = 0; a < nout; a++)
    {
        const long long m = iv_off[a + 1] - iv_off[a];
        const int k = ex_off[a + 1] - ex_off[a];
        if (k == 0 || m <= k)
        {
            plan.status[(size_t)a] = 1;
            continue;
        }
        const long long nch = (m + kMvChunk - 1) / kMvChunk;
        if (plan.total_chunks + nch > INT_MAX)
        {
            msg = "more than 2^31 - 1 chunks in one call";
            return 1;
        }
        MvOutcome q;
        q.iv0 = iv_off[a];
        q.part0 = 0;
        q.chunk0 = (int)plan.total_chunks;
        q.nchunks = (int)nch;
        q.m = (int)m;
        q.k = k;
        q.ex0 = ex_off[a];
        q.o = outcome[a];
        q.out = a;
        q.pad = 0;
        plan.outcomes.push_back(q);
        plan.total_chunks += nch;
    }
    const size_t bound_doubles = std::max<size_t>(part_bound / sizeof(double), 1);
    const int na = (int)plan.outcomes.size();
    for (int first = 0; first < na;)
    {
        MvGroup g;
        g.first = first;
        g.part_doubles = 0;
        int last = first;
        while (last < na)
        {
            MvOutcome &q = plan.outcomes[(size_t)last];
            const size_t need = (size_t)q.nchunks * ((size_t)(q.k + 1) * (q.k + 2) / 2);
            if (last > first && g.part_doubles + need > bound_doubles) break;
            q.part0 = (long long)g.part_doubles;
            g.part_doubles += need;
            last++;
        }
        g.last = last;
        for (int c = 0; c < kMvClasses; c++)
        {
            g.class_first[c] = plan.chunks.size();
            for (int s = first; s < last; s++)
                if (mv_class_of(plan.outcomes[(size_t)s].k) == c)
                    for (int ch = 0; ch < plan.outcomes[(size_t)s].nchunks; ch++) plan.chunks.push_back(MvChunk{s, ch});
        }
        g.class_first[kMvClasses] = plan.chunks.size();
        plan.max_part_doubles = std::max(plan.max_part_doubles, g.part_doubles);
        plan.groups.push_back(g);
        first = last;
    }
    return 0;
}

}  // namespace cusk
