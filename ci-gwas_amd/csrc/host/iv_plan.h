// iv_plan.h -- host side of cusk_iv_check (csrc/iv_check.hip): argument checks and the launch plan.  Plain C++, no HIP:
// the stand-alone program tools/iv_plan_selftest.cpp drives it under the host sanitizers.
//
// The item kernel wants the items of one (conditioning set, y) together: a workgroup forms W c_Sy once and every lane
// adds its own x.  So the items are sorted by (set, y), cut into tiles of at most kIvTile, and the tiles are grouped by
// the size class of their set (one launch per class, LDS sized to the class).  The set-up kernel gets the same classes and
// only the sets that some item names.  `order` maps a sorted position back to
// the caller's index; the kernel writes z and flags there, so nothing is permuted afterwards.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

namespace cusk {

constexpr int kIvCaps[] = {8, 16, 32, 64, 127};  // set-size classes of the item kernel (127: 129.5 KB of LDS)
constexpr int kIvClasses = 5;
constexpr int kIvMaxSet = 127;
constexpr int kIvTile = 64;  // items per workgroup: one wavefront, one x per lane

struct IvTile
{
    int set;    // -1: the empty set
    int y;
    int start;  // first sorted position
    int count;  // 1 .. kIvTile
};

struct IvPlan
{
    std::vector<int> order;               // sorted position -> caller's item index
    std::vector<int> xs;                  // x of the item at a sorted position
    std::vector<IvTile> tiles;            // grouped by class
    size_t class_first[kIvClasses + 1];   // tiles of class c: class_first[c] .. class_first[c + 1]
    std::vector<long long> w_off;         // nsets + 1: offset (doubles) of a set's packed lower triangle of W
    std::vector<int> setup_sets;          // the non-empty sets some item names, grouped by class: only these are inverted
    size_t setup_first[kIvClasses + 1];   // sets of class c: setup_first[c] .. setup_first[c + 1]
    int max_len = 0;                      // longest set
};

inline int iv_class_of(int len)
{
    int c = 0;
    while (c < kIvClasses - 1 && len > kIvCaps[c]) c++;
    return c;
}

// 0, or 1 with `msg` set: an argument the kernels must never see.  Every index they form is checked here.
inline int iv_plan_build(long long n, int p, int nsets, const int *set_off, const int *set, long long nitems,
                         const int *item_x, const int *item_y, const int *item_set, IvPlan &plan, std::string &msg)
{
    plan = IvPlan();
    if (n <= 0 || p <= 0 || nsets < 0 || nitems < 0 || (nsets > 0 && !set_off) || (nitems > 0 && (!item_x || !item_y || !item_set)))
    {
        msg = "bad arguments";
        return 1;
    }
    if (n < p)
    {
        msg = "fewer variables than traits";
        return 1;
    }
    if (nitems > INT_MAX)
    {
        msg = "more than 2^31 - 1 items in one call";
        return 1;
    }
    plan.w_off.assign((size_t)nsets + 1, 0);
    std::vector<int> stamp((size_t)p, -1);
    for (int s = 0; s < nsets; s++)
    {
        const long long a = set_off[s], b = set_off[s + 1];
        if ((s == 0 && a != 0) || b < a)
        {
            msg = "bad set offsets";
            return 1;
        }
        const long long len = b - a;
        if (len > kIvMaxSet)
        {
            msg = "set " + std::to_string(s) + " is longer than " + std::to_string(kIvMaxSet);
            return 1;
        }
        if (len > 0 && !set)
        {
            msg = "bad arguments";
            return 1;
        }
        for (long long k = a; k < b; k++)
        {
            const int t = set[k];
            if (t < 0 || t >= p)
            {
                msg = "set " + std::to_string(s) + " holds " + std::to_string(t) + ", which is not a trait index";
                return 1;
            }
            if (stamp[(size_t)t] == s)
            {
                msg = "set " + std::to_string(s) + " holds trait " + std::to_string(t) + " twice";
                return 1;
            }
            stamp[(size_t)t] = s;
        }
        plan.max_len = std::max(plan.max_len, (int)len);
        plan.w_off[(size_t)s + 1] = plan.w_off[(size_t)s] + len * (len + 1) / 2;
    }
    // membership of a trait in a set, for the items' own x and y
    std::vector<unsigned char> member((size_t)nsets * (size_t)p, 0);
    for (int s = 0; s < nsets; s++)
        for (int k = set_off[s]; k < set_off[s + 1]; k++) member[(size_t)s * p + set[k]] = 1;
    for (long long k = 0; k < nitems; k++)
    {
        const int x = item_x[k], y = item_y[k], s = item_set[k];
        const std::string who = "item " + std::to_string(k);
        if (x < 0 || x >= n || y < 0 || y >= n)
        {
            msg = who + ": x or y is not a variable index";
            return 1;
        }
        if (x == y)
        {
            msg = who + ": x equals y";
            return 1;
        }
        if (x >= p && y >= p)
        {
            msg = who + ": neither x nor y is a trait (trait_corr holds no marker x marker entries)";
            return 1;
        }
        if (s < -1 || s >= nsets)
        {
            msg = who + ": set index out of range";
            return 1;
        }
        if (s >= 0 && ((x < p && member[(size_t)s * p + x]) || (y < p && member[(size_t)s * p + y])))
        {
            msg = who + ": x or y lies in its own conditioning set";
            return 1;
        }
    }
    const int ni = (int)nitems;
    plan.order.resize((size_t)ni);
    for (int k = 0; k < ni; k++) plan.order[(size_t)k] = k;
    std::sort(plan.order.begin(), plan.order.end(), [&](int a, int b) {
        if (item_set[a] != item_set[b]) return item_set[a] < item_set[b];
        if (item_y[a] != item_y[b]) return item_y[a] < item_y[b];
        return a < b;
    });
    plan.xs.resize((size_t)ni);
    std::vector<IvTile> tiles;
    for (int k = 0; k < ni; k++)
    {
        const int it = plan.order[(size_t)k];
        plan.xs[(size_t)k] = item_x[it];
        if (tiles.empty() || tiles.back().set != item_set[it] || tiles.back().y != item_y[it] || tiles.back().count == kIvTile)
            tiles.push_back(IvTile{item_set[it], item_y[it], k, 0});
        tiles.back().count++;
    }
    auto cls = [&](const IvTile &t) { return t.set < 0 ? 0 : iv_class_of(set_off[t.set + 1] - set_off[t.set]); };
    plan.tiles.reserve(tiles.size());
    for (int c = 0; c < kIvClasses; c++)
    {
        plan.class_first[c] = plan.tiles.size();
        for (const IvTile &t : tiles)
            if (cls(t) == c) plan.tiles.push_back(t);
    }
    plan.class_first[kIvClasses] = plan.tiles.size();
    std::vector<unsigned char> used((size_t)nsets, 0);
    for (const IvTile &t : tiles)
        if (t.set >= 0) used[(size_t)t.set] = 1;
    for (int c = 0; c < kIvClasses; c++)
    {
        plan.setup_first[c] = plan.setup_sets.size();
        for (int s = 0; s < nsets; s++)
            if (used[(size_t)s] && set_off[s + 1] > set_off[s] && iv_class_of(set_off[s + 1] - set_off[s]) == c)
                plan.setup_sets.push_back(s);
    }
    plan.setup_first[kIvClasses] = plan.setup_sets.size();
    return 0;
}

}  // namespace cusk
