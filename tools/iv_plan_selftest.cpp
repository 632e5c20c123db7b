// iv_plan_selftest.cpp -- host side of cusk_iv_check (csrc/host/iv_plan.h) under the host sanitizers: the argument
// checks and the item sort, with a stand-in for the device calls that walks the tiles the way the item kernel does and
// checks every index it would form.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/iv_plan_selftest.cpp -o iv_plan_selftest
//   ./iv_plan_selftest
#include "../ci-gwas_amd/csrc/host/iv_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace cusk;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

// what the item kernel does with a plan: one "workgroup" per tile, one "lane" per item
static void device_stand_in(const IvPlan &plan, const std::vector<int> &set_off, const std::vector<int> &item_x,
                            const std::vector<int> &item_y, const std::vector<int> &item_set, std::vector<int> &written)
{
    const int nsets = (int)set_off.size() - 1;
    for (int c = 0; c < kIvClasses; c++)
        for (size_t t = plan.class_first[c]; t < plan.class_first[c + 1]; t++)
        {
            const IvTile &tile = plan.tiles[t];
            EXPECT(tile.count >= 1 && tile.count <= kIvTile);
            EXPECT(tile.set >= -1 && tile.set < nsets);
            const int len = tile.set < 0 ? 0 : set_off[(size_t)tile.set + 1] - set_off[(size_t)tile.set];
            EXPECT(len <= kIvCaps[c]);
            EXPECT(c == 0 || len > kIvCaps[c - 1]);
            for (int lane = 0; lane < tile.count; lane++)
            {
                const size_t pos = (size_t)tile.start + lane;
                const int out = plan.order.at(pos);
                EXPECT(plan.xs.at(pos) == item_x.at((size_t)out));
                EXPECT(item_y.at((size_t)out) == tile.y && item_set.at((size_t)out) == tile.set);
                written.at((size_t)out)++;
            }
        }
}

static int build(long long n, int p, const std::vector<int> &set_off, const std::vector<int> &set, const std::vector<int> &x,
                 const std::vector<int> &y, const std::vector<int> &s, IvPlan &plan, std::string &msg)
{
    return iv_plan_build(n, p, (int)set_off.size() - 1, set_off.data(), set.data(), (long long)x.size(), x.data(), y.data(),
                         s.data(), plan, msg);
}

int main()
{
    std::mt19937 rng(7);
    const int p = 140;
    const long long n = 400;
    // random batches: every class, shuffled items
    for (int round = 0; round < 40; round++)
    {
        std::vector<int> set_off{0}, set;
        const int lens[] = {0, 1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 127};
        const int nsets = 1 + (int)(rng() % 12);
        std::vector<std::vector<char>> member;
        for (int s = 0; s < nsets; s++)
        {
            const int len = lens[rng() % 12];
            std::vector<char> in((size_t)p, 0);
            for (int k = 0; k < len;)
            {
                const int t = (int)(rng() % p);
                if (in[(size_t)t]) continue;
                in[(size_t)t] = 1;
                set.push_back(t);
                k++;
            }
            set_off.push_back((int)set.size());
            member.push_back(in);
        }
        const int nitems = (int)(rng() % 3000);
        std::vector<int> x, y, s;
        while ((int)x.size() < nitems)
        {
            const int si = (int)(rng() % (nsets + 1)) - 1;
            const int yy = (int)(rng() % 4), xx = (int)(rng() % n);
            if (xx == yy) continue;
            if (si >= 0 && (member[(size_t)si][(size_t)yy] || (xx < p && member[(size_t)si][(size_t)xx]))) continue;
            x.push_back(xx), y.push_back(yy), s.push_back(si);
        }
        IvPlan plan;
        std::string msg;
        EXPECT(build(n, p, set_off, set, x, y, s, plan, msg) == 0);
        EXPECT(plan.order.size() == x.size() && plan.xs.size() == x.size());
        EXPECT(plan.w_off.size() == set_off.size());
        for (int k = 0; k < nsets; k++)
        {
            const long long len = set_off[(size_t)k + 1] - set_off[(size_t)k];
            EXPECT(plan.w_off[(size_t)k + 1] - plan.w_off[(size_t)k] == len * (len + 1) / 2);
        }
        for (size_t k = 1; k < plan.order.size(); k++)
        {  // sorted by (set, y), ties in the caller's order
            const int a = plan.order[k - 1], b = plan.order[k];
            EXPECT(s[(size_t)a] < s[(size_t)b] || (s[(size_t)a] == s[(size_t)b] && (y[(size_t)a] < y[(size_t)b] || (y[(size_t)a] == y[(size_t)b] && a < b))));
        }
        {  // the set-up launches: every non-empty set an item names, once, in its class
            std::vector<int> want((size_t)nsets, 0), got((size_t)nsets, 0);
            for (int si : s)
                if (si >= 0 && set_off[(size_t)si + 1] > set_off[(size_t)si]) want[(size_t)si] = 1;
            for (int c = 0; c < kIvClasses; c++)
                for (size_t k = plan.setup_first[c]; k < plan.setup_first[c + 1]; k++)
                {
                    const int si = plan.setup_sets.at(k);
                    const int len = set_off.at((size_t)si + 1) - set_off.at((size_t)si);
                    EXPECT(len >= 1 && len <= kIvCaps[c] && (c == 0 || len > kIvCaps[c - 1]));
                    got.at((size_t)si)++;
                }
            EXPECT(plan.setup_first[kIvClasses] == plan.setup_sets.size());
            EXPECT(want == got);
        }
        std::vector<int> written(x.size(), 0);
        device_stand_in(plan, set_off, x, y, s, written);
        for (int w : written) EXPECT(w == 1);
    }
    // argument errors
    {
        IvPlan plan;
        std::string msg;
        std::vector<int> big;
        for (int k = 0; k < 128; k++) big.push_back(k);
        EXPECT(build(n, p, {0, 128}, big, {200}, {130}, {0}, plan, msg) == 1 && msg.find("longer than 127") != std::string::npos);
        EXPECT(build(n, p, {0, 3}, {1, 2, 1}, {200}, {0}, {0}, plan, msg) == 1 && msg.find("twice") != std::string::npos);
        EXPECT(build(n, p, {0, 2}, {1, p}, {200}, {0}, {0}, plan, msg) == 1 && msg.find("not a trait index") != std::string::npos);
        EXPECT(build(n, p, {0, 2}, {1, -1}, {200}, {0}, {0}, plan, msg) == 1 && msg.find("not a trait index") != std::string::npos);
        EXPECT(build(n, p, {0, 2}, {1, 2}, {1}, {0}, {0}, plan, msg) == 1 && msg.find("own conditioning set") != std::string::npos);
        EXPECT(build(n, p, {0, 2}, {1, 2}, {200}, {2}, {0}, plan, msg) == 1 && msg.find("own conditioning set") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {(int)n}, {0}, {0}, plan, msg) == 1 && msg.find("not a variable index") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {200}, {-1}, {0}, plan, msg) == 1 && msg.find("not a variable index") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {5}, {5}, {0}, plan, msg) == 1 && msg.find("x equals y") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {200}, {201}, {0}, plan, msg) == 1 && msg.find("neither x nor y") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {200}, {0}, {1}, plan, msg) == 1 && msg.find("set index out of range") != std::string::npos);
        EXPECT(build(n, p, {0, 1}, {1}, {200}, {0}, {-2}, plan, msg) == 1);
        EXPECT(build(n, p, {1, 2}, {1, 2}, {200}, {0}, {0}, plan, msg) == 1 && msg.find("bad set offsets") != std::string::npos);
        EXPECT(build(n, p, {0, 2, 1}, {1, 2}, {200}, {0}, {0}, plan, msg) == 1 && msg.find("bad set offsets") != std::string::npos);
        EXPECT(build(10, p, {0, 1}, {1}, {2}, {0}, {0}, plan, msg) == 1 && msg.find("fewer variables") != std::string::npos);
        // no sets, no items
        EXPECT(iv_plan_build(n, p, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, plan, msg) == 0 && plan.tiles.empty());
        EXPECT(build(n, p, {0}, {}, {200, 201}, {0, 0}, {-1, -1}, plan, msg) == 0 && plan.tiles.size() == 1 && plan.tiles[0].count == 2);
    }
    std::printf(failures ? "iv_plan_selftest: %d FAILED\n" : "iv_plan_selftest: ok\n", failures);
    return failures ? 1 : 0;
}
