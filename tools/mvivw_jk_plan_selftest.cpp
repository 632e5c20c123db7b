// mvivw_jk_plan_selftest.cpp -- host side of cusk_mvivw_jackknife (csrc/host/mvivw_jk_plan.h) under the host sanitizers:
// the checks of the group boundaries, the work items and the batches, with a stand-in for the device calls that walks the
// items the way the kernels do and checks every index they would form.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/mvivw_jk_plan_selftest.cpp -o mvivw_jk_plan_selftest
//   ./mvivw_jk_plan_selftest
#include "../ci-gwas_amd/csrc/host/mvivw_jk_plan.h"

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

struct Call
{
    long long M;
    int p;
    std::vector<int> outcome, iv, ex_off, ex, grp;
    std::vector<long long> iv_off, grp_off;
};

static int build(const Call &c, size_t bound, MvPlan &plan, MvJkPlan &jk, std::string &msg)
{
    const int nout = (int)c.outcome.size();
    if (mvivw_plan_build(c.M, c.p, nout, c.outcome.data(), c.iv_off.data(), c.iv.data(), c.ex_off.data(), c.ex.data(), 0,
                         kMvPartBound, plan, msg))
        return 2;
    return mvivw_jk_plan_build(plan, nout, c.iv_off.data(), c.ex_off.data(), c.grp_off.data(), c.grp.data(), bound, jk, msg);
}

// what the kernels do with a plan: one "workgroup" per item, theta_-g and the group's words at the planned places
static void device_stand_in(const Call &c, const MvPlan &plan, const MvJkPlan &jk)
{
    const size_t na = plan.outcomes.size();
    EXPECT(jk.outcomes.size() == na);
    std::vector<int> slot_seen(na, 0);
    std::vector<long long> items_of(na, 0);
    for (const MvJkBatch &bt : jk.batches)
    {
        EXPECT(bt.first < bt.last && bt.last <= (int)na);
        EXPECT(bt.ws_doubles <= jk.max_ws_doubles && bt.ngroups <= jk.max_groups);
        std::vector<char> ws(bt.ws_doubles, 0), words((size_t)bt.ngroups, 0);
        for (int cl = 0; cl < kMvClasses; cl++)
            for (size_t t = bt.class_first[cl]; t < bt.class_first[cl + 1]; t++)
            {
                const MvJkItem it = jk.items.at(t);
                EXPECT(it.slot >= bt.first && it.slot < bt.last);
                const MvOutcome &q = plan.outcomes.at((size_t)it.slot);
                const MvJkOutcome &j = jk.outcomes.at((size_t)it.slot);
                EXPECT(mv_class_of(q.k) == cl && j.active && it.group >= 0 && it.group < j.ng);
                const int r0 = c.grp.at((size_t)(j.grp0 + it.group)), r1 = c.grp.at((size_t)(j.grp0 + it.group + 1));
                EXPECT(0 <= r0 && r0 < r1 && r1 <= q.m && q.m - (r1 - r0) > q.k);
                for (int r = r0; r < r1; r++)
                {
                    const int row = c.iv.at((size_t)(q.iv0 + r));  // the rows the slabs stage, and where pres goes
                    EXPECT(row >= 0 && row < c.M);
                }
                for (int e = 0; e < q.k; e++) ws.at((size_t)j.ws0 + (size_t)it.group * q.k + e)++;
                words.at((size_t)(j.gi0 + it.group))++;
                items_of.at((size_t)it.slot)++;
            }
        for (char v : ws) EXPECT(v == 1);  // every double of the workspace belongs to exactly one refit
        for (char v : words) EXPECT(v == 1);
        for (int s = bt.first; s < bt.last; s++) slot_seen.at((size_t)s)++;  // the reduce kernel's workgroups
    }
    for (size_t s = 0; s < na; s++)
    {
        EXPECT(slot_seen[s] == 1);
        EXPECT(items_of[s] == jk.outcomes[s].ng);
    }
}

static Call random_call(std::mt19937 &rng, long long M, int p, int nout)
{
    Call c;
    c.M = M;
    c.p = p;
    c.iv_off.push_back(0);
    c.ex_off.push_back(0);
    c.grp_off.push_back(0);
    const int ks[] = {0, 1, 2, 43, 44, 87, 88, 126, 127};
    for (int a = 0; a < nout; a++)
    {
        const int o = (int)(rng() % p);
        c.outcome.push_back(o);
        const int k = std::min(ks[rng() % 9], p - 1);
        std::vector<int> all;
        for (int t = 0; t < p; t++)
            if (t != o) all.push_back(t);
        std::shuffle(all.begin(), all.end(), rng);
        all.resize((size_t)k);
        std::sort(all.begin(), all.end());
        c.ex.insert(c.ex.end(), all.begin(), all.end());
        c.ex_off.push_back((int)c.ex.size());
        const long long ms[] = {0, 1, k, k + 1, k + 2, 255, 256, 257, 511, M};
        const long long m = std::min(ms[rng() % 10], M);
        std::vector<int> rows;
        for (int r = 0; r < M; r++) rows.push_back(r);
        std::shuffle(rows.begin(), rows.end(), rng);
        rows.resize((size_t)m);
        std::sort(rows.begin(), rows.end());
        c.iv.insert(c.iv.end(), rows.begin(), rows.end());
        c.iv_off.push_back((long long)c.iv.size());
        // groups: leave-one-out, B equal groups, one group, or random cuts
        const int kind = (int)(rng() % 4);
        if (m > 0 || rng() % 2)
        {
            c.grp.push_back(0);
            for (long long r = 1; r < m; r++)
            {
                const long long B = 2 + (long long)(rng() % 7);
                const bool cut = kind == 0 || (kind == 1 && (r * B / m) != ((r - 1) * B / m)) || (kind == 3 && rng() % 5 == 0);
                if (cut) c.grp.push_back((int)r);
            }
            if (m > 0) c.grp.push_back((int)m);
        }
        c.grp_off.push_back((long long)c.grp.size());
    }
    return c;
}

int main()
{
    std::mt19937 rng(23);
    for (int round = 0; round < 80; round++)
    {
        const Call c = random_call(rng, 700, 130, 1 + (int)(rng() % 12));
        const size_t bounds[] = {kMvJkBytes, 1, 20000, 400000};
        MvPlan plan;
        MvJkPlan jk;
        std::string msg;
        EXPECT(build(c, bounds[round % 4], plan, jk, msg) == 0);
        if (!msg.empty()) std::printf("  got: %s\n", msg.c_str());
        EXPECT(jk.status.size() == c.outcome.size() && jk.refit_off.size() == c.outcome.size() + 1);
        size_t slot = 0;
        for (size_t a = 0; a < c.outcome.size(); a++)
        {
            const long long m = c.iv_off[a + 1] - c.iv_off[a], nb = c.grp_off[a + 1] - c.grp_off[a];
            const int k = c.ex_off[a + 1] - c.ex_off[a];
            const long long ng = nb > 0 ? nb - 1 : 0;
            bool ok = k > 0 && m > k && ng >= 2;
            for (long long g = 0; ok && g < ng; g++)
                ok = m - (c.grp[(size_t)(c.grp_off[a] + g + 1)] - c.grp[(size_t)(c.grp_off[a] + g)]) > k;
            EXPECT(jk.status[a] == (ok ? 0 : 1));
            EXPECT(jk.refit_off[a + 1] - jk.refit_off[a] == ng * k);
            if (plan.status[a] == 0)
            {
                const MvJkOutcome &j = jk.outcomes.at(slot++);
                EXPECT(j.active == (ok ? 1 : 0) && j.ng == (ok ? ng : 0) && j.grp0 == c.grp_off[a]);
            }
        }
        EXPECT(slot == plan.outcomes.size());
        if (bounds[round % 4] == 1)
            for (const MvJkBatch &bt : jk.batches)
            {  // an outcome that exceeds the bound stands alone with those that take nothing
                int with_ws = 0;
                for (int s = bt.first; s < bt.last; s++) with_ws += jk.outcomes[(size_t)s].ng > 0;
                EXPECT(with_ws <= 1);
            }
        device_stand_in(c, plan, jk);
    }
    // argument errors
    {
        MvPlan plan;
        MvJkPlan jk;
        std::string msg;
        Call ok;
        ok.M = 10, ok.p = 4;
        ok.outcome = {0, 1};
        ok.iv_off = {0, 4, 7};
        ok.iv = {0, 2, 5, 9, 1, 2, 3};
        ok.ex_off = {0, 1, 2};
        ok.ex = {1, 0};
        ok.grp_off = {0, 3, 7};
        ok.grp = {0, 2, 4, 0, 1, 2, 3};
        EXPECT(build(ok, kMvJkBytes, plan, jk, msg) == 0 && jk.status[0] == 0 && jk.status[1] == 0 && jk.items.size() == 5);
        device_stand_in(ok, plan, jk);
        auto bad = [&](const Call &c, const char *what) {
            MvPlan pl;
            MvJkPlan j2;
            std::string m2;
            EXPECT(build(c, kMvJkBytes, pl, j2, m2) == 1 && m2.find(what) != std::string::npos);
            if (m2.find(what) == std::string::npos) std::printf("  got: %s\n", m2.c_str());
        };
        Call c = ok;
        c.grp[0] = 1;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp[2] = 3;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp[2] = 5;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp[1] = 0;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp[5] = 1;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp[4] = 3, c.grp[5] = 2;
        bad(c, "strictly ascending from 0 to m");
        c = ok, c.grp_off = {0, 1, 7};
        bad(c, "no groups");
        c = ok, c.grp_off = {0, 0, 7};
        bad(c, "no groups");
        c = ok, c.grp_off = {0, 3, 2};
        bad(c, "not monotone");
        c = ok, c.grp_off = {-1, 3, 7};
        bad(c, "bad offsets");
        {
            MvPlan pl;
            MvJkPlan j2;
            std::string m2;
            EXPECT(mvivw_plan_build(ok.M, ok.p, 2, ok.outcome.data(), ok.iv_off.data(), ok.iv.data(), ok.ex_off.data(), ok.ex.data(), 0,
                                    kMvPartBound, pl, m2) == 0);
            EXPECT(mvivw_jk_plan_build(pl, 2, ok.iv_off.data(), ok.ex_off.data(), nullptr, ok.grp.data(), kMvJkBytes, j2, m2) == 1);
            EXPECT(mvivw_jk_plan_build(pl, 2, ok.iv_off.data(), ok.ex_off.data(), ok.grp_off.data(), nullptr, kMvJkBytes, j2, m2) == 1);
            EXPECT(mvivw_jk_plan_build(pl, 0, nullptr, nullptr, nullptr, nullptr, kMvJkBytes, j2, m2) == 0 && j2.batches.empty());
        }
        // the precondition: one group; a group that leaves k rows; an outcome without instruments and without boundaries
        c = ok, c.grp_off = {0, 2, 6}, c.grp = {0, 4, 0, 1, 2, 3};
        EXPECT(build(c, kMvJkBytes, plan, jk, msg) == 0 && jk.status[0] == 1 && jk.status[1] == 0 && jk.items.size() == 3);
        device_stand_in(c, plan, jk);
        c = ok, c.grp = {0, 1, 4, 0, 1, 2, 3};  // outcome 0: the second group leaves 1 = k rows
        EXPECT(build(c, kMvJkBytes, plan, jk, msg) == 0 && jk.status[0] == 1 && jk.status[1] == 0 && jk.items.size() == 3);
        device_stand_in(c, plan, jk);
        c = ok, c.iv_off = {0, 4, 4}, c.grp_off = {0, 3, 3};
        EXPECT(build(c, kMvJkBytes, plan, jk, msg) == 0 && jk.status[1] == 1 && jk.refit_off[2] == 2);
        c.grp_off = {0, 3, 4}, c.grp = {0, 2, 4, 0};
        EXPECT(build(c, kMvJkBytes, plan, jk, msg) == 0 && jk.status[1] == 1 && jk.refit_off[2] == 2);
    }
    std::printf(failures ? "mvivw_jk_plan_selftest: %d FAILED\n" : "mvivw_jk_plan_selftest: ok\n", failures);
    return failures ? 1 : 0;
}
