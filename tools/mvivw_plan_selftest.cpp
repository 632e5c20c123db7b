// mvivw_plan_selftest.cpp -- host side of cusk_mvivw (csrc/host/mvivw_plan.h) under the host sanitizers: the argument
// checks and the chunk plan, with a stand-in for the device calls that walks the chunks the way the kernels do and checks
// every index they would form.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/mvivw_plan_selftest.cpp -o mvivw_plan_selftest
//   ./mvivw_plan_selftest
#include "../ci-gwas_amd/csrc/host/mvivw_plan.h"

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
    std::vector<int> outcome, iv, ex_off, ex;
    std::vector<long long> iv_off;
};

static int build(const Call &c, int model, size_t bound, MvPlan &plan, std::string &msg)
{
    return mvivw_plan_build(c.M, c.p, (int)c.outcome.size(), c.outcome.data(), c.iv_off.data(), c.iv.data(), c.ex_off.data(),
                            c.ex.data(), model, bound, plan, msg);
}

// what the kernels do with a plan: one "workgroup" per chunk, partials and flags at the planned places
static void device_stand_in(const Call &c, const MvPlan &plan)
{
    std::vector<int> chunk_seen((size_t)plan.total_chunks, 0);
    std::vector<int> slot_seen(plan.outcomes.size(), 0);
    for (const MvGroup &g : plan.groups)
    {
        EXPECT(g.first < g.last && g.last <= (int)plan.outcomes.size());
        std::vector<char> part(g.part_doubles, 0);
        EXPECT(g.part_doubles <= plan.max_part_doubles);
        for (int cl = 0; cl < kMvClasses; cl++)
            for (size_t t = g.class_first[cl]; t < g.class_first[cl + 1]; t++)
            {
                const MvChunk ch = plan.chunks.at(t);
                EXPECT(ch.slot >= g.first && ch.slot < g.last);
                const MvOutcome &q = plan.outcomes.at((size_t)ch.slot);
                const int K = q.k + 1, ts = kMvTile[cl];
                EXPECT(K <= kMvCols[cl] && (cl == 0 || K > kMvCols[cl - 1]));
                const int T = (K + ts - 1) / ts;
                EXPECT(T * ts <= kMvCols[cl] && T * (T + 1) / 2 <= 256);
                EXPECT(ch.chunk >= 0 && ch.chunk < q.nchunks);
                const int rows = std::min(kMvChunk, q.m - ch.chunk * kMvChunk);
                EXPECT(rows >= 1);
                for (int r = 0; r < rows; r++)
                {
                    const int row = c.iv.at((size_t)(q.iv0 + (long long)ch.chunk * kMvChunk + r));
                    EXPECT(row >= 0 && row < c.M);
                }
                for (int j = 0; j < q.k; j++) EXPECT(c.ex.at((size_t)q.ex0 + j) >= 0 && c.ex.at((size_t)q.ex0 + j) < c.p);
                const size_t E = (size_t)K * (K + 1) / 2;
                for (size_t e = 0; e < E; e++) part.at((size_t)q.part0 + (size_t)ch.chunk * E + e)++;
                chunk_seen.at((size_t)q.chunk0 + ch.chunk)++;
            }
        for (char v : part) EXPECT(v == 1);  // every double of the group's buffer belongs to exactly one chunk
        for (int s = g.first; s < g.last; s++) slot_seen.at((size_t)s)++;
    }
    for (int v : chunk_seen) EXPECT(v == 1);
    for (int v : slot_seen) EXPECT(v == 1);
}

static Call random_call(std::mt19937 &rng, long long M, int p, int nout)
{
    Call c;
    c.M = M;
    c.p = p;
    c.iv_off.push_back(0);
    c.ex_off.push_back(0);
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
        const long long ms[] = {0, 1, k, k + 1, 255, 256, 257, 511, 513, M};
        const long long m = std::min(ms[rng() % 10], M);
        std::vector<int> rows;
        for (int r = 0; r < M; r++) rows.push_back(r);
        std::shuffle(rows.begin(), rows.end(), rng);
        rows.resize((size_t)m);
        std::sort(rows.begin(), rows.end());
        c.iv.insert(c.iv.end(), rows.begin(), rows.end());
        c.iv_off.push_back((long long)c.iv.size());
    }
    return c;
}

int main()
{
    std::mt19937 rng(11);
    for (int round = 0; round < 60; round++)
    {
        const Call c = random_call(rng, 700, 130, 1 + (int)(rng() % 12));
        const size_t bounds[] = {kMvPartBound, 1, 100000, 3000000};
        MvPlan plan;
        std::string msg;
        EXPECT(build(c, round % 3, bounds[round % 4], plan, msg) == 0);
        EXPECT(plan.status.size() == c.outcome.size());
        size_t active = 0;
        for (size_t a = 0; a < c.outcome.size(); a++)
        {
            const long long m = c.iv_off[a + 1] - c.iv_off[a];
            const int k = c.ex_off[a + 1] - c.ex_off[a];
            EXPECT(plan.status[a] == ((k == 0 || m <= k) ? 1 : 0));
            if (plan.status[a] == 0)
            {
                const MvOutcome &q = plan.outcomes.at(active++);
                EXPECT(q.out == (int)a && q.m == m && q.k == k && q.o == c.outcome[a] && q.iv0 == c.iv_off[a] && q.ex0 == c.ex_off[a]);
                EXPECT(q.nchunks == (m + kMvChunk - 1) / kMvChunk);
            }
        }
        EXPECT(active == plan.outcomes.size());
        if (bounds[round % 4] == 1)
            for (const MvGroup &g : plan.groups) EXPECT(g.last == g.first + 1);  // an outcome that exceeds the bound stands alone
        device_stand_in(c, plan);
    }
    // argument errors
    {
        MvPlan plan;
        std::string msg;
        Call ok;
        ok.M = 10, ok.p = 4;
        ok.outcome = {0, 1};
        ok.iv_off = {0, 3, 6};
        ok.iv = {0, 2, 9, 1, 2, 3};
        ok.ex_off = {0, 2, 3};
        ok.ex = {1, 3, 0};
        EXPECT(build(ok, 0, kMvPartBound, plan, msg) == 0 && plan.outcomes.size() == 2);
        auto bad = [&](const Call &c, int model, const char *what) {
            MvPlan pl;
            std::string m2;
            EXPECT(build(c, model, kMvPartBound, pl, m2) == 1 && m2.find(what) != std::string::npos);
            if (m2.find(what) == std::string::npos) std::printf("  got: %s\n", m2.c_str());
        };
        Call c = ok;
        c.outcome[1] = 4;
        bad(c, 0, "not a trait index");
        c = ok, c.outcome[0] = -1;
        bad(c, 0, "not a trait index");
        c = ok, c.iv[2] = 10;
        bad(c, 0, "not a marker row");
        c = ok, c.iv[0] = -1;
        bad(c, 0, "not a marker row");
        c = ok, c.iv[1] = 0;
        bad(c, 0, "instrument list is not strictly ascending");
        c = ok, c.iv[4] = 0;
        bad(c, 0, "instrument list is not strictly ascending");
        c = ok, c.ex[1] = 1;
        bad(c, 0, "exposure list is not strictly ascending");
        c = ok, c.ex[0] = 0, c.ex[1] = 1;
        bad(c, 0, "own exposures");
        c = ok, c.ex[1] = 4;
        bad(c, 0, "not a trait index");
        c = ok, c.ex[0] = -1;
        bad(c, 0, "not a trait index");
        c = ok, c.iv_off[1] = 7, c.iv_off[2] = 6;
        bad(c, 0, "not monotone");
        c = ok, c.ex_off[1] = 3, c.ex_off[2] = 2;
        bad(c, 0, "not monotone");
        bad(ok, 3, "model");
        bad(ok, -1, "model");
        {  // 128 exposures
            Call big;
            big.M = 300, big.p = 130;
            big.outcome = {129};
            for (int r = 0; r < 300; r++) big.iv.push_back(r);
            big.iv_off = {0, 300};
            for (int t = 0; t < 128; t++) big.ex.push_back(t);
            big.ex_off = {0, 128};
            bad(big, 0, "more than 127 exposures");
            big.ex.pop_back();
            big.ex_off[1] = 127;
            EXPECT(build(big, 0, kMvPartBound, plan, msg) == 0 && plan.outcomes.size() == 1 && plan.outcomes[0].nchunks == 2);
            device_stand_in(big, plan);
        }
        // no outcomes; outcomes that all have status 1
        EXPECT(mvivw_plan_build(10, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, kMvPartBound, plan, msg) == 0 && plan.groups.empty());
        c = ok, c.ex_off = {0, 0, 0};
        EXPECT(build(c, 0, kMvPartBound, plan, msg) == 0 && plan.outcomes.empty() && plan.groups.empty() && plan.status[0] == 1 && plan.status[1] == 1);
        c = ok, c.iv_off = {0, 2, 3};
        EXPECT(build(c, 0, kMvPartBound, plan, msg) == 0 && plan.status[0] == 1 && plan.status[1] == 1);  // m = k
    }
    std::printf(failures ? "mvivw_plan_selftest: %d FAILED\n" : "mvivw_plan_selftest: ok\n", failures);
    return failures ? 1 : 0;
}
