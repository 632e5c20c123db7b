// mvivw_ld_plan_selftest.cpp -- host/mvivw_ld_plan.h (the host side of cusk_mvivw_ld) walked with a stand-in for the
// kernels of csrc/mvivw_ld.hip.  Host code only; build and run under the sanitizers:
//   g++ -std=c++17 -g -O1 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/mvivw_ld_plan_selftest.cpp -o mvivw_ld_plan_selftest && ./mvivw_ld_plan_selftest
//
// The stand-in repeats the index arithmetic of the kernels (thread maps included) on a table of counters of the same
// shape as the workspace, (m + K) rows of m columns, and checks per panel that
//   * every index a kernel forms lies inside the workspace, and inside the lower triangle for a row of R;
//   * the factor kernel touches exactly the diagonal block, the solve kernel exactly the rows below it, once;
//   * every element of the trailing rows (lower triangle of R, every column >= c0 of the K extra rows) is updated
//     exactly once, and nothing else is.
// It also drives the argument checks: the errors of cusk_mvivw, ridge, the workspace bound.
#include "../ci-gwas_amd/csrc/host/mvivw_ld_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace cusk;

static long long g_checks = 0;
#define CHECK(cond)                                                                  \
    do                                                                               \
    {                                                                                \
        g_checks++;                                                                  \
        if (!(cond))                                                                 \
        {                                                                            \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);                   \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

struct Table
{
    int m, K;
    std::vector<int> n;
    Table(int m_, int K_) : m(m_), K(K_), n((size_t)(m_ + K_) * (size_t)m_, 0) {}
    int &at(long long r, long long c)
    {
        CHECK(r >= 0 && r < (long long)m + K && c >= 0 && c < m);
        CHECK(r >= m || c <= r);  // a row of R: the lower triangle only
        return n[(size_t)r * (size_t)m + (size_t)c];
    }
    void clear() { std::fill(n.begin(), n.end(), 0); }
};

// ld_factor_kernel: idx -> (r, c) of the nb x nb block, c <= r
static void factor(Table &t, const LdPanel &pn)
{
    for (int idx = 0; idx < pn.nb * pn.nb; idx++)
    {
        const int r = idx / pn.nb, c = idx - r * pn.nb;
        if (c <= r) t.at(pn.j0 + r, pn.j0 + c)++;
    }
}

// ld_solve_kernel: block x thread -> (row, 8 columns)
static void solve(Table &t, const LdPanel &pn)
{
    const int rows = t.m + t.K;
    for (int blk = 0; blk < pn.solve_blocks; blk++)
        for (int tid = 0; tid < 256; tid++)
        {
            const int r = tid >> 3, cg = tid & 7, gr = pn.j0 + pn.nb + blk * kLdSolveRows + r;
            if (gr >= rows) continue;
            for (int i = 0; i < 8; i++)
            {
                const int c = cg + 8 * i;
                if (c < pn.nb) t.at(gr, pn.j0 + c)++;
            }
        }
}

// ld_update_kernel: grid (tc, tr), thread -> 4 x 4 elements; the staging reads are walked too
static void update(Table &t, const LdPanel &pn, Table &reads)
{
    const int rows = t.m + t.K, c0 = pn.j0 + kLdPanel;
    for (int ti = 0; ti < pn.tr; ti++)
        for (int tj = 0; tj < pn.tc; tj++)
        {
            if (!ld_tile_active(ti, tj)) continue;
            const int rbase = c0 + ti * kLdTile, cbase = c0 + tj * kLdTile;
            for (int kh = 0; kh < kLdPanel; kh += 32)
                for (int idx = 0; idx < 32 * kLdTile; idx++)
                {
                    const int kk = idx & 31, r = idx >> 5;
                    if (rbase + r < rows) reads.at(rbase + r, pn.j0 + kh + kk)++;
                    if (cbase + r < t.m) reads.at(cbase + r, pn.j0 + kh + kk)++;
                }
            for (int tid = 0; tid < 256; tid++)
            {
                const int ty = tid >> 4, tx = tid & 15;
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++)
                    {
                        const int gr = rbase + ty * 4 + i, gc = cbase + tx * 4 + j;
                        if (gr < rows && gc < t.m && (gr >= t.m || gc <= gr)) t.at(gr, gc)++;
                    }
            }
        }
}

static int walk(int m, int K)
{
    Table f(m, K), s(m, K), u(m, K), reads(m, K);
    const std::vector<LdPanel> panels = ld_panels(m, K);
    CHECK(!panels.empty() && panels.front().j0 == 0);
    int next = 0;
    for (const LdPanel &pn : panels)
    {
        CHECK(pn.j0 == next && pn.nb >= 1 && pn.nb <= kLdPanel && pn.j0 + pn.nb <= m);
        next = pn.j0 + pn.nb;
        const int c0 = next;
        CHECK(pn.tc == 0 || pn.nb == kLdPanel);  // a trailing update always has the full depth
        CHECK(pn.tr >= pn.tc && pn.tr <= 65535);
        f.clear();
        s.clear();
        u.clear();
        factor(f, pn);
        solve(s, pn);
        if (pn.tc > 0) update(u, pn, reads);
        for (int r = 0; r < m + K; r++)
            for (int c = 0; c < m; c++)
            {
                if (r < m && c > r) continue;
                const size_t at = (size_t)r * (size_t)m + (size_t)c;
                const bool in_panel = c >= pn.j0 && c < c0;
                CHECK(f.n[at] == ((in_panel && r < c0) ? 1 : 0));
                CHECK(s.n[at] == ((in_panel && r >= c0) ? 1 : 0));
                CHECK(u.n[at] == ((c >= c0 && r >= c0) ? 1 : 0));  // every trailing element exactly once per panel
            }
    }
    CHECK(next == m);
    return (int)panels.size();
}

static void arguments()
{
    const long long M = 1000;
    const int p = 6;
    std::vector<int> iv(900), ex = {0, 1, 2, 0, 1};
    for (int i = 0; i < 600; i++) iv[(size_t)i] = i;
    for (int i = 0; i < 300; i++) iv[(size_t)(600 + i)] = 2 * i;
    const int outcome[2] = {4, 5};
    const long long iv_off[3] = {0, 600, 900};
    const int ex_off[3] = {0, 3, 5};
    LdPlan plan;
    std::string msg;
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, kLdBytes, plan, msg) == 0);
    CHECK(plan.outcomes.size() == 2 && plan.ws_doubles == 600u * 600u && plan.zt_doubles == 4u * 600u && plan.max_chunks == 3);
    CHECK(plan.outcomes[1].iv0 == 600 && plan.outcomes[1].m == 300 && plan.outcomes[1].k == 2 && plan.outcomes[1].ex0 == 3);
    // the outcomes are those of cusk_mvivw's plan, each at the start of the one workspace
    CHECK(plan.outcomes[0].nchunks == 3 && plan.outcomes[1].nchunks == 2 && plan.outcomes[1].o == 5 && plan.outcomes[1].out == 1);
    for (const MvOutcome &q : plan.outcomes) CHECK(q.part0 == 0 && q.chunk0 == 0);
    // the bound: exactly m * m * 8 fits, one byte less does not, and the message names the outcome
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, 600ll * 600 * 8, plan, msg) == 0);
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, 600ll * 600 * 8 - 1, plan, msg) == 1);
    CHECK(msg.find("outcome 0") != std::string::npos && msg.find("mvivw_ld_bytes") != std::string::npos);
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, 300ll * 300 * 8, plan, msg) == 1);
    CHECK(msg.find("outcome 0") != std::string::npos);
    const int swapped[2] = {5, 4};
    const long long iv_off2[3] = {0, 300, 900};
    std::vector<int> iv2(900);
    for (int i = 0; i < 300; i++) iv2[(size_t)i] = 2 * i;
    for (int i = 0; i < 600; i++) iv2[(size_t)(300 + i)] = i;
    CHECK(mvivw_ld_plan_build(M, p, 2, swapped, iv_off2, iv2.data(), ex_off, ex.data(), 0, 0.0, 300ll * 300 * 8, plan, msg) == 1);
    CHECK(msg.find("outcome 1") != std::string::npos);
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, 0, plan, msg) == 1);
    // ridge
    for (double bad : {1.0, -1e-300, 2.0, std::nan(""), -(double)INFINITY, (double)INFINITY})
    {
        CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, bad, kLdBytes, plan, msg) == 1);
        CHECK(msg.find("ridge") != std::string::npos);
    }
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.999, kLdBytes, plan, msg) == 0);
    // the errors of cusk_mvivw come first
    iv[5] = 4;
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 0, 0.0, kLdBytes, plan, msg) == 1);
    CHECK(msg.find("strictly ascending") != std::string::npos);
    iv[5] = 5;
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off, iv.data(), ex_off, ex.data(), 3, 0.0, kLdBytes, plan, msg) == 1);
    // status 1 never reaches the device and does not count against the bound
    const long long iv_off3[3] = {0, 3, 600};
    CHECK(mvivw_ld_plan_build(M, p, 2, outcome, iv_off3, iv.data(), ex_off, ex.data(), 0, 0.0, kLdBytes, plan, msg) == 0);
    CHECK(plan.status[0] == 1 && plan.status[1] == 0 && plan.outcomes.size() == 1 && plan.outcomes[0].out == 1);
}

int main()
{
    int cases = 0, panels = 0;
    for (int m : {2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 513, 700})
        for (int K : {2, 3, 31, 32, 33, 64, 65, 127, 128})
        {
            if (m < K) continue;  // m > k = K - 1 on the device
            panels += walk(m, K);
            cases++;
        }
    std::mt19937 rng(12345);
    for (int it = 0; it < 40; it++)
    {
        const int K = 2 + (int)(rng() % 127);
        const int m = K + (int)(rng() % 600);
        panels += walk(m, K);
        cases++;
    }
    arguments();
    std::printf("mvivw_ld_plan_selftest: ok (%d shapes, %d panels, %lld checks)\n", cases, panels, g_checks);
    return 0;
}
