// batch_plan_selftest.cpp -- the index arithmetic of a batched run and the separating-set remap (csrc/host/batch_plan.h)
// against tables written out by hand for small cases, and the remap against a restatement of the reference's rule with the
// containers the reference uses (a std::map keyed by the stage-one index; a search of the retained list)
// over seeded random cases.  Stand-alone, no HIP, not linked to the library:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/batch_plan_selftest.cpp -o batch_plan_selftest
//   ./batch_plan_selftest
#include "../ci-gwas_amd/csrc/host/batch_plan.h"

#include <cstdio>
#include <map>
#include <random>

using namespace host;

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

using VI = std::vector<int>;
using VL = std::vector<long long>;
using VF = std::vector<float>;

static void test_layout()
{
    VI base;
    size_t n1 = 0, msum = 0;
    EXPECT(plan_layout({59}, 5, base, n1, msum) && base == VI{0} && n1 == 64 && msum == 59);  // m + p = 64
    EXPECT(plan_layout({60}, 5, base, n1, msum) && base == VI{0} && n1 == 128 && msum == 60);  // 65
    EXPECT(plan_layout({1}, 0, base, n1, msum) && base == VI{0} && n1 == 64 && msum == 1);     // 1
    EXPECT(plan_layout({0}, 1, base, n1, msum) && base == VI{0} && n1 == 64 && msum == 0);
    EXPECT(plan_layout({64, 1, 65}, 0, base, n1, msum) && base == (VI{0, 64, 128}) && n1 == 256 && msum == 130);  // p = 0
    EXPECT(plan_layout({10, 0, 3}, 2, base, n1, msum) && base == (VI{0, 64, 128}) && n1 == 192 && msum == 13);    // a block of size 0
    EXPECT(plan_layout({5, 0, 7}, 0, base, n1, msum) && base == (VI{0, 64, 64}) && n1 == 128 && msum == 12);      // ... of no variable
    EXPECT(plan_layout({59, 60, 1}, 5, base, n1, msum) && base == (VI{0, 64, 192}) && n1 == 256 && msum == 120);
    EXPECT(plan_layout({}, 5, base, n1, msum) && base.empty() && n1 == 0 && msum == 0);
    EXPECT(plan_layout({2147483584}, 0, base, n1, msum) && n1 == 2147483584u);  // the largest batch: 2^31 - 64 variables
    EXPECT(!plan_layout({2147483584, 1}, 0, base, n1, msum));

    VI ix;
    std::vector<size_t> row0;
    using VS = std::vector<size_t>;
    EXPECT(plan_count_pass({100, 40, 0}, {3, 2, 4}, ix, row0));  // blocks named in descending order of first marker
    EXPECT(ix == (VI{0, 1, 2, 3, 40, 41, 100, 101, 102}) && row0 == (VS{6, 4, 0}));
    EXPECT(plan_count_pass({0, 3}, {3, 2}, ix, row0) && ix == (VI{0, 1, 2, 3, 4}) && row0 == (VS{0, 3}));  // adjacent blocks
    EXPECT(!plan_count_pass({5, 5}, {2, 2}, ix, row0));  // the same block twice
    EXPECT(!plan_count_pass({0, 2}, {3, 2}, ix, row0));  // one shared marker
    EXPECT(!plan_count_pass({7, 40, 7}, {3, 2, 3}, ix, row0));
    EXPECT(plan_count_pass({10, 10, 0}, {2, 0, 1}, ix, row0) && ix == (VI{0, 10, 11}) && row0 == (VS{1, 0, 0}));  // a block of size 0
    EXPECT(plan_count_pass({}, {}, ix, row0) && ix.empty() && row0.empty());
}

static void test_kept()
{
    const VI m{2, 1, 3}, base{0, 64, 128};
    const VL first{10, 20, 30};
    const size_t p = 2;
    const VF mxp_ess{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};  // 2 x 2, 1 x 2, 3 x 2
    const VF pxp_ess{100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111};
    VI lo1, hi1, mk, rows{-7};
    VF me, pe;
    // the middle block skipped
    plan_kept({0, 2}, m, base, p, lo1, hi1);
    compact_sizes({0, 2}, m, p, mxp_ess, pxp_ess, mk, me, pe);
    EXPECT(lo1 == (VI{0, 128}) && hi1 == (VI{4, 133}) && mk == (VI{2, 3}));
    EXPECT(me == (VF{0, 1, 2, 3, 6, 7, 8, 9, 10, 11}) && pe == (VF{100, 101, 102, 103, 108, 109, 110, 111}));
    EXPECT(rows == VI{-7});  // (without the marker-row list: nobody touched it)
    kept_marker_rows({0, 2}, first, m, rows);
    EXPECT(rows == (VI{10, 11, 30, 31, 32}));
    // only the last block kept
    plan_kept({2}, m, base, p, lo1, hi1);
    compact_sizes({2}, m, p, mxp_ess, pxp_ess, mk, me, pe);
    kept_marker_rows({2}, first, m, rows);
    EXPECT(lo1 == VI{128} && hi1 == VI{133} && mk == VI{3} && rows == (VI{30, 31, 32}));
    EXPECT(me == (VF{6, 7, 8, 9, 10, 11}) && pe == (VF{108, 109, 110, 111}));
    // all kept
    plan_kept({0, 1, 2}, m, base, p, lo1, hi1);
    compact_sizes({0, 1, 2}, m, p, mxp_ess, pxp_ess, mk, me, pe);
    EXPECT(lo1 == base && hi1 == (VI{4, 67, 133}) && mk == m && me == mxp_ess && pe == pxp_ess);
    // none kept
    plan_kept({}, m, base, p, lo1, hi1);
    compact_sizes({}, m, p, mxp_ess, pxp_ess, mk, me, pe);
    kept_marker_rows({}, first, m, rows);
    EXPECT(lo1.empty() && hi1.empty() && mk.empty() && me.empty() && pe.empty() && rows.empty());
    // a block named twice repeats its rows
    kept_marker_rows({0, 1}, {10, 10}, {2, 2}, rows);
    EXPECT(rows == (VI{10, 11, 10, 11}));
}

static void test_gather()
{
    GatherTables g;
    // two blocks of 3 and 1 markers with p = 2 traits at the variables 0 and 64 of stage one
    // (a) their trait rows to a host table of p columns per block
    plan_gather({3, 65}, {{0, 1}, {0, 1}}, nullptr, 0, g);
    EXPECT(g.idx == (VI{3, 4, 65, 66}) && g.row_src == g.idx && g.row_k == (VI{2, 2, 2, 2}));
    EXPECT(g.row_first == (VL{0, 0, 2, 2}) && g.row_out == (VL{0, 2, 4, 6}) && g.cells == 8 && g.rows() == 4);
    // (b) what they retain -- the second its traits only -- onto the diagonal of stage two
    const VI lo2{0, 64};
    plan_gather({0, 64}, {{1, 3, 4}, {1, 2}}, &lo2, 128, g);
    EXPECT(g.idx == (VI{1, 3, 4, 65, 66}) && g.row_src == g.idx && g.row_k == (VI{3, 3, 3, 2, 2}));
    EXPECT(g.row_first == (VL{0, 0, 0, 3, 3}) && g.row_out == (VL{0, 128, 256, 8256, 8384}) && g.rows() == 5);
    // (c) what stage two retains as dense cells back to back
    plan_gather({0, 64}, {{0, 1, 2}, {0, 1}}, nullptr, 0, g);
    EXPECT(g.idx == (VI{0, 1, 2, 64, 65}) && g.row_src == g.idx && g.row_k == (VI{3, 3, 3, 2, 2}));
    EXPECT(g.row_first == (VL{0, 0, 0, 3, 3}) && g.row_out == (VL{0, 3, 6, 9, 11}) && g.cells == 13);
    // retained lists of 64 and of 65 variables: the next block moves by 64 and by 128
    EXPECT(pad64(0) == 0 && pad64(1) == 64 && pad64(64) == 64 && pad64(65) == 128);
    std::vector<VI> keep{VI(64), VI(65), VI{5}};
    for (int i = 0; i < 64; i++) keep[0][(size_t)i] = 2 * i;
    for (int i = 0; i < 65; i++) keep[1][(size_t)i] = i + 3;
    const VI lo3{0, 64, 192};
    plan_gather({0, 128, 256}, keep, &lo3, 256, g);
    EXPECT(g.rows() == 130 && g.idx[63] == 126 && g.idx[64] == 131 && g.idx[128] == 195 && g.idx[129] == 261);
    EXPECT(g.row_k[63] == 64 && g.row_k[64] == 65 && g.row_k[128] == 65 && g.row_k[129] == 1);
    EXPECT(g.row_first[63] == 0 && g.row_first[64] == 64 && g.row_first[128] == 64 && g.row_first[129] == 129);
    EXPECT(g.row_out[63] == 63 * 256 && g.row_out[64] == 64 * 256 + 64 && g.row_out[128] == 128 * 256 + 64 && g.row_out[129] == 192 * 256 + 192);
    plan_gather({0, 128, 256}, keep, nullptr, 0, g);
    EXPECT(g.row_out[63] == 63 * 64 && g.row_out[64] == 4096 && g.row_out[128] == 4096 + 64 * 65 && g.row_out[129] == 4096 + 4225);
    EXPECT(g.cells == 4096 + 4225 + 1);
    plan_gather({}, {}, nullptr, 0, g);
    EXPECT(g.rows() == 0 && g.cells == 0 && g.row_out.empty());
}

static void test_slicer()
{
    EXPECT(bits_words(64, 64) == 64 && bits_words(65, 65) == 130 && bits_words(1, 64) == 1 && bits_words(3, 65) == 6 && bits_words(0, 65) == 0);
    std::vector<uint64_t> packed(64 + 130 + 1 + 6);
    for (size_t i = 0; i < packed.size(); i++) packed[i] = 1000 + i;
    packed[64 + 64 * 2 + 1] = 1;  // row 64, column 64 of the second block
    size_t pos = 0;
    const Bits A = slice_bits(packed, pos, 64, 64);  // one word per row
    EXPECT(pos == 64 && A.n == 64 && A.words == 1 && A.w.size() == 64 && A.w[0] == 1000 && A.w[63] == 1063);
    const Bits B = slice_bits(packed, pos, 65, 65);  // two words per row
    EXPECT(pos == 194 && B.n == 65 && B.words == 2 && B.w.size() == 130 && B.w[0] == 1064 && B.w[128] == 1192 && B.w[129] == 1);
    EXPECT(B.get(64, 64) && !B.get(64, 65) && B.get(64, 3) == ((1192 >> 3) & 1));
    const Bits T1 = slice_bits(packed, pos, 1, 64);  // traits only, p = 1
    EXPECT(pos == 195 && T1.n == 1 && T1.words == 1 && T1.w == std::vector<uint64_t>{1194});
    const Bits T3 = slice_bits(packed, pos, 3, 65);  // traits only, p = 3
    EXPECT(pos == 201 && T3.n == 3 && T3.words == 2 && T3.w == (std::vector<uint64_t>{1195, 1196, 1197, 1198, 1199, 1200}));
}

// sparse records as the engine hands them out: x, y and ML members (-1: none) per record
struct Records
{
    VI x, y, rs;
    void add(int xx, int yy, const VI &members)
    {
        x.push_back(xx);
        y.push_back(yy);
        for (int l = 0; l < ML; l++) rs.push_back((size_t)l < members.size() ? members[(size_t)l] : -1);
    }
    long long cnt() const { return (long long)x.size(); }
};

static bool same(const SepRec &q, int ix, int iy, const VI &s)
{
    return q.ix == ix && q.iy == iy && q.cnt == (int)s.size() && std::equal(s.begin(), s.end(), q.s);
}

struct Sunk
{
    size_t k;
    SepRec q;
};

static void test_remap_cases()
{
    // a block of 6 stage-two variables with the stage-one indices `orig`, of which 1, 2, 4, 5 are retained: the keys are
    // orig[1] = 2 -> 0 and orig[2] = 4 -> 1; orig[4] = 9 and orig[5] = 11 are no variable of this run
    const VI orig{0, 2, 4, 5, 9, 11}, P{1, 2, 4, 5};
    VI pos, o2n;
    remap_tables(P, &orig, 6, pos, o2n);
    EXPECT(pos == (VI{-1, 0, 1, -1, 2, 3}) && o2n == (VI{-1, -1, 0, -1, 1, -1}));
    SepRec q;
    const int none[ML] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    EXPECT(!remap_sepset(pos, o2n, 0, 0, 1, none, ML, q) && !remap_sepset(pos, o2n, 0, 1, 3, none, ML, q));  // x, y not retained
    EXPECT(!remap_sepset(pos, o2n, 0, 6, 1, none, ML, q) && !remap_sepset(pos, o2n, 0, 1, -1, none, ML, q));  // ... no variable at all
    EXPECT(remap_sepset(pos, o2n, 0, 2, 1, none, ML, q) && same(q, 1, 0, {}));
    Records R;
    R.add(0, 1, {2});        // x not retained: skipped
    R.add(1, 2, {3, 4, 1});  // 3 is not retained: dropped, the rest compacted; 4 is the key of 1; 1 is no key: 0
    R.add(4, 5, {5, 2, 4});  // 5 is retained, its stage-one index 11 is no variable and 5 is no key: 0
    std::vector<SepRec> out;
    EXPECT(reduce_records_sparse(R.cnt(), R.x.data(), R.y.data(), R.rs.data(), 6, P, ML, &orig, out));
    EXPECT(out.size() == 2 && same(out[0], 0, 1, {1, 0}) && same(out[1], 2, 3, {0, 0, 1}));
    EXPECT(reduce_records_sparse(R.cnt(), R.x.data(), R.y.data(), R.rs.data(), 6, P, 2, &orig, out));  // two entries read
    EXPECT(out.size() == 2 && same(out[0], 0, 1, {1}) && same(out[1], 2, 3, {0, 0}));
    EXPECT(reduce_records_sparse(R.cnt(), R.x.data(), R.y.data(), R.rs.data(), 6, P, ML, nullptr, out));  // stage one: own keys
    EXPECT(out.size() == 2 && same(out[0], 0, 1, {2, 0}) && same(out[1], 2, 3, {3, 1, 2}));

    // keys that collide: the later one wins
    const VI orig2{3, 3, 0, 3}, P2{0, 1, 3};
    remap_tables(P2, &orig2, 4, pos, o2n);
    EXPECT(pos == (VI{0, 1, -1, 2}) && o2n == (VI{-1, -1, -1, 2}));
    Records C;
    C.add(0, 1, {3, 0});
    EXPECT(reduce_records_sparse(1, C.x.data(), C.y.data(), C.rs.data(), 4, P2, ML, &orig2, out) && out.size() == 1 && same(out[0], 0, 1, {2, 0}));

    // all ML members
    VI all(20), members;
    std::iota(all.begin(), all.end(), 0);
    for (int l = 0; l < ML; l++) members.push_back(l + 2);
    Records F;
    F.add(0, 1, members);
    EXPECT(reduce_records_sparse(1, F.x.data(), F.y.data(), F.rs.data(), 20, all, ML, &all, out) && out.size() == 1 && same(out[0], 0, 1, members));

    // two cells out of order are sorted, two records of one cell are refused
    Records D;
    D.add(2, 1, {});
    D.add(1, 2, {4});
    EXPECT(reduce_records_sparse(2, D.x.data(), D.y.data(), D.rs.data(), 6, P, ML, &orig, out) && out.size() == 2 && same(out[0], 0, 1, {1}) &&
           same(out[1], 1, 0, {}));
    D.add(2, 1, {4});
    EXPECT(!reduce_records_sparse(3, D.x.data(), D.y.data(), D.rs.data(), 6, P, ML, &orig, out) && out.empty());
    const VI S = reduce_records(3, D.x.data(), D.y.data(), D.rs.data(), 6, P, 3, &orig);  // the dense form takes the later record
    EXPECT(S.size() == 48 && S[(0 * 4 + 1) * 3] == 1 && S[(0 * 4 + 1) * 3 + 1] == -1 && S[(1 * 4 + 0) * 3] == 1 && S[0] == -1);

    // the records of two blocks in (x, y) order, the first block above at variables 0-5, the colliding one at 64-67
    Records T;
    T.add(1, 2, {3, 4, 1});
    T.add(4, 5, {5, 2, 4});
    T.add(64, 65, {67, 64});
    T.add(66, 64, {});  // 66 is not retained
    T.add(67, 65, {65, 66, 67});
    const VI lo2{0, 64}, hi2{6, 68};
    std::vector<Sunk> got;
    auto sink = [&](size_t k, const SepRec &r) { got.push_back({k, r}); };
    EXPECT(remap_batch_records(T.cnt(), T.x.data(), T.y.data(), T.rs.data(), lo2, hi2, {orig, orig2}, {P, P2}, sink));
    EXPECT(got.size() == 4 && got[0].k == 0 && same(got[0].q, 0, 1, {1, 0}) && got[1].k == 0 && same(got[1].q, 2, 3, {0, 0, 1}));
    EXPECT(got.size() == 4 && got[2].k == 1 && same(got[2].q, 0, 1, {2, 0}) && got[3].k == 1 && same(got[3].q, 2, 1, {0, 2}));
    T.add(68, 64, {});  // padding behind the last block
    EXPECT(!remap_batch_records(T.cnt(), T.x.data(), T.y.data(), T.rs.data(), lo2, hi2, {orig, orig2}, {P, P2}, sink));
    Records U;
    U.add(10, 1, {});  // padding between the blocks
    EXPECT(!remap_batch_records(1, U.x.data(), U.y.data(), U.rs.data(), lo2, hi2, {orig, orig2}, {P, P2}, sink));
    EXPECT(remap_batch_records(0, nullptr, nullptr, nullptr, lo2, hi2, {orig, orig2}, {P, P2}, sink));
}

// The rule in the reference's own terms.  `retained` lists the kept variables of a run in ascending order; old_to_new maps
// index_map[retained[i]] (stage two: the stage-one index) or retained[i] to i, assigned in that order; a set member that is
// not retained is dropped, one that is looked up in old_to_new as it stands, where a missing key reads as 0.
struct Expected
{
    bool kept = false;
    int ix = -1, iy = -1;
    VI s;
};

static int where(const VI &retained, int v)
{
    for (size_t i = 0; i < retained.size(); i++)
        if (retained[i] == v) return (int)i;
    return -1;
}

static Expected brute(const VI &retained, const VI *index_map, int x, int y, const int *rs, size_t max_level)
{
    std::map<int, int> old_to_new;
    for (size_t i = 0; i < retained.size(); i++) old_to_new[index_map ? (*index_map)[(size_t)retained[i]] : retained[i]] = (int)i;
    Expected ex;
    ex.ix = where(retained, x);
    ex.iy = where(retained, y);
    ex.kept = ex.ix >= 0 && ex.iy >= 0;
    for (size_t l = 0; ex.kept && l < max_level && l < (size_t)ML; l++)
        if (rs[l] != -1 && where(retained, rs[l]) >= 0) ex.s.push_back(old_to_new.count(rs[l]) ? old_to_new[rs[l]] : 0);
    return ex;
}

// one random block of n stage-two variables: the stage-one indices (ascending as the pipeline makes them, or with repeats),
// the retained list, and records over the block's variables lo .. lo + n (sorted by (x, y); the same pair twice now and then)
struct RandomBlock
{
    int n = 0;
    VI orig, P;
    std::vector<std::pair<int, int>> pairs;
    std::vector<VI> members;
};

static RandomBlock random_block(std::mt19937 &rng, bool with_duplicates)
{
    RandomBlock b;
    b.n = 1 + (int)(rng() % 12);
    int o = 0;
    for (int i = 0; i < b.n; i++)
    {
        const bool repeats = rng() % 8 == 0;
        o = repeats ? (int)(rng() % (unsigned)(b.n + 2)) : o + (int)(rng() % 3) + (i > 0);
        b.orig.push_back(o);
        if (rng() % 3 != 0) b.P.push_back(i);
    }
    const int nrec = (int)(rng() % 12);
    for (int r = 0; r < nrec; r++) b.pairs.push_back({(int)(rng() % (unsigned)b.n), (int)(rng() % (unsigned)b.n)});
    std::sort(b.pairs.begin(), b.pairs.end());
    if (!with_duplicates) b.pairs.erase(std::unique(b.pairs.begin(), b.pairs.end()), b.pairs.end());
    for (size_t r = 0; r < b.pairs.size(); r++)
    {
        VI s((size_t)(rng() % (ML + 1)));
        for (int &v : s) v = rng() % 7 == 0 ? -1 : (int)(rng() % (unsigned)b.n);
        b.members.push_back(s);
    }
    return b;
}

static void test_remap_random()
{
    std::mt19937 rng(20240611);
    const size_t levels[3] = {3, (size_t)ML, 16};
    for (int it = 0; it < 400; it++)
    {
        // single block: dense and sparse form against the restated rule, with and without an index map
        const RandomBlock b = random_block(rng, it % 4 == 0);
        const size_t max_level = levels[it % 3], k = b.P.size();
        const VI *index_map = (it % 5 == 0) ? nullptr : &b.orig;
        Records R;
        for (size_t r = 0; r < b.pairs.size(); r++) R.add(b.pairs[r].first, b.pairs[r].second, b.members[r]);
        VI want(k * k * max_level, -1);
        std::vector<Expected> cells;
        bool twice = false;
        for (size_t r = 0; r < b.pairs.size(); r++)
        {
            const Expected ex = brute(b.P, index_map, R.x[r], R.y[r], &R.rs[r * ML], max_level);
            if (!ex.kept) continue;
            for (const Expected &c : cells) twice = twice || (c.ix == ex.ix && c.iy == ex.iy);
            cells.push_back(ex);
            std::copy(ex.s.begin(), ex.s.end(), want.begin() + (long)(((size_t)ex.ix * k + (size_t)ex.iy) * max_level));
        }
        EXPECT(reduce_records(R.cnt(), R.x.data(), R.y.data(), R.rs.data(), b.n, b.P, max_level, index_map) == want);
        std::vector<SepRec> out;
        const bool ok = reduce_records_sparse(R.cnt(), R.x.data(), R.y.data(), R.rs.data(), b.n, b.P, max_level, index_map, out);
        EXPECT(ok == !twice && out.size() == (twice ? 0 : cells.size()));
        VI from_list(k * k * max_level, -1);  // the list gives the cells of the dense form
        for (const SepRec &q : out) std::copy(q.s, q.s + q.cnt, from_list.begin() + (long)(((size_t)q.ix * k + (size_t)q.iy) * max_level));
        EXPECT(twice || from_list == want);
        for (size_t i = 1; i < out.size(); i++) EXPECT(out[i - 1].ix * (int)k + out[i - 1].iy < out[i].ix * (int)k + out[i].iy);

        // three such blocks at multiples of 64 in one batch
        std::vector<VI> P1, P2;
        VI lo2, hi2;
        Records T;
        std::vector<std::pair<size_t, Expected>> expect;
        int lo = 64 * (it % 2);
        for (size_t kb = 0; kb < 3; kb++)
        {
            const RandomBlock c = random_block(rng, true);
            for (size_t r = 0; r < c.pairs.size(); r++)
            {
                VI s = c.members[r];
                Records local;
                local.add(c.pairs[r].first, c.pairs[r].second, s);
                const Expected ex = brute(c.P, &c.orig, local.x[0], local.y[0], local.rs.data(), ML);
                if (ex.kept) expect.push_back({kb, ex});
                for (int &v : s) v = v == -1 ? -1 : v + lo;
                T.add(c.pairs[r].first + lo, c.pairs[r].second + lo, s);
            }
            P1.push_back(c.orig);
            P2.push_back(c.P);
            lo2.push_back(lo);
            hi2.push_back(lo + c.n);
            lo += pad64((size_t)c.n) * (1 + (int)(rng() % 2));
        }
        std::vector<Sunk> got;
        EXPECT(remap_batch_records(T.cnt(), T.x.data(), T.y.data(), T.rs.data(), lo2, hi2, P1, P2,
                                   [&](size_t kk, const SepRec &q) { got.push_back({kk, q}); }));
        EXPECT(got.size() == expect.size());
        for (size_t i = 0; i < got.size() && i < expect.size(); i++)
            EXPECT(got[i].k == expect[i].first && same(got[i].q, expect[i].second.ix, expect[i].second.iy, expect[i].second.s));
    }
}

int main()
{
    test_layout();
    test_kept();
    test_gather();
    test_slicer();
    test_remap_cases();
    test_remap_random();
    if (failures)
    {
        std::printf("batch_plan_selftest: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("batch_plan_selftest: ok\n");
    return 0;
}
