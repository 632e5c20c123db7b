// batch_plan.h -- the index arithmetic of a batched run (batch_pipeline.h) and the separating-set remap every reduction
// shares (reduce.h), as plain functions over std::vector with no engine call in them: where each block lies in the two
// batch allocations, the tables of cusk_gather_rows, the slices of the packed adjacency words, what is kept after the
// prefilter, and the records in each block's retained numbering.  Tabulated on the CPU by tools/batch_plan_selftest.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <numeric>

#include "result_types.h"

namespace host {

inline int pad64(size_t v) { return (int)((v + 63) / 64 * 64); }

// Stage-one layout: block b = variables [base[b], base[b] + m[b] + p) of one n1 x n1 allocation, bases multiples of 64;
// msum = the markers of all blocks.  False when n1 is no int.
inline bool plan_layout(const std::vector<int> &m, size_t p, std::vector<int> &base, size_t &n1, size_t &msum)
{
    base.resize(m.size());
    n1 = msum = 0;
    for (size_t b = 0; b < m.size(); b++)
    {
        base[b] = (int)n1;
        n1 += (size_t)pad64((size_t)m[b] + p);
        msum += (size_t)m[b];
    }
    return n1 <= (size_t)0x7fffffff;
}

// The count pass of a batch at per-pair sample sizes: cusk_pair_counts takes ONE ascending, distinct list of marker rows,
// a batch names its blocks in any order.  ix = the markers of all blocks in ascending order of the blocks' first marker;
// row0[b] = where block b's (blocks[b] of the caller: first[b], m[b] markers) rows start in that list.  False when two
// blocks share a marker (the same block named twice): no such list exists, the caller counts block by block.
inline bool plan_count_pass(const std::vector<long long> &first, const std::vector<int> &m, std::vector<int> &ix,
                            std::vector<size_t> &row0)
{
    const size_t B = first.size();
    std::vector<size_t> order(B);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return first[a] < first[b]; });
    ix.clear();
    row0.assign(B, 0);
    long long end = 0;
    for (size_t b : order)
    {
        if (m[b] <= 0) continue;
        if (first[b] < end) return false;
        row0[b] = ix.size();
        for (int i = 0; i < m[b]; i++) ix.push_back((int)(first[b] + i));
        end = first[b] + m[b];
    }
    return true;
}

// The tables of one cusk_gather_rows call, one row per retained variable, block after block.  Row i of block k is row
// idx = row_src = src_base[k] + keep[k][i] of the source matrix; of it the row_k = keep[k].size() columns
// idx[row_first .. row_first + row_k) go to row_out:
//   lo2 given: onto the diagonal of an n2 x n2 matrix, row_out = (lo2[k] + i) * n2 + lo2[k];
//   otherwise: dense row_k x row_k cells laid back to back, `cells` floats in all (keep[k] = the p traits of every
//              block: a table of p columns, row_out = row * p).
struct GatherTables
{
    std::vector<int> idx, row_src, row_k;
    std::vector<long long> row_first, row_out;
    size_t cells = 0;
    long long rows() const { return (long long)idx.size(); }
};

inline void plan_gather(const std::vector<int> &src_base, const std::vector<std::vector<int>> &keep, const std::vector<int> *lo2,
                        size_t n2, GatherTables &g)
{
    size_t rows = 0, r = 0;
    for (const std::vector<int> &P : keep) rows += P.size();
    g.idx.resize(rows);
    g.row_src.resize(rows);
    g.row_k.resize(rows);
    g.row_first.resize(rows);
    g.row_out.resize(rows);
    g.cells = 0;
    for (size_t k = 0; k < keep.size(); k++)
    {
        const size_t f0 = r, kk = keep[k].size();
        for (size_t i = 0; i < kk; i++, r++)
        {
            g.idx[r] = g.row_src[r] = src_base[k] + keep[k][i];
            g.row_k[r] = (int)kk;
            g.row_first[r] = (long long)f0;
            g.row_out[r] = lo2 ? ((long long)(*lo2)[k] + (long long)i) * (long long)n2 + (*lo2)[k] : (long long)(g.cells + i * kk);
        }
        g.cells += kk * kk;
    }
}

// `rows` rows over `cols` columns of one block out of the packed words of cusk_result_adj_bits_blocks (rows = cols = the
// block) or cusk_result_adj_bits_blocks_tail (rows = the p trait rows); pos runs on to the next block
inline size_t bits_words(int rows, int cols) { return (size_t)rows * (size_t)((cols + 63) / 64); }

inline Bits slice_bits(const std::vector<uint64_t> &packed, size_t &pos, int rows, int cols)
{
    Bits b;
    b.n = rows;
    b.words = (cols + 63) / 64;
    b.w.assign(packed.begin() + (long)pos, packed.begin() + (long)(pos + bits_words(rows, cols)));
    pos += bits_words(rows, cols);
    return b;
}

// The blocks that passed the prefilter (kept: their positions in the batch, ascending): their variable ranges in stage one
inline void plan_kept(const std::vector<int> &kept, const std::vector<int> &m, const std::vector<int> &base, size_t p,
                      std::vector<int> &lo1, std::vector<int> &hi1)
{
    lo1.resize(kept.size());
    hi1.resize(kept.size());
    for (size_t k = 0; k < kept.size(); k++)
    {
        lo1[k] = base[(size_t)kept[k]];
        hi1[k] = lo1[k] + m[(size_t)kept[k]] + (int)p;
    }
}

// Their size tables (mxp_ess: m[b] x p per block of the batch, back to back; pxp_ess: p x p per block) and marker counts,
// compacted to the kept blocks
inline void compact_sizes(const std::vector<int> &kept, const std::vector<int> &m, size_t p, const std::vector<float> &mxp_ess,
                          const std::vector<float> &pxp_ess, std::vector<int> &mk, std::vector<float> &me, std::vector<float> &pe)
{
    std::vector<size_t> off(m.size() + 1, 0);
    for (size_t b = 0; b < m.size(); b++) off[b + 1] = off[b] + (size_t)m[b] * p;
    mk.resize(kept.size());
    me.clear();
    me.reserve(mxp_ess.size());
    pe.resize(kept.size() * p * p);
    for (size_t k = 0; k < kept.size(); k++)
    {
        const size_t b = (size_t)kept[k];
        mk[k] = m[b];
        me.insert(me.end(), mxp_ess.begin() + (long)off[b], mxp_ess.begin() + (long)off[b + 1]);
        std::copy_n(pxp_ess.begin() + (long)(b * p * p), p * p, pe.begin() + (long)(k * p * p));
    }
}

// Their marker rows in one list, block after block (a block named twice repeats its rows)
inline void kept_marker_rows(const std::vector<int> &kept, const std::vector<long long> &first, const std::vector<int> &m,
                             std::vector<int> &rows)
{
    rows.clear();
    for (int b : kept)
        for (int i = 0; i < m[(size_t)b]; i++) rows.push_back((int)(first[(size_t)b] + i));
}

// ---- separating sets in the retained variables' numbering (parent_set.cpp:84-175) ----
// A run over n variables retains P (ascending).  pos: variable -> its position in P, or -1.  o2n: the reference's
// old_to_new, keyed by index_map[P[i]] when there is an index_map (stage two: the STAGE-ONE index of the variable)
// although the set members it is asked for are variables of this run; only keys below n can be asked
// for, a later key overwrites an earlier one.
inline void remap_tables(const std::vector<int> &P, const std::vector<int> *index_map, int n, std::vector<int> &pos, std::vector<int> &o2n)
{
    pos.assign((size_t)n, -1);
    o2n.assign((size_t)n, -1);
    for (size_t i = 0; i < P.size(); i++)
    {
        pos[(size_t)P[i]] = (int)i;
        const int key = index_map ? (*index_map)[(size_t)P[i]] : P[i];
        if (key >= 0 && key < n) o2n[(size_t)key] = (int)i;
    }
}

// One record: the pair (x, y) separated by the members rs[0 .. ML) (-1: none), all of them variables lo .. lo + n of a
// batch.  False when x or y is not retained.  Members that are not retained are dropped, the rest is compacted; a retained
// member that is no key of o2n maps to 0; at most max_level source entries are read.
inline bool remap_sepset(const std::vector<int> &pos, const std::vector<int> &o2n, int lo, int x, int y, const int *rs, size_t max_level,
                         SepRec &q)
{
    auto at = [&](int v) { return (size_t)(v - lo) < pos.size() ? pos[(size_t)(v - lo)] : -1; };
    q.ix = at(x);
    q.iy = at(y);
    q.cnt = 0;
    if (q.ix < 0 || q.iy < 0) return false;
    for (size_t l = 0; l < max_level && l < (size_t)ML; l++)
        if (rs[l] != -1 && at(rs[l]) >= 0) q.s[q.cnt++] = std::max(o2n[(size_t)(rs[l] - lo)], 0);
    return true;
}

// The `cnt` records (x, y, rs[ML]) of a batched stage-two run, ordered by (x, y), i.e. block after block: the record of
// block k (lo2[k] <= x < hi2[k]) in the numbering of P2[k], P1[k] = the stage-one index of the block's stage-two
// variables; sink(k, record) for every record kept.  False when a record lies outside every block.
template <class Sink>
inline bool remap_batch_records(long long cnt, const int *x, const int *y, const int *rs, const std::vector<int> &lo2,
                                const std::vector<int> &hi2, const std::vector<std::vector<int>> &P1,
                                const std::vector<std::vector<int>> &P2, Sink sink)
{
    const size_t K = lo2.size();
    size_t k = 0, cur = K;
    std::vector<int> pos, o2n;
    SepRec q;
    for (long long r = 0; r < cnt; r++)
    {
        while (k < K && x[r] >= hi2[k]) k++;
        if (k >= K || x[r] < lo2[k]) return false;
        if (cur != k) remap_tables(P2[k], &P1[k], hi2[k] - lo2[k], pos, o2n);
        cur = k;
        if (remap_sepset(pos, o2n, lo2[k], x[r], y[r], rs + (size_t)r * ML, ML, q)) sink(k, q);
    }
    return true;
}

// arrival order -> ascending cells of a k x k result; records of one cell keep their order (the later one overwrites the
// head of the earlier, as in the dense reduction)
inline void sort_recs(std::vector<SepRec> &recs, size_t k)
{
    auto less = [k](const SepRec &a, const SepRec &b) { return (size_t)a.ix * k + (size_t)a.iy < (size_t)b.ix * k + (size_t)b.iy; };
    if (!std::is_sorted(recs.begin(), recs.end(), less)) std::stable_sort(recs.begin(), recs.end(), less);
}

// One run's records as the dense array: P.size()^2 * max_level ints, -1 where there is none
inline std::vector<int> reduce_records(long long cnt, const int *x, const int *y, const int *rs, int n, const std::vector<int> &P,
                                       size_t max_level, const std::vector<int> *index_map)
{
    const size_t k = P.size();
    std::vector<int> S(k * k * max_level, -1), pos, o2n;
    remap_tables(P, index_map, n, pos, o2n);
    SepRec q;
    for (long long r = 0; r < cnt; r++)
        if (remap_sepset(pos, o2n, 0, x[r], y[r], rs + (size_t)r * ML, max_level, q))
            std::memcpy(S.data() + ((size_t)q.ix * k + (size_t)q.iy) * max_level, q.s, sizeof(int) * (size_t)q.cnt);
    return S;
}

// The same cells as a list in ascending (ix, iy) order.  Returns false (and leaves the list empty) when two records name
// the same cell -- the dense form's "the later record overwrites the head of the earlier" is then what the caller must
// reproduce (never seen: an ordered pair has one record).
inline bool reduce_records_sparse(long long cnt, const int *x, const int *y, const int *rs, int n, const std::vector<int> &P,
                                  size_t max_level, const std::vector<int> *index_map, std::vector<SepRec> &out)
{
    out.clear();
    out.reserve((size_t)cnt);
    std::vector<int> pos, o2n;
    remap_tables(P, index_map, n, pos, o2n);
    SepRec q;
    for (long long r = 0; r < cnt; r++)
        if (remap_sepset(pos, o2n, 0, x[r], y[r], rs + (size_t)r * ML, max_level, q)) out.push_back(q);
    sort_recs(out, P.size());
    for (size_t i = 1; i < out.size(); i++)
        if (out[i].ix == out[i - 1].ix && out[i].iy == out[i - 1].iy)
        {
            out.clear();
            return false;
        }
    return true;
}

}  // namespace host
