// reduce.h -- from a finished skeleton run to the result files: which variables are retained (parent_set.cpp:8-53), the
// retained adjacency and separating sets in the retained variables' own numbering (parent_set.cpp:84-175), and the writers
// of .mdim / .ixs / .adj / .corr / .sep.
#pragma once
#include <algorithm>
#include <cstring>

#include "batch_plan.h"
#include "engine_util.h"
#include "host_io.h"

namespace host {

// parent_set.cpp:8-53: all traits, plus markers reached from a trait through marker nodes in
// at most max_depth hops.  Sorted ascending.
inline std::vector<int> subset_variables(const Bits &G, int num_var, int num_markers, int max_depth)
{
    std::vector<char> keep(num_var, 0);
    for (int i = num_markers; i < num_var; i++) keep[i] = 1;
    for (int start = num_markers; start < num_var; start++)
    {
        std::vector<char> seen(num_var, 0);
        for (int i = num_markers; i < num_var; i++) seen[i] = 1;
        std::vector<int> q{start}, nq;
        for (int depth = 0; depth < max_depth; depth++)
        {
            nq.clear();
            for (int node : q)
            {
                const uint64_t *row = &G.w[(size_t)node * G.words];
                for (int wv = 0; wv * 64 < num_markers; wv++)
                {
                    uint64_t bits = row[wv];
                    while (bits)
                    {
                        const int c = wv * 64 + __builtin_ctzll(bits);
                        bits &= bits - 1;
                        if (c < num_markers && !seen[c])
                        {
                            seen[c] = 1;
                            nq.push_back(c);
                        }
                    }
                }
            }
            q.swap(nq);
        }
        for (int i = 0; i < num_var; i++)
            if (seen[i]) keep[i] = 1;
    }
    std::vector<int> out;
    for (int i = 0; i < num_var; i++)
        if (keep[i]) out.push_back(i);
    return out;
}

// The same for max_depth == 1 from the TRAIT rows alone (`traits`: the last num_var - num_markers rows of the bitmap, row t
// = trait t): one round from every trait reaches exactly its marker neighbours.
inline std::vector<int> subset_variables_depth1(const Bits &traits, int num_var, int num_markers)
{
    std::vector<uint64_t> any((size_t)traits.words, 0ull);
    for (int t = 0; t < traits.n; t++)
        for (int w = 0; w < traits.words; w++) any[(size_t)w] |= traits.w[(size_t)t * traits.words + w];
    std::vector<int> out;
    for (int c = 0; c < num_markers; c++)
        if ((any[(size_t)(c >> 6)] >> (c & 63)) & 1ull) out.push_back(c);
    for (int i = num_markers; i < num_var; i++) out.push_back(i);
    return out;
}

inline std::vector<int> gather_adj(const Bits &G, const std::vector<int> &P)
{
    std::vector<int> out(P.size() * P.size());
    for (size_t a = 0; a < P.size(); a++)
        for (size_t b = 0; b < P.size(); b++) out[a * P.size() + b] = G.get(P[a], P[b]) ? 1 : 0;
    return out;
}

inline std::vector<int> compose(const std::vector<int> &P, const std::vector<int> *index_map)
{
    std::vector<int> out(P.size());
    for (size_t i = 0; i < P.size(); i++) out[i] = index_map ? (*index_map)[P[i]] : P[i];
    return out;
}

// ReducedGC / ReducedGCS of include/mps/parent_set.h (SepRec, one separating set of it: result_types.h)
struct Reduced
{
    size_t num_var = 0, num_phen = 0, max_level = 0;
    std::vector<int> new_to_old;
    std::vector<int> G;
    std::vector<float> C;
    std::vector<float> ess;  // cuskss
    // cusk: the separating sets, num_var^2 * max_level ints, -1 where there is none (570 retained variables: 18 MB for a
    // few thousand sets).  The single-block pipeline keeps the sets as a sorted list (sep_sparse = true) and the dense
    // array is only built for whoever asks for it (dense_sep); the .sep file is written without it (write_sep_streaming).
    mutable std::vector<int> S;
    std::vector<SepRec> sep_recs;  // ascending (ix, iy), one per cell
    bool sep_sparse = false;
    size_t num_markers() const { return num_var - num_phen; }
    bool has_sep() const { return sep_sparse || !S.empty(); }
    const std::vector<int> &dense_sep() const
    {
        if (sep_sparse && S.empty())
        {
            S.assign(num_var * num_var * max_level, -1);
            for (const SepRec &q : sep_recs)
                std::memcpy(&S[((size_t)q.ix * num_var + (size_t)q.iy) * max_level], q.s, sizeof(int) * (size_t)q.cnt);
        }
        return S;
    }
};

inline void sort_sep_recs(Reduced &r) { sort_recs(r.sep_recs, r.num_var); }

// The .sep file of a sparse result: the array goes out in pieces of ~1 MB that are a whole number of cells, from ONE buffer
// of -1 that is patched with the sets of the piece and restored afterwards -- no 18 MB array to fill and to read back
// from memory (the buffer stays in cache), same bytes.
inline void write_sep_streaming(const std::string &path, const Reduced &r)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) die("cannot write " + path);
    const size_t ml = r.max_level, total = r.num_var * r.num_var * ml;
    const size_t piece = ml * ((size_t)(1 << 18) / (ml ? ml : 1));  // ints
    std::vector<int> buf(std::min(piece, total), -1);
    size_t q = 0;
    for (size_t c0 = 0; c0 < total; c0 += piece)
    {
        const size_t c1 = std::min(total, c0 + piece), q0 = q;
        for (; q < r.sep_recs.size(); q++)
        {
            const SepRec &s = r.sep_recs[q];
            const size_t base = ((size_t)s.ix * r.num_var + (size_t)s.iy) * ml;
            if (base >= c1) break;
            std::memcpy(&buf[base - c0], s.s, sizeof(int) * (size_t)s.cnt);
        }
        std::fwrite(buf.data(), sizeof(int), c1 - c0, f);
        for (size_t z = q0; z < q; z++)
        {
            const SepRec &s = r.sep_recs[z];
            const size_t base = ((size_t)s.ix * r.num_var + (size_t)s.iy) * ml;
            for (int t = 0; t < s.cnt; t++) buf[base - c0 + (size_t)t] = -1;
        }
    }
    std::fclose(f);
}

inline void write_reduced(const Reduced &r, const std::string &base, bool with_sep)
{
    {
        char line[96];
        const int len = std::snprintf(line, sizeof(line), "%zu\t%zu\t%zu\n", r.num_var, r.num_phen, r.max_level);
        write_binary(base + ".mdim", line, (size_t)len);
    }
    write_binary(base + ".ixs", r.new_to_old.data(), r.new_to_old.size());
    write_binary(base + ".adj", r.G.data(), r.G.size());
    write_binary(base + ".corr", r.C.data(), r.C.size());
    if (with_sep && r.sep_sparse && r.S.empty())
        write_sep_streaming(base + ".sep", r);
    else if (with_sep)
        write_binary(base + ".sep", r.S.data(), r.S.size());
}

// parent_set.cpp:84-175 on the sparse records of the engine's last run.  Entries of a set that are not retained are dropped,
// the rest is compacted and padded with -1 to `max_level`; at most `max_level` source entries are read.  With an index_map
// (stage two) the reference keys old_to_new by index_map[P[i]] although the set members are still in the P index space
// (SURVEY App. C.3): a member that is not a key maps to 0.  The rule itself: remap_sepset of batch_plan.h.
inline std::vector<int> reduce_sepsets(cusk_engine *e, const std::vector<int> &P, size_t max_level,
                                       const std::vector<int> *index_map)
{
    const int *x = nullptr, *y = nullptr, *rs = nullptr;  // engine-owned pinned memory
    const long long cnt = cusk_result_sepsets_view(e, &x, &y, &rs);
    if (cnt < 0) engine_die("sepsets", e);
    return reduce_records(cnt, x, y, rs, cusk_result_n(e), P, max_level, index_map);
}

// reduce_sepsets without the dense array: the same cells as a list in ascending (ix, iy) order; false (and an empty list)
// when two records name the same cell (reduce_records_sparse)
inline bool reduce_sepsets_sparse(cusk_engine *e, const std::vector<int> &P, size_t max_level, const std::vector<int> *index_map,
                                  std::vector<SepRec> &out)
{
    const int *x = nullptr, *y = nullptr, *rs = nullptr;  // engine-owned pinned memory
    const long long cnt = cusk_result_sepsets_view(e, &x, &y, &rs);
    if (cnt < 0) engine_die("sepsets", e);
    return reduce_records_sparse(cnt, x, y, rs, cusk_result_n(e), P, max_level, index_map, out);
}

}  // namespace host
