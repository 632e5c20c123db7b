// cuskss_run.h -- what `mps cuskss` and `mps cuskss-bed` share: the graph-and-correlations bundle of one stage, the stage
// itself (cli.cpp:29-60), its files, and the time index of the traits.
#pragma once
#include <memory>

#include "reduce.h"

namespace host {

struct GC
{
    size_t num_var = 0, num_phen = 0;
    std::vector<int> new_to_old;
    std::vector<int> G;      // empty = complete graph
    std::vector<float> C;    // num_var^2
    std::vector<float> ess;  // num_var^2 when heterogeneous, else empty
    size_t num_markers() const { return num_var - num_phen; }
};

// run_cusk, cli.cpp:29-60: hetcor_skeleton, prune to depth, extract the retained sub-matrices.  C_resident: the
// num_var^2 matrix where a correlation build left it in HBM (gc.C is empty then); otherwise gc.C is uploaded.
inline GC run_cusk(cusk_engine *e, const GC &gc, float th, float ess_uniform, bool het, int depth, int max_level,
                   const std::vector<int> &time_index_traits, const float *C_resident = nullptr)
{
    const int n = (int)gc.num_var;
    std::vector<int> ti(n, 0);
    for (size_t i = gc.num_markers(), r = 0; i < gc.num_var; i++, r++) ti[i] = time_index_traits[r];
    std::unique_ptr<DevMat> uploaded;
    if (!C_resident) uploaded.reset(new DevMat(gc.C));
    const float *Cd = C_resident ? C_resident : uploaded->p;
    std::unique_ptr<DevMat> Nd;
    if (het) Nd.reset(new DevMat(gc.ess));
    int *Gd = nullptr;
    if (!gc.G.empty())
    {
        Gd = static_cast<int *>(cusk_dev_alloc(sizeof(int) * gc.G.size()));
        if (!Gd || cusk_dev_upload(Gd, gc.G.data(), sizeof(int) * gc.G.size()) != CUSK_OK) engine_die("upload G", e);
    }
    cusk_stats st;
    if (cusk_run_hetcor(e, Cd, het ? Nd->p : nullptr, ess_uniform, Gd, n, th, max_level, ti.data(), &st) != CUSK_OK)
        engine_die("hetcor_skeleton", e);
    cusk_dev_free(Gd);
    Bits G = fetch_adjacency(e);
    std::vector<int> P = subset_variables(G, n, (int)gc.num_markers(), depth);
    GC out;
    out.num_var = P.size();
    out.num_phen = gc.num_phen;
    out.new_to_old = compose(P, &gc.new_to_old);
    out.G = gather_adj(G, P);
    out.C = gather(e, Cd, n, P);
    if (het) out.ess = gather(e, Nd->p, n, P);
    return out;
}

inline void write_gc(const GC &gc, const std::string &base)
{
    Reduced r;
    r.num_var = gc.num_var;
    r.num_phen = gc.num_phen;
    r.max_level = ML;  // cli.cpp:58 passes ML
    r.new_to_old = gc.new_to_old;
    r.G = gc.G;
    r.C = gc.C;
    write_reduced(r, base, false);
    // heterogeneous runs: the sample sizes of the retained variables beside .corr, same order (float32, num_var^2), for
    // sepselect --het
    if (!gc.ess.empty()) write_binary(base + ".ess", gc.ess.data(), gc.ess.size());
}

// one time index per trait: 1 for all of them without a file ("NULL")
inline std::vector<int> load_time_index(const std::string &path, size_t p)
{
    std::vector<int> time_index_traits(p, 1);
    if (path != "NULL")
    {
        std::cout << "Loading time_indices" << std::endl;
        time_index_traits = read_ints_lines(path);
        if (time_index_traits.size() < p) die("time index file has fewer lines than traits");
    }
    return time_index_traits;
}

}  // namespace host
