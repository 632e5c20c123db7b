// mvivw_ld_plan.h -- host side of cusk_mvivw_ld (csrc/mvivw_ld.hip): argument checks, the workspace bound and the panel
// schedule of the blocked Cholesky factorisation.  Plain C++, no HIP: the stand-alone program
// tools/mvivw_ld_plan_selftest.cpp walks it with a stand-in for the kernels under the host sanitizers.
//
// One outcome at a time.  Its m x m matrix R stands row-major (leading dimension m) in the engine's workspace, lower
// triangle and diagonal only; the k + 1 right-hand sides stand below it as K = k + 1 more ROWS of length m (the table Zt,
// row c = column c of diag(1/s) (X, y)), so that the rows of the problem are 0 .. m + K - 1 and the columns 0 .. m - 1.
// Factoring the m columns of that (m + K) x m lower trapezoid leaves C in the first m rows and (C^-1 diag(1/s) (X, y))'
// in the last K: the forward substitution of the whitening is the panel solve and the trailing update of those rows.
//
// Panel j covers columns [j0, j0 + nb), nb = kLdPanel except for the last one.
//   factor   one workgroup: the nb x nb diagonal block, the pivot test, the block's inverse
//   solve    the rows [j0 + nb, m + K) in row tiles of kLdSolveRows: row block times the transposed inverse
//   update   the tiles of kLdTile x kLdTile of rows >= c0 and columns [c0, m), c0 = j0 + nb; grid (TC, TR), tile (tj, ti)
//            is updated when ld_tile_active(ti, tj): the lower triangle of R and every tile of the K extra rows
#pragma once

#include "mvivw_plan.h"

#include <cmath>

namespace cusk {

constexpr int kLdPanel = 64;      // panel width = depth of one trailing update
constexpr int kLdTile = 64;       // a workgroup of the trailing update owns a kLdTile x kLdTile tile
constexpr int kLdSolveRows = 32;  // rows per workgroup of the panel solve
constexpr long long kLdBytes = 8ll << 30;  // default of engine option "mvivw_ld_bytes"
static_assert(kLdPanel == kLdTile, "a trailing tile starts where a panel ends");

// the tile at tile row ti, tile column tj (both counted from c0) holds an element on or below the diagonal, or a row of Zt
constexpr bool ld_tile_active(int ti, int tj) { return ti >= tj; }

struct LdPanel
{
    int j0, nb;
    int solve_blocks;  // workgroups of the panel solve (0: nothing below)
    int tc, tr;        // grid of the trailing update (tc = 0: no trailing columns)
};

struct LdPlan
{
    std::vector<int> status;          // per caller's outcome: 1 where nothing is computed, else 0
    // the active ones, in the caller's order.  One workspace serves them one after another, so every outcome's chunk
    // partials and residual partials start at 0: part0 = 0, chunk0 = 0; nchunks counts rows of the whitened table
    std::vector<MvOutcome> outcomes;
    int max_m = 0, max_chunks = 0;
    size_t ws_doubles = 0;  // max m * m
    size_t zt_doubles = 0;  // max (k + 1) * m
};

inline std::vector<LdPanel> ld_panels(int m, int K)
{
    std::vector<LdPanel> out;
    const long long rows = (long long)m + K;
    for (int j0 = 0; j0 < m; j0 += kLdPanel)
    {
        LdPanel pn;
        pn.j0 = j0;
        pn.nb = std::min(kLdPanel, m - j0);
        const int c0 = j0 + pn.nb;
        pn.solve_blocks = (int)((rows - c0 + kLdSolveRows - 1) / kLdSolveRows);
        pn.tc = (m - c0 + kLdTile - 1) / kLdTile;
        pn.tr = (int)((rows - c0 + kLdTile - 1) / kLdTile);
        out.push_back(pn);
    }
    return out;
}

// 0, or 1 with `msg` set.  The checks of cusk_mvivw first (mvivw_plan_build), then ridge and the workspace bound.
inline int mvivw_ld_plan_build(long long M, int p, int nout, const int *outcome, const long long *iv_off, const int *iv,
                               const int *ex_off, const int *ex, int model, double ridge, long long ws_bytes, LdPlan &plan,
                               std::string &msg)
{
    plan = LdPlan();
    MvPlan base;
    if (mvivw_plan_build(M, p, nout, outcome, iv_off, iv, ex_off, ex, model, kMvPartBound, base, msg)) return 1;
    if (!(ridge >= 0.0 && ridge < 1.0))
    {
        msg = "ridge is not in [0, 1)";
        return 1;
    }
    if (M > INT_MAX)
    {
        msg = "more than 2^31 - 1 marker rows";
        return 1;
    }
    plan.status = base.status;
    for (const MvOutcome &q : base.outcomes)
    {
        const unsigned long long need = (unsigned long long)q.m * (unsigned long long)q.m * sizeof(double);
        if (ws_bytes <= 0 || need > (unsigned long long)ws_bytes)
        {
            msg = "outcome " + std::to_string(q.out) + ": the " + std::to_string(q.m) + " x " + std::to_string(q.m) +
                  " LD matrix needs " + std::to_string(need) + " bytes, more than mvivw_ld_bytes = " + std::to_string(ws_bytes);
            return 1;
        }
        plan.outcomes.push_back(q);
        plan.outcomes.back().part0 = 0;
        plan.outcomes.back().chunk0 = 0;
        plan.max_m = std::max(plan.max_m, q.m);
        plan.max_chunks = std::max(plan.max_chunks, q.nchunks);
        plan.ws_doubles = std::max(plan.ws_doubles, (size_t)q.m * (size_t)q.m);
        plan.zt_doubles = std::max(plan.zt_doubles, (size_t)(q.k + 1) * (size_t)q.m);
    }
    return 0;
}

}  // namespace cusk
