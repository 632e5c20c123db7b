// result_types.h -- the plain types a skeleton run's results come back in, for the code that talks to the engine
// (engine_util.h, reduce.h) and for the host-only planning code (batch_plan.h) alike.  Only constants of the C ABI are used.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../../include/cusk_hip.h"

namespace host {

constexpr int ML = CUSK_ML;

// adjacency rows as 64-bit words: n rows of `words` words
struct Bits
{
    int n = 0, words = 0;
    std::vector<uint64_t> w;
    bool get(int i, int j) const { return (w[(size_t)i * words + (j >> 6)] >> (j & 63)) & 1ull; }
};

// One separating set of the reduced result: the cell (ix, iy) of the num_var x num_var x max_level array holds s[0 .. cnt)
// followed by -1
struct SepRec
{
    int ix, iy, cnt;
    int s[ML];
};

}  // namespace host
