// ordinal_host.h -- host side of `ordinal=<1-based,...>` (mps sumstats / mps cuskss-bed): the list of ordinal traits and
// their levels.  Header only and free of the engine, so that tools/ordinal_selftest.cpp can run it under sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace host {

constexpr int kOrdinalLevels = 8;

struct OrdinalSpec
{
    std::vector<int> ix;        // 0-based trait indices, in the order given
    std::vector<float> levels;  // ix.size() x 8, ascending, unused ones 0
    std::vector<int> nlev;
    size_t q() const { return ix.size(); }
};

// Polychoric / polyserial estimates of every pair of a trait with an ordinal trait, as float32 the files hold: r and se
// are formed in double on the device and rounded once (ordinal_estimates.h).
struct OrdinalTraitEstimates
{
    std::vector<float> r, se;  // p x q: trait a with ordinal trait spec.ix[t]; its own entry is not set
};

// "ordinal=2,5" -> {1, 4}; every error is a std::runtime_error with a message for the user
inline std::vector<int> parse_ordinal_arg(const std::string &arg, size_t num_phen)
{
    const std::string key = "ordinal=";
    if (arg.compare(0, key.size(), key) != 0) throw std::runtime_error("expected ordinal=<trait numbers>, got " + arg);
    std::vector<int> out;
    size_t pos = key.size();
    if (pos >= arg.size()) throw std::runtime_error("ordinal=: no trait numbers given");
    while (pos <= arg.size())
    {
        size_t end = arg.find(',', pos);
        if (end == std::string::npos) end = arg.size();
        const std::string tok = arg.substr(pos, end - pos);
        if (tok.empty() || tok.size() > 9 || !std::all_of(tok.begin(), tok.end(), [](char c) { return c >= '0' && c <= '9'; }))
            throw std::runtime_error("ordinal=: '" + tok + "' is not a trait number");
        const long v = std::stol(tok);
        if (v < 1 || (size_t)v > num_phen)
            throw std::runtime_error("ordinal=: trait number " + tok + " is out of range (1 .. " + std::to_string(num_phen) + ")");
        if (std::find(out.begin(), out.end(), (int)v - 1) != out.end()) throw std::runtime_error("ordinal=: trait number " + tok + " is given twice");
        out.push_back((int)v - 1);
        pos = end + 1;
    }
    return out;
}

// the sorted distinct non-NaN values of each listed trait; phen: num_phen x N, trait-major
inline OrdinalSpec ordinal_levels(const std::vector<int> &ix, const float *phen, size_t N, const std::vector<std::string> &names)
{
    OrdinalSpec s;
    s.ix = ix;
    s.levels.assign(ix.size() * kOrdinalLevels, 0.0f);
    s.nlev.assign(ix.size(), 0);
    for (size_t t = 0; t < ix.size(); t++)
    {
        std::vector<float> seen;
        const float *col = phen + (size_t)ix[t] * N;
        for (size_t i = 0; i < N; i++)
        {
            const float v = col[i];
            if (std::isnan(v)) continue;
            const auto it = std::lower_bound(seen.begin(), seen.end(), v);
            if (it != seen.end() && *it == v) continue;
            seen.insert(it, v);
            if (seen.size() > 4096) break;  // a continuous trait: no need to sort all of it to say so
        }
        const std::string name = (size_t)ix[t] < names.size() ? names[ix[t]] : std::to_string(ix[t] + 1);
        if (seen.size() > (size_t)kOrdinalLevels)
            throw std::runtime_error("ordinal trait " + name + " has " + (seen.size() > 4096 ? std::string("more than 4096") : std::to_string(seen.size())) +
                                     " distinct values; at most 8 levels are supported");
        if (seen.size() < 2) throw std::runtime_error("ordinal trait " + name + " has " + std::to_string(seen.size()) + " distinct values; at least 2 levels are needed");
        std::copy(seen.begin(), seen.end(), s.levels.begin() + t * kOrdinalLevels);
        s.nlev[t] = (int)seen.size();
    }
    return s;
}

}  // namespace host
