// ordinal_estimates.h -- the engine side of `ordinal=` (mps sumstats / mps cuskss-bed): the contingency tables and the
// polychoric / polyserial fits on the device, rounded once to the float32 the files hold.  Where the estimates go is
// square_inputs.h's business.
#pragma once
#include "geno_inputs.h"
#include "ordinal_host.h"

namespace host {

inline OrdinalSpec load_ordinal_spec(const std::string &arg, const GenoInputs &in)
{
    try
    {
        return ordinal_levels(parse_ordinal_arg(arg, in.p()), in.phen.data.data(), in.N(), in.trait_names);
    }
    catch (const std::exception &ex)
    {
        die(ex.what());
    }
    return OrdinalSpec();
}

inline OrdinalTraitEstimates ordinal_trait_estimates(cusk_engine *e, const GenoInputs &in, const OrdinalSpec &spec)
{
    const size_t p = in.p(), q = spec.q();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    OrdinalTraitEstimates out;
    out.r.assign(p * q, nan);
    out.se.assign(p * q, nan);
    std::vector<int> oxo(q * q * 64);
    if (cusk_ordinal_tables(e, nullptr, in.dev.phen, nullptr, 0, 0, in.N(), p, spec.ix.data(), q, spec.levels.data(), spec.nlev.data(),
                            nullptr, oxo.data()) != CUSK_OK)
        engine_die("ordinal trait tables", e);
    std::vector<double> r(q * q), se(q * q);
    std::vector<int> status(q * q);
    if (cusk_polychoric_fit(e, oxo.data(), q * q, 8, 8, r.data(), se.data(), status.data()) != CUSK_OK)
        engine_die("polychoric fit (traits)", e);
    for (size_t a = 0; a < q; a++)
        for (size_t b = a + 1; b < q; b++)
        {  // one fit per pair, mirrored: the two orientations of a table need not agree to the last bit
            out.r[(size_t)spec.ix[a] * q + b] = out.r[(size_t)spec.ix[b] * q + a] = (float)r[a * q + b];
            out.se[(size_t)spec.ix[a] * q + b] = out.se[(size_t)spec.ix[b] * q + a] = (float)se[a * q + b];
        }
    std::vector<int> cont;
    for (size_t t = 0; t < p; t++)
        if (std::find(spec.ix.begin(), spec.ix.end(), (int)t) == spec.ix.end()) cont.push_back((int)t);
    if (!cont.empty())
    {
        const size_t nc = cont.size();
        r.resize(nc * q), se.resize(nc * q), status.resize(nc * q);
        if (cusk_polyserial_fit(e, in.dev.phen, in.N(), p, cont.data(), nc, spec.ix.data(), q, spec.levels.data(), spec.nlev.data(),
                                r.data(), se.data(), status.data()) != CUSK_OK)
            engine_die("polyserial fit", e);
        for (size_t c = 0; c < nc; c++)
            for (size_t t = 0; t < q; t++)
            {
                out.r[(size_t)cont[c] * q + t] = (float)r[c * q + t];
                out.se[(size_t)cont[c] * q + t] = (float)se[c * q + t];
            }
    }
    return out;
}

// r and se (rows x q, float32) of the markers `marker_ix` (NULL: rows 0 .. rows-1 of bed) with every ordinal trait
inline void ordinal_marker_estimates(cusk_engine *e, const GenoInputs &in, const OrdinalSpec &spec, const unsigned char *bed,
                                     const int *marker_ix, size_t rows, size_t m_total, float *r_out, float *se_out)
{
    const size_t q = spec.q();
    std::vector<int> tab(rows * q * 24);
    if (cusk_ordinal_tables(e, bed, in.dev.phen, marker_ix, rows, m_total, in.N(), in.p(), spec.ix.data(), q, spec.levels.data(),
                            spec.nlev.data(), tab.data(), nullptr) != CUSK_OK)
        engine_die("ordinal marker tables", e);
    std::vector<double> r(rows * q), se(rows * q);
    std::vector<int> status(rows * q);
    if (cusk_polychoric_fit(e, tab.data(), rows * q, 3, 8, r.data(), se.data(), status.data()) != CUSK_OK)
        engine_die("polychoric fit (markers)", e);
    for (size_t i = 0; i < rows * q; i++)
    {
        r_out[i] = (float)r[i];
        se_out[i] = (float)se[i];
    }
}

}  // namespace host
