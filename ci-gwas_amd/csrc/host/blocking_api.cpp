// blocking_api.cpp -- cusk_block_chr / cusk_hanning_weights of include/cusk_hip.h: "row sums to blocks" for one
// chromosome, the code path of `mps block` (host/blocking.h with the smoothing on the device), behind the C ABI so
// that the host program and the tests run the same thing.  Plain host C++ on top of the engine ABI.
#include <vector>

#include "../../../include/cusk_hip.h"
#include "blocking.h"

namespace {
struct SmoothFailed
{
    int rc;
};
}  // namespace

extern "C" int cusk_hanning_weights(int window, double *out)
{
    if (window <= 0 || !out) return CUSK_ERR_ARG;
    const std::vector<double> w = host::hanning_weights(window);
    for (int i = 0; i < window; i++) out[i] = w[(size_t)i];
    return CUSK_OK;
}

extern "C" int cusk_block_chr(cusk_engine *e, const float *row_sums, size_t n, int max_block_size, long long *first,
                              long long *last, size_t cap, size_t *count)
{
    if (count) *count = 0;
    // n = 0 has no blocks (the reference forms size() - 1 of an empty profile); the smoothing takes n as an int-sized window bound
    if (!e || !row_sums || !count || n == 0 || n > (size_t)0x7fffffff || (cap > 0 && (!first || !last))) return CUSK_ERR_ARG;
    std::vector<host::ChrBlock> blocks;
    try
    {
        const std::vector<float> v(row_sums, row_sums + n);
        blocks = host::blocks_of_chromosome(v, max_block_size, [&](const std::vector<float> &p, const std::vector<double> &w) {
            std::vector<double> out(p.size());
            const int rc = cusk_hanning_smooth(e, p.data(), p.size(), w.data(), (int)w.size(), out.data());
            if (rc != CUSK_OK) throw SmoothFailed{rc};  // message in cusk_last_error(e)
            return out;
        });
    }
    catch (const SmoothFailed &f)
    {
        return f.rc;
    }
    *count = blocks.size();
    if (blocks.size() > cap) return CUSK_ERR_ARG;
    for (size_t k = 0; k < blocks.size(); k++)
    {
        first[k] = (long long)blocks[k].first;
        last[k] = (long long)blocks[k].last;
    }
    return CUSK_OK;
}
