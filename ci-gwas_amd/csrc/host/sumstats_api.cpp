// sumstats_api.cpp -- the three summary-statistic files `mps cuskss` reads, written from arrays (cusk_sumstats_write of
// include/cusk_hip.h).  Host only: the formats are those of host_io.h's loaders (load_mxm_into, load_mxp, load_pxp;
// /root/reference/cusk/src/marker_summary_stats.cpp:8-24, marker_trait_summary_stats.cpp:40-299,
// trait_summary_stats.cpp:5-169).  Floats go out with nine significant digits, which a parser that rounds to float32
// reads back exactly.  Every write and close is checked: a full disk must not leave a truncated mxp behind a zero status.
//
// cusk_sumstats_write_se adds the two standard-error files from per-pair observation counts (cusk_pair_counts).  The
// loaders turn a standard error back into a sample size with ess = ((1 - r^2) / se)^2 (host::ess_from_se), and the sweep
// truncates every sample size to int before it averages them (mean_ess of the reference), so cusk_se_from_count picks the
// float se from which that chain gives back the count itself, not count - 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../include/cusk_hip.h"
#include "host_io.h"

namespace {

// buffered text file whose every operation is checked; the first failure is kept and reported by close()
struct CheckedFile
{
    std::string path;
    FILE *f = nullptr;
    bool ok = true;
    explicit CheckedFile(const std::string &p, const char *mode) : path(p), f(std::fopen(p.c_str(), mode)) { ok = f != nullptr; }
    void write(const void *data, size_t bytes)
    {
        if (ok && bytes && std::fwrite(data, 1, bytes, f) != bytes) ok = false;
    }
    void close()
    {
        if (f && std::fclose(f) != 0) ok = false;
        f = nullptr;
        if (!ok) host::die("cannot write " + path);
    }
    ~CheckedFile()
    {
        if (f) std::fclose(f);  // only on the way out of a failure that is already being reported
    }
};

// %.9g, or `nan_token` for a NaN (whatever its sign or payload: printf would write "-nan" for some)
inline void append_value(std::string &line, float v, const char *nan_token)
{
    if (std::isnan(v))
    {
        line += nan_token;
        return;
    }
    char buf[32];
    const int len = std::snprintf(buf, sizeof(buf), "%.9g", (double)v);
    line.append(buf, (size_t)len);
}

void write_mxm(const std::string &path, const float *tri, size_t k)
{
    CheckedFile out(path, "wb");
    const size_t total = k * (k + 1) / 2, piece = (size_t)1 << 20;
    std::vector<float> buf;
    for (size_t t0 = 0; t0 < total && out.ok; t0 += piece)
    {
        const size_t cnt = std::min(piece, total - t0);
        const float *src = tri + t0;
        bool has_nan = false;
        for (size_t t = 0; t < cnt; t++) has_nan = has_nan || std::isnan(src[t]);
        if (has_nan)
        {  // the file never holds a NaN (the loaders would turn it into 0 anyway)
            buf.assign(src, src + cnt);
            for (float &v : buf)
                if (std::isnan(v)) v = 0.0f;
            src = buf.data();
        }
        out.write(src, sizeof(float) * cnt);
    }
    out.close();
}

void write_mxp(const std::string &path, const float *mxp, size_t m_total, size_t p, const char *const *chr, const char *const *snp,
               const char *const *ref, const char *const *trait_names)
{
    CheckedFile out(path, "w");
    std::string line = "chr snp ref";
    for (size_t t = 0; t < p; t++) line += std::string(" ") + trait_names[t];
    line += "\n";
    for (size_t i = 0; i < m_total && out.ok; i++)
    {
        line += chr[i];
        line += ' ';
        line += snp[i];
        line += ' ';
        line += ref[i];
        for (size_t t = 0; t < p; t++)
        {
            line += ' ';
            append_value(line, mxp[i * p + t], "NA");
        }
        line += '\n';
        if (line.size() >= ((size_t)1 << 20))
        {
            out.write(line.data(), line.size());
            line.clear();
        }
    }
    out.write(line.data(), line.size());
    out.close();
}

void write_pxp(const std::string &path, const float *pxp, size_t p, const char *const *trait_names)
{
    CheckedFile out(path, "w");
    std::string text;
    for (size_t t = 0; t < p; t++) text += std::string(t ? " " : "") + trait_names[t];
    text += "\n";
    for (size_t a = 0; a < p; a++)
    {
        text += trait_names[a];
        for (size_t b = 0; b < p; b++)
        {
            text += ' ';
            append_value(text, pxp[a * p + b], "nan");
        }
        text += '\n';
    }
    out.write(text.data(), text.size());
    out.close();
}

// (int)ess == count without converting an out-of-range float
inline bool recovers(float r, float se, int count)
{
    const double e = (double)host::ess_from_se(r, se);
    return e >= (double)count && e < (double)count + 1.0;
}

}  // namespace

extern "C" float cusk_ess_from_se(float r, float se) { return host::ess_from_se(r, se); }

// se = (1 - r^2) / sqrt(count) in the loaders' float/double mix, moved by one ulp towards the side that makes
// (int)cusk_ess_from_se(r, se) == count when the plain value gives count - 1 or count + 1 (it does for about three pairs
// in ten).  One ulp is enough for every count up to two million; beyond that the spacing of float32 near `count` exceeds
// what one ulp of se can correct for some pairs, and where neither neighbour works the plain value is returned.
extern "C" float cusk_se_from_count(float r, int count)
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (std::isnan(r) || count <= 0 || !(r * r < 1.0f)) return nan;
    const float se = (float)((1.0 - (double)(r * r)) / std::sqrt((double)count));
    if (recovers(r, se, count)) return se;
    const float inf = std::numeric_limits<float>::infinity();
    for (const float cand : {std::nextafterf(se, 0.0f), std::nextafterf(se, inf)})
        if (cand > 0.0f && recovers(r, cand, count)) return cand;
    return se;
}

extern "C" int cusk_sumstats_write_se(const char *outdir, const float *mxp, const int *mxp_n, size_t m_total, size_t p,
                                      const float *pxp_square, const int *pxp_n, const char *const *chr, const char *const *snp,
                                      const char *const *ref, const char *const *trait_names, char *err, size_t err_len)
{
    auto report = [&](const std::string &msg, int code) {
        if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
        return code;
    };
    if (!outdir || !mxp || !mxp_n || !pxp_square || !pxp_n || !chr || !snp || !ref || !trait_names || m_total == 0 || p == 0)
        return report("cusk_sumstats_write_se: bad arguments", CUSK_ERR_ARG);
    try
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> se(m_total * p);
        for (size_t i = 0; i < m_total * p; i++) se[i] = std::isnan(mxp[i]) ? nan : cusk_se_from_count(mxp[i], mxp_n[i]);
        write_mxp(host::make_path(outdir, "mxp_se", ".txt"), se.data(), m_total, p, chr, snp, ref, trait_names);
        se.assign(p * p, nan);  // the diagonal stays NaN: see cusk_hip.h
        for (size_t a = 0; a < p; a++)
            for (size_t b = 0; b < p; b++)
                if (a != b && !std::isnan(pxp_square[a * p + b])) se[a * p + b] = cusk_se_from_count(pxp_square[a * p + b], pxp_n[a * p + b]);
        write_pxp(host::make_path(outdir, "pxp_se", ".txt"), se.data(), p, trait_names);
    }
    catch (const std::exception &ex)
    {
        return report(ex.what(), CUSK_ERR_ARG);
    }
    return CUSK_OK;
}

// the two standard-error files from finished arrays (polychoric / polyserial standard errors do not come from a count)
extern "C" int cusk_sumstats_write_se_values(const char *outdir, const float *mxp_se, size_t m_total, size_t p, const float *pxp_se,
                                             const char *const *chr, const char *const *snp, const char *const *ref,
                                             const char *const *trait_names, char *err, size_t err_len)
{
    auto report = [&](const std::string &msg, int code) {
        if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
        return code;
    };
    if (!outdir || !mxp_se || !pxp_se || !chr || !snp || !ref || !trait_names || m_total == 0 || p == 0)
        return report("cusk_sumstats_write_se_values: bad arguments", CUSK_ERR_ARG);
    try
    {
        write_mxp(host::make_path(outdir, "mxp_se", ".txt"), mxp_se, m_total, p, chr, snp, ref, trait_names);
        write_pxp(host::make_path(outdir, "pxp_se", ".txt"), pxp_se, p, trait_names);
    }
    catch (const std::exception &ex)
    {
        return report(ex.what(), CUSK_ERR_ARG);
    }
    return CUSK_OK;
}

extern "C" int cusk_sumstats_write(const char *outdir, const float *mxm_tri, size_t k, const float *mxp, size_t m_total, size_t p,
                                   const float *pxp_square, const char *const *chr, const char *const *snp, const char *const *ref,
                                   const char *const *trait_names, char *err, size_t err_len)
{
    auto report = [&](const std::string &msg, int code) {
        if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
        return code;
    };
    if (!outdir || !mxm_tri || !mxp || !pxp_square || !chr || !snp || !ref || !trait_names || k == 0 || m_total == 0 || p == 0)
        return report("cusk_sumstats_write: bad arguments", CUSK_ERR_ARG);
    try
    {
        write_mxm(host::make_path(outdir, "mxm", ".bin"), mxm_tri, k);
        write_mxp(host::make_path(outdir, "mxp", ".txt"), mxp, m_total, p, chr, snp, ref, trait_names);
        write_pxp(host::make_path(outdir, "pxp", ".txt"), pxp_square, p, trait_names);
    }
    catch (const std::exception &ex)
    {
        return report(ex.what(), CUSK_ERR_ARG);
    }
    return CUSK_OK;
}
