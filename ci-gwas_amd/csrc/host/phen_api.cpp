// phen_api.cpp -- the table reader, the alignment to a .fam and the .phen writer of `mps prep-phen` behind the C ABI
// (cusk_phen_table_*, cusk_phen_write of include/cusk_hip.h).  Host only: no call here touches a device.
#include <cstring>
#include <filesystem>
#include <memory>

#include "../../../include/cusk_hip.h"
#include "phen_table.h"

struct cusk_phen_table
{
    host::AlignedPhen a;
};

namespace {

int report(char *err, size_t err_len, const std::string &msg, int code)
{
    if (err && err_len)
    {
        std::strncpy(err, msg.c_str(), err_len - 1);
        err[err_len - 1] = '\0';
    }
    return code;
}

}  // namespace

extern "C" int cusk_phen_table_load(cusk_phen_table **out, const char *table_path, const char *fam_path, char *err, size_t err_len)
{
    if (out) *out = nullptr;
    if (!out || !table_path) return report(err, err_len, "cusk_phen_table_load: bad arguments", CUSK_ERR_ARG);
    try
    {
        const host::PhenTable t = host::read_phen_table(table_path);
        std::unique_ptr<cusk_phen_table> h(new cusk_phen_table);
        if (fam_path)
        {
            const host::FamIds fam = host::read_fam_ids(fam_path);
            h->a = host::align_phen_table(t, &fam);
        }
        else
            h->a = host::align_phen_table(t, nullptr);
        *out = h.release();
    }
    catch (const host::Fatal &f)
    {
        return report(err, err_len, f.what(), CUSK_ERR_ARG);
    }
    return CUSK_OK;
}

extern "C" size_t cusk_phen_table_rows(const cusk_phen_table *t) { return t ? t->a.N : 0; }
extern "C" size_t cusk_phen_table_cols(const cusk_phen_table *t) { return t ? t->a.p() : 0; }
extern "C" const char *cusk_phen_table_name(const cusk_phen_table *t, size_t col)
{
    return t && col < t->a.p() ? t->a.names[col].c_str() : nullptr;
}
extern "C" const float *cusk_phen_table_data(const cusk_phen_table *t) { return t ? t->a.data.data() : nullptr; }
extern "C" size_t cusk_phen_table_matched(const cusk_phen_table *t) { return t ? t->a.matched : 0; }
extern "C" size_t cusk_phen_table_dropped(const cusk_phen_table *t) { return t ? t->a.dropped : 0; }
extern "C" int cusk_phen_table_in_order(const cusk_phen_table *t) { return t && t->a.in_order ? 1 : 0; }
extern "C" void cusk_phen_table_free(cusk_phen_table *t) { delete t; }

extern "C" int cusk_phen_write(const char *path, const char *fam_path, const char *const *names, size_t p, const float *data, size_t N,
                               char *err, size_t err_len)
{
    if (!path || !fam_path || !names || !data || p == 0) return report(err, err_len, "cusk_phen_write: bad arguments", CUSK_ERR_ARG);
    std::error_code ec;
    if (std::string(path) == fam_path || (std::filesystem::equivalent(path, fam_path, ec) && !ec))
        return report(err, err_len, std::string("cusk_phen_write: ") + path + " is the .fam", CUSK_ERR_ARG);
    host::FamIds fam;
    try
    {
        fam = host::read_fam_ids(fam_path);
    }
    catch (const host::Fatal &f)
    {
        return report(err, err_len, f.what(), CUSK_ERR_ARG);
    }
    if (fam.n() != N)
        return report(err, err_len, std::string(fam_path) + " has " + std::to_string(fam.n()) + " individuals, not " + std::to_string(N), CUSK_ERR_ARG);
    std::vector<std::string> nm(p);
    for (size_t j = 0; j < p; j++)
    {
        if (!names[j]) return report(err, err_len, "cusk_phen_write: bad arguments", CUSK_ERR_ARG);
        nm[j] = names[j];
    }
    try
    {
        host::write_phen_file(path, fam, nm, data);
    }
    catch (const host::Fatal &f)
    {
        return report(err, err_len, f.what(), CUSK_ERR_STATE);
    }
    return CUSK_OK;
}
