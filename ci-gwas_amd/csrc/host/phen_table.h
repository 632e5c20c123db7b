// phen_table.h -- trait and covariate tables of `mps prep-phen` / `mps check-phen`: the reader, the alignment to a .fam by
// IID and the .phen writer (cusk_phen_table_* and cusk_phen_write of include/cusk_hip.h state the formats).  The
// reference's loader (phen.cpp:9-74, load_phen of host_io.h) takes rows as they come; its cusk/scripts/phen_prep.py
// reindexes by IID, and so does this.  Pure host code: tools/phen_table_selftest.cpp runs it under the sanitizers.
#pragma once
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_io.h"

namespace host {

struct PhenTable
{
    std::vector<std::string> names;     // value columns
    std::vector<std::string> fid, iid;  // per row
    std::vector<float> rows;            // row-major, iid.size() x names.size()
    size_t n() const { return iid.size(); }
    size_t p() const { return names.size(); }
};

// the words of a line; '\r' is white space, so CRLF files read like any other
inline void split_words(const std::string &line, std::vector<std::string> &out)
{
    out.clear();
    size_t i = 0;
    const size_t n = line.size();
    while (i < n)
    {
        while (i < n && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r' || line[i] == '\n' || line[i] == '\v' || line[i] == '\f')) i++;
        size_t j = i;
        while (j < n && !(line[j] == ' ' || line[j] == '\t' || line[j] == '\r' || line[j] == '\n' || line[j] == '\v' || line[j] == '\f')) j++;
        if (j > i) out.emplace_back(line, i, j - i);
        i = j;
    }
}

// the value load_phen gives the token ((float)atof), with the NA tokens of is_na_token; anything else that is not a number
// in full is refused
inline bool parse_value(const std::string &tok, float &v)
{
    if (is_na_token(tok, true))
    {
        v = std::numeric_limits<float>::quiet_NaN();
        return true;
    }
    char *end = nullptr;
    const double d = std::strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end != '\0') return false;
    v = (float)d;
    return true;
}

inline PhenTable read_phen_table(const std::string &path)
{
    std::ifstream f(path);
    if (!f) die("cannot read " + path);
    PhenTable t;
    std::string line;
    std::vector<std::string> w;
    if (!std::getline(f, line)) die(path + " is empty");
    split_words(line, w);
    int fid_col = -1, iid_col = -1;
    for (int q = 0; q < 2 && q < (int)w.size(); q++)
    {
        if (w[q] == "FID") fid_col = q;
        if (w[q] == "IID" || w[q] == "EID") iid_col = q;
    }
    if (w.size() < 2 || fid_col < 0 || iid_col < 0)
        die(path + ": line 1: the header must start with the id columns FID and IID (or EID), in either order");
    t.names.assign(w.begin() + 2, w.end());
    const size_t p = t.names.size();
    std::unordered_map<std::string, size_t> seen;
    size_t ln = 1;
    while (std::getline(f, line))
    {
        ++ln;
        split_words(line, w);
        if (w.empty()) continue;  // blank line
        if (w.size() != p + 2)
            die(path + ": line " + std::to_string(ln) + ": " + std::to_string(w.size()) + " columns, the header has " + std::to_string(p + 2));
        if (!seen.emplace(w[iid_col], ln).second)
            die(path + ": line " + std::to_string(ln) + ": duplicate IID " + w[iid_col] + " (first on line " + std::to_string(seen[w[iid_col]]) + ")");
        t.fid.push_back(w[fid_col]);
        t.iid.push_back(w[iid_col]);
        for (size_t j = 0; j < p; j++)
        {
            float v;
            if (!parse_value(w[j + 2], v))
                die(path + ": line " + std::to_string(ln) + ", column " + std::to_string(j + 3) + " (" + t.names[j] + "): '" + w[j + 2] +
                    "' is neither a number nor NA");
            t.rows.push_back(v);
        }
    }
    return t;
}

struct FamIds
{
    std::vector<std::string> fid, iid;
    size_t n() const { return iid.size(); }
};

// .fam: FID IID father mother sex phenotype; only the first two columns are read
inline FamIds read_fam_ids(const std::string &path)
{
    std::ifstream f(path);
    if (!f) die("cannot read " + path);
    FamIds fam;
    std::string line;
    std::vector<std::string> w;
    std::unordered_map<std::string, size_t> seen;
    size_t ln = 0;
    while (std::getline(f, line))
    {
        ++ln;
        split_words(line, w);
        if (w.empty()) continue;
        if (w.size() < 2) die(path + ": line " + std::to_string(ln) + ": fewer than two columns");
        if (!seen.emplace(w[1], ln).second) die(path + ": line " + std::to_string(ln) + ": duplicate IID " + w[1]);
        fam.fid.push_back(w[0]);
        fam.iid.push_back(w[1]);
    }
    return fam;
}

struct AlignedPhen
{
    std::vector<std::string> names;
    std::vector<float> data;  // names.size() x N, column-major (trait-major)
    size_t N = 0, matched = 0, dropped = 0;
    bool in_order = false;  // as many rows as the .fam, the same IID line by line
    size_t p() const { return names.size(); }
};

// one row per individual of the .fam, in its order; without a .fam (fam == nullptr) the rows as they come
inline AlignedPhen align_phen_table(const PhenTable &t, const FamIds *fam)
{
    AlignedPhen a;
    a.names = t.names;
    const size_t p = t.p();
    a.N = fam ? fam->n() : t.n();
    a.data.assign(p * a.N, std::numeric_limits<float>::quiet_NaN());
    if (!fam)
    {
        a.matched = t.n();
        for (size_t i = 0; i < t.n(); i++)
            for (size_t j = 0; j < p; j++) a.data[j * a.N + i] = t.rows[i * p + j];
        return a;
    }
    std::unordered_map<std::string, size_t> row_of;
    row_of.reserve(t.n());
    for (size_t i = 0; i < t.n(); i++) row_of.emplace(t.iid[i], i);
    a.in_order = t.n() == fam->n();
    for (size_t i = 0; i < fam->n(); i++)
    {
        const auto it = row_of.find(fam->iid[i]);
        if (a.in_order && t.iid[i] != fam->iid[i]) a.in_order = false;
        if (it == row_of.end()) continue;
        ++a.matched;
        for (size_t j = 0; j < p; j++) a.data[j * a.N + i] = t.rows[it->second * p + j];
    }
    a.dropped = t.n() - a.matched;
    return a;
}

// text output file whose every write and the close are checked; a failure removes the file
struct CheckedTextFile
{
    std::string path;
    FILE *f;
    explicit CheckedTextFile(const std::string &p) : path(p), f(std::fopen(p.c_str(), "wb"))
    {
        if (!f) die("cannot write " + path);
    }
    void put(const std::string &s)
    {
        if (!s.empty() && std::fwrite(s.data(), 1, s.size(), f) != s.size()) fail();
    }
    void close()
    {
        FILE *g = f;
        f = nullptr;
        if (std::fclose(g) != 0)
        {
            ::unlink(path.c_str());
            die("cannot write " + path);
        }
    }
    [[noreturn]] void fail()
    {
        std::fclose(f);
        f = nullptr;
        ::unlink(path.c_str());
        die("cannot write " + path);
    }
    ~CheckedTextFile()
    {
        if (!f) return;
        std::fclose(f);  // on the way out of a failure that is already being reported
        ::unlink(path.c_str());
    }
};

// header FID IID <names>, the .fam's ids, %.9g, NaN as NA; data: names.size() x fam.n() trait-major
inline void write_phen_file(const std::string &path, const FamIds &fam, const std::vector<std::string> &names, const float *data)
{
    const size_t N = fam.n(), p = names.size();
    CheckedTextFile out(path);
    std::string buf = "FID\tIID";
    for (const std::string &nm : names) buf += "\t" + nm;
    buf += "\n";
    char num[64];
    for (size_t i = 0; i < N; i++)
    {
        buf += fam.fid[i];
        buf += '\t';
        buf += fam.iid[i];
        for (size_t j = 0; j < p; j++)
        {
            const float v = data[j * N + i];
            buf += '\t';
            if (v != v)
                buf += "NA";
            else
            {
                std::snprintf(num, sizeof(num), "%.9g", (double)v);
                buf += num;
            }
        }
        buf += '\n';
        if (buf.size() >= ((size_t)1 << 16))
        {
            out.put(buf);
            buf.clear();
        }
    }
    out.put(buf);
    out.close();
}

}  // namespace host
