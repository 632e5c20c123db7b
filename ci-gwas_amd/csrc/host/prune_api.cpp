// prune_api.cpp -- the pruned fileset of `mps prune`, written from the per-marker statuses of cusk_ld_prune
// (cusk_prune_write of include/cusk_hip.h).  Host only.  Rows of the .bed and lines of the .bim are copied byte for byte;
// nothing is opened for writing before every input has been opened and measured and the output stem is known to name other
// files, every write and close is checked, and a call that fails takes the files it created away again.
#include <unistd.h>

#include <cstdio>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "../../../include/cusk_hip.h"
#include "host_io.h"

namespace {

struct WriteFailed
{
    std::string path;
};

// output file whose every operation is checked
struct OutFile
{
    std::string path;
    FILE *f;
    explicit OutFile(const std::string &p) : path(p), f(std::fopen(p.c_str(), "wb"))
    {
        if (!f) throw WriteFailed{path};
    }
    void write(const void *data, size_t bytes)
    {
        if (bytes && std::fwrite(data, 1, bytes, f) != bytes) throw WriteFailed{path};
    }
    void write(const std::string &s) { write(s.data(), s.size()); }
    void close()
    {
        FILE *g = f;
        f = nullptr;
        if (std::fclose(g) != 0) throw WriteFailed{path};
    }
    ~OutFile()
    {
        if (!f) return;
        std::fclose(f);  // only on the way out of a failure that is already being reported:
        ::unlink(path.c_str());  // nothing half-written stays behind
    }
};

// both exist and are the same file (another spelling of the path, a link)
bool same_file(const std::string &a, const std::string &b)
{
    std::error_code ec;
    return std::filesystem::equivalent(a, b, ec) && !ec;
}

long long file_size(const std::string &path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    return f ? (long long)f.tellg() : -1;
}

int refuse(const std::string &msg, int code)
{
    std::fprintf(stderr, "cusk_prune_write: %s\n", msg.c_str());
    return code;
}

}  // namespace

extern "C" int cusk_prune_write(const char *bfiles, const char *out_stem, const unsigned char *status, size_t m_total)
{
    if (!bfiles || !out_stem || !status || m_total == 0) return refuse("bad arguments", CUSK_ERR_ARG);
    const std::string in = bfiles, out = out_stem;
    if (in == out) return refuse("the output stem is the input stem", CUSK_ERR_ARG);
    for (const char *osfx : {".bed", ".bim", ".fam", ".prune.in", ".prune.out"})
        for (const char *isfx : {".bed", ".bim", ".fam"})
            if (same_file(out + osfx, in + isfx)) return refuse(out + osfx + " is the input file " + in + isfx, CUSK_ERR_ARG);
    for (const char *sfx : {".bed", ".bim", ".fam"})
        if (!host::path_exists(in + sfx)) return refuse("file not found: " + in + sfx, CUSK_ERR_ARG);
    if (!host::bed_has_valid_magic(in + ".bed")) return refuse("unexpected magic number in " + in + ".bed", CUSK_ERR_ARG);
    const size_t N = host::count_lines(in + ".fam"), clb = (N + 3) / 4;
    if (N == 0) return refuse(in + ".fam is empty", CUSK_ERR_ARG);
    if (host::count_lines(in + ".bim") != m_total) return refuse(in + ".bim does not have m_total lines", CUSK_ERR_ARG);
    for (size_t i = 0; i < m_total; i++)
        if (status[i] > CUSK_PRUNE_LD) return refuse("unknown status value", CUSK_ERR_ARG);
    if (file_size(in + ".bed") < (long long)(3 + m_total * clb)) return refuse(in + ".bed is shorter than its .bim and .fam say", CUSK_ERR_ARG);
    try
    {
        std::ifstream bed(in + ".bed", std::ios::binary), bim(in + ".bim"), fam(in + ".fam", std::ios::binary);
        OutFile obed(out + ".bed"), obim(out + ".bim"), ofam(out + ".fam"), oin(out + ".prune.in"), oout(out + ".prune.out");
        const unsigned char magic[3] = {0x6c, 0x1b, 0x01};
        obed.write(magic, 3);
        bed.seekg(3);
        std::vector<char> row(clb);
        std::string line;
        for (size_t i = 0; i < m_total; i++)
        {
            if (!bed.read(row.data(), (std::streamsize)clb) || !std::getline(bim, line))
                return refuse("cannot read marker " + std::to_string(i) + " of " + in, CUSK_ERR_ARG);  // the outputs are removed
            const bool ended = !bim.eof();  // false for a last line without a newline: it is copied as it is
            const std::vector<std::string> w = host::split_ws(line);
            const std::string id = w.size() > 1 ? w[1] : std::string(".");
            if (status[i] == CUSK_PRUNE_KEEP)
            {
                obed.write(row.data(), clb);
                obim.write(ended ? line + "\n" : line);
                oin.write(id + "\n");
            }
            else
                oout.write(id + (status[i] == CUSK_PRUNE_CONSTANT ? "\tconstant\n" : "\tld\n"));
        }
        std::vector<char> buf((size_t)1 << 16);
        while (fam.read(buf.data(), (std::streamsize)buf.size()) || fam.gcount() > 0) ofam.write(buf.data(), (size_t)fam.gcount());
        for (OutFile *f : {&obed, &obim, &ofam, &oin, &oout}) f->close();
    }
    catch (const WriteFailed &w)
    {
        return refuse("cannot write " + w.path, CUSK_ERR_STATE);
    }
    return CUSK_OK;
}
