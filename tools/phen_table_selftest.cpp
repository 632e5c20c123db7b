// phen_table_selftest.cpp -- host side of `mps prep-phen` (csrc/host/phen_table.h behind csrc/host/phen_api.cpp) under the
// host sanitizers: the table reader, the alignment to a .fam and the .phen writer, through the C entry points, on the
// inputs that break parsers -- ragged rows, an empty file, a header alone, CRLF, a line of 10^5 characters, ids the .fam
// does not have, a duplicate id, EID -- and a write / read round trip of every kind of float32.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/phen_table_selftest.cpp \
//       ci-gwas_amd/csrc/host/phen_api.cpp -o phen_table_selftest
//   ./phen_table_selftest
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../include/cusk_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static std::string dir;

static std::string put(const std::string &name, const std::string &text)
{
    const std::string path = dir + "/" + name;
    std::ofstream f(path, std::ios::binary);
    f << text;
    return path;
}

struct Loaded
{
    int rc;
    std::string err;
    cusk_phen_table *t;
    ~Loaded() { cusk_phen_table_free(t); }
};

static Loaded load(const std::string &table, const char *fam)
{
    char err[256] = "";
    cusk_phen_table *t = nullptr;
    const int rc = cusk_phen_table_load(&t, table.c_str(), fam, err, sizeof(err));
    return Loaded{rc, err, t};
}

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main()
{
    char tmpl[] = "/tmp/phen_table_selftest_XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    dir = tmpl;
    const std::string fam = put("s.fam", "f1 a 0 0 1 -9\nf2 b 0 0 2 -9\nf3 c 0 0 1 -9\nf4 d 0 0 2 -9\n");

    {  // plain, shuffled, one individual absent, one extra; NA tokens
        Loaded l = load(put("t1.tsv", "FID IID x y\nq d 4 NA\nq b 2 nan\nq zz 9 9\nq a 1 -1e3\n"), fam.c_str());
        EXPECT(l.rc == CUSK_OK && l.t);
        if (l.t)
        {
            EXPECT(cusk_phen_table_rows(l.t) == 4 && cusk_phen_table_cols(l.t) == 2);
            EXPECT(cusk_phen_table_matched(l.t) == 3 && cusk_phen_table_dropped(l.t) == 1 && cusk_phen_table_in_order(l.t) == 0);
            EXPECT(std::string(cusk_phen_table_name(l.t, 1)) == "y" && cusk_phen_table_name(l.t, 2) == nullptr);
            const float *d = cusk_phen_table_data(l.t);
            EXPECT(d[0] == 1.0f && d[1] == 2.0f && std::isnan(d[2]) && d[3] == 4.0f);
            EXPECT(d[4] == -1000.0f && std::isnan(d[5]) && std::isnan(d[6]) && std::isnan(d[7]));
        }
    }
    {  // CRLF, IID first, EID; in order
        Loaded l = load(put("t2.tsv", "EID\tFID\tx\r\na\tq\t0.5\r\nb\tq\tNAN\r\nc\tq\t1e-45\r\nd\tq\t-0\r\n"), fam.c_str());
        EXPECT(l.rc == CUSK_OK && l.t && cusk_phen_table_in_order(l.t) == 1 && cusk_phen_table_matched(l.t) == 4);
        if (l.t)
        {
            const float *d = cusk_phen_table_data(l.t);
            EXPECT(d[0] == 0.5f && std::isnan(d[1]) && d[2] > 0.0f && d[2] < 1e-44f && d[3] == 0.0f && std::signbit(d[3]));
        }
    }
    {  // without a .fam: the rows as they come; a last line without a newline; blank lines
        Loaded l = load(put("t3.tsv", "FID IID x\n\nq z 3\n   \nq y 4"), nullptr);
        EXPECT(l.rc == CUSK_OK && l.t && cusk_phen_table_rows(l.t) == 2);
        if (l.t) EXPECT(cusk_phen_table_data(l.t)[0] == 3.0f && cusk_phen_table_data(l.t)[1] == 4.0f);
    }
    {  // a header alone, with and without columns
        Loaded l = load(put("t4.tsv", "FID IID x y z\n"), fam.c_str());
        EXPECT(l.rc == CUSK_OK && l.t && cusk_phen_table_rows(l.t) == 4 && cusk_phen_table_cols(l.t) == 3 && cusk_phen_table_matched(l.t) == 0);
        if (l.t)
            for (int i = 0; i < 12; i++) EXPECT(std::isnan(cusk_phen_table_data(l.t)[i]));
        Loaded m = load(put("t4b.tsv", "IID FID"), nullptr);
        EXPECT(m.rc == CUSK_OK && m.t && cusk_phen_table_rows(m.t) == 0 && cusk_phen_table_cols(m.t) == 0);
    }
    {  // the refusals, each with its place
        Loaded a = load(put("e1.tsv", ""), fam.c_str());
        EXPECT(a.rc == CUSK_ERR_ARG && !a.t && has(a.err, "empty"));
        Loaded b = load(put("e2.tsv", "FID IID x y\nq a 1 2\nq b 1\n"), fam.c_str());
        EXPECT(b.rc == CUSK_ERR_ARG && !b.t && has(b.err, "line 3") && has(b.err, "3 columns"));
        Loaded c = load(put("e3.tsv", "FID IID x y\nq a 1 2 3\n"), fam.c_str());
        EXPECT(c.rc == CUSK_ERR_ARG && has(c.err, "line 2"));
        Loaded d = load(put("e4.tsv", "FID IID x\nq a 1\nq b 2\nr a 3\n"), fam.c_str());
        EXPECT(d.rc == CUSK_ERR_ARG && has(d.err, "line 4") && has(d.err, "duplicate IID a"));
        Loaded e = load(put("e5.tsv", "FID IID x y\nq a 1 2\nq b 1 abc\n"), fam.c_str());
        EXPECT(e.rc == CUSK_ERR_ARG && has(e.err, "line 3, column 4") && has(e.err, "abc"));
        Loaded f = load(put("e6.tsv", "FID IID x\nq a 1.5e\n"), fam.c_str());
        EXPECT(f.rc == CUSK_ERR_ARG && has(f.err, "1.5e"));
        Loaded g = load(put("e7.tsv", "id x y\n1 2 3\n"), fam.c_str());
        EXPECT(g.rc == CUSK_ERR_ARG && has(g.err, "line 1"));
        Loaded h = load(put("e8.tsv", "FID\n"), fam.c_str());
        EXPECT(h.rc == CUSK_ERR_ARG && has(h.err, "line 1"));
        Loaded i = load(dir + "/absent.tsv", fam.c_str());
        EXPECT(i.rc == CUSK_ERR_ARG && !i.t);
        Loaded j = load(put("t5.tsv", "FID IID x\nq a 1\n"), (dir + "/absent.fam").c_str());
        EXPECT(j.rc == CUSK_ERR_ARG && !j.t);
        Loaded k = load(put("t6.tsv", "FID IID x\nq a 1\n"), put("dup.fam", "f a 0 0 1 -9\nf a 0 0 1 -9\n").c_str());
        EXPECT(k.rc == CUSK_ERR_ARG && has(k.err, "duplicate IID a"));
        char small[8];
        cusk_phen_table *t = nullptr;
        EXPECT(cusk_phen_table_load(&t, (dir + "/e5.tsv").c_str(), fam.c_str(), small, sizeof(small)) == CUSK_ERR_ARG && std::strlen(small) == 7);
        EXPECT(cusk_phen_table_load(&t, (dir + "/e5.tsv").c_str(), fam.c_str(), nullptr, 0) == CUSK_ERR_ARG);
        EXPECT(cusk_phen_table_load(nullptr, "x", nullptr, nullptr, 0) == CUSK_ERR_ARG);
        EXPECT(cusk_phen_table_rows(nullptr) == 0 && cusk_phen_table_data(nullptr) == nullptr);
        cusk_phen_table_free(nullptr);
    }
    {  // one line of more than 10^5 characters, and a token of 10^5 characters that is no number
        std::string head = "FID IID", row = "q c";
        for (int j = 0; j < 25000; j++)
        {
            head += " v" + std::to_string(j);
            row += " " + std::to_string(j) + ".5";
        }
        Loaded l = load(put("wide.tsv", head + "\n" + row + "\n"), fam.c_str());
        EXPECT(l.rc == CUSK_OK && l.t && cusk_phen_table_cols(l.t) == 25000 && row.size() > 100000);
        if (l.t) EXPECT(cusk_phen_table_data(l.t)[(size_t)24999 * 4 + 2] == 24999.5f && std::isnan(cusk_phen_table_data(l.t)[(size_t)24999 * 4]));
        Loaded m = load(put("long.tsv", "FID IID x\nq a " + std::string(100000, '7') + "x\n"), fam.c_str());
        EXPECT(m.rc == CUSK_ERR_ARG && has(m.err, "line 2, column 3"));
    }
    {  // writer: every kind of float32 comes back with its bits; the refusals
        const size_t N = 4000, p = 3;
        std::string famtext;
        for (size_t i = 0; i < N; i++) famtext += "F" + std::to_string(i) + "\tI" + std::to_string(i) + " 0 0 1 -9\n";
        const std::string big_fam = put("big.fam", famtext);
        std::mt19937 rng(7);
        std::vector<float> v(N * p);
        for (float &x : v)
        {
            const uint32_t b = rng();
            std::memcpy(&x, &b, 4);
            if (!std::isfinite(x)) x = std::numeric_limits<float>::quiet_NaN();
        }
        v[0] = std::numeric_limits<float>::denorm_min();
        v[1] = -std::numeric_limits<float>::max();
        v[2] = std::numeric_limits<float>::min();
        v[3] = std::numeric_limits<float>::quiet_NaN();
        const char *names[3] = {"a", "b", "c"};
        char err[256] = "";
        const std::string out = dir + "/out.phen";
        EXPECT(cusk_phen_write(out.c_str(), big_fam.c_str(), names, p, v.data(), N, err, sizeof(err)) == CUSK_OK);
        Loaded l = load(out, big_fam.c_str());
        EXPECT(l.rc == CUSK_OK && l.t && cusk_phen_table_in_order(l.t) == 1 && cusk_phen_table_cols(l.t) == 3);
        if (l.t)
        {
            const float *d = cusk_phen_table_data(l.t);
            size_t bad = 0;
            for (size_t i = 0; i < N * p; i++) bad += !(std::memcmp(&d[i], &v[i], 4) == 0 || (std::isnan(d[i]) && std::isnan(v[i])));
            EXPECT(bad == 0);
        }
        EXPECT(cusk_phen_write(big_fam.c_str(), big_fam.c_str(), names, p, v.data(), N, err, sizeof(err)) == CUSK_ERR_ARG);
        EXPECT(cusk_phen_write(out.c_str(), big_fam.c_str(), names, p, v.data(), N - 1, err, sizeof(err)) == CUSK_ERR_ARG);
        EXPECT(cusk_phen_write(out.c_str(), big_fam.c_str(), names, 0, v.data(), N, err, sizeof(err)) == CUSK_ERR_ARG);
        EXPECT(cusk_phen_write(out.c_str(), nullptr, names, p, v.data(), N, nullptr, 0) == CUSK_ERR_ARG);
        const std::string nowhere = dir + "/no_such_dir/out.phen";
        EXPECT(cusk_phen_write(nowhere.c_str(), big_fam.c_str(), names, p, v.data(), N, err, sizeof(err)) == CUSK_ERR_STATE && has(err, "cannot write"));
    }
    const std::string cleanup = "rm -rf '" + dir + "'";
    if (std::system(cleanup.c_str()) != 0) std::printf("could not remove %s\n", dir.c_str());
    std::printf(failures ? "phen_table_selftest: %d FAILED\n" : "phen_table_selftest: all passed\n", failures);
    return failures ? 1 : 0;
}
