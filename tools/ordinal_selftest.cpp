// ordinal_selftest.cpp -- the host-only parts of `ordinal=` under the host sanitizers: the argument parser and the level
// scan of csrc/host/ordinal_host.h, the standard-error writer cusk_sumstats_write_se_values of csrc/host/sumstats_api.cpp
// (written and read back), and the estimators' arithmetic of csrc/ordinal_math.h, which the device kernels compile from the
// same text, against closed forms.  Stand-alone, no HIP:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/ordinal_selftest.cpp
//       ci-gwas_amd/csrc/host/sumstats_api.cpp -o ordinal_selftest        (one command line)
//   ./ordinal_selftest <scratch directory>
// `./ordinal_selftest fit` reads tables "ka kb n_00 n_01 ..." from standard input, one per line, and prints r, se, status
// of the host build of the fit with 17 digits (to compare the arithmetic with another implementation).
#include "../ci-gwas_amd/csrc/host/ordinal_host.h"
#include "../ci-gwas_amd/csrc/ordinal_math.h"
#include "../include/cusk_hip.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>

using namespace host;
namespace ord = cusk::ord;

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

struct VecCell
{
    const int *T;
    int kb;
    int operator()(int a, int b) const { return T[a * kb + b]; }
};

static void fit(const std::vector<int> &t, int ka, int kb, double &r, double &se, int &status)
{
    double alpha[8], beta[8];
    ord::polychoric_fit(VecCell{t.data(), kb}, ka, kb, alpha, 1, beta, 1, r, se, status);
}

static bool throws(const std::string &arg, size_t p)
{
    try
    {
        parse_ordinal_arg(arg, p);
    }
    catch (const std::runtime_error &)
    {
        return true;
    }
    return false;
}

static void test_parser()
{
    EXPECT((parse_ordinal_arg("ordinal=2,5", 6) == std::vector<int>{1, 4}));
    EXPECT((parse_ordinal_arg("ordinal=6", 6) == std::vector<int>{5}));
    for (const char *bad : {"ordinal=", "ordinal=0", "ordinal=7", "ordinal=2,,3", "ordinal=2,", "ordinal=,2", "ordinal=a", "ordinal=-1",
                            "ordinal=2,2", "ordinal=99999999999999999999", "ordinal", "ordina=1", "ordinal=1 2", ""})
        EXPECT(throws(bad, 6));
}

static void test_levels()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const size_t N = 7;
    // trait 0: binary with NaN; trait 1: seven values; trait 2: constant; trait 3: all NaN; trait 4: seven values, unsorted
    std::vector<float> phen = {0, 1, nan, 1, 0, 0, 1, /**/ 1, 2, 3, 4, 5, 6, 7, /**/ 3, 3, 3, nan, 3, 3, 3,
                               /**/ nan, nan, nan, nan, nan, nan, nan, /**/ 7, 1, 5, 3, 2, 6, 4};
    std::vector<std::string> names = {"bin", "grades", "const", "none", "seven"};
    const OrdinalSpec s = ordinal_levels({0, 4}, phen.data(), N, names);
    EXPECT(s.q() == 2 && s.nlev[0] == 2 && s.nlev[1] == 7);
    EXPECT(s.levels[0] == 0.0f && s.levels[1] == 1.0f && s.levels[8] == 1.0f && s.levels[8 + 6] == 7.0f);
    auto message = [&](int t, const std::vector<float> &ph, size_t n) {
        try
        {
            ordinal_levels({t}, ph.data(), n, names);
        }
        catch (const std::runtime_error &ex)
        {
            return std::string(ex.what());
        }
        return std::string();
    };
    EXPECT(message(2, phen, N).find("const has 1 distinct") != std::string::npos);
    EXPECT(message(3, phen, N).find("none has 0 distinct") != std::string::npos);
    std::vector<float> nine(9);
    for (int i = 0; i < 9; i++) nine[i] = (float)(9 - i);
    names[0] = "grade";
    EXPECT(message(0, nine, 9).find("grade has 9 distinct") != std::string::npos);
    std::vector<float> many(10000);
    for (size_t i = 0; i < many.size(); i++) many[i] = (float)i * 0.5f;
    EXPECT(message(0, many, many.size()).find("more than 4096") != std::string::npos);
}

static void test_writer(const std::string &dir)
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const size_t m = 3, p = 2;
    const float mxp_se[] = {0.0123456789f, nan, 1e-9f, 0.5f, -nan, 3.25f};
    const float pxp_se[] = {nan, 0.03125f, 0.03125f, nan};
    const char *chr[] = {"1", "1", "2"}, *snp[] = {"rs1", "rs2", "rs3"}, *ref[] = {"A", "C", "G"}, *names[] = {"t1", "t2"};
    char err[256] = "";
    EXPECT(cusk_sumstats_write_se_values(dir.c_str(), mxp_se, m, p, pxp_se, chr, snp, ref, names, err, sizeof(err)) == CUSK_OK);
    std::ifstream f(dir + "/mxp_se.txt");
    std::string line;
    std::getline(f, line);
    EXPECT(line == "chr snp ref t1 t2");
    for (size_t i = 0; i < m; i++)
    {
        std::getline(f, line);
        std::istringstream ls(line);
        std::string c, s, r, v;
        ls >> c >> s >> r;
        EXPECT(c == chr[i] && s == snp[i] && r == ref[i]);
        for (size_t t = 0; t < p; t++)
        {
            ls >> v;
            const float want = mxp_se[i * p + t];
            if (std::isnan(want))
                EXPECT(v == "NA");
            else
                EXPECT(std::stof(v) == want);
        }
    }
    std::ifstream g(dir + "/pxp_se.txt");
    std::getline(g, line);
    EXPECT(line == "t1 t2");
    std::getline(g, line);
    EXPECT(line == "t1 nan 0.03125");
    std::getline(g, line);
    EXPECT(line == "t2 0.03125 nan");
    EXPECT(cusk_sumstats_write_se_values(dir.c_str(), nullptr, m, p, pxp_se, chr, snp, ref, names, err, sizeof(err)) != CUSK_OK);
    EXPECT(cusk_sumstats_write_se_values((dir + "/no/such/dir").c_str(), mxp_se, m, p, pxp_se, chr, snp, ref, names, err, sizeof(err)) !=
           CUSK_OK);
    EXPECT(std::strlen(err) > 0);
}

static void test_math()
{
    const double pi = 3.14159265358979323846;
    // Phi2 at zero thresholds: 1/4 + asin(rho) / (2 pi), across the three quadrature ranges and the expansion near one
    for (double rho : {-0.9999, -0.95, -0.8, -0.5, -0.1, 0.0, 0.2, 0.6, 0.9, 0.93, 0.99, 0.9999})
        EXPECT(std::fabs(ord::Phi2(0.0, 0.0, rho) - (0.25 + std::asin(rho) / (2.0 * pi))) < 1e-15);
    EXPECT(ord::Phi2(-INFINITY, 1.0, 0.3) == 0.0 && ord::Phi2(INFINITY, INFINITY, 0.3) == 1.0);
    EXPECT(std::fabs(ord::Phi2(INFINITY, 0.0, 0.3) - 0.5) < 1e-16);
    EXPECT(std::fabs(ord::threshold_of(1, 2)) < 1e-16 && ord::threshold_of(0, 5) == -INFINITY && ord::threshold_of(5, 5) == INFINITY);
    EXPECT(std::fabs(ord::threshold_of(975, 1000) - 1.959963984540054) < 1e-13);
    double r, se;
    int status;
    // 2 x 2 with all margins 1/2: rho = sin(pi / 2 (p11 + p00 - p10 - p01))
    fit({300, 200, 200, 300}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusOk && std::fabs(r - std::sin(pi / 2.0 * 0.2)) < 1e-12 && se > 0.0);
    fit({200, 300, 300, 200}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusOk && std::fabs(r + std::sin(pi / 2.0 * 0.2)) < 1e-12);
    // independence
    fit({20, 30, 50, 40, 60, 100}, 2, 3, r, se, status);
    EXPECT(status == ord::kStatusOk && std::fabs(r) < 1e-12);
    // padded cells change nothing
    double r2, se2;
    fit({20, 30, 50, 0, 40, 60, 100, 0, 0, 0, 0, 0}, 3, 4, r2, se2, status);
    EXPECT(status == ord::kStatusOk && r2 == r && se2 == se);
    // monotone: boundary; one level on a side: degenerate
    fit({50, 0, 0, 50}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusBoundary && r == ord::kRhoMax && std::isnan(se));
    fit({0, 50, 50, 0}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusBoundary && r == -ord::kRhoMax && std::isnan(se));
    fit({50, 50, 0, 0}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusDegenerate && std::isnan(r) && std::isnan(se));
    fit({0, 0, 0, 0}, 2, 2, r, se, status);
    EXPECT(status == ord::kStatusDegenerate);
}

static int fit_stdin()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream ls(line);
        int ka, kb;
        if (!(ls >> ka >> kb) || ka < 1 || kb < 1 || ka > 8 || kb > 8) return 1;
        std::vector<int> t((size_t)(ka * kb));
        for (int &v : t)
            if (!(ls >> v) || v < 0) return 1;
        double r, se;
        int status;
        fit(t, ka, kb, r, se, status);
        std::printf("%.17g %.17g %d\n", r, se, status);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "fit") return fit_stdin();
    if (argc < 2)
    {
        std::printf("usage: ordinal_selftest <scratch directory> | fit\n");
        return 2;
    }
    test_parser();
    test_levels();
    test_writer(argv[1]);
    test_math();
    std::printf(failures ? "%d FAILED\n" : "ordinal_selftest ok\n", failures);
    return failures ? 1 : 0;
}
