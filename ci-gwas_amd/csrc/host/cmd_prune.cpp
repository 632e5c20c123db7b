// cmd_prune.cpp -- mps prune (not in the reference, whose README leaves both preconditions to the user): drop constant
// markers and LD-prune a fileset on the device; goes in front of `mps prep`.
#include <filesystem>

#include "engine_util.h"
#include "host_io.h"
#include "mps.h"

using namespace host;

namespace {

const char *PRUNE_USAGE = R"(
Drop markers without recorded variation and LD-prune a fileset on the correlation the skeleton tests

usage: mps prune <bfiles> <out-stem> <r-max> <window>

arguments:
    bfiles          stem of .bed, .bim, .fam fileset
    out-stem        stem of the pruned fileset (.bed, .bim, .fam) and of .prune.in / .prune.out; not bfiles itself
    r-max           a marker is dropped when |r| >= r-max with an earlier kept marker of its chromosome within the
                    window; in (0, 1]; r is the banded Kendall-npn correlation of `mps block`
    window          number of following markers every marker is compared with (at most 4096)

Markers are walked in .bim order per chromosome and the first kept marker wins (PLINK's --indep-pairwise keeps the marker
with the higher minor allele frequency and prunes on the Pearson r^2 of the dosages).  A marker with at most one
genotype among its non-missing calls is dropped as constant and blocks no other marker.
)";

}  // namespace

int host::cmd_prune(int argc, char **argv)
{
    if (argc != 6)
    {
        std::cout << PRUNE_USAGE << std::endl;
        std::exit(1);
    }
    const std::string bfiles = argv[2], out_stem = argv[3];
    float r_max = 0.0f;
    long long window = 0;
    try
    {
        r_max = std::stof(argv[4]);
        window = std::stoll(argv[5]);
    }
    catch (const std::exception &)
    {
        die("r-max and window must be numbers");
    }
    if (!(r_max > 0.0f && r_max <= 1.0f)) die("r-max must be in (0, 1]");
    if (window < 1 || window > CUSK_PRUNE_MAX_WINDOW) die("window must be between 1 and " + std::to_string(CUSK_PRUNE_MAX_WINDOW));
    if (out_stem == bfiles) die("out-stem must differ from bfiles");
    for (const char *sfx : {".bed", ".bim", ".fam"})
    {  // another spelling of the same stem, or a link: found before the device work, cusk_prune_write checks again
        std::error_code ec;
        if (std::filesystem::equivalent(out_stem + sfx, bfiles + sfx, ec) && !ec) die("out-stem must differ from bfiles: " + out_stem + sfx + " is the input file");
    }
    PhaseTimer tm;

    std::cout << "Checking paths" << std::endl;
    for (const char *sfx : {".bed", ".bim", ".fam"}) check_path(bfiles + sfx);
    if (!bed_has_valid_magic(bfiles + ".bed")) die("unexpected magic number in bed file.");
    const BimInfo bim = read_bim(bfiles + ".bim");
    const size_t N = count_lines(bfiles + ".fam");
    if (bim.num_lines == 0 || N == 0) die("empty .bim or .fam file");

    cusk_engine *e = open_engine();
    std::vector<unsigned char> status(bim.num_lines);
    for (size_t c = 0; c < bim.chr_ids.size(); c++)
    {
        // (by position, not by id: the statuses of a chromosome id that occurs twice must not land on its first run)
        const std::string &cid = bim.chr_ids[c];
        const size_t m = bim.num_on_chr[c], start = bim.chr_start[c];
        std::vector<unsigned char> bed(m * ((N + 3) / 4));
        {
            std::ifstream f(bfiles + ".bed", std::ios::binary);
            f.seekg(3 + (std::streamoff)(start * ((N + 3) / 4)));
            if (!f.read(reinterpret_cast<char *>(bed.data()), (std::streamsize)bed.size())) die("bed file is shorter than its .bim and .fam say");
        }
        tm.mark("read chromosome");
        if (cusk_ld_prune(e, bed.data(), m, N, (size_t)window, r_max, status.data() + start, nullptr) != CUSK_OK)
            engine_die("ld prune", e);
        tm.mark("banded correlations, counts, bitmap, scan (device)");
        size_t n[3] = {0, 0, 0};
        for (size_t j = 0; j < m; j++) n[status[start + j]]++;
        std::cout << "[Chr " << cid << "]: " << m << " markers: " << n[CUSK_PRUNE_KEEP] << " kept, " << n[CUSK_PRUNE_CONSTANT]
                  << " constant, " << n[CUSK_PRUNE_LD] << " dropped for LD." << std::endl;
    }
    cusk_engine_destroy(e);
    if (cusk_prune_write(bfiles.c_str(), out_stem.c_str(), status.data(), status.size()) != CUSK_OK) die("cannot write the pruned fileset " + out_stem);
    tm.mark("write fileset");
    std::cout << "Done." << std::endl;
    return 0;
}
