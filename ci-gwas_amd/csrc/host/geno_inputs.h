// geno_inputs.h -- a prepared fileset (.bed with the .dim / .means / .stds of `mps prep`) and a .phen on their way to the
// device: the checks every command that reads genotypes makes (each a step of its own; `mps cusk` and the commands on a
// marker selection make them in different orders and keep those), the inputs on the device, and GenoInputs, what
// `mps sumstats` and `mps cuskss-bed` load.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <numeric>

#include "engine_util.h"
#include "host_io.h"

namespace host {

// read-only memory map of the .bed (a whole-genome file is read block by block, by whichever rank owns the block)
struct MappedFile
{
    const unsigned char *data = nullptr;
    size_t size = 0;
    int fd = -1;
    void open(const std::string &path)
    {
        close();
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) die("file or directory not found: " + path);
        struct stat st;
        if (fstat(fd, &st) != 0) die("cannot stat " + path);
        size = (size_t)st.st_size;
        if (size)
        {
            void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (p == MAP_FAILED) die("cannot map " + path);
            data = static_cast<const unsigned char *>(p);
        }
    }
    void close()
    {
        if (data) munmap(const_cast<unsigned char *>(data), size);
        if (fd >= 0) ::close(fd);
        data = nullptr;
        size = 0;
        fd = -1;
    }
    ~MappedFile() { close(); }
    MappedFile() = default;
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

// ---- the steps of a load ----
inline void check_prep_paths(const std::string &bfiles)
{
    for (const char *sfx : {".bed", ".dim", ".means", ".stds", ".bim"}) check_path(bfiles + sfx);
}

inline void check_bed_magic(const std::string &bfiles)
{
    if (!bed_has_valid_magic(bfiles + ".bed")) die("unexpected magic number in bed file.");
}

// .phen (trait_names: also the names in its header) and .dim, which must agree on the number of individuals
inline void load_phen_dims(const std::string &phen_path, const std::string &bfiles, Phen &phen, BedDims &dims,
                           std::vector<std::string> *trait_names = nullptr)
{
    phen = load_phen(phen_path);
    if (trait_names)
    {
        std::ifstream f(phen_path);
        std::string header;
        std::getline(f, header);
        const auto w = split_ws(header);
        if (w.size() != phen.num_phen + 2) die("header and rows of the .phen file differ in width");
        trait_names->assign(w.begin() + 2, w.end());
    }
    dims = read_dims(bfiles + ".dim");
    if (phen.num_samples != dims.num_samples) die("different num samples in phen and dims");
}

// maps the .bed; markers > 0: it must hold that many (a caller that passes 0 checks the rows of each block it reads)
inline void map_bed(MappedFile &bed, const std::string &bfiles, const BedDims &dims, size_t markers)
{
    bed.open(bfiles + ".bed");
    if (markers && bed.size < 3 + markers * dims.bytes_per_col()) die(".bed file is smaller than .dim says");
}

// the inputs all blocks or chunks share, resident on one device: marker g's genotypes start at bed + g * bytes_per_col,
// means / stds are indexed by global marker
struct StagedInputs
{
    unsigned char *bed = nullptr;
    float *phen = nullptr, *means = nullptr, *stds = nullptr;
    void release()
    {
        cusk_dev_free(bed);
        cusk_dev_free(phen);
        cusk_dev_free(means);
        cusk_dev_free(stds);
        bed = nullptr;
        phen = means = stds = nullptr;
    }
};

// phen, means, stds and the .bed rows (bed_bytes from bed_rows on) to the current device, each allocation `pad` bytes
// longer than its array.  Returns NULL, or the name of the step that failed with everything released.  host_bed_log: a
// .bed the device has no room for is no failure -- st.bed stays NULL, the stream is told, and the caller hands the kernels
// the file mapping (the same entry points take either).
inline const char *stage_inputs(StagedInputs &st, const unsigned char *bed_rows, size_t bed_bytes, const std::vector<float> &phen,
                                const std::vector<float> &means, const std::vector<float> &stds, size_t pad, std::ostream *host_bed_log)
{
    const char *failed = nullptr;
    auto up = [&](const void *src, size_t bytes, const char *what) -> void * {
        void *d = failed ? nullptr : cusk_dev_alloc(bytes + pad);
        if (!failed && (!d || cusk_dev_upload(d, src, bytes) != CUSK_OK)) failed = what;
        return d;
    };
    st.phen = static_cast<float *>(up(phen.data(), sizeof(float) * phen.size(), "upload phenotypes"));
    st.means = static_cast<float *>(up(means.data(), sizeof(float) * means.size(), "upload means"));
    st.stds = static_cast<float *>(up(stds.data(), sizeof(float) * stds.size(), "upload stds"));
    if (!failed)
    {
        st.bed = static_cast<unsigned char *>(cusk_dev_alloc(bed_bytes + pad));
        if (!st.bed && host_bed_log)
            *host_bed_log << "The .bed (" << bed_bytes << " bytes) does not fit the device: reading it from the host" << std::endl;
        else if (!st.bed || cusk_dev_upload(st.bed, bed_rows, bed_bytes) != CUSK_OK)
            failed = "upload .bed";
    }
    if (failed) st.release();
    return failed;
}

// .phen, the prep files and the marker selection; the arrays every kernel reads are copied to the device once
struct GenoInputs
{
    Phen phen;
    std::vector<std::string> trait_names, chr, snp, ref;
    BedDims dims;
    MappedFile bed;
    std::vector<float> means, stds;
    std::vector<int> ixs;
    StagedInputs dev;
    size_t N() const { return dims.num_samples; }
    size_t m() const { return dims.num_markers; }
    size_t p() const { return phen.num_phen; }
    size_t k() const { return ixs.size(); }
    // the .bed rows where the kernels find them: HBM, or the file mapping when the device has no room for all of them
    const unsigned char *bed_rows() const { return dev.bed ? dev.bed : bed.data + 3; }

    void load(const std::string &phen_path, const std::string &bfiles, const std::string &index_path, bool want_bim)
    {
        std::cout << "Checking paths" << std::endl;
        check_prep_paths(bfiles);
        check_path(phen_path);
        if (index_path != "NULL") check_path(index_path);
        check_bed_magic(bfiles);
        load_phen_dims(phen_path, bfiles, phen, dims, &trait_names);
        std::cout << "Found " << phen.num_phen << " phenotypes" << std::endl;
        if (phen.num_phen == 0 || m() == 0 || N() == 0) die("nothing to correlate");
        means = read_floats_line_range(bfiles + ".means", 0, std::numeric_limits<size_t>::max());
        stds = read_floats_line_range(bfiles + ".stds", 0, std::numeric_limits<size_t>::max());
        if (means.size() != m() || stds.size() != m()) die("number of markers and number of means or stds differ");
        map_bed(bed, bfiles, dims, m());
        if (want_bim)
        {  // columns 1, 2, 5 of the .bim: the `chr snp ref` columns of an mxp file
            std::ifstream f(bfiles + ".bim");
            std::string line;
            while (std::getline(f, line))
            {
                const auto w = split_ws(line);
                if (w.size() < 5) continue;
                chr.push_back(w[0]);
                snp.push_back(w[1]);
                ref.push_back(w[4]);
            }
            if (chr.size() != m()) die("number of markers in .bim and .dim differ");
        }
        if (index_path == "NULL")
        {
            ixs.resize(m());
            std::iota(ixs.begin(), ixs.end(), 0);
        }
        else
        {
            std::cout << "Loading marker indices" << std::endl;
            ixs = read_binary<int>(index_path);
            if (ixs.empty()) die("marker index file is empty");
            for (size_t i = 0; i < ixs.size(); i++)
                if (ixs[i] < 0 || (size_t)ixs[i] >= m() || (i > 0 && ixs[i] <= ixs[i - 1]))
                    die("marker indices must be ascending, distinct and smaller than the number of markers");
        }
        if (k() + p() > (size_t)std::numeric_limits<int>::max() / 2) die("too many variables");
    }

    void stage(cusk_engine *e)
    {
        if (const char *failed = stage_inputs(dev, bed.data + 3, m() * dims.bytes_per_col(), phen.data, means, stds, 0, &std::cout))
            engine_die(failed, e);
    }

    // n x n matrix (selected markers, then traits) built where the sweep reads it
    void build_square(cusk_engine *e, float *C_dev, float *mxp_host = nullptr)
    {
        if (cusk_corr_build_indexed(e, bed_rows(), dev.phen, ixs.data(), k(), m(), N(), p(), dev.means, dev.stds, C_dev, mxp_host) !=
            CUSK_OK)
            engine_die("correlation build", e);
    }

    ~GenoInputs() { dev.release(); }
};

}  // namespace host
