// engine_util.h -- what every host command that talks to the engine needs: the error type of a failed engine call, the one
// place an engine is opened, a device matrix, and the two read-backs (adjacency bitmap, gathered sub-matrix).  Host code
// against the C ABI only.
#pragma once
#include <stdexcept>
#include <string>

#include "result_types.h"

namespace host {

// a failed engine call: the CLI prints the message and exits with EXIT_FAILURE (gpuerrors.h:6-15), the library
// entry points return CUSK_ERR_* with the message retrievable
struct EngineError : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

[[noreturn]] inline void engine_die(const char *what, cusk_engine *e)
{
    throw EngineError(std::string(what) + ": " + (e ? cusk_last_error(e) : "no engine"));
}

// the engine of an `mps` command: device 0, its own stream
inline cusk_engine *open_engine()
{
    cusk_engine *e = nullptr;
    if (cusk_engine_create(&e, 0, nullptr) != CUSK_OK) engine_die("engine create (is a HIP device visible?)", nullptr);
    return e;
}

inline Bits fetch_adjacency(cusk_engine *e)
{
    Bits b;
    b.n = cusk_result_n(e);
    b.words = cusk_result_words(e);
    b.w.resize((size_t)b.n * b.words);
    if (cusk_engine_download(e, b.w.data(), cusk_result_adj_bits_dev(e), b.w.size() * sizeof(uint64_t)) != CUSK_OK)
        engine_die("adjacency download", e);
    return b;
}

inline std::vector<float> gather(cusk_engine *e, const float *M_dev, int n, const std::vector<int> &P)
{
    std::vector<float> out(P.size() * P.size());
    if (cusk_gather_submatrix(e, M_dev, n, P.data(), (int)P.size(), out.data()) != CUSK_OK) engine_die("gather", e);
    return out;
}

// device matrix that is reused from block to block (grows, never shrinks)
struct DevMat
{
    float *p = nullptr;
    size_t cap = 0;
    DevMat() = default;
    explicit DevMat(size_t count) { reserve(count); }
    DevMat(const std::vector<float> &h) { upload(h); }
    void reserve(size_t count)
    {
        if (count <= cap) return;
        cusk_dev_free(p);
        p = static_cast<float *>(cusk_dev_alloc(sizeof(float) * count));
        cap = p ? count : 0;
        if (!p) throw EngineError("device allocation of " + std::to_string(sizeof(float) * count) + " bytes failed");
    }
    void upload(const std::vector<float> &h)
    {
        reserve(h.size());
        if (cusk_dev_upload(p, h.data(), sizeof(float) * h.size()) != CUSK_OK) throw EngineError("device upload failed");
    }
    ~DevMat() { cusk_dev_free(p); }
    DevMat(const DevMat &) = delete;
    DevMat &operator=(const DevMat &) = delete;
};

}  // namespace host
