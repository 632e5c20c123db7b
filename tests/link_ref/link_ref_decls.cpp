// Link boundary without the reference checkout: the same calls as link_ref_headers.cpp, against this project's own
// declarations of the reference's entry points (the signatures csrc/compat_cxx.cpp and compat_api.hip define).  The
// test checks that this TU refers to exactly the library symbols a TU built on the reference's own headers refers to
// (tests/golden/ref_link_symbols.json, written by tests/golden/make_link_golden.py), then links and runs it.
#include <cstddef>
#include <cstdio>
#include <vector>

void cu_marker_phen_corr_pearson(const unsigned char *marker_vals, const float *phen_vals, const size_t num_markers,
                                 const size_t num_individuals, const size_t num_phen, const float *marker_mean,
                                 const float *marker_std, float *marker_phen_corrs);
void cu_corr_pearson_npn(const unsigned char *marker_vals, const float *phen_vals, const size_t num_markers,
                         const size_t num_individuals, const size_t num_phen, const float *marker_mean,
                         const float *marker_std, float *marker_corrs, float *marker_phen_corrs, float *phen_corrs);
std::vector<float> threshold_array(const int n, const float alpha);
float hetcor_threshold(const float alpha);
float std_normal_qnorm(const float p);
extern "C" void Skeleton(float *C, int *P, int *G, float *Th, int *l, const int *maxlevel, float *pMax, int *SepSet);
extern "C" void hetcor_skeleton(float *C, int *P, int *G, float *N, float *Th, int *l, const int *maxlevel,
                                const int *time_index);

int main()
{
    const std::vector<float> thr = threshold_array(500000, 1e-8f);
    std::printf("%zu %.9g %.9g %.9g\n", thr.size(), thr[0], hetcor_threshold(1e-4f), std_normal_qnorm(0.025f));
    void (*f1)(const unsigned char *, const float *, const size_t, const size_t, const size_t, const float *, const float *,
               float *) = &cu_marker_phen_corr_pearson;
    void (*f2)(const unsigned char *, const float *, const size_t, const size_t, const size_t, const float *, const float *,
               float *, float *, float *) = &cu_corr_pearson_npn;
    void (*f3)(float *, int *, int *, float *, int *, const int *, float *, int *) = &Skeleton;
    void (*f4)(float *, int *, int *, float *, float *, int *, const int *, const int *) = &hetcor_skeleton;
    std::printf("%d\n", (f1 != nullptr) + (f2 != nullptr) + (f3 != nullptr) + (f4 != nullptr));
    return 0;
}
