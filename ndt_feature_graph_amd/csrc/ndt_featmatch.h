// ndt_featmatch.h -- what the feature-set RANSAC matcher's kernel (csrc/ndt_featmatch.hip) and its C-ABI (csrc/ndtgpu_featmatch.hip)
// share: the device view of a bank of feature sets, the sample draws, and the host-side packing of a set.
// tests/featmatch_model.py restates the algorithm (include/ndtgpu.h "feature-set RANSAC matching", steps 1-8) in NumPy.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_mcl.h"   // ndt_hash_uniform: the counter-based uniform of the sample draws

#define NDT_FEATMATCH_THREADS 256                 // one workgroup per pair of sets
#define NDT_FEATMATCH_WAVES (NDT_FEATMATCH_THREADS / 64)
#define NDT_FEATMATCH_MAX_POINTS 1024             // positions of both sets in LDS: 2 x 16 KB
#define NDT_FEATMATCH_MAX_DESC 128                // bins of a descriptor
#define NDT_FEATMATCH_TILE 16                     // ref descriptors of an LDS tile: 16 accumulators per lane
#define NDT_FEATMATCH_FAIL_SCORE 1e17

struct NdtFeatMatchParamsDev {
    double acceptance_threshold, inlier_probability, distance_threshold, rigidity_threshold;
    unsigned long long seed;
    int n_hypotheses;
};

// a bank of n_sets feature sets, every array with room for max_points per set
struct NdtFeatBankView {
    unsigned n_sets, max_points, desc_len;
    const uint32_t *count;                        // [n_sets]                        points of a set
    const double *pos;                            // [n_sets][max_points][3]         (x, y, theta)
    const double *desc;                           // [n_sets][desc_len][max_points]  TRANSPOSED: bin k of point i at k * max_points + i,
                                                  //                                 so lanes over points read a bin coalesced
};

// H of step 3; 0 where the parameters give none or more than 2^20
inline int ndt_featmatch_hypotheses(double success_probability, double inlier_probability)
{
    const double h = ceil(log(1.0 - success_probability) / log(1.0 - inlier_probability * inlier_probability));
    return (h >= 1.0 && h <= 1048576.0) ? (int)h : 0;
}

// the two candidates of hypothesis h among n_c >= 2 (step 3)
NDT_HD void ndt_featmatch_sample(unsigned long long seed, unsigned h, unsigned n_c, unsigned &a, unsigned &b)
{
#pragma clang fp contract(off)
    a = (unsigned)(ndt_hash_uniform(seed, 0, h) * (double)n_c);
    b = (unsigned)(ndt_hash_uniform(seed, 1, h) * (double)(n_c - 1));
    if (b >= a) b++;
}

// host-side packing of one set into the bank's layout: desc (n x desc_len row-major) -> out ([desc_len][max_points]); the
// columns n .. max_points stay zero
inline void ndt_featmatch_pack_desc(const double *desc, size_t n, size_t desc_len, size_t max_points, double *out)
{
    for (size_t k = 0; k < desc_len; k++) {
        for (size_t i = 0; i < n; i++) out[k * max_points + i] = desc[i * desc_len + k];
        for (size_t i = n; i < max_points; i++) out[k * max_points + i] = 0.0;
    }
}

// what ndtgpu_featbank_create / _set check before the handle is read and the device is looked for; NULL: fine, else the message
inline const char *ndt_featmatch_check_shape(size_t n_sets, size_t max_points, size_t desc_len)
{
    if (n_sets == 0 || n_sets > (1u << 24)) return "n_sets must be 1 .. 2^24";
    if (max_points == 0 || max_points > NDT_FEATMATCH_MAX_POINTS) return "max_points must be 1 .. 1024";
    if (desc_len == 0 || desc_len > NDT_FEATMATCH_MAX_DESC) return "desc_len must be 1 .. 128";
    return nullptr;
}
inline const char *ndt_featmatch_check_params(const ndtgpu_featmatch_params &p)
{
    if (p.adaptive != 0) return "the adaptive matcher is not offered (adaptive must be 0)";
    const bool ok = p.acceptance_threshold >= 0.0 && p.acceptance_threshold < 1e300 && p.distance_threshold >= 0.0 &&
                    p.distance_threshold < 1e300 && p.rigidity_threshold >= 0.0 && p.rigidity_threshold < 1e300 &&
                    p.success_probability > 0.0 && p.success_probability < 1.0 && p.inlier_probability > 0.0 &&
                    p.inlier_probability < 1.0;                          // (NaN fails)
    if (!ok) return "bad parameter (thresholds finite and >= 0, probabilities inside (0, 1))";
    if (!ndt_featmatch_hypotheses(p.success_probability, p.inlier_probability)) return "the probabilities give no or more than 2^20 hypotheses";
    return nullptr;
}

// host launcher (csrc/ndt_featmatch.hip): n_pairs workgroups of one launch.  T16 and corr may be NULL.
hipError_t ndt_featmatch_launch(const NdtFeatBankView &v, const uint32_t *ref_idx_dev, const uint32_t *mov_idx_dev, size_t n_pairs,
                                const NdtFeatMatchParamsDev &prm, ndtgpu_featmatch_result *results_dev, double *T16_dev,
                                uint32_t *corr_dev, hipStream_t st);
