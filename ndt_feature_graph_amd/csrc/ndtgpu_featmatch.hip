// ndtgpu_featmatch.hip -- C-ABI (include/ndtgpu.h) of the feature-set RANSAC matcher: matchFeatureMap (ndt_feature_map.h:104-122;
// call sites ndt_feature_node.h:256, ndt_feature_graph.cpp:162-177, ndt_feature_fuser_hmt.cpp:251) for a batch of pairs of a bank
// of feature sets.  Host side only: the handle, the checks, the packing of a set into the bank's layout and the order of the
// launches; the matching runs in csrc/ndt_featmatch.hip.  The bank's sets are filled by ndtgpu_featbank_set or, from laser scans, by
// ndtgpu_featbank_extract* (detector_->detect + descriptor_->describe, ndt_feature2d_fuser.cpp:766-779; the kernel is
// csrc/ndt_featextract.hip).
#include "ndtgpu_featbank.h"
#include "ndt_featextract.h"

ndtgpu_status featmatch_params_dev(const char *what, const ndtgpu_featmatch_params *prm, NdtFeatMatchParamsDev &d)
{
    const ndtgpu_featmatch_params p = params_or_default(prm, ndtgpu_default_featmatch_params);
    if (const char *msg = ndt_featmatch_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, what, msg);
    d.acceptance_threshold = p.acceptance_threshold;
    d.inlier_probability = p.inlier_probability;
    d.distance_threshold = p.distance_threshold;
    d.rigidity_threshold = p.rigidity_threshold;
    d.seed = p.seed;
    d.n_hypotheses = ndt_featmatch_hypotheses(p.success_probability, p.inlier_probability);
    return NDTGPU_OK;
}

// the checks that need no handle, then the handle's shape
static ndtgpu_status featextract_params_dev(const char *what, const ndtgpu_featbank *h, size_t n_scans, size_t n_beams, double angle_min,
                                            double angle_increment, const ndtgpu_featextract_params *prm, NdtFeatExtractParamsDev &d)
{
    const ndtgpu_featextract_params p = params_or_default(prm, ndtgpu_default_featextract_params);
    const char *msg = ndt_featextract_check_args(n_scans, n_beams, angle_min, angle_increment);
    if (!msg) msg = ndt_featextract_check_params(p);
    if (msg) return fail_in(NDTGPU_ERR_INVALID, what, msg);
    if (!h) return fail_in(NDTGPU_ERR_INVALID, what, "null handle");
    if ((size_t)p.bin_rho * (size_t)p.bin_phi != h->v.desc_len)
        return fail_in(NDTGPU_ERR_INVALID, what, "the bank's desc_len must equal bin_rho * bin_phi");
    d = ndt_featextract_params_dev(p);
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_featextract_params(ndtgpu_featextract_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // flirtlib_utils.h:15-42: SimpleMinMaxPeakFinder(0.34, 0.001), CurvatureDetector(peak, 5, 0.2, 1.4, 2.0),
    // BetaGridGenerator(0.02, 1.0, 4, 12)
    p->scales = 5;
    p->base_sigma = 0.2;
    p->sigma_step = 1.4;
    p->dmst = 2.0;
    p->min_value = 0.34;
    p->min_diff = 0.001;
    p->min_rho = 0.02;
    p->max_rho = 1.0;
    p->bin_rho = 4;
    p->bin_phi = 12;
    p->min_separation = 0.2;         // (this project's: step 6)
    p->r_min = 0.5;                  // (the launch files' min and sensor range)
    p->r_max = 30.0;
}

void ndtgpu_default_featmatch_params(ndtgpu_featmatch_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // ndt_feature_map.h:104-122: RansacFeatureSetMatcher(0.0599, 0.9, 0.1, 0.6, 0.0499, false)
    p->acceptance_threshold = 0.0599;
    p->success_probability = 0.9;
    p->inlier_probability = 0.1;
    p->distance_threshold = 0.6;
    p->rigidity_threshold = 0.0499;
}

ndtgpu_status ndtgpu_featbank_destroy(ndtgpu_featbank *h) { return handle_destroy(h, "featbank_destroy"); }

ndtgpu_status ndtgpu_featbank_create(size_t n_sets, size_t max_points, size_t desc_len, ndtgpu_featbank **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "featbank_create: out is NULL");
    *out = nullptr;
    if (const char *msg = ndt_featmatch_check_shape(n_sets, max_points, desc_len)) return fail_in(NDTGPU_ERR_INVALID, "featbank_create", msg);
    ndtgpu_featbank *h;
    const ndtgpu_status rc = handle_new("featbank_create", h);
    if (rc != NDTGPU_OK) return rc;
    NdtFeatBankView &v = h->v;
    v.n_sets = (unsigned)n_sets;
    v.max_points = (unsigned)max_points;
    v.desc_len = (unsigned)desc_len;
    uint32_t *count = nullptr;
    double *pos = nullptr, *desc = nullptr;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "featbank_create: device buffers", expr)
    TRY(h->count.alloc(n_sets, &count));
    TRY(h->pos.alloc(n_sets * max_points * 3, &pos));
    TRY(h->desc.alloc(n_sets * desc_len * max_points, &desc));
    TRY(hipMemset(count, 0, n_sets * sizeof(uint32_t)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    v.count = count;
    v.pos = pos;
    v.desc = desc;
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_set(ndtgpu_featbank *h, size_t k, size_t n, const double *pos3, const double *desc)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_set: null handle");
    if (n > NDT_FEATMATCH_MAX_POINTS) return fail(NDTGPU_ERR_CAPACITY, "featbank_set: more points than a set can hold (1024)");
    if (n && (!pos3 || !desc)) return fail(NDTGPU_ERR_INVALID, "featbank_set: positions and descriptors are required");
    if (k >= h->v.n_sets) return fail(NDTGPU_ERR_INVALID, "featbank_set: set index out of range");
    if (n > h->v.max_points) return fail(NDTGPU_ERR_CAPACITY, "featbank_set: more points than the handle was created for");
    const NdtFeatBankView &v = h->v;
    const size_t MP = v.max_points, D = v.desc_len;
    const uint32_t cnt = (uint32_t)n;
    std::vector<double> packed(D * MP);
    ndt_featmatch_pack_desc(desc, n, D, MP, packed.data());
    hipStream_t st = h->hst.get();
    HIP_TRY(h->used.order(st));                                   // (a match may still read the set)
    if (n) HIP_TRY(hipMemcpyAsync(h->pos.get() + k * MP * 3, pos3, 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->desc.get() + k * D * MP, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->count.get() + k, &cnt, sizeof cnt, hipMemcpyHostToDevice, st));
    HIP_TRY(h->used.record(st));
    HIP_TRY(hipStreamSynchronize(st));                            // (the staging vector ends with this function)
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_match_device(ndtgpu_featbank *h, const uint32_t *ref_idx_dev, const uint32_t *mov_idx_dev,
                                           size_t n_pairs, const ndtgpu_featmatch_params *prm,
                                           ndtgpu_featmatch_result *results_dev, double *T16_dev, uint32_t *corr_dev,
                                           ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_match_device: null handle");
    if (n_pairs > (1u << 24)) return fail(NDTGPU_ERR_INVALID, "featbank_match_device: more than 2^24 pairs");
    if (n_pairs && (!ref_idx_dev || !mov_idx_dev || !results_dev))
        return fail(NDTGPU_ERR_INVALID, "featbank_match_device: indices and results are required");
    NdtFeatMatchParamsDev d;
    ndtgpu_status rc = featmatch_params_dev("featbank_match_device", prm, d);
    if (rc != NDTGPU_OK) return rc;
    if (!n_pairs) return NDTGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));   // (the previous call may have run on another stream)
    hipError_t e = ndt_featmatch_launch(h->v, ref_idx_dev, mov_idx_dev, n_pairs, d, results_dev, T16_dev, corr_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "featbank_match_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_match(ndtgpu_featbank *h, const uint32_t *ref_idx, const uint32_t *mov_idx, size_t n_pairs,
                                    const ndtgpu_featmatch_params *prm, ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_match: null handle");
    if (n_pairs > (1u << 24)) return fail(NDTGPU_ERR_INVALID, "featbank_match: more than 2^24 pairs");
    if (n_pairs && (!ref_idx || !mov_idx)) return fail(NDTGPU_ERR_INVALID, "featbank_match: indices are required");
    NdtFeatMatchParamsDev d;
    ndtgpu_status rc = featmatch_params_dev("featbank_match", prm, d);
    if (rc != NDTGPU_OK) return rc;
    h->n_last = 0;
    if (!n_pairs) return NDTGPU_OK;
    // (the buffers that grow may still be in use by the previous call)
    HIP_TRY(h->idx.reserve(2 * n_pairs, h->used));
    HIP_TRY(h->results.reserve(n_pairs, h->used));
    HIP_TRY(h->T16.reserve(16 * n_pairs, h->used));
    HIP_TRY(h->corr.reserve(n_pairs * h->v.max_points * 2, h->used));
    HIP_TRY(h->used.sync());                                      // (the pinned indices of the previous call have been copied)
    HIP_TRY(h->idx_pin.reserve(2 * n_pairs));
    memcpy(h->idx_pin.get(), ref_idx, n_pairs * sizeof(uint32_t));
    memcpy(h->idx_pin.get() + n_pairs, mov_idx, n_pairs * sizeof(uint32_t));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->idx.get(), h->idx_pin.get(), 2 * n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipError_t e = ndt_featmatch_launch(h->v, h->idx.get(), h->idx.get() + n_pairs, n_pairs, d, h->results.get(), h->T16.get(),
                                        h->corr.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "featbank_match: launch", e);
    HIP_TRY(h->used.record(st));
    h->n_last = n_pairs;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_results(ndtgpu_featbank *h, size_t first, size_t count, ndtgpu_featmatch_result *results, double *T16,
                                      uint32_t *corr)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_results: null handle");
    if (first > h->n_last || count > h->n_last - first)
        return fail(NDTGPU_ERR_INVALID, "featbank_results: pairs [first, first + count) are not of the last match");
    if (!count) return NDTGPU_OK;
    HIP_TRY(h->used.sync());
    const size_t MP = h->v.max_points;
    if (results) HIP_TRY(hipMemcpy(results, h->results.get() + first, count * sizeof *results, hipMemcpyDeviceToHost));
    if (T16) HIP_TRY(hipMemcpy(T16, h->T16.get() + 16 * first, 16 * count * sizeof(double), hipMemcpyDeviceToHost));
    if (corr) HIP_TRY(hipMemcpy(corr, h->corr.get() + first * MP * 2, count * MP * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_extract_device(ndtgpu_featbank *h, const uint32_t *set_idx_dev, const double *ranges_dev, size_t n_scans,
                                             size_t n_beams, double angle_min, double angle_increment,
                                             const ndtgpu_featextract_params *prm, ndtgpu_featextract_result *results_dev,
                                             uint32_t *beam_dev, int32_t *level_dev, double *response_dev, ndtgpu_stream stream)
{
    if (n_scans && (!set_idx_dev || !ranges_dev || !results_dev))
        return fail(NDTGPU_ERR_INVALID, "featbank_extract_device: set indices, ranges and results are required");
    NdtFeatExtractParamsDev d;
    ndtgpu_status rc = featextract_params_dev("featbank_extract_device", h, n_scans, n_beams, angle_min, angle_increment, prm, d);
    if (rc != NDTGPU_OK) return rc;
    if (!n_scans) return NDTGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));   // (a match on another stream may still read the sets)
    hipError_t e = ndt_featextract_launch(h->v, h->count.get(), h->pos.get(), h->desc.get(), set_idx_dev, ranges_dev, n_scans, n_beams,
                                          angle_min, angle_increment, d, results_dev, beam_dev, level_dev, response_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "featbank_extract_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_extract(ndtgpu_featbank *h, const uint32_t *set_idx, const double *ranges, size_t n_scans, size_t n_beams,
                                      double angle_min, double angle_increment, const ndtgpu_featextract_params *prm,
                                      ndtgpu_stream stream)
{
    if (n_scans && (!set_idx || !ranges)) return fail(NDTGPU_ERR_INVALID, "featbank_extract: set indices and ranges are required");
    NdtFeatExtractParamsDev d;
    ndtgpu_status rc = featextract_params_dev("featbank_extract", h, n_scans, n_beams, angle_min, angle_increment, prm, d);
    if (rc != NDTGPU_OK) return rc;
    h->n_last_extract = 0;
    if (!n_scans) return NDTGPU_OK;
    const size_t MP = h->v.max_points;
    // (the buffers that grow may still be in use by the previous call)
    HIP_TRY(h->ex_idx.reserve(n_scans, h->used));
    HIP_TRY(h->ex_ranges.reserve(n_scans * n_beams, h->used));
    HIP_TRY(h->ex_results.reserve(n_scans, h->used));
    HIP_TRY(h->ex_beam.reserve(n_scans * MP, h->used));
    HIP_TRY(h->ex_level.reserve(n_scans * MP, h->used));
    HIP_TRY(h->ex_response.reserve(n_scans * MP, h->used));
    HIP_TRY(h->used.sync());                                      // (the pinned inputs of the previous call have been copied)
    HIP_TRY(h->ex_idx_pin.reserve(n_scans));
    HIP_TRY(h->ex_ranges_pin.reserve(n_scans * n_beams));
    memcpy(h->ex_idx_pin.get(), set_idx, n_scans * sizeof(uint32_t));
    memcpy(h->ex_ranges_pin.get(), ranges, n_scans * n_beams * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->ex_idx.get(), h->ex_idx_pin.get(), n_scans * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ex_ranges.get(), h->ex_ranges_pin.get(), n_scans * n_beams * sizeof(double), hipMemcpyHostToDevice, st));
    hipError_t e = ndt_featextract_launch(h->v, h->count.get(), h->pos.get(), h->desc.get(), h->ex_idx.get(), h->ex_ranges.get(), n_scans,
                                          n_beams, angle_min, angle_increment, d, h->ex_results.get(), h->ex_beam.get(),
                                          h->ex_level.get(), h->ex_response.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "featbank_extract: launch", e);
    HIP_TRY(h->used.record(st));
    h->n_last_extract = n_scans;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_extract_results(ndtgpu_featbank *h, size_t first, size_t count, ndtgpu_featextract_result *results,
                                              uint32_t *beam, int32_t *level, double *response)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_extract_results: null handle");
    if (first > h->n_last_extract || count > h->n_last_extract - first)
        return fail(NDTGPU_ERR_INVALID, "featbank_extract_results: scans [first, first + count) are not of the last extraction");
    if (!count) return NDTGPU_OK;
    HIP_TRY(h->used.sync());
    const size_t MP = h->v.max_points;
    if (results) HIP_TRY(hipMemcpy(results, h->ex_results.get() + first, count * sizeof *results, hipMemcpyDeviceToHost));
    if (beam) HIP_TRY(hipMemcpy(beam, h->ex_beam.get() + first * MP, count * MP * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (level) HIP_TRY(hipMemcpy(level, h->ex_level.get() + first * MP, count * MP * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (response) HIP_TRY(hipMemcpy(response, h->ex_response.get() + first * MP, count * MP * sizeof(double), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_get(ndtgpu_featbank *h, size_t k, size_t *n, double *pos3, double *desc)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_get: null handle");
    if (!n) return fail(NDTGPU_ERR_INVALID, "featbank_get: n is NULL");
    *n = 0;
    if (k >= h->v.n_sets) return fail(NDTGPU_ERR_INVALID, "featbank_get: set index out of range");
    HIP_TRY(h->used.sync());
    const size_t MP = h->v.max_points, D = h->v.desc_len;
    uint32_t cnt = 0;
    HIP_TRY(hipMemcpy(&cnt, h->count.get() + k, sizeof cnt, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cnt, MP);
    if (m && pos3) HIP_TRY(hipMemcpy(pos3, h->pos.get() + k * MP * 3, 3 * m * sizeof(double), hipMemcpyDeviceToHost));
    if (m && desc) {
        std::vector<double> packed(D * MP);
        HIP_TRY(hipMemcpy(packed.data(), h->desc.get() + k * D * MP, packed.size() * sizeof(double), hipMemcpyDeviceToHost));
        ndt_featextract_unpack_desc(packed.data(), m, D, MP, desc);
    }
    *n = m;
    return NDTGPU_OK;
}

}   // extern "C"
