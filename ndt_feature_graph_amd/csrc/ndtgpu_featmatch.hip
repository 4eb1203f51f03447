// ndtgpu_featmatch.hip -- C-ABI (include/ndtgpu.h) of the feature-set RANSAC matcher: matchFeatureMap (ndt_feature_map.h:104-122;
// call sites ndt_feature_node.h:256, ndt_feature_graph.cpp:162-177, ndt_feature_fuser_hmt.cpp:251) for a batch of pairs of a bank
// of feature sets.  Host side only: the handle, the checks, the packing of a set into the bank's layout and the order of the
// launches; the matching runs in csrc/ndt_featmatch.hip.
#include "ndtgpu_host.h"
#include "ndt_featmatch.h"

#include <new>

struct ndtgpu_featbank {
    NdtFeatBankView v{};                   // what the kernel receives: filled from the owners below at create
    DeviceBuffer<uint32_t> count;
    DeviceBuffer<double> pos, desc;
    // the last host-index match: its indices and outputs
    size_t n_last = 0;
    DeviceBuffer<uint32_t> idx, corr;      // idx: ref indices, then mov indices
    DeviceBuffer<ndtgpu_featmatch_result> results;
    DeviceBuffer<double> T16;
    PinnedBuffer<uint32_t> idx_pin;
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // set's copies (last: ndtgpu_resource.h)
};

static ndtgpu_status featmatch_params_dev(const char *what, const ndtgpu_featmatch_params *prm, NdtFeatMatchParamsDev &d)
{
    ndtgpu_featmatch_params p;
    ndtgpu_default_featmatch_params(&p);
    if (prm) p = *prm;
    if (const char *msg = ndt_featmatch_check_params(p)) return fail(NDTGPU_ERR_INVALID, (std::string(what) + ": " + msg).c_str());
    d.acceptance_threshold = p.acceptance_threshold;
    d.inlier_probability = p.inlier_probability;
    d.distance_threshold = p.distance_threshold;
    d.rigidity_threshold = p.rigidity_threshold;
    d.seed = p.seed;
    d.n_hypotheses = ndt_featmatch_hypotheses(p.success_probability, p.inlier_probability);
    return NDTGPU_OK;
}

extern "C" {

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

ndtgpu_status ndtgpu_featbank_destroy(ndtgpu_featbank *h)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "featbank_destroy: null");
    (void)h->used.sync();                  // (the last call may have run on a stream of the caller's)
    delete h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_featbank_create(size_t n_sets, size_t max_points, size_t desc_len, ndtgpu_featbank **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "featbank_create: out is NULL");
    *out = nullptr;
    if (const char *msg = ndt_featmatch_check_shape(n_sets, max_points, desc_len))
        return fail(NDTGPU_ERR_INVALID, (std::string("featbank_create: ") + msg).c_str());
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "featbank_create: no HIP device");
    ndtgpu_featbank *h = new (std::nothrow) ndtgpu_featbank();
    if (!h) return fail(NDTGPU_ERR_ALLOC, "featbank_create: host alloc");
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

}   // extern "C"
