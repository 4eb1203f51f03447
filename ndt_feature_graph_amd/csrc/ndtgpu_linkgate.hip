// ndtgpu_linkgate.hip -- C-ABI (include/ndtgpu.h "link gating") of the step that decides which loop-closure links exist: the
// candidate pairs of computeAllPossibleLinks (ndt_feature_graph.cpp:395-405) gated by index distance and odometry, and
// getValidLinks (ndt_feature_graph.cpp:527-556) of the registered links, with the gather that packs what stays behind the
// incremental links for ndtgpu_pgo_set_links_device.  Host side only: the handle, the argument checks and the order of the
// launches; the selection runs in csrc/ndt_linkgate.hip.
#include "ndtgpu_host.h"
#include "ndt_linkgate.h"

struct ndtgpu_linkgate {
    size_t max_nodes = 0, max_links = 0;
    NdtLinkGateView v{};                   // what the kernels receive: filled from the owners below at create
    DeviceBuffer<double> nodes;
    DeviceBuffer<uint32_t> tile, total, keep;
    int last = -1;                         // which total the last selection wrote: 0 candidates, 1 valid
    size_t last_capacity = 0;              // ... and the capacity it was given (SIZE_MAX: none)
    bool have_keep = false;                // a valid call has been made
    size_t keep_links = 0;                 // ... over this many links
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the synchronous entries' stream (last: ndtgpu_resource.h)
};

static NdtLinkGateParamsDev linkgate_params_dev(const ndtgpu_linkgate_params *prm)
{
    const ndtgpu_linkgate_params p = params_or_default(prm, ndtgpu_default_linkgate_params);
    NdtLinkGateParamsDev d;
    d.max_score = p.max_score;
    d.max_dist = p.max_dist;
    d.max_angle = p.max_angle;
    d.min_idx_dist = p.min_idx_dist;
    d.clip_cosine = p.clip_cosine != 0;
    return d;
}

extern "C" {

void ndtgpu_default_linkgate_params(ndtgpu_linkgate_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_score = 0.1;                    // ndt_feature_graph_opt.cpp:49-52
    p->max_dist = 1.0;
    p->max_angle = 0.2;
    p->min_idx_dist = 2;
    p->clip_cosine = 0;                    // upstream's acos of an unclipped cosine
}

ndtgpu_status ndtgpu_linkgate_check(size_t max_nodes, size_t max_links, size_t n_nodes, size_t n_links, size_t row_bytes)
{
    if (max_nodes == 0 || max_nodes > NDT_LINKGATE_MAX_NODES || max_links > NDT_LINKGATE_MAX_LINKS)
        return fail(NDTGPU_ERR_INVALID, "linkgate: max_nodes must be 1 .. 65536, max_links <= 2^27");
    if (n_nodes > max_nodes) return fail(NDTGPU_ERR_CAPACITY, "linkgate: more nodes than the handle was created for");
    if (n_links > max_links) return fail(NDTGPU_ERR_CAPACITY, "linkgate: more links than the handle was created for");
    if (row_bytes % 4 != 0 || row_bytes > NDT_LINKGATE_MAX_ROW_BYTES)
        return fail(NDTGPU_ERR_INVALID, "linkgate: row_bytes must be a multiple of 4, at most 4096");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_create(size_t max_nodes, size_t max_links, ndtgpu_linkgate **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "linkgate_create: out is NULL");
    *out = nullptr;
    ndtgpu_status rc = ndtgpu_linkgate_check(max_nodes, max_links, 0, 0, 0);
    if (rc != NDTGPU_OK) return rc;
    ndtgpu_linkgate *h;
    if ((rc = handle_new("linkgate_create", h)) != NDTGPU_OK) return rc;
    h->max_nodes = max_nodes;
    h->max_links = max_links;
    const size_t pairs = max_nodes * (max_nodes - 1) / 2;
    const size_t tiles = (std::max(pairs, max_links) + NDT_LINKGATE_TILE - 1) / NDT_LINKGATE_TILE;
    NdtLinkGateView &v = h->v;
    double *nodes = nullptr;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "linkgate_create: device buffers", expr)
    TRY(h->nodes.alloc(16 * max_nodes, &nodes));
    TRY(h->tile.alloc(std::max<size_t>(tiles, 1), &v.tile));                 // (no zero-byte allocations)
    TRY(h->total.alloc(2, &v.total));
    TRY(h->keep.alloc(std::max<size_t>(max_links, 1), &v.keep));
    TRY(hipMemset(v.total, 0, 2 * sizeof(uint32_t)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    v.nodes = nodes;
    v.n_nodes = 0;
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_destroy(ndtgpu_linkgate *h) { return handle_destroy(h, "linkgate_destroy"); }

ndtgpu_status ndtgpu_linkgate_set_nodes(ndtgpu_linkgate *h, size_t n_nodes, const double *T16)
{
    if (n_nodes && !T16) return fail(NDTGPU_ERR_INVALID, "linkgate_set_nodes: null poses");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_set_nodes: null handle");
    const ndtgpu_status rc = ndtgpu_linkgate_check(h->max_nodes, h->max_links, n_nodes, 0, 0);
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(h->used.order(h->hst.get()));
    if (n_nodes)
        HIP_TRY(hipMemcpyAsync(h->nodes.get(), T16, 16 * n_nodes * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    h->v.n_nodes = (uint32_t)n_nodes;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_set_nodes_device(ndtgpu_linkgate *h, size_t n_nodes, const double *T16_dev, ndtgpu_stream stream)
{
    if (n_nodes && !T16_dev) return fail(NDTGPU_ERR_INVALID, "linkgate_set_nodes_device: null poses");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_set_nodes_device: null handle");
    const ndtgpu_status rc = ndtgpu_linkgate_check(h->max_nodes, h->max_links, n_nodes, 0, 0);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));
    if (n_nodes)
        HIP_TRY(hipMemcpyAsync(h->nodes.get(), T16_dev, 16 * n_nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(h->used.record(st));
    h->v.n_nodes = (uint32_t)n_nodes;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_candidates(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, uint32_t *ref_idx_dev,
                                         uint32_t *mov_idx_dev, double *T16_dev, size_t capacity, ndtgpu_stream stream)
{
    if (capacity && (!ref_idx_dev || !mov_idx_dev)) return fail(NDTGPU_ERR_INVALID, "linkgate_candidates: null index output");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_candidates: null handle");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));            // (the previous call may have run on another stream)
    const hipError_t e = ndt_linkgate_launch_candidates(h->v, linkgate_params_dev(prm), ref_idx_dev, mov_idx_dev, T16_dev, capacity, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "linkgate_candidates: launch", e);
    HIP_TRY(h->used.record(st));
    h->last = 0;
    h->last_capacity = capacity;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_valid(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, size_t n_links, const uint32_t *ref_idx_dev,
                                    const uint32_t *mov_idx_dev, const double *T16_dev, const double *score_dev, uint32_t *keep_dev,
                                    size_t capacity, ndtgpu_stream stream)
{
    if (n_links && (!ref_idx_dev || !mov_idx_dev || !T16_dev))
        return fail(NDTGPU_ERR_INVALID, "linkgate_valid: null link indices or poses");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_valid: null handle");
    const ndtgpu_status rc = ndtgpu_linkgate_check(h->max_nodes, h->max_links, 0, n_links, 0);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));
    const hipError_t e = ndt_linkgate_launch_valid(h->v, linkgate_params_dev(prm), n_links, ref_idx_dev, mov_idx_dev, T16_dev, score_dev,
                                                   keep_dev, capacity, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "linkgate_valid: launch", e);
    HIP_TRY(h->used.record(st));
    h->last = 1;
    h->last_capacity = keep_dev ? capacity : SIZE_MAX;
    h->have_keep = true;
    h->keep_links = n_links;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_candidates_host(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, uint32_t *ref_idx, uint32_t *mov_idx,
                                              double *T16, size_t capacity)
{
    if (capacity && (!ref_idx || !mov_idx)) return fail(NDTGPU_ERR_INVALID, "linkgate_candidates_host: null index output");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_candidates_host: null handle");
    const size_t n = h->v.n_nodes, cap = std::min(capacity, n * (n ? n - 1 : 0) / 2);
    DeviceBuffer<uint32_t> ref_dev, mov_dev;                  // temporaries: gone on return
    DeviceBuffer<double> T_dev;
    if (cap) {
        if (ref_dev.alloc(cap) != hipSuccess || mov_dev.alloc(cap) != hipSuccess || (T16 && T_dev.alloc(16 * cap) != hipSuccess))
            return fail(NDTGPU_ERR_ALLOC, "linkgate_candidates_host: device buffers");
    }
    ndtgpu_status rc = ndtgpu_linkgate_candidates(h, prm, ref_dev.get(), mov_dev.get(), T_dev.get(), cap, (ndtgpu_stream)h->hst.get());
    if (rc != NDTGPU_OK) return rc;
    size_t count = 0;
    if ((rc = ndtgpu_linkgate_count(h, &count, nullptr)) != NDTGPU_OK) return rc;
    h->last_capacity = capacity;                              // (what the caller gave, not what the temporaries held)
    const size_t m = std::min(count, cap);
    if (m) {
        HIP_TRY(hipMemcpy(ref_idx, ref_dev.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(mov_idx, mov_dev.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (T16) HIP_TRY(hipMemcpy(T16, T_dev.get(), 16 * m * sizeof(double), hipMemcpyDeviceToHost));
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_valid_host(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, size_t n_links, const uint32_t *ref_idx,
                                         const uint32_t *mov_idx, const double *T16, const double *score)
{
    if (n_links && (!ref_idx || !mov_idx || !T16)) return fail(NDTGPU_ERR_INVALID, "linkgate_valid_host: null link indices or poses");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_valid_host: null handle");
    ndtgpu_status rc = ndtgpu_linkgate_check(h->max_nodes, h->max_links, 0, n_links, 0);
    if (rc != NDTGPU_OK) return rc;
    DeviceBuffer<uint32_t> ref_dev, mov_dev;                  // temporaries: gone on return
    DeviceBuffer<double> T_dev, score_dev;
    hipStream_t st = h->hst.get();
    if (n_links) {
        if (ref_dev.alloc(n_links) != hipSuccess || mov_dev.alloc(n_links) != hipSuccess || T_dev.alloc(16 * n_links) != hipSuccess ||
            (score && score_dev.alloc(n_links) != hipSuccess))
            return fail(NDTGPU_ERR_ALLOC, "linkgate_valid_host: device buffers");
        HIP_TRY(hipMemcpyAsync(ref_dev.get(), ref_idx, n_links * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mov_dev.get(), mov_idx, n_links * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(T_dev.get(), T16, 16 * n_links * sizeof(double), hipMemcpyHostToDevice, st));
        if (score) HIP_TRY(hipMemcpyAsync(score_dev.get(), score, n_links * sizeof(double), hipMemcpyHostToDevice, st));
    }
    rc = ndtgpu_linkgate_valid(h, prm, n_links, ref_dev.get(), mov_dev.get(), T_dev.get(), score_dev.get(), nullptr, 0, (ndtgpu_stream)st);
    HIP_TRY(hipStreamSynchronize(st));                        // (the temporaries are read until here)
    return rc;
}

ndtgpu_status ndtgpu_linkgate_gather(ndtgpu_linkgate *h, const void *src_dev, size_t row_bytes, void *dst_dev, size_t dst_first_row,
                                     ndtgpu_stream stream)
{
    if (!src_dev || !dst_dev) return fail(NDTGPU_ERR_INVALID, "linkgate_gather: null source or destination");
    if (row_bytes == 0 || row_bytes % 4 != 0 || row_bytes > NDT_LINKGATE_MAX_ROW_BYTES)
        return fail(NDTGPU_ERR_INVALID, "linkgate_gather: row_bytes must be a multiple of 4, 4 .. 4096");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_gather: null handle");
    if (!h->have_keep) return fail(NDTGPU_ERR_INVALID, "linkgate_gather: no ndtgpu_linkgate_valid call has been made");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));
    const hipError_t e = ndt_linkgate_launch_gather(h->v, h->keep_links, (const uint32_t *)src_dev, row_bytes / 4, (uint32_t *)dst_dev,
                                                    dst_first_row, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "linkgate_gather: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_count(ndtgpu_linkgate *h, size_t *count, int32_t *overflow)
{
    if (!count) return fail(NDTGPU_ERR_INVALID, "linkgate_count: null count");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_count: null handle");
    if (h->last < 0) return fail(NDTGPU_ERR_INVALID, "linkgate_count: no candidates or valid call has been made");
    HIP_TRY(h->used.sync());
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, h->v.total + h->last, sizeof n, hipMemcpyDeviceToHost));
    *count = n;
    if (overflow) *overflow = (size_t)n > h->last_capacity ? 1 : 0;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_linkgate_keep(ndtgpu_linkgate *h, size_t first, size_t n, uint32_t *keep)
{
    if (n && !keep) return fail(NDTGPU_ERR_INVALID, "linkgate_keep: null output");
    if (!h) return fail(NDTGPU_ERR_INVALID, "linkgate_keep: null handle");
    if (!h->have_keep) return fail(NDTGPU_ERR_INVALID, "linkgate_keep: no ndtgpu_linkgate_valid call has been made");
    HIP_TRY(h->used.sync());
    uint32_t kept = 0;
    HIP_TRY(hipMemcpy(&kept, h->v.total + 1, sizeof kept, hipMemcpyDeviceToHost));
    if (first > kept || n > kept - first) return fail(NDTGPU_ERR_INVALID, "linkgate_keep: [first, first + n) beyond the kept links");
    if (n) HIP_TRY(hipMemcpy(keep, h->v.keep + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

}   // extern "C"
