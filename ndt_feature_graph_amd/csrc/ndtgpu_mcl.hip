// ndtgpu_mcl.hip -- C-ABI (include/ndtgpu.h) of the NDT Monte Carlo localisation bank: NDTMCL3D (perception_oru's ndt_mcl) for
// n_filters independent filters in borrowed NDT maps (call sites ndt_feature/src/ndt_feature_mcl_node.cpp:174-184, 335, 361,
// 377-396).  Host side only: handle, staging and the order of the launches; the local scan maps are built by the library's build
// kernels (mapset_build_core), everything else runs in csrc/ndt_mcl.hip.
#include "ndtgpu_host.h"
#include "ndt_mcl.h"

#include <new>

struct ndtgpu_mcl {
    ndtgpu_mapset *map = nullptr;          // borrowed
    ndtgpu_mcl_params prm{};
    size_t F = 0;
    unsigned N = 0;
    unsigned chunk = 0, n_chunks = 0;      // scan cells per likelihood chunk, chunks per filter (fixed per handle)
    // what the kernels receive: plain pointers, filled from the owners below at create
    uint32_t *map_idx = nullptr;           // device [F]
    rigid *T = nullptr, *T_tmp = nullptr;  // device [F][N]
    double *w = nullptr, *lik = nullptr;   // device [F][N]
    double *partial = nullptr;             // device [F][n_chunks][N]
    long long *cum = nullptr;              // device [F][N]
    NdtMclState *state = nullptr;          // device [F]
    NdtMclMotion *motion = nullptr;        // device [F]
    double *pose12 = nullptr;              // device [F][12]
    double *mean16 = nullptr;              // device [F][16]
    DeviceBuffer<uint32_t> map_idx_buf;
    DeviceBuffer<rigid> T_buf, T_tmp_buf;
    DeviceBuffer<double> w_buf, lik_buf, partial_buf, pose12_buf, mean16_buf;
    DeviceBuffer<long long> cum_buf;
    DeviceBuffer<NdtMclState> state_buf;
    DeviceBuffer<NdtMclMotion> motion_buf;
    PinnedBuffer<NdtMclMotion> pin_motion[2];   // pinned host staging of the motion records, two calls in flight
    Fence pin_used[2];                     // ... recorded behind a slot's copy to the device
    int pin_slot = 0;
    Fence used;                            // recorded after the last launch of a call
    DeviceBuffer<char> h_cloud;            // update_host's device copy of the clouds
    MapsetOwner scan;                      // the local scan maps, one per filter.  After the buffers: it goes first, and
                                           // ndtgpu_mapset_destroy's hipDeviceSynchronize covers them too, also after a call
                                           // that failed midway on a stream of the caller's and never recorded `used`
    Stream hst;                            // the synchronous entries' stream (last: ndtgpu_resource.h)
};

extern "C" {

void ndtgpu_default_mcl_params(ndtgpu_mcl_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->map_res = 0.0;
    p->sensor_res = 0.0;
    p->scan_size[0] = 100.0; p->scan_size[1] = 100.0; p->scan_size[2] = 8.0;   // guessSize(0,0,0, 100,100,8) (recalled)
    p->range_limit = -1.0;
    p->zfilt_min = -5.0;                                                       // :174
    // NDTMCL3D's motion_model / motion_model_offset defaults (recalled, not readable in the reference; the node overrides them
    // from its parameters, :183-184)
    static const double mm[36] = {0.05, 0.05, 0.02, 0.01, 0.01, 0.02,
                                  0.05, 0.10, 0.02, 0.01, 0.01, 0.02,
                                  0.01, 0.01, 0.02, 0.01, 0.01, 0.01,
                                  0.01, 0.01, 0.01, 0.02, 0.01, 0.01,
                                  0.01, 0.01, 0.01, 0.01, 0.02, 0.01,
                                  0.05, 0.05, 0.01, 0.01, 0.01, 0.10};
    static const double off[6] = {0.005, 0.005, 0.001, 0.001, 0.001, 0.005};
    memcpy(p->motion_model, mm, sizeof mm);
    memcpy(p->motion_model_offset, off, sizeof off);
    p->force_sir = 0;                                                          // :175-176
    p->sir_max_iters_wo_resampling = 25;                                       // :179
    p->sir_varp_threshold = 0.006;                                             // :178
    p->max_scan_cells = 0;
    p->seed = 1;
}

ndtgpu_status ndtgpu_mcl_destroy(ndtgpu_mcl *h)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "mcl_destroy: null");
    (void)h->used.sync();                  // (the last call may have run on a stream of the caller's)
    for (Fence &p : h->pin_used) (void)p.sync();   // (... and a call that failed behind its copy from the pinned block never recorded `used`)
    delete h;
    return NDTGPU_OK;
}

static bool finite_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

ndtgpu_status ndtgpu_mcl_create(ndtgpu_mapset *map_set, const uint32_t *map_idx, const ndtgpu_mcl_params *params, size_t n_filters,
                                size_t n_particles, ndtgpu_mcl **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "mcl_create: out is NULL");
    *out = nullptr;
    if (!map_set || !map_idx) return fail(NDTGPU_ERR_INVALID, "mcl_create: map set and map indices are required");
    if (n_filters == 0 || n_particles == 0 || n_particles > 65536 || n_filters > (1u << 24) || n_filters * n_particles > (1u << 24))
        return fail(NDTGPU_ERR_INVALID, "mcl_create: n_particles must be 1..65536 and n_filters * n_particles <= 2^24");
    ndtgpu_mcl_params p = params_or_default(params, ndtgpu_default_mcl_params);
    bool ok = finite_nonneg(p.map_res) && finite_nonneg(p.sensor_res) && std::isfinite(p.range_limit) && !std::isnan(p.zfilt_min) &&
              std::isfinite(p.sir_varp_threshold);
    for (int a = 0; a < 3; a++) ok = ok && std::isfinite(p.scan_size[a]) && p.scan_size[a] > 0.0;
    for (double v : p.motion_model) ok = ok && std::isfinite(v);
    for (double v : p.motion_model_offset) ok = ok && std::isfinite(v);
    if (!ok) return fail(NDTGPU_ERR_INVALID, "mcl_create: bad parameter (resolutions >= 0, scan_size > 0, finite values)");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "mcl_create: no HIP device");
    const double map_res = map_set->v.grid.res;
    if (p.map_res != 0.0 && p.map_res != map_res)
        return fail(NDTGPU_ERR_INVALID, "mcl_create: the map set's cell size differs from the filter's map resolution");
    for (size_t k = 0; k < n_filters; k++)
        if (map_idx[k] >= map_set->n_maps) return fail(NDTGPU_ERR_INVALID, "mcl_create: map index out of range");
    p.map_res = map_res;
    if (p.sensor_res == 0.0) p.sensor_res = map_res;

    ndtgpu_mcl *h = new (std::nothrow) ndtgpu_mcl();
    if (!h) return fail(NDTGPU_ERR_ALLOC, "mcl_create: host alloc");
    h->map = map_set;
    h->prm = p;
    h->F = n_filters;
    h->N = (unsigned)n_particles;
    ndtgpu_grid_params g{};
    g.res = p.sensor_res;
    g.centre[0] = g.centre[1] = g.centre[2] = 0.0;
    for (int a = 0; a < 3; a++) g.size[a] = p.scan_size[a];
    g.max_cells = p.max_scan_cells;
    ndtgpu_status rc = mapset_create_owned(&g, n_filters, h->scan);
    if (rc != NDTGPU_OK) { delete h; return rc; }
    // chunks of the scan cells: at most NDT_MCL_MAX_CHUNKS per filter, whole LDS stages each
    const unsigned cap = h->scan->v.grid.max_cells;
    const unsigned per = (cap + NDT_MCL_MAX_CHUNKS - 1) / NDT_MCL_MAX_CHUNKS;
    h->chunk = std::max(1u, (per + NDT_MCL_STAGE - 1) / NDT_MCL_STAGE) * NDT_MCL_STAGE;
    h->n_chunks = std::max(1u, (cap + h->chunk - 1) / h->chunk);
    const size_t FN = n_filters * n_particles;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "mcl_create: device buffers", expr)
    TRY(h->map_idx_buf.alloc(n_filters, &h->map_idx));
    TRY(h->T_buf.alloc(FN, &h->T));
    TRY(h->T_tmp_buf.alloc(FN, &h->T_tmp));
    TRY(h->w_buf.alloc(FN, &h->w));
    TRY(h->lik_buf.alloc(FN, &h->lik));
    TRY(h->partial_buf.alloc(FN * h->n_chunks, &h->partial));
    TRY(h->cum_buf.alloc(FN, &h->cum));
    TRY(h->state_buf.alloc(n_filters, &h->state));
    TRY(h->motion_buf.alloc(n_filters, &h->motion));
    TRY(h->pose12_buf.alloc(n_filters * 12, &h->pose12));
    TRY(h->mean16_buf.alloc(n_filters * 16, &h->mean16));
    for (int k = 0; k < 2; k++) {
        TRY(h->pin_motion[k].alloc(n_filters));
        TRY(h->pin_used[k].create());
    }
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
    TRY(hipMemcpy(h->map_idx, map_idx, n_filters * sizeof(uint32_t), hipMemcpyHostToDevice));
    TRY(hipMemset(h->state, 0, n_filters * sizeof(NdtMclState)));
    TRY(hipMemset(h->lik, 0, FN * sizeof(double)));
    // until initialize / set_particles: every particle at the origin with weight 1/N
    std::vector<rigid> T0(n_particles, rigid{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}});
    std::vector<double> w0(n_particles, 1.0 / (double)n_particles);
    for (size_t f = 0; f < n_filters; f++) {
        TRY(hipMemcpy(h->T + f * n_particles, T0.data(), n_particles * sizeof(rigid), hipMemcpyHostToDevice));
        TRY(hipMemcpy(h->w + f * n_particles, w0.data(), n_particles * sizeof(double), hipMemcpyHostToDevice));
    }
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

static ndtgpu_status mcl_range(const ndtgpu_mcl *h, size_t first, size_t count, const char *what)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, what, "null handle");
    if (count == 0 || first >= h->F || count > h->F - first)
        return fail_in(NDTGPU_ERR_INVALID, what, "filters [first, first + count) out of range");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_initialize(ndtgpu_mcl *h, size_t first, size_t count, const double *pose6, const double *sigma6)
{
    ndtgpu_status rc = mcl_range(h, first, count, "mcl_initialize");
    if (rc != NDTGPU_OK) return rc;
    if (!pose6 || !sigma6) return fail(NDTGPU_ERR_INVALID, "mcl_initialize: pose6 and sigma6 are required");
    std::vector<double> buf(count * 12);
    for (size_t k = 0; k < count; k++)
        for (int d = 0; d < 6; d++) {
            buf[k * 12 + d] = pose6[k * 6 + d];
            buf[k * 12 + 6 + d] = sigma6[k * 6 + d];
        }
    HIP_TRY(h->used.order(h->hst.get()));     // (the synchronous entries run on the handle's stream, behind the previous call)
    HIP_TRY(hipMemcpyAsync(h->pose12, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
    hipError_t e = ndt_mcl_launch_init(first, count, h->N, h->pose12, h->prm.seed, h->state, h->T, h->w, h->hst.get());
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mcl_initialize: launch", e);
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_set_particles(ndtgpu_mcl *h, size_t first, size_t count, const double *T16, const double *weights)
{
    ndtgpu_status rc = mcl_range(h, first, count, "mcl_set_particles");
    if (rc != NDTGPU_OK) return rc;
    if (!T16) return fail(NDTGPU_ERR_INVALID, "mcl_set_particles: T16 is required");
    const size_t n = count * h->N;
    std::vector<rigid> T(n);
    std::vector<double> w(n);
    for (size_t k = 0; k < n; k++) {
        ndt_rigid_from16(T16 + 16 * k, T[k]);
        w[k] = weights ? weights[k] : 1.0 / (double)h->N;
    }
    HIP_TRY(h->used.order(h->hst.get()));     // (the synchronous entries run on the handle's stream, behind the previous call)
    HIP_TRY(hipMemcpyAsync(h->T + first * h->N, T.data(), n * sizeof(rigid), hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(hipMemcpyAsync(h->w + first * h->N, w.data(), n * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    return NDTGPU_OK;
}

static ndtgpu_status mcl_update_core(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, double subsample_level,
                                     const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes, hipStream_t st)
{
    HIP_TRY(h->used.order(st));   // (the previous call may have run on another stream)
    // the motion records: pinned staging, one of two slots (its previous copy has long been queued)
    const int s = h->pin_slot;
    h->pin_slot ^= 1;
    HIP_TRY(h->pin_used[s].sync());
    for (size_t k = 0; k < count; k++)
        ndt_mcl_motion(Tmotion16 + 16 * k, h->prm.motion_model, h->prm.motion_model_offset, h->pin_motion[s].get()[k]);
    HIP_TRY(hipMemcpyAsync(h->motion + first, h->pin_motion[s].get(), count * sizeof(NdtMclMotion), hipMemcpyHostToDevice, st));
    HIP_TRY(h->pin_used[s].record(st));

    ndtgpu_cell_params cp;
    ndtgpu_default_cell_params(&cp);
    ndtgpu_status rc = mapset_build_core(h->scan.get(), first, count, xyz_dev, n_points, stride_bytes, map_stride_bytes, h->prm.range_limit,
                                         nullptr, &cp, st);
    if (rc != NDTGPU_OK) return rc;
    NdtMclParamsDev pd;
    pd.zfilt_min = h->prm.zfilt_min;
    pd.subsample_level = (subsample_level < 0.0 || subsample_level > 1.0 || std::isnan(subsample_level)) ? 1.0 : subsample_level;
    pd.sir_varp_threshold = h->prm.sir_varp_threshold;
    pd.force_sir = h->prm.force_sir;
    pd.sir_max_iters_wo_resampling = h->prm.sir_max_iters_wo_resampling;
    pd.seed = h->prm.seed;
    hipError_t e = ndt_mcl_launch_predict(first, count, h->N, h->motion, pd.seed, h->state, h->T, st);
    if (e == hipSuccess)
        e = ndt_mcl_launch_likelihood(h->map->v, h->map_idx, h->scan->v, first, count, h->N, h->chunk, h->n_chunks, pd, h->state, h->T,
                                      h->partial, st);
    if (e == hipSuccess)
        e = ndt_mcl_launch_normalise(first, count, h->N, h->chunk, h->n_chunks, pd, h->scan->v, h->state, h->T, h->T_tmp, h->w, h->lik,
                                     h->partial, h->cum, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mcl_update: launch", e);
    if ((rc = h->map->touch(st)) != NDTGPU_OK) return rc;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

static ndtgpu_status mcl_update_check(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, const void *xyz,
                                      size_t n_points, size_t stride_bytes)
{
    ndtgpu_status rc = mcl_range(h, first, count, "mcl_update");
    if (rc != NDTGPU_OK) return rc;
    if (!Tmotion16 || (!xyz && n_points) || stride_bytes < 12 || (stride_bytes & 3) || n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "mcl_update: bad argument");
    for (size_t k = 0; k < 16 * count; k++)
        if (!std::isfinite(Tmotion16[k])) return fail(NDTGPU_ERR_INVALID, "mcl_update: Tmotion is not finite");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_update(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, double subsample_level,
                                const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                ndtgpu_stream stream)
{
    ndtgpu_status rc = mcl_update_check(h, first, count, Tmotion16, xyz_dev, n_points, stride_bytes);
    if (rc != NDTGPU_OK) return rc;
    return mcl_update_core(h, first, count, Tmotion16, subsample_level, xyz_dev, n_points, stride_bytes, map_stride_bytes,
                           (hipStream_t)stream);
}

ndtgpu_status ndtgpu_mcl_update_host(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, double subsample_level,
                                     const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes)
{
    ndtgpu_status rc = mcl_update_check(h, first, count, Tmotion16, xyz_host, n_points, stride_bytes);
    if (rc != NDTGPU_OK) return rc;
    const size_t bytes = n_points ? (count - 1) * map_stride_bytes + n_points * stride_bytes : 0;
    HIP_TRY(h->h_cloud.reserve(bytes, h->used));     // (the last update may still read the block that is replaced)
    HIP_TRY(h->used.order(h->hst.get()));     // (the synchronous entries run on the handle's stream, behind the previous call)
    if (bytes) HIP_TRY(hipMemcpyAsync(h->h_cloud.get(), xyz_host, bytes, hipMemcpyHostToDevice, h->hst.get()));
    rc = mcl_update_core(h, first, count, Tmotion16, subsample_level, h->h_cloud.get(), n_points, stride_bytes, map_stride_bytes, h->hst.get());
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_particles(ndtgpu_mcl *h, size_t first, size_t count, double *T16, double *weights, double *lik)
{
    ndtgpu_status rc = mcl_range(h, first, count, "mcl_particles");
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(h->used.sync());
    const size_t n = count * h->N, off = first * h->N;
    if (T16) {
        std::vector<rigid> T(n);
        HIP_TRY(hipMemcpy(T.data(), h->T + off, n * sizeof(rigid), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; k++) ndt_rigid_to16(T[k], T16 + 16 * k);
    }
    if (weights) HIP_TRY(hipMemcpy(weights, h->w + off, n * sizeof(double), hipMemcpyDeviceToHost));
    if (lik) HIP_TRY(hipMemcpy(lik, h->lik + off, n * sizeof(double), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_mean(ndtgpu_mcl *h, size_t first, size_t count, double *T16_mean, ndtgpu_mcl_result *results)
{
    ndtgpu_status rc = mcl_range(h, first, count, "mcl_mean");
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(h->used.order(h->hst.get()));     // (the synchronous entries run on the handle's stream, behind the previous call)
    if (T16_mean) {
        hipError_t e = ndt_mcl_launch_mean(first, count, h->N, h->T, h->w, h->mean16, h->hst.get());
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mcl_mean: launch", e);
        HIP_TRY(hipMemcpyAsync(T16_mean, h->mean16, count * 16 * sizeof(double), hipMemcpyDeviceToHost, h->hst.get()));
    }
    std::vector<NdtMclState> st(count);
    HIP_TRY(hipMemcpyAsync(st.data(), h->state + first, count * sizeof(NdtMclState), hipMemcpyDeviceToHost, h->hst.get()));
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    if (results)
        for (size_t k = 0; k < count; k++) {
            ndtgpu_mcl_result &r = results[k];
            r.var_p = st[k].var_p;
            r.lik_sum = st[k].lik_sum;
            r.terms = (int64_t)st[k].terms;
            r.draws = st[k].draws;
            r.resampled = st[k].resampled;
            r.since_sir = st[k].since_sir;
            r.n_scan_cells = st[k].n_scan_cells;
            r.overflow = st[k].overflow;
        }
    return NDTGPU_OK;
}

}   // extern "C"

// the particle poses of filters [first, first + count) in place, for the marker export (ndtgpu_marker.hip)
ndtgpu_status mcl_particles_view(ndtgpu_mcl *h, size_t first, size_t count, const char *who, MclParticles &out)
{
    const ndtgpu_status rc = mcl_range(h, first, count, who);
    if (rc != NDTGPU_OK) return rc;
    out.T = h->T + first * h->N;
    out.n = count * h->N;
    out.used = &h->used;
    out.hst = h->hst.get();
    return NDTGPU_OK;
}
