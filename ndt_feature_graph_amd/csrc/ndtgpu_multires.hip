// ndtgpu_multires.hip -- C-ABI (include/ndtgpu.h) of the coarse-to-fine registrar: NDTMatcherD2D(irregular, useDefault,
// resolutions).match(target_pc, source_pc, T, useInitialGuess) for batches of raw scan pairs.  Host side only: handle, level
// map sets, staging, and the order of the launches; the kernels are the builds (csrc/ndt_build*.hip), the matcher
// (csrc/ndtgpu_matcher.hip's per-batch dispatch), ndt_cloud_transform_kernel (csrc/ndt_fuser.hip) and the two small kernels
// of csrc/ndt_multires.hip.
#include "ndtgpu_host.h"

#include <new>

struct ndtgpu_multires {
    int n_levels = 0;
    double res[NDTGPU_MAX_LEVELS] = {};
    ndtgpu_grid_params grid{};
    size_t per = 0;                                        // pairs per sub-batch
    // device, per sub-batch pair: iota (target index), source index, Temp / X (16 doubles each), {Tacc, Tinit} (32), stopped,
    // the matcher's results of one level
    DeviceBuffer<uint32_t> iota, sidx;
    DeviceBuffer<double> temp, xf, state;
    DeviceBuffer<int> stopped;
    DeviceBuffer<NdtMatchResultDev> res_lvl;
    // the moved source clouds, packed xyz (ping-pong: a level reads one and writes the other)
    DeviceBuffer<float> cloud[2];
    size_t cloud_points = 0;                               // n_points the buffers hold per pair
    Fence used;                                            // recorded after the last launch of a call (every internal buffer
                                                           // and map set is free once it has passed)
    uint64_t levels_fused = 0, levels_unfused = 0;         // source builds so far: moved on load / moved, then built
    // host entry: staging on a stream of its own (last: ndtgpu_resource.h)
    DeviceBuffer<char> h_tg, h_sc;
    DeviceBuffer<double> h_T;
    DeviceBuffer<ndtgpu_match_result> h_res;
    // the level map sets after the buffers: they go first, and ndtgpu_mapset_destroy's hipDeviceSynchronize covers the buffers
    // above too, also after a call that failed midway on a stream of the caller's and never recorded `used`
    MapsetOwner tset[NDTGPU_MAX_LEVELS], sset[NDTGPU_MAX_LEVELS];
    Stream hst;
};

void ndtgpu_default_resolutions(double res[4], int *n_levels)
{
    // NDTMatcherD2D(.., useDefaultGridResolutions = true, ..) (perception_oru, restated; include/ndtgpu.h)
    if (res) { res[0] = 0.2; res[1] = 0.5; res[2] = 1.0; res[3] = 2.0; }
    if (n_levels) *n_levels = 4;
}

ndtgpu_status ndtgpu_multires_destroy(ndtgpu_multires *mr)
{
    if (!mr) return NDTGPU_ERR_INVALID;
    (void)mr->used.sync();                 // (the last call may have run on a stream of the caller's)
    delete mr;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_multires_create(const ndtgpu_grid_params *grid, const double *resolutions, int n_levels, size_t pairs_per_batch,
                                     ndtgpu_multires **out)
{
    if (!grid || !resolutions || !out || n_levels < 1 || n_levels > NDTGPU_MAX_LEVELS || pairs_per_batch == 0 ||
        pairs_per_batch > 0xFFFFFFFFu)
        return fail(NDTGPU_ERR_INVALID, "multires_create: bad argument (n_levels must be 1..8)");
    for (int j = 0; j < n_levels; j++)
        if (!(resolutions[j] > 0) || !std::isfinite(resolutions[j]))
            return fail(NDTGPU_ERR_INVALID, "multires_create: every resolution must be > 0");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "multires_create: no HIP device");
    ndtgpu_multires *mr = new (std::nothrow) ndtgpu_multires();
    if (!mr) return fail(NDTGPU_ERR_ALLOC, "multires_create: host alloc");
    mr->n_levels = n_levels;
    mr->grid = *grid;
    mr->per = pairs_per_batch;
    const size_t p = pairs_per_batch;
    for (int j = 0; j < n_levels; j++) {
        mr->res[j] = resolutions[j];
        ndtgpu_grid_params g = *grid;
        g.res = resolutions[j];
        ndtgpu_status rc = mapset_create_owned(&g, p, mr->tset[j]);
        if (rc == NDTGPU_OK) rc = mapset_create_owned(&g, p, mr->sset[j]);
        if (rc != NDTGPU_OK) { delete mr; return rc; }
    }
#define TRY(expr) CREATE_TRY(mr, NDTGPU_ERR_ALLOC, "multires_create: device buffers", expr)
    TRY(mr->iota.alloc(p));
    TRY(mr->sidx.alloc(p));
    TRY(mr->temp.alloc(p * 16));
    TRY(mr->xf.alloc(p * 16));
    TRY(mr->state.alloc(p * 32));
    TRY(mr->stopped.alloc(p));
    TRY(mr->res_lvl.alloc(p));
    TRY(mr->used.create());
    std::vector<uint32_t> iota(p);
    for (size_t k = 0; k < p; k++) iota[k] = (uint32_t)k;
    TRY(hipMemcpy(mr->iota.get(), iota.data(), p * sizeof(uint32_t), hipMemcpyHostToDevice));
#undef TRY
    *out = mr;
    return NDTGPU_OK;
}

// room for n_points per pair in both cloud buffers; the last call's launches may still use the ones that are replaced
static ndtgpu_status ensure_clouds(ndtgpu_multires *mr, size_t n_points)
{
    if (n_points <= mr->cloud_points) return NDTGPU_OK;
    HIP_TRY(mr->used.sync());
    mr->cloud_points = 0;
    for (DeviceBuffer<float> &c : mr->cloud) HIP_TRY(c.reserve(mr->per * n_points * 3));
    mr->cloud_points = n_points;
    return NDTGPU_OK;
}

// One sub-batch of p <= per pairs, every level, on `st`.
static ndtgpu_status multires_subbatch(ndtgpu_multires *mr, const char *tg, const char *sc, size_t n_points, size_t stride_bytes,
                                       size_t map_stride_bytes, double range_limit, const ndtgpu_cell_params *cell, double *T16_dev,
                                       size_t p, const ndtgpu_match_params &mp, int use_initial_guess,
                                       ndtgpu_match_result *results_dev, bool fused, hipStream_t st)
{
    const ndtgpu_cell_params cp = params_or_default(cell, ndtgpu_default_cell_params);
    const int L = mr->n_levels;
    NdtMatchResultDev *res_out = reinterpret_cast<NdtMatchResultDev *>(results_dev);
    hipError_t e = ndt_launch_multires_step(p, -1, 0, L, 0, use_initial_guess, T16_dev, mr->temp.get(), mr->xf.get(), mr->state.get(), mr->stopped.get(),
                                            mr->sidx.get(), mr->res_lvl.get(), res_out, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: init launch", e);
    // the source cloud the first level moves: the caller's, or its range-filtered packed copy
    const char *in = sc;
    size_t in_stride = stride_bytes, in_map_stride = map_stride_bytes;
    int next = 0;
    if (range_limit > 0) {
        e = ndt_launch_multires_range(sc, p, n_points, stride_bytes, map_stride_bytes, range_limit, mr->cloud[0].get(), st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: range filter launch", e);
        in = (const char *)mr->cloud[0].get();
        in_stride = 12;
        in_map_stride = n_points * 12;
        next = 1;
    }
    for (int i = 0; i < L; i++) {
        const int j = L - 1 - i;                           // list position: from the last entry to the first
        const bool last = i == L - 1;
        ndtgpu_mapset *ts = mr->tset[j].get(), *ss = mr->sset[j].get();
        ndtgpu_status rc = mapset_build_core(ts, 0, p, tg, n_points, stride_bytes, map_stride_bytes, range_limit, nullptr, cell, st);
        if (rc != NDTGPU_OK) return rc;
        float *out = mr->cloud[next].get();
        e = hipErrorNotSupported;
        if (fused) {
            if (ss->v.occ) HIP_TRY(hipMemsetAsync(ss->v.occ, 0, p * (size_t)ss->v.grid.slots * sizeof(float), st));
            e = ndt_launch_build_flat_xf(ss->v, 0, p, in, n_points, in_stride, in_map_stride, cp.n_min, cp.eval_factor,
                                         ss->nice_range(0, p), mr->xf.get(), last ? nullptr : out, st);
            if (e != hipSuccess && e != hipErrorNotSupported) return fail(NDTGPU_ERR_HIP, "multires: source build launch", e);
            if (e == hipSuccess) {
                mr->levels_fused++;
                rc = ss->touch(st);
                if (rc != NDTGPU_OK) return rc;
            }
        }
        if (e == hipErrorNotSupported) {
            // the move, then the general build on the moved clouds
            e = ndt_launch_cloud_transform(in, p, n_points, in_stride, in_map_stride, mr->xf.get(), nullptr, 16, out, st);
            if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: transform launch", e);
            rc = mapset_build_core(ss, 0, p, out, n_points, 12, n_points * 12, 0.0, nullptr, cell, st);
            if (rc != NDTGPU_OK) return rc;
            mr->levels_unfused++;
        }
        in = (const char *)out;
        in_stride = 12;
        in_map_stride = n_points * 12;
        next ^= 1;
        rc = match_batch_device_ex(ts, mr->iota.get(), ss, mr->sidx.get(), mr->temp.get(), p, &mp, reinterpret_cast<ndtgpu_match_result *>(mr->res_lvl.get()),
                                   st, -1, nullptr, nullptr, nullptr);
        if (rc != NDTGPU_OK) return rc;
        e = ndt_launch_multires_step(p, i, j, L, last ? 1 : 0, use_initial_guess, T16_dev, mr->temp.get(), mr->xf.get(), mr->state.get(), mr->stopped.get(),
                                     mr->sidx.get(), mr->res_lvl.get(), res_out, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: level step launch", e);
    }
    HIP_TRY(mr->used.record(st));
    return NDTGPU_OK;
}

static ndtgpu_status multires_check(ndtgpu_multires *mr, const void *tg, const void *sc, size_t n_points, size_t stride_bytes,
                                    size_t map_stride_bytes, double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                    ndtgpu_match_result *results, ndtgpu_match_params &mp)
{
    if (!mr || (n_pairs && (!tg || !sc || !T16 || !results)) || stride_bytes < 12 || (stride_bytes & 3) || n_points == 0 ||
        n_points > 0xFFFFFFFFull || map_stride_bytes < n_points * stride_bytes)
        return fail(NDTGPU_ERR_INVALID, "register_multires: bad argument");
    mp = params_or_default(prm, ndtgpu_default_match_params);
    mp.use_initial_guess = 0;                              // every level matches from the identity
    NdtMatchParamsDev p;
    return match_params_dev(&mp, 0, p);
}

static bool fused_enabled() { return env_int("NDTGPU_MR_FUSED", 1) != 0; }

ndtgpu_status ndtgpu_multires_get_info(const ndtgpu_multires *mr, ndtgpu_multires_info *info)
{
    if (!mr || !info) return fail(NDTGPU_ERR_INVALID, "multires_get_info: bad argument");
    info->n_levels = mr->n_levels;
    info->pairs_per_batch = mr->per;
    info->levels_fused = mr->levels_fused;
    info->levels_unfused = mr->levels_unfused;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_register_multires_device(ndtgpu_multires *mr, const void *targets_dev, const void *sources_dev, size_t n_points,
                                              size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                              const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                              const ndtgpu_match_params *prm, int use_initial_guess, ndtgpu_match_result *results_dev,
                                              ndtgpu_stream stream)
{
    ndtgpu_match_params mp;
    ndtgpu_status rc = multires_check(mr, targets_dev, sources_dev, n_points, stride_bytes, map_stride_bytes, T16_dev, n_pairs, prm,
                                      results_dev, mp);
    if (rc != NDTGPU_OK) return rc;
    if (n_pairs == 0) return NDTGPU_OK;
    rc = ensure_clouds(mr, n_points);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(mr->used.order(st));   // (the previous call may have run on another stream)
    const bool fused = fused_enabled();
    for (size_t off = 0; off < n_pairs; off += mr->per) {
        const size_t p = std::min(mr->per, n_pairs - off);
        rc = multires_subbatch(mr, (const char *)targets_dev + off * map_stride_bytes, (const char *)sources_dev + off * map_stride_bytes,
                               n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16_dev + off * 16, p, mp,
                               use_initial_guess ? 1 : 0, results_dev + off * mr->n_levels, fused, st);
        if (rc != NDTGPU_OK) return rc;
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_register_multires_host(ndtgpu_multires *mr, const void *targets_host, const void *sources_host, size_t n_points,
                                            size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                            const ndtgpu_cell_params *cell, double *T16, size_t n_pairs,
                                            const ndtgpu_match_params *prm, int use_initial_guess, ndtgpu_match_result *results)
{
    ndtgpu_match_params mp;
    ndtgpu_status rc = multires_check(mr, targets_host, sources_host, n_points, stride_bytes, map_stride_bytes, T16, n_pairs, prm,
                                      results, mp);
    if (rc != NDTGPU_OK) return rc;
    if (n_pairs == 0) return NDTGPU_OK;
    rc = ensure_clouds(mr, n_points);
    if (rc != NDTGPU_OK) return rc;
    if (!mr->hst.get()) HIP_TRY(mr->hst.create(hipStreamNonBlocking));
    hipStream_t st = mr->hst.get();
    HIP_TRY(mr->used.order(st));
    // one sub-batch of clouds at a time: p clouds map_stride_bytes apart, the last one n_points records long
    const size_t cloud_bytes = (mr->per - 1) * map_stride_bytes + n_points * stride_bytes;
    if (cloud_bytes > std::min(mr->h_tg.capacity(), mr->h_sc.capacity())) {
        HIP_TRY(hipStreamSynchronize(st));                 // (the copies and builds of the last call read the old blocks)
        HIP_TRY(mr->h_tg.reserve(cloud_bytes));
        HIP_TRY(mr->h_sc.reserve(cloud_bytes));
    }
    HIP_TRY(mr->h_T.reserve(mr->per * 16));
    HIP_TRY(mr->h_res.reserve(mr->per * NDTGPU_MAX_LEVELS));
    const bool fused = fused_enabled();
    const size_t L = (size_t)mr->n_levels;
    for (size_t off = 0; off < n_pairs; off += mr->per) {
        const size_t p = std::min(mr->per, n_pairs - off);
        const size_t bytes = (p - 1) * map_stride_bytes + n_points * stride_bytes;
        HIP_TRY(hipMemcpyAsync(mr->h_tg.get(), (const char *)targets_host + off * map_stride_bytes, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mr->h_sc.get(), (const char *)sources_host + off * map_stride_bytes, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mr->h_T.get(), T16 + off * 16, p * 16 * sizeof(double), hipMemcpyHostToDevice, st));
        rc = multires_subbatch(mr, mr->h_tg.get(), mr->h_sc.get(), n_points, stride_bytes, map_stride_bytes, range_limit,
                               cell, mr->h_T.get(), p, mp, use_initial_guess ? 1 : 0, mr->h_res.get(), fused, st);
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(hipMemcpyAsync(T16 + off * 16, mr->h_T.get(), p * 16 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(results + off * L, mr->h_res.get(), p * L * sizeof(ndtgpu_match_result), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return NDTGPU_OK;
}
