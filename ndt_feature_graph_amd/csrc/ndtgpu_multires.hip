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
    ndtgpu_mapset *tset[NDTGPU_MAX_LEVELS] = {}, *sset[NDTGPU_MAX_LEVELS] = {};
    // device, per sub-batch pair: iota (target index), source index, Temp / X (16 doubles each), {Tacc, Tinit} (32), stopped,
    // the matcher's results of one level
    uint32_t *iota = nullptr, *sidx = nullptr;
    double *temp = nullptr, *xf = nullptr, *state = nullptr;
    int *stopped = nullptr;
    NdtMatchResultDev *res_lvl = nullptr;
    // the moved source clouds, packed xyz (ping-pong: a level reads one and writes the other)
    float *cloud[2] = {nullptr, nullptr};
    size_t cloud_points = 0;                               // n_points the buffers hold per pair
    hipEvent_t used = nullptr;                             // recorded after the last launch of a call (every internal buffer
    bool used_valid = false;                               // and map set is free once it has passed)
    uint64_t levels_fused = 0, levels_unfused = 0;         // source builds so far: moved on load / moved, then built
    // host entry: staging on a stream of its own
    hipStream_t hst = nullptr;
    void *h_tg = nullptr, *h_sc = nullptr;
    size_t h_cloud_bytes = 0;
    double *h_T = nullptr;
    ndtgpu_match_result *h_res = nullptr;
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
    if (mr->used_valid) (void)hipEventSynchronize(mr->used);
    if (mr->hst) (void)hipStreamSynchronize(mr->hst);
    for (int j = 0; j < NDTGPU_MAX_LEVELS; j++) {
        if (mr->tset[j]) ndtgpu_mapset_destroy(mr->tset[j]);
        if (mr->sset[j]) ndtgpu_mapset_destroy(mr->sset[j]);
    }
    void *bufs[] = {mr->iota, mr->sidx, mr->temp, mr->xf, mr->state, mr->stopped, mr->res_lvl, mr->cloud[0], mr->cloud[1],
                    mr->h_tg, mr->h_sc, mr->h_T, mr->h_res};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (mr->used) (void)hipEventDestroy(mr->used);
    if (mr->hst) (void)hipStreamDestroy(mr->hst);
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
        ndtgpu_status rc = ndtgpu_mapset_create(&g, p, &mr->tset[j]);
        if (rc == NDTGPU_OK) rc = ndtgpu_mapset_create(&g, p, &mr->sset[j]);
        if (rc != NDTGPU_OK) { ndtgpu_multires_destroy(mr); return rc; }
    }
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&mr->iota, p * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->sidx, p * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->temp, p * 16 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->xf, p * 16 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->state, p * 32 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->stopped, p * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&mr->res_lvl, p * sizeof(NdtMatchResultDev));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&mr->used, hipEventDisableTiming);
    if (e == hipSuccess) {
        std::vector<uint32_t> iota(p);
        for (size_t k = 0; k < p; k++) iota[k] = (uint32_t)k;
        e = hipMemcpy(mr->iota, iota.data(), p * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        ndtgpu_multires_destroy(mr);
        return fail(NDTGPU_ERR_ALLOC, "multires_create: device buffers", e);
    }
    *out = mr;
    return NDTGPU_OK;
}

static ndtgpu_status ensure_clouds(ndtgpu_multires *mr, size_t n_points)
{
    if (n_points <= mr->cloud_points) return NDTGPU_OK;
    if (mr->used_valid) HIP_TRY(hipEventSynchronize(mr->used));
    for (float *&c : mr->cloud) {
        if (c) (void)hipFree(c);
        c = nullptr;
    }
    mr->cloud_points = 0;
    for (float *&c : mr->cloud) HIP_TRY(hipMalloc((void **)&c, mr->per * n_points * 3 * sizeof(float)));
    mr->cloud_points = n_points;
    return NDTGPU_OK;
}

// One sub-batch of p <= per pairs, every level, on `st`.
static ndtgpu_status multires_subbatch(ndtgpu_multires *mr, const char *tg, const char *sc, size_t n_points, size_t stride_bytes,
                                       size_t map_stride_bytes, double range_limit, const ndtgpu_cell_params *cell, double *T16_dev,
                                       size_t p, const ndtgpu_match_params &mp, int use_initial_guess,
                                       ndtgpu_match_result *results_dev, bool fused, hipStream_t st)
{
    ndtgpu_cell_params cp;
    ndtgpu_default_cell_params(&cp);
    if (cell) cp = *cell;
    const int L = mr->n_levels;
    NdtMatchResultDev *res_out = reinterpret_cast<NdtMatchResultDev *>(results_dev);
    hipError_t e = ndt_launch_multires_step(p, -1, 0, L, 0, use_initial_guess, T16_dev, mr->temp, mr->xf, mr->state, mr->stopped,
                                            mr->sidx, mr->res_lvl, res_out, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: init launch", e);
    // the source cloud the first level moves: the caller's, or its range-filtered packed copy
    const char *in = sc;
    size_t in_stride = stride_bytes, in_map_stride = map_stride_bytes;
    int next = 0;
    if (range_limit > 0) {
        e = ndt_launch_multires_range(sc, p, n_points, stride_bytes, map_stride_bytes, range_limit, mr->cloud[0], st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: range filter launch", e);
        in = (const char *)mr->cloud[0];
        in_stride = 12;
        in_map_stride = n_points * 12;
        next = 1;
    }
    for (int i = 0; i < L; i++) {
        const int j = L - 1 - i;                           // list position: from the last entry to the first
        const bool last = i == L - 1;
        ndtgpu_mapset *ts = mr->tset[j], *ss = mr->sset[j];
        ndtgpu_status rc = mapset_build_core(ts, 0, p, tg, n_points, stride_bytes, map_stride_bytes, range_limit, nullptr, cell, st);
        if (rc != NDTGPU_OK) return rc;
        float *out = mr->cloud[next];
        e = hipErrorNotSupported;
        if (fused) {
            if (ss->v.occ) HIP_TRY(hipMemsetAsync(ss->v.occ, 0, p * (size_t)ss->v.grid.slots * sizeof(float), st));
            e = ndt_launch_build_flat_xf(ss->v, 0, p, in, n_points, in_stride, in_map_stride, cp.n_min, cp.eval_factor,
                                         ss->nice_range(0, p), mr->xf, last ? nullptr : out, st);
            if (e != hipSuccess && e != hipErrorNotSupported) return fail(NDTGPU_ERR_HIP, "multires: source build launch", e);
            if (e == hipSuccess) {
                mr->levels_fused++;
                rc = ss->touch(st);
                if (rc != NDTGPU_OK) return rc;
            }
        }
        if (e == hipErrorNotSupported) {
            // the move, then the general build on the moved clouds
            e = ndt_launch_cloud_transform(in, p, n_points, in_stride, in_map_stride, mr->xf, nullptr, 16, out, st);
            if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: transform launch", e);
            rc = mapset_build_core(ss, 0, p, out, n_points, 12, n_points * 12, 0.0, nullptr, cell, st);
            if (rc != NDTGPU_OK) return rc;
            mr->levels_unfused++;
        }
        in = (const char *)out;
        in_stride = 12;
        in_map_stride = n_points * 12;
        next ^= 1;
        rc = match_batch_device_ex(ts, mr->iota, ss, mr->sidx, mr->temp, p, &mp, reinterpret_cast<ndtgpu_match_result *>(mr->res_lvl),
                                   st, -1, nullptr, nullptr, nullptr);
        if (rc != NDTGPU_OK) return rc;
        e = ndt_launch_multires_step(p, i, j, L, last ? 1 : 0, use_initial_guess, T16_dev, mr->temp, mr->xf, mr->state, mr->stopped,
                                     mr->sidx, mr->res_lvl, res_out, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "multires: level step launch", e);
    }
    HIP_TRY(hipEventRecord(mr->used, st));
    mr->used_valid = true;
    return NDTGPU_OK;
}

static ndtgpu_status multires_check(ndtgpu_multires *mr, const void *tg, const void *sc, size_t n_points, size_t stride_bytes,
                                    size_t map_stride_bytes, double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                    ndtgpu_match_result *results, ndtgpu_match_params &mp)
{
    if (!mr || (n_pairs && (!tg || !sc || !T16 || !results)) || stride_bytes < 12 || (stride_bytes & 3) || n_points == 0 ||
        n_points > 0xFFFFFFFFull || map_stride_bytes < n_points * stride_bytes)
        return fail(NDTGPU_ERR_INVALID, "register_multires: bad argument");
    ndtgpu_default_match_params(&mp);
    if (prm) mp = *prm;
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
    if (mr->used_valid) HIP_TRY(hipStreamWaitEvent(st, mr->used, 0));   // (the previous call may have run on another stream)
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
    if (!mr->hst) HIP_TRY(hipStreamCreateWithFlags(&mr->hst, hipStreamNonBlocking));
    hipStream_t st = mr->hst;
    if (mr->used_valid) HIP_TRY(hipStreamWaitEvent(st, mr->used, 0));
    // one sub-batch of clouds at a time: p clouds map_stride_bytes apart, the last one n_points records long
    const size_t cloud_bytes = (mr->per - 1) * map_stride_bytes + n_points * stride_bytes;
    if (cloud_bytes > mr->h_cloud_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (mr->h_tg) (void)hipFree(mr->h_tg);
        if (mr->h_sc) (void)hipFree(mr->h_sc);
        mr->h_tg = mr->h_sc = nullptr;
        mr->h_cloud_bytes = 0;
        HIP_TRY(hipMalloc(&mr->h_tg, cloud_bytes));
        HIP_TRY(hipMalloc(&mr->h_sc, cloud_bytes));
        mr->h_cloud_bytes = cloud_bytes;
    }
    if (!mr->h_T) HIP_TRY(hipMalloc((void **)&mr->h_T, mr->per * 16 * sizeof(double)));
    if (!mr->h_res) HIP_TRY(hipMalloc((void **)&mr->h_res, mr->per * NDTGPU_MAX_LEVELS * sizeof(ndtgpu_match_result)));
    const bool fused = fused_enabled();
    const size_t L = (size_t)mr->n_levels;
    for (size_t off = 0; off < n_pairs; off += mr->per) {
        const size_t p = std::min(mr->per, n_pairs - off);
        const size_t bytes = (p - 1) * map_stride_bytes + n_points * stride_bytes;
        HIP_TRY(hipMemcpyAsync(mr->h_tg, (const char *)targets_host + off * map_stride_bytes, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mr->h_sc, (const char *)sources_host + off * map_stride_bytes, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mr->h_T, T16 + off * 16, p * 16 * sizeof(double), hipMemcpyHostToDevice, st));
        rc = multires_subbatch(mr, (const char *)mr->h_tg, (const char *)mr->h_sc, n_points, stride_bytes, map_stride_bytes, range_limit,
                               cell, mr->h_T, p, mp, use_initial_guess ? 1 : 0, mr->h_res, fused, st);
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(hipMemcpyAsync(T16 + off * 16, mr->h_T, p * 16 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(results + off * L, mr->h_res, p * L * sizeof(ndtgpu_match_result), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return NDTGPU_OK;
}
