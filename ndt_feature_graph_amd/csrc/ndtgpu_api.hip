// ndtgpu_api.hip -- C-ABI (include/ndtgpu.h) over the HIP kernels: map sets (create, build, host clouds, cells, occupancy,
// overlap score, pack / unpack).  The matcher, the registrar and the fuser bank have files of their own (ndtgpu_*.hip), what
// they share is in ndtgpu_host.h.  Host side only: handle and arena management, argument checking, staging copies.  No CPU compute path exists here: without a
// device every compute entry point fails with NDTGPU_ERR_NO_DEVICE.
#include "ndtgpu_host.h"

#include <atomic>
#include <functional>
#include <new>
#include <thread>

thread_local std::string g_err;

// the build proper; `orig_dev`: per-map range origins already in device memory (or NULL: the grid centres)
ndtgpu_status mapset_build_core(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_dev, size_t n_points,
                                size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                const double *orig_dev, const ndtgpu_cell_params *cell, hipStream_t st)
{
    if (!s || first + count > s->n_maps || (!xyz_dev && n_points) || stride_bytes < 12 || (stride_bytes & 3) ||
        n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "mapset_build: bad argument");
    const ndtgpu_cell_params cp = params_or_default(cell, ndtgpu_default_cell_params);
    if (s->v.occ && count)   // a rebuilt map starts from cells without readings
        HIP_TRY(hipMemsetAsync(s->v.occ + first * (size_t)s->v.grid.slots, 0, count * (size_t)s->v.grid.slots * sizeof(float), st));
    if (s->profiling && !s->profile_span) HIP_TRY(s->ev[0].record(st));
    hipError_t e = ndt_launch_build(s->v, first, count, xyz_dev, n_points, stride_bytes, map_stride_bytes, range_limit,
                         orig_dev, cp.n_min, cp.eval_factor, s->nice_range(first, count), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mapset_build: launch", e);
    if (s->profiling && !s->profile_span) HIP_TRY(s->ev[1].record(st));
    return s->touch(st);
}

// host-side packing of caller-provided Gaussians into NdtCell records keyed by LazyGrid slot
ndtgpu_status pack_cells(const NdtGrid &g, const double *centre, const double *mean3, const double *cov9,
                         size_t n, bool need_slot, std::vector<NdtCell> &out)
{
    out.clear();
    out.reserve(n);
    for (size_t i = 0; i < n; i++) {
        NdtCell c;
        for (int a = 0; a < 3; a++) c.mean[a] = mean3[3 * i + a];
        const double *v = cov9 + 9 * i;
        c.cov[0] = v[0]; c.cov[1] = v[1]; c.cov[2] = v[2]; c.cov[3] = v[4]; c.cov[4] = v[5]; c.cov[5] = v[8];
        c.n = 1;
        c.slot = 0;
        if (need_slot) {
            int idx[3];
            bool inside = true;
            for (int a = 0; a < 3; a++) {
                idx[a] = lazygrid_index(c.mean[a], centre[a], g.res, g.size[a]);
                inside = inside && idx[a] >= 0 && idx[a] < g.size[a];
            }
            if (!inside) continue;   // LazyGrid::addPoint drops what falls outside the grid
            c.slot = (uint32_t)((idx[0] * g.size[1] + idx[1]) * g.size[2] + idx[2]);
        }
        out.push_back(c);
    }
    return NDTGPU_OK;
}

extern "C" {

// (bumped whenever a kernel changes: bench.py only quotes PMC figures taken with the same version)
const char *ndtgpu_version(void) { return "ndtgpu 0.13.0 (gfx950)"; }
const char *ndtgpu_last_error(void) { return g_err.c_str(); }

ndtgpu_status ndtgpu_live_resources(uint64_t counts[4])
{
    if (!counts) return fail(NDTGPU_ERR_INVALID, "live_resources: null");
    for (int k = 0; k < 4; k++) counts[k] = g_live[k].load(std::memory_order_relaxed);
    return NDTGPU_OK;
}

int ndtgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ndtgpu_default_cell_params(ndtgpu_cell_params *p)
{
    p->n_min = 3;
    p->eval_factor = 1000.0;
}

void ndtgpu_default_match_params(ndtgpu_match_params *p)
{
    // the fuser preset: ndt_feature_fuser_hmt.cpp:356-357 with the production launch values
    p->n_neighbours = 2;
    p->itr_max = 30;
    p->delta_score = 1e-6;
    p->step_control = 1;
    p->lfd1 = 1.0;
    p->lfd2 = 0.05;
    p->dof_mask = 0x3f;
    p->use_initial_guess = 1;
}

const char *ndtgpu_kernel_name(int which)
{
    switch (which) {
    case 0: return "ndt_build_kernel";
    case 1: return "ndt_match_kernel";
    case 2: return "ndt_derivatives_kernel";
    default: return "";
    }
}

ndtgpu_status ndtgpu_mapset_create(const ndtgpu_grid_params *grid, size_t n_maps, ndtgpu_mapset **out)
{
    if (!grid || !out || n_maps == 0 || !(grid->res > 0)) return fail(NDTGPU_ERR_INVALID, "mapset_create: bad argument");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "mapset_create: no HIP device");
    ndtgpu_mapset *s = new (std::nothrow) ndtgpu_mapset();
    if (!s) return fail(NDTGPU_ERR_ALLOC, "mapset_create: host alloc");
    s->n_maps = n_maps;
    s->v.n_maps = (uint32_t)n_maps;
    NdtGrid &g = s->v.grid;
    g.res = grid->res;
    long long slots = 1;
    for (int a = 0; a < 3; a++) {
        // LazyGrid::initialize: sizeX = abs(ceil(sizeXmeters / cellSizeX))
        g.size[a] = std::abs((int)std::ceil(grid->size[a] / grid->res));
        if (g.size[a] <= 0) { delete s; return fail(NDTGPU_ERR_INVALID, "mapset_create: empty grid axis"); }
        slots *= g.size[a];
    }
    if (slots > (1ll << 30)) { delete s; return fail(NDTGPU_ERR_INVALID, "mapset_create: grid too large"); }
    g.slots = (int)slots;
    for (int a = 0; a < 3; a++) g.half[a] = g.size[a] / 2.0;
    uint32_t cap = grid->max_cells ? grid->max_cells : (uint32_t)std::min<long long>(slots, 16384);
    if (cap > (1u << 24) - 1) cap = (1u << 24) - 1;
    g.max_cells = cap;
    s->centres_host.resize(n_maps * 3);
    for (size_t m = 0; m < n_maps; m++)
        for (int a = 0; a < 3; a++) s->centres_host[m * 3 + a] = grid->centre[a];
    s->nice_host.assign(n_maps, ndt_grid_is_nice(g, grid->centre) ? 1 : 0);

    NdtSetView &v = s->v;
#define ALLOC(buf, n) CREATE_TRY(s, NDTGPU_ERR_ALLOC, "mapset_create: device buffer " #buf, s->buf.alloc((n), &v.buf))
    ALLOC(rankmap, n_maps * ndt_rm_stride(g));
    ALLOC(wtable, n_maps * (size_t)g.slots);
    ALLOC(bitmap, n_maps * (size_t)((g.slots + 31) / 32));
    ALLOC(cells, n_maps * (size_t)cap);
    ALLOC(acc, n_maps * (size_t)cap);
    ALLOC(acc_slot, n_maps * (size_t)cap);
    ALLOC(rank_agg, n_maps * (size_t)(NDT_RANK_SEGS + 2));
    ALLOC(counters, n_maps);
    ALLOC(centres, n_maps * 3);
#undef ALLOC
#define INIT(expr) CREATE_TRY(s, NDTGPU_ERR_HIP, "mapset_create: init", expr)
    INIT(hipMemset(v.rankmap, 0, n_maps * ndt_rm_stride(g) * sizeof(uint2)));
    INIT(hipMemset(v.wtable, 0xFF, n_maps * (size_t)g.slots * sizeof(int32_t)));
    INIT(hipMemset(v.bitmap, 0, n_maps * (size_t)((g.slots + 31) / 32) * sizeof(uint32_t)));
    INIT(hipMemset(v.acc, 0, n_maps * (size_t)cap * sizeof(NdtAcc)));
    INIT(hipMemset(v.counters, 0, n_maps * sizeof(NdtMapCounters)));
    INIT(hipMemset(v.rank_agg, 0, n_maps * (size_t)(NDT_RANK_SEGS + 2) * sizeof(uint32_t)));
    INIT(hipMemcpy(v.centres, s->centres_host.data(), n_maps * 3 * sizeof(double), hipMemcpyHostToDevice));
#undef INIT
    *out = s;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_destroy(ndtgpu_mapset *s)
{
    if (!s) return NDTGPU_OK;
    (void)hipDeviceSynchronize();       // (work on the caller's streams included)
    delete s;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_set_centre(ndtgpu_mapset *s, size_t map, const double centre[3])
{
    if (!s || !centre || map >= s->n_maps) return fail(NDTGPU_ERR_INVALID, "set_centre: bad argument");
    for (int a = 0; a < 3; a++) s->centres_host[map * 3 + a] = centre[a];
    s->nice_host[map] = ndt_grid_is_nice(s->v.grid, centre) ? 1 : 0;
    HIP_TRY(hipMemcpy(s->v.centres + map * 3, centre, 3 * sizeof(double), hipMemcpyHostToDevice));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_info(const ndtgpu_mapset *s, size_t *n_maps, int32_t cells_per_axis[3], uint32_t *max_cells)
{
    if (!s) return fail(NDTGPU_ERR_INVALID, "mapset_info: null");
    if (n_maps) *n_maps = s->n_maps;
    if (cells_per_axis)
        for (int a = 0; a < 3; a++) cells_per_axis[a] = s->v.grid.size[a];
    if (max_cells) *max_cells = s->v.grid.max_cells;
    return NDTGPU_OK;
}


// per-map range origins from host memory into the set's buffer, ordered behind the last launch that read it
static ndtgpu_status upload_origins(ndtgpu_mapset *s, const double *range_origins, size_t count, hipStream_t st, const double **orig_dev)
{
    *orig_dev = nullptr;
    if (!range_origins || !count) return NDTGPU_OK;
    ndtgpu_status orc = s->origins_reserve(count * 3, st);
    if (orc != NDTGPU_OK) return orc;
    HIP_TRY(hipMemcpyAsync(s->origins.get(), range_origins, count * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    *orig_dev = s->origins.get();
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_build(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_dev, size_t n_points,
                                  size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                  const double *range_origins, const ndtgpu_cell_params *cell, ndtgpu_stream stream)
{
    if (!s || first + count > s->n_maps) return fail(NDTGPU_ERR_INVALID, "mapset_build: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const double *orig_dev = nullptr;
    ndtgpu_status rc = upload_origins(s, range_origins, count, st, &orig_dev);
    if (rc != NDTGPU_OK) return rc;
    rc = mapset_build_core(s, first, count, xyz_dev, n_points, stride_bytes, map_stride_bytes, range_limit, orig_dev, cell, st);
    if (orig_dev && s->origins_used.record(st) != hipSuccess && rc == NDTGPU_OK) rc = fail(NDTGPU_ERR_HIP, "mapset_build: origins event");
    return rc;
}

ndtgpu_status ndtgpu_profiling_enable(ndtgpu_mapset *s, int on)
{
    if (!s) return fail(NDTGPU_ERR_INVALID, "profiling_enable: null");
    if (on)
        for (int k = 0; k < 4; k++)
            HIP_TRY(s->ev[k].create(hipEventDefault));
    s->profiling = on != 0;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_last_kernel_ms(ndtgpu_mapset *s, int which, float *ms)
{
    if (!s || !ms || which < 0 || which > 1 || !s->ev[2 * which + 1].valid())
        return fail(NDTGPU_ERR_INVALID, "last_kernel_ms: nothing recorded");
    HIP_TRY(s->ev[2 * which + 1].sync());
    HIP_TRY(hipEventElapsedTime(ms, s->ev[2 * which].get(), s->ev[2 * which + 1].get()));
    return NDTGPU_OK;
}

// Host clouds -> device staging area -> per-chunk kernel launches.  `count` clouds of n_points records, map_stride bytes
// apart, are cut into chunks of whole clouds that fit a pinned slot (16 MB); worker threads copy chunk after chunk from the
// caller's (pageable) memory into the ring of pinned slots, the calling thread sends every filled slot to the device on the
// copy stream and launches `launch(first_cloud, n_clouds, device pointer)` on `st` behind that copy: the copy of chunk
// k + 1 runs under the kernels of chunk k, nothing waits for the whole device.  Returns when the caller's memory has been
// read completely (the kernels may still be running on `st`).  Small inputs (< 24 MB) skip the ring: one ordinary copy.
static ndtgpu_status stage_host_clouds(ndtgpu_mapset *s, const void *xyz_host, size_t count, size_t n_points, size_t stride_bytes,
                                       size_t map_stride_bytes, hipStream_t st,
                                       const std::function<ndtgpu_status(size_t, size_t, const void *)> &launch)
{
    if (count == 0) return NDTGPU_OK;
    const size_t cloud_bytes = n_points * stride_bytes;
    size_t bytes = (count - 1) * map_stride_bytes + cloud_bytes;
    if (bytes == 0) bytes = 16;
    ndtgpu_status rc = s->ensure_stage(bytes);
    if (rc != NDTGPU_OK) return rc;
    // the staging area may still be read by the kernels of the previous call (another stream): order behind them
    HIP_TRY(s->stage_free.order(st));
    const size_t slot = ndtgpu_mapset::HOST_SLOT_BYTES;
    const char *force = getenv("NDTGPU_HOST_PIPE");            // 0: never the ring, 1: always (tests)
    // (the ring cuts the input into chunks of WHOLE clouds that lie one after the other: clouds that overlap in memory --
    //  map_stride_bytes < cloud_bytes, e.g. sliding windows over one point stream, or stride 0 -- take the single copy)
    const bool ring = n_points && map_stride_bytes >= cloud_bytes && map_stride_bytes <= slot && cloud_bytes <= slot &&
                      (force ? atoi(force) != 0 : bytes >= (24u << 20));
    if (!ring) {
        if (n_points) HIP_TRY(hipMemcpyAsync(s->stage.get(), xyz_host, bytes, hipMemcpyHostToDevice, st));   // (pageable: returns when read)
        rc = launch(0, count, s->stage.get());
    } else {
        rc = s->ensure_host_ring();
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(s->stage_free.order(s->host_copy_stream.get()));
        // clouds per chunk: a chunk of `per` clouds occupies (per - 1) * map_stride_bytes + cloud_bytes of its slot
        const size_t per = std::max<size_t>(1, std::min(count, 1 + (slot - cloud_bytes) / map_stride_bytes));
        const size_t n_chunks = (count + per - 1) / per;
        constexpr int R = ndtgpu_mapset::HOST_SLOTS;
        const int n_workers = (int)std::min<size_t>(4, n_chunks);
        std::vector<std::atomic<int>> staged(n_chunks);
        for (auto &a : staged) a.store(0, std::memory_order_relaxed);
        std::atomic<long> allowed((long)std::min<size_t>(n_chunks, R));     // chunks < allowed may be written into their slots
        std::atomic<int> stop(0);
        auto chunk_bytes = [&](size_t c) {
            const size_t c0 = c * per, cnt = std::min(per, count - c0);
            return (cnt - 1) * map_stride_bytes + cloud_bytes;
        };
        // a slot that an earlier CALL sent off may still be in flight
        for (int k = 0; k < R; k++)
            if (s->host_ev[k].valid()) { HIP_TRY(s->host_ev[k].sync()); s->host_ev[k].clear(); }
        std::vector<std::thread> workers;
        for (int w = 0; w < n_workers; w++)
            workers.emplace_back([&, w]() {
                for (size_t c = (size_t)w; c < n_chunks && !stop.load(std::memory_order_relaxed); c += (size_t)n_workers) {
                    while ((long)c >= allowed.load(std::memory_order_acquire) && !stop.load(std::memory_order_relaxed)) std::this_thread::yield();
                    if (stop.load(std::memory_order_relaxed)) break;
                    memcpy(s->host_ring[c % R].get(), (const char *)xyz_host + c * per * map_stride_bytes, chunk_bytes(c));
                    staged[c].store(1, std::memory_order_release);
                }
            });
        hipError_t herr = hipSuccess;
        ndtgpu_status lrc = NDTGPU_OK;
        // (profiling: one bracket around all chunks' launches -- ndtgpu_last_kernel_ms then reports the whole build, copies
        //  that the chunks wait for included -- instead of the last chunk's alone)
        const bool span = s->profiling && s->ev[0].get() && s->ev[1].get();
        if (span) { herr = s->ev[0].record(st); s->profile_span = true; }
        for (size_t c = 0; c < n_chunks && herr == hipSuccess && lrc == NDTGPU_OK; c++) {
            while (!staged[c].load(std::memory_order_acquire)) std::this_thread::yield();
            const int k = (int)(c % R);
            char *dst = s->stage.get() + c * per * map_stride_bytes;
            herr = hipMemcpyAsync(dst, s->host_ring[k].get(), chunk_bytes(c), hipMemcpyHostToDevice, s->host_copy_stream.get());
            if (herr == hipSuccess) herr = s->host_ev[k].record(s->host_copy_stream.get());
            if (herr == hipSuccess) herr = s->host_ev[k].order(st);
            if (herr == hipSuccess) lrc = launch(c * per, std::min(per, count - c * per), dst);
            // chunk c + R will reuse this slot: it may be written once this copy has left the host.  (The calling thread
            // waits here while the workers fill the other slots and the device builds chunk c under the next copies.)
            if (c + R < n_chunks && herr == hipSuccess) {
                herr = s->host_ev[k].sync();
                s->host_ev[k].clear();
                allowed.store((long)(c + R) + 1, std::memory_order_release);
            }
        }
        if (span) {
            s->profile_span = false;
            if (herr == hipSuccess && lrc == NDTGPU_OK) (void)s->ev[1].record(st);
        }
        if (herr != hipSuccess || lrc != NDTGPU_OK) stop.store(1);
        for (auto &t : workers) t.join();
        rc = herr != hipSuccess ? fail(NDTGPU_ERR_HIP, "host clouds: staging copy", herr) : lrc;
    }
    // (also after a failure: chunks that were launched before it may still be reading the staging area)
    if (s->stage_free.record(st) != hipSuccess && rc == NDTGPU_OK) return fail(NDTGPU_ERR_HIP, "host clouds: event");
    return rc;
}

ndtgpu_status ndtgpu_mapset_build_host_async(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_host,
                                             size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                             double range_limit, const double *range_origins, const ndtgpu_cell_params *cell,
                                             ndtgpu_stream stream)
{
    if (!s || (!xyz_host && n_points) || count == 0 || first + count > s->n_maps)
        return fail(NDTGPU_ERR_INVALID, "mapset_build_host: bad argument");
    // (the range origins of ALL maps go up once, before the first chunk: a copy from pageable memory per chunk made the calling
    //  thread wait behind the previous chunk's build every time)
    hipStream_t st = (hipStream_t)stream;
    const double *orig_dev = nullptr;
    ndtgpu_status rc = upload_origins(s, range_origins, count, st, &orig_dev);
    if (rc != NDTGPU_OK) return rc;
    rc = stage_host_clouds(s, xyz_host, count, n_points, stride_bytes, map_stride_bytes, st,
                           [&](size_t c0, size_t cnt, const void *dev) {
                               return mapset_build_core(s, first + c0, cnt, dev, n_points, stride_bytes, map_stride_bytes,
                                                        range_limit, orig_dev ? orig_dev + 3 * c0 : nullptr, cell, st);
                           });
    if (orig_dev && s->origins_used.record(st) != hipSuccess && rc == NDTGPU_OK) rc = fail(NDTGPU_ERR_HIP, "mapset_build: origins event");
    return rc;
}

ndtgpu_status ndtgpu_mapset_build_host(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_host,
                                       size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                       double range_limit, const double *range_origins, const ndtgpu_cell_params *cell)
{
    if (!s) return fail(NDTGPU_ERR_INVALID, "mapset_build_host: bad argument");
    ndtgpu_status rc = s->ensure_host_build_stream();
    if (rc != NDTGPU_OK) return rc;
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }             // (earlier work on these maps, whatever stream it used)
    rc = ndtgpu_mapset_build_host_async(s, first, count, xyz_host, n_points, stride_bytes, map_stride_bytes, range_limit,
                                        range_origins, cell, (ndtgpu_stream)s->host_build_stream.get());
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->host_build_stream.get()));       // the stream the maps were built on: no device-wide wait
    return NDTGPU_OK;
}

static ndtgpu_status read_counters(ndtgpu_mapset *s, size_t map, NdtMapCounters *c)
{
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    HIP_TRY(hipMemcpy(c, s->v.counters + map, sizeof *c, hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_counters(ndtgpu_mapset *s, size_t map, uint32_t out[8])
{
    if (!s || !out || map >= s->n_maps) return fail(NDTGPU_ERR_INVALID, "counters: bad argument");
    static_assert(sizeof(NdtMapCounters) == 32, "counter layout");
    NdtMapCounters c;
    ndtgpu_status rc = read_counters(s, map, &c);
    if (rc != NDTGPU_OK) return rc;
    memcpy(out, &c, 32);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_num_cells(ndtgpu_mapset *s, size_t map, uint32_t *n)
{
    if (!s || !n || map >= s->n_maps) return fail(NDTGPU_ERR_INVALID, "num_cells: bad argument");
    NdtMapCounters c;
    ndtgpu_status rc = read_counters(s, map, &c);
    if (rc != NDTGPU_OK) return rc;
    *n = c.n_cells;
    if (c.overflow) return fail(NDTGPU_ERR_CAPACITY, "map needs more cells than max_cells");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_export_cells(ndtgpu_mapset *s, size_t map, double *mean3, double *cov9, int32_t *idx3,
                                         uint32_t *npts)
{
    if (!s || map >= s->n_maps) return fail(NDTGPU_ERR_INVALID, "export_cells: bad argument");
    NdtMapCounters c;
    ndtgpu_status rc = read_counters(s, map, &c);
    if (rc != NDTGPU_OK) return rc;
    std::vector<NdtCell> host(c.n_cells);
    uint32_t sel = 0;
    if (s->v.cell_sel) HIP_TRY(hipMemcpy(&sel, s->v.cell_sel + map, sizeof sel, hipMemcpyDeviceToHost));
    if (c.n_cells)
        HIP_TRY(hipMemcpy(host.data(), ndt_cells_of(s->v, map, sel), c.n_cells * sizeof(NdtCell), hipMemcpyDeviceToHost));
    const NdtGrid &g = s->v.grid;
    for (uint32_t i = 0; i < c.n_cells; i++) {
        const NdtCell &k = host[i];
        if (mean3)
            for (int a = 0; a < 3; a++) mean3[3 * i + a] = k.mean[a];
        if (cov9) {
            double *o = cov9 + 9 * i;
            o[0] = k.cov[0]; o[1] = k.cov[1]; o[2] = k.cov[2];
            o[3] = k.cov[1]; o[4] = k.cov[3]; o[5] = k.cov[4];
            o[6] = k.cov[2]; o[7] = k.cov[4]; o[8] = k.cov[5];
        }
        if (idx3) {
            idx3[3 * i + 2] = (int32_t)(k.slot % g.size[2]);
            idx3[3 * i + 1] = (int32_t)((k.slot / g.size[2]) % g.size[1]);
            idx3[3 * i + 0] = (int32_t)(k.slot / ((uint32_t)g.size[2] * g.size[1]));
        }
        if (npts) npts[i] = k.n;
    }
    if (c.overflow) return fail(NDTGPU_ERR_CAPACITY, "map needs more cells than max_cells");
    return NDTGPU_OK;
}


ndtgpu_status ndtgpu_mapset_set_cells(ndtgpu_mapset *s, size_t map, const double *mean3, const double *cov9,
                                      size_t n_cells)
{
    if (!s || map >= s->n_maps || (n_cells && (!mean3 || !cov9)))
        return fail(NDTGPU_ERR_INVALID, "set_cells: bad argument");
    std::vector<NdtCell> cells;
    pack_cells(s->v.grid, &s->centres_host[map * 3], mean3, cov9, n_cells, true, cells);
    // one Gaussian per slot (a later cell replaces an earlier one, like setMean/setCov on the same
    // NDTCell), sorted by slot = the canonical cell order of the build kernel
    std::stable_sort(cells.begin(), cells.end(), [](const NdtCell &a, const NdtCell &b) { return a.slot < b.slot; });
    std::vector<NdtCell> uniq;
    for (size_t i = 0; i < cells.size(); i++) {
        if (!uniq.empty() && uniq.back().slot == cells[i].slot) uniq.back() = cells[i];
        else uniq.push_back(cells[i]);
    }
    if (uniq.size() > s->v.grid.max_cells) return fail(NDTGPU_ERR_CAPACITY, "set_cells: more cells than max_cells");
    ndtgpu_status rc = s->ensure_stage(std::max<size_t>(uniq.size() * sizeof(NdtCell), 16));
    if (rc != NDTGPU_OK) return rc;
    if (!uniq.empty()) HIP_TRY(hipMemcpy(s->stage.get(), uniq.data(), uniq.size() * sizeof(NdtCell), hipMemcpyHostToDevice));
    hipError_t e = ndt_launch_install_cells(s->v, map, (const NdtCell *)s->stage.get(), uniq.size(), nullptr);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "set_cells: launch", e);
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NDTGPU_OK;
}


ndtgpu_status ndtgpu_mapset_discard_cells(ndtgpu_mapset *s, size_t map, const float *xyz, size_t n_points)
{
    if (!s || map >= s->n_maps || (n_points && !xyz)) return fail(NDTGPU_ERR_INVALID, "discard_cells: bad argument");
    if (n_points == 0) return NDTGPU_OK;
    ndtgpu_status rc = s->ensure_stage(n_points * 3 * sizeof(float));
    if (rc != NDTGPU_OK) return rc;
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    HIP_TRY(hipMemcpy(s->stage.get(), xyz, n_points * 3 * sizeof(float), hipMemcpyHostToDevice));
    hipError_t e = ndt_launch_discard(s->v, map, (const float *)s->stage.get(), n_points, nullptr);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "discard_cells: launch", e);
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_enable_occupancy(ndtgpu_mapset *s)
{
    if (!s) return fail(NDTGPU_ERR_INVALID, "enable_occupancy: null");
    if (s->v.occ) return NDTGPU_OK;
    const size_t slots = (size_t)s->v.grid.slots, cap = s->v.grid.max_cells, n = s->n_maps;
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    // (locals until all of them exist: a failure leaves the set as it was, without occupancies)
    DeviceBuffer<float> occ;
    DeviceBuffer<long long> delta;
    DeviceBuffer<unsigned char> touched;
    DeviceBuffer<NdtCell> alt;
    DeviceBuffer<uint32_t> sel;
    const size_t blocks = (slots + 255) / 256;
    hipError_t e;
    if ((e = occ.alloc(n * slots)) != hipSuccess ||
        (e = delta.alloc(n * slots)) != hipSuccess ||
        (e = touched.alloc(n * blocks)) != hipSuccess ||
        (e = hipMemset(touched.get(), 0, n * blocks)) != hipSuccess ||
        (e = alt.alloc(n * cap)) != hipSuccess ||
        (e = sel.alloc(n)) != hipSuccess ||
        (e = hipMemset(occ.get(), 0, n * slots * sizeof(float))) != hipSuccess ||
        (e = hipMemset(delta.get(), 0, n * slots * sizeof(long long))) != hipSuccess ||
        (e = hipMemset(sel.get(), 0, n * sizeof(uint32_t))) != hipSuccess)
        return fail(NDTGPU_ERR_ALLOC, "enable_occupancy: device memory", e);
    s->occ = std::move(occ); s->occ_delta = std::move(delta); s->occ_touched = std::move(touched);
    s->cells_alt = std::move(alt); s->cell_sel = std::move(sel);
    s->v.occ = s->occ.get(); s->v.occ_delta = s->occ_delta.get(); s->v.occ_touched = s->occ_touched.get();
    s->v.cells_alt = s->cells_alt.get(); s->v.cell_sel = s->cell_sel.get();
    return NDTGPU_OK;
}

void ndtgpu_default_fuse_params(ndtgpu_fuse_params *p)
{
    p->maxz = 25.0;             // fuser_hmt.cpp:485
    p->sensor_noise = 0.06;
    p->maxnumpoints = 1e5;      // fuser_hmt.cpp:486
    p->occupancy_limit = 255.0;
    p->n_min = 3;
    p->eval_factor = 1000.0;
}

ndtgpu_status ndtgpu_mapset_add_cloud(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_dev, size_t n_points,
                                      size_t stride_bytes, size_t map_stride_bytes, const double *origins,
                                      const ndtgpu_fuse_params *prm, ndtgpu_stream stream)
{
    if (!s || first + count > s->n_maps || (!xyz_dev && n_points) || stride_bytes < 12 || (stride_bytes & 3) ||
        n_points > 0xFFFFFFFFull || (count && !origins))
        return fail(NDTGPU_ERR_INVALID, "add_cloud: bad argument");
    if (!s->v.occ) return fail(NDTGPU_ERR_INVALID, "add_cloud: call ndtgpu_mapset_enable_occupancy first (NDTMap::initialize)");
    if (count == 0) return NDTGPU_OK;
    const ndtgpu_fuse_params fp = params_or_default(prm, ndtgpu_default_fuse_params);
    if (!(fp.occupancy_limit > 0)) return fail(NDTGPU_ERR_INVALID, "add_cloud: occupancy_limit must be positive");
    hipStream_t st = (hipStream_t)stream;
    {
        ndtgpu_status orc = s->origins_reserve(count * 3, st);
        if (orc != NDTGPU_OK) return orc;
    }
    HIP_TRY(hipMemcpyAsync(s->origins.get(), origins, count * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    NdtFuseParams p;
    p.maxz = fp.maxz; p.sensor_noise = fp.sensor_noise; p.maxnumpoints = fp.maxnumpoints;
    p.occupancy_limit = fp.occupancy_limit; p.eval_factor = fp.eval_factor; p.n_min = fp.n_min;
    hipError_t e = ndt_launch_fuse(s->v, first, count, xyz_dev, n_points, stride_bytes, map_stride_bytes, s->origins.get(), p,
                                   s->nice_range(first, count), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "add_cloud: launch", e);
    { ndtgpu_status trc = s->touch(st); if (trc != NDTGPU_OK) return trc; }
    HIP_TRY(s->origins_used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_add_cloud_host_async(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_host,
                                                 size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                 const double *origins, const ndtgpu_fuse_params *prm, ndtgpu_stream stream)
{
    if (!s || (!xyz_host && n_points) || count == 0 || first + count > s->n_maps || !origins)
        return fail(NDTGPU_ERR_INVALID, "add_cloud_host: bad argument");
    return stage_host_clouds(s, xyz_host, count, n_points, stride_bytes, map_stride_bytes, (hipStream_t)stream,
                             [&](size_t c0, size_t cnt, const void *dev) {
                                 return ndtgpu_mapset_add_cloud(s, first + c0, cnt, dev, n_points, stride_bytes, map_stride_bytes,
                                                                origins + 3 * c0, prm, stream);
                             });
}

ndtgpu_status ndtgpu_mapset_add_cloud_host(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_host,
                                           size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                           const double *origins, const ndtgpu_fuse_params *prm)
{
    if (!s) return fail(NDTGPU_ERR_INVALID, "add_cloud_host: bad argument");
    ndtgpu_status rc = s->ensure_host_build_stream();
    if (rc != NDTGPU_OK) return rc;
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    rc = ndtgpu_mapset_add_cloud_host_async(s, first, count, xyz_host, n_points, stride_bytes, map_stride_bytes, origins, prm,
                                            (ndtgpu_stream)s->host_build_stream.get());
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->host_build_stream.get()));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_clear(ndtgpu_mapset *s, size_t first, size_t count)
{
    if (!s || first + count > s->n_maps) return fail(NDTGPU_ERR_INVALID, "mapset_clear: bad argument");
    if (count == 0) return NDTGPU_OK;
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    const NdtGrid &g = s->v.grid;
    const size_t slots = (size_t)g.slots;
    HIP_TRY(hipMemset(s->v.rankmap + first * ndt_rm_stride(g), 0, count * ndt_rm_stride(g) * sizeof(uint2)));
    HIP_TRY(hipMemset(s->v.counters + first, 0, count * sizeof(NdtMapCounters)));
    if (s->v.occ) {
        HIP_TRY(hipMemset(s->v.occ + first * slots, 0, count * slots * sizeof(float)));
        HIP_TRY(hipMemset(s->v.cell_sel + first, 0, count * sizeof(uint32_t)));
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_export_occupancy(ndtgpu_mapset *s, size_t map, float *occ_out)
{
    if (!s || map >= s->n_maps || !occ_out) return fail(NDTGPU_ERR_INVALID, "export_occupancy: bad argument");
    if (!s->v.occ) return fail(NDTGPU_ERR_INVALID, "export_occupancy: occupancy not enabled on this set");
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    HIP_TRY(hipMemcpy(occ_out, s->v.occ + map * (size_t)s->v.grid.slots, (size_t)s->v.grid.slots * sizeof(float), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_import_occupancy(ndtgpu_mapset *s, size_t map, const float *occ)
{
    if (!s || map >= s->n_maps || !occ) return fail(NDTGPU_ERR_INVALID, "import_occupancy: bad argument");
    if (!s->v.occ) return fail(NDTGPU_ERR_INVALID, "import_occupancy: occupancy not enabled on this set");
    { ndtgpu_status wrc_ = s->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    HIP_TRY(hipMemcpy(s->v.occ + map * (size_t)s->v.grid.slots, occ, (size_t)s->v.grid.slots * sizeof(float), hipMemcpyHostToDevice));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_overlap_score_batch(ndtgpu_mapset *rs, const uint32_t *ridx, ndtgpu_mapset *ms, const uint32_t *midx,
                                         const double *T16, size_t n_links, double *score, int64_t *nb_sum,
                                         ndtgpu_stream stream)
{
    if (!rs || !ms || (n_links && (!ridx || !midx || !T16 || !score)))
        return fail(NDTGPU_ERR_INVALID, "overlap_score: bad argument");
    if (!rs->v.occ || !ms->v.occ) return fail(NDTGPU_ERR_INVALID, "overlap_score: occupancy not enabled on both sets");
    if (n_links == 0) return NDTGPU_OK;
    for (size_t k = 0; k < n_links; k++)
        if (ridx[k] >= rs->n_maps || midx[k] >= ms->n_maps) return fail(NDTGPU_ERR_INVALID, "overlap_score: map index");
    hipStream_t st = (hipStream_t)stream;
    { ndtgpu_status wrc_ = rs->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    { ndtgpu_status wrc_ = ms->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    // Every link walks a LIST of its moving map's cells with a reading: every distinct moving map of the batch is scanned twice
    // (count, then its (slot, occupancy) pairs in slot order), a link then visits a few thousand pairs instead of the map's whole
    // dense array.  Which kernel serves a link does NOT depend on the other links of its batch (the dense kernel adds in
    // another order: a link's score must not change with the way links are chunked or sharded over ranks).
    // NDTGPU_OVERLAP_DENSE=1: the dense kernel for every link (A/B).
    const char *dense_env = getenv("NDTGPU_OVERLAP_DENSE");
    std::vector<uint32_t> list_of_link, list_maps;
    if (!(dense_env && atoi(dense_env) != 0)) {
        std::vector<int32_t> list_of_map(ms->n_maps, -1);
        list_of_link.resize(n_links);
        for (size_t k = 0; k < n_links; k++) {
            int32_t &u = list_of_map[midx[k]];
            if (u < 0) { u = (int32_t)list_maps.size(); list_maps.push_back(midx[k]); }
            list_of_link[k] = (uint32_t)u;
        }
    }
    const size_t U = list_maps.size();
    const size_t bT = n_links * 16 * sizeof(double), bI = n_links * sizeof(uint32_t), bS = n_links * sizeof(double);
    StageLayout L;
    const size_t off_T = L.take(bT), off_r = L.take(bI), off_m = L.take(bI), off_s = L.take(bS),
                 off_n = L.take(n_links * sizeof(long long)),
                 off_l = L.take(U ? bI : 0),                        // list of every link
                 off_u = L.take(U * sizeof(uint32_t)),              // the maps of the lists
                 off_o = L.take((U + 1) * sizeof(unsigned)),        // counts, then offsets
                 off_p = L.at;                                      // the pairs
    ndtgpu_status rc = rs->ensure_stage(off_p);
    if (rc != NDTGPU_OK) return rc;
    std::vector<unsigned> offs(U + 1, 0u);
    if (U) {
        // pass 1: how many cells with a reading every listed map has (before the buffer is laid out for good: it may move)
        char *b0 = rs->stage.get();
        HIP_TRY(hipMemcpyAsync(b0 + off_u, list_maps.data(), U * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipError_t e0 = ndt_launch_occ_count(ms->v, 0, (const uint32_t *)(b0 + off_u), U, (unsigned *)(b0 + off_o), st);
        if (e0 != hipSuccess) return fail(NDTGPU_ERR_HIP, "overlap_score: count launch", e0);
        HIP_TRY(hipMemcpyAsync(offs.data(), b0 + off_o, U * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        unsigned long long at = 0;
        for (size_t u = 0; u < U; u++) { const unsigned c = offs[u]; offs[u] = (unsigned)at; at += c; }
        if (at > 0xFFFFFFFFull) return fail(NDTGPU_ERR_CAPACITY, "overlap_score: too many occupied cells in one batch");
        offs[U] = (unsigned)at;
        rc = rs->ensure_stage(off_p + (size_t)at * 8u);
        if (rc != NDTGPU_OK) return rc;
    }
    char *base = rs->stage.get();
    HIP_TRY(hipMemcpyAsync(base + off_T, T16, bT, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_r, ridx, bI, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_m, midx, bI, hipMemcpyHostToDevice, st));
    hipError_t e;
    if (U) {
        HIP_TRY(hipMemcpyAsync(base + off_l, list_of_link.data(), bI, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + off_u, list_maps.data(), U * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + off_o, offs.data(), (U + 1) * sizeof(unsigned), hipMemcpyHostToDevice, st));
        e = ndt_launch_occ_list(ms->v, (const uint32_t *)(base + off_u), U, (const unsigned *)(base + off_o), base + off_p, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "overlap_score: list launch", e);
        e = ndt_launch_overlap_lists(rs->v, (const uint32_t *)(base + off_r), ms->v, (const uint32_t *)(base + off_m),
                                     (const uint32_t *)(base + off_l), (const unsigned *)(base + off_o), base + off_p,
                                     (const double *)(base + off_T), n_links, (double *)(base + off_s), (long long *)(base + off_n), st);
    } else {
        e = ndt_launch_overlap(rs->v, (const uint32_t *)(base + off_r), ms->v, (const uint32_t *)(base + off_m),
                               (const double *)(base + off_T), n_links, (double *)(base + off_s), (long long *)(base + off_n), st);
    }
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "overlap_score: launch", e);
    HIP_TRY(hipMemcpyAsync(score, base + off_s, bS, hipMemcpyDeviceToHost, st));
    if (nb_sum) HIP_TRY(hipMemcpyAsync(nb_sum, base + off_n, n_links * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NDTGPU_OK;
}

static_assert(sizeof(ndtgpu_cell_record) == sizeof(NdtCell) && offsetof(ndtgpu_cell_record, slot) == offsetof(NdtCell, slot) &&
              offsetof(ndtgpu_cell_record, cov) == offsetof(NdtCell, cov), "the exchange record is the device cell record");

size_t ndtgpu_mapset_pack_bytes(const ndtgpu_mapset *s, uint32_t cells_cap, int with_occupancy)
{
    if (!s) return 0;
    size_t b = sizeof(ndtgpu_packed_header) + (size_t)cells_cap * sizeof(NdtCell);
    if (with_occupancy) b += (size_t)s->v.grid.slots * sizeof(float);
    return (b + 15u) & ~(size_t)15u;
}

ndtgpu_status ndtgpu_mapset_pack_cells_device(ndtgpu_mapset *s, size_t first, size_t count, void *buf_dev, size_t stride,
                                              uint32_t cells_cap, int with_occupancy, ndtgpu_stream stream)
{
    if (!s || first + count > s->n_maps || (count && !buf_dev) || ((uintptr_t)buf_dev & 15u) || (stride & 15u) ||
        stride < ndtgpu_mapset_pack_bytes(s, cells_cap, with_occupancy))
        return fail(NDTGPU_ERR_INVALID, "pack_cells: bad argument (16-byte aligned buffer, stride >= ndtgpu_mapset_pack_bytes)");
    if (with_occupancy && !s->v.occ) return fail(NDTGPU_ERR_INVALID, "pack_cells: the set carries no occupancies");
    hipError_t e = ndt_launch_pack(s->v, first, count, buf_dev, stride, cells_cap, with_occupancy ? 1 : 0, 0u, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pack_cells: launch", e);
    return NDTGPU_OK;
}

size_t ndtgpu_mapset_pack_bytes_sparse(const ndtgpu_mapset *s, uint32_t cells_cap, uint32_t occ_cap)
{
    if (!s) return 0;
    const size_t b = sizeof(ndtgpu_packed_header) + (size_t)cells_cap * sizeof(NdtCell) + ndt_pack_sparse_occ_bytes(occ_cap);
    return (b + 15u) & ~(size_t)15u;
}

ndtgpu_status ndtgpu_mapset_occupied_cells_max(ndtgpu_mapset *s, size_t first, size_t count, uint32_t *max_occupied,
                                               ndtgpu_stream stream)
{
    if (!s || !max_occupied || first + count > s->n_maps) return fail(NDTGPU_ERR_INVALID, "occupied_cells_max: bad argument");
    if (!s->v.occ) return fail(NDTGPU_ERR_INVALID, "occupied_cells_max: the set carries no occupancies");
    *max_occupied = 0;
    if (count == 0) return NDTGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    DeviceBuffer<unsigned> counts_dev;
    HIP_TRY(counts_dev.alloc(count));
    std::vector<unsigned> counts(count);
    hipError_t e = ndt_launch_occ_count(s->v, first, nullptr, count, counts_dev.get(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), counts_dev.get(), count * sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // (counts_dev is free once the stream has drained)
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "occupied_cells_max", e);
    for (unsigned c : counts) *max_occupied = std::max<uint32_t>(*max_occupied, c);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_pack_cells_sparse_device(ndtgpu_mapset *s, size_t first, size_t count, void *buf_dev, size_t stride,
                                                     uint32_t cells_cap, uint32_t occ_cap, ndtgpu_stream stream)
{
    if (!s || first + count > s->n_maps || (count && !buf_dev) || ((uintptr_t)buf_dev & 15u) || (stride & 15u) ||
        stride < ndtgpu_mapset_pack_bytes_sparse(s, cells_cap, occ_cap))
        return fail(NDTGPU_ERR_INVALID, "pack_cells_sparse: bad argument (16-byte aligned buffer, stride >= ndtgpu_mapset_pack_bytes_sparse)");
    if (!s->v.occ) return fail(NDTGPU_ERR_INVALID, "pack_cells_sparse: the set carries no occupancies");
    hipError_t e = ndt_launch_pack(s->v, first, count, buf_dev, stride, cells_cap, 2, occ_cap, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pack_cells_sparse: launch", e);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_unpack_cells_device(ndtgpu_mapset *s, size_t first, size_t count, const void *buf_dev, size_t stride,
                                                int with_occupancy, ndtgpu_stream stream)
{
    if (!s || first + count > s->n_maps || (count && !buf_dev) || ((uintptr_t)buf_dev & 15u) || (stride & 15u) ||
        stride < sizeof(ndtgpu_packed_header))
        return fail(NDTGPU_ERR_INVALID, "unpack_cells: bad argument");
    if (with_occupancy && !s->v.occ) return fail(NDTGPU_ERR_INVALID, "unpack_cells: call ndtgpu_mapset_enable_occupancy first");
    hipError_t e = ndt_launch_unpack(s->v, first, count, buf_dev, stride, with_occupancy ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "unpack_cells: launch", e);
    return s->touch((hipStream_t)stream);
}

}  // extern "C"
