// ndtgpu_marker.hip -- C-ABI (include/ndtgpu.h "marker export") of ndt_visualisation::markerNDTCells (ndt_rviz.h:1090-1153, 1163-1233),
// markerParticlesNDTMCL3D (ndt_rviz.h:1277-1297) and ndt_feature::markerNDTFeatureLinks (ndt_feature_rviz.h:282-313).  Host side only:
// the handle, the argument checks, the staging of the host forms and the pure host entries; the work runs in csrc/ndt_marker.hip.
#include "ndtgpu_host.h"
#include "ndt_marker.h"

struct ndtgpu_marker {
    size_t max_maps = 0, max_links = 0;
    DeviceBuffer<uint32_t> tile;           // the tile words of a selection: made by the first call, grown by later ones
    DeviceBuffer<uint32_t> count;          // [4]: written, true total, overflow, flags of the last selection
    bool counted = false;                  // a selection has been made
    HostStage host;                        // the host forms' staging
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the host forms' stream (last: ndtgpu_resource.h)
};

static ndtgpu_marker_params marker_params(const ndtgpu_marker_params *prm) { return params_or_default(prm, ndtgpu_default_marker_params); }

// room for a selection of n_tiles tiles on `st`, behind the handle's previous call (which may have run on another stream)
static ndtgpu_status marker_selection(ndtgpu_marker *h, const char *who, size_t n_tiles, size_t capacity, hipStream_t st, NdtMarkerSel &sel)
{
    if (h->tile.reserve(std::max<size_t>(n_tiles, 1), h->used) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "tile counts");
    HIP_TRY(h->used.order(st));
    sel.tile = h->tile.get();
    sel.count = h->count.get();
    sel.capacity = capacity;
    return NDTGPU_OK;
}

static ndtgpu_status marker_cells_args(const char *who, const ndtgpu_mapset *s, size_t first, size_t count, const ndtgpu_marker_params &p,
                                       const void *points, size_t capacity)
{
    if (const char *bad = ndt_marker_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (capacity && !points) return fail_in(NDTGPU_ERR_INVALID, who, "null points with a capacity");
    if (!s) return fail_in(NDTGPU_ERR_INVALID, who, "null map set");
    if (const char *bad = ndt_marker_check_maps(s->n_maps, first, count, s->v.grid.max_cells, capacity)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    return NDTGPU_OK;
}

static ndtgpu_status marker_links_args(const char *who, const void *T16_nodes, size_t n_nodes, const void *ref, const void *mov, size_t n_links,
                                       const ndtgpu_marker_params &p, const void *points, size_t capacity)
{
    const char *bad = ndt_marker_check_params(p);
    if (!bad) bad = ndt_marker_check_links(n_nodes, n_links, capacity);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (n_links && (!ref || !mov)) return fail_in(NDTGPU_ERR_INVALID, who, "null ref or mov");
    if (n_nodes && !T16_nodes) return fail_in(NDTGPU_ERR_INVALID, who, "null node poses");
    if (capacity && !points) return fail_in(NDTGPU_ERR_INVALID, who, "null points with a capacity");
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_marker_params(ndtgpu_marker_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->min_eval = 0.0001;                  // ndt_rviz.h: `if (evals(j) < 0.0001) continue;`
    p->particle_length = 0.3;              // ndt_rviz.h:1292: T * (0.3, 0, 0)
    p->skip_negative = 0;                  // markerNDTFeatureLinks: skipOdom
}

uint32_t ndtgpu_marker_tile(void) { return NDT_MARKER_TILE; }

ndtgpu_status ndtgpu_marker_check(size_t max_maps_per_call, size_t max_links, size_t n_maps, size_t first, size_t count, size_t max_cells,
                                  size_t n_nodes, size_t n_links, size_t capacity, const ndtgpu_marker_params *prm)
{
    const char *bad = ndt_marker_check(max_maps_per_call, max_links, n_maps, first, count, max_cells, n_nodes, n_links, capacity, marker_params(prm));
    return bad ? fail_in(NDTGPU_ERR_INVALID, "marker_check", bad) : NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_eig3(const double cov6[6], double evals3[3], double V9[9])
{
    if (!cov6 || !evals3 || !V9) return fail(NDTGPU_ERR_INVALID, "marker_eig3: null cov6, evals3 or V9");
    double ev[3], V[3][3];
    ndt_marker_eig3(cov6, ev, V);
    memcpy(evals3, ev, sizeof ev);
    memcpy(V9, V, sizeof V);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_cell(const double mean3[3], const double cov6[6], const double *T16, const ndtgpu_marker_params *prm, double seg18[18],
                                 double evals3[3], uint32_t *n_seg, uint32_t *flags)
{
    const ndtgpu_marker_params p = marker_params(prm);
    if (const char *bad = ndt_marker_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, "marker_cell", bad);
    if (!mean3 || !cov6 || !seg18 || !n_seg || !flags) return fail(NDTGPU_ERR_INVALID, "marker_cell: null mean3, cov6, seg18, n_seg or flags");
    double seg[3][2][3], ev[3], T12[12] = {};
    if (T16) ndt_marker_pose12(T16, T12);
    uint32_t f = 0;
    *n_seg = ndt_marker_cell(mean3, cov6, T16 != nullptr, T12, p.min_eval, seg, f, ev);
    *flags = f;
    memset(seg18, 0, 18 * sizeof(double));
    memcpy(seg18, seg, (size_t)*n_seg * 6 * sizeof(double));
    if (evals3) memcpy(evals3, ev, sizeof ev);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_create(size_t max_maps_per_call, size_t max_links, ndtgpu_marker **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "marker_create: out is NULL");
    *out = nullptr;
    if (const char *bad = ndt_marker_check_handle(max_maps_per_call, max_links)) return fail_in(NDTGPU_ERR_INVALID, "marker_create", bad);
    ndtgpu_marker *h;
    const ndtgpu_status rc = handle_new("marker_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->max_maps = max_maps_per_call;
    h->max_links = max_links;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "marker_create: device buffers", expr)
    TRY(h->count.alloc(4));
    TRY(h->tile.alloc(std::max<size_t>(ndt_marker_tiles(max_links), 1)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_destroy(ndtgpu_marker *h) { return handle_destroy(h, "marker_destroy"); }

ndtgpu_status ndtgpu_mapset_markers_device(ndtgpu_marker *h, ndtgpu_mapset *set, size_t first, size_t count, const double *T16_dev,
                                           const ndtgpu_marker_params *prm, double *points_dev, uint32_t *src_dev, size_t capacity,
                                           ndtgpu_stream stream)
{
    const char *who = "mapset_markers_device";
    const ndtgpu_marker_params p = marker_params(prm);
    ndtgpu_status rc = marker_cells_args(who, set, first, count, p, points_dev, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (count > h->max_maps) return fail_in(NDTGPU_ERR_CAPACITY, who, "more maps than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    NdtMarkerCells c{};
    c.first = (uint32_t)first;
    c.count = (uint32_t)count;
    c.tiles_per_map = (uint32_t)ndt_marker_tiles(set->v.grid.max_cells);
    c.T16 = T16_dev;
    c.min_eval = p.min_eval;
    c.points = points_dev;
    c.src = src_dev;
    NdtMarkerSel sel{};
    if ((rc = marker_selection(h, who, (size_t)c.count * c.tiles_per_map, capacity, st, sel)) != NDTGPU_OK) return rc;
    if ((rc = set->wait_all_on(st)) != NDTGPU_OK) return rc;       // (builds on other streams)
    const hipError_t e = ndt_marker_cells_launch(set->v, c, sel, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mapset_markers_device: launch", e);
    h->counted = true;
    HIP_TRY(h->used.record(st));
    return set->touch(st);
}

ndtgpu_status ndtgpu_marker_count(ndtgpu_marker *h, size_t *n_segments, int32_t *overflow, uint32_t *flags)
{
    if (!n_segments) return fail(NDTGPU_ERR_INVALID, "marker_count: null n_segments");
    if (!h) return fail(NDTGPU_ERR_INVALID, "marker_count: null handle");
    if (!h->counted) return fail(NDTGPU_ERR_INVALID, "marker_count: no cell or link call has been made");
    HIP_TRY(h->used.sync());
    uint32_t w[4];
    HIP_TRY(hipMemcpy(w, h->count.get(), sizeof w, hipMemcpyDeviceToHost));
    *n_segments = w[1];
    if (overflow) *overflow = (int32_t)w[2];
    if (flags) *flags = w[3];
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_markers(ndtgpu_marker *h, ndtgpu_mapset *set, size_t first, size_t count, const double *T16,
                                    const ndtgpu_marker_params *prm, double *points, uint32_t *src, size_t capacity, size_t *n_segments,
                                    int32_t *overflow, uint32_t *flags)
{
    const char *who = "mapset_markers";
    const ndtgpu_marker_params p = marker_params(prm);
    ndtgpu_status rc = marker_cells_args(who, set, first, count, p, points, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!n_segments) return fail_in(NDTGPU_ERR_INVALID, who, "null n_segments");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    StageLayout in, outl;
    in.take(sizeof(double));               // (never an empty block)
    outl.take(sizeof(double));
    const size_t o_T = in.take(T16 ? count * 16 * sizeof(double) : 0);
    const size_t o_pts = outl.take(capacity * 6 * sizeof(double)), o_src = outl.take(src ? capacity * 2 * sizeof(uint32_t) : 0);
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    if (T16 && count) memcpy(hs.in_host(o_T), T16, count * 16 * sizeof(double));
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_mapset_markers_device(h, set, first, count, T16 ? (const double *)hs.in_dev(o_T) : nullptr, &p,
                                      capacity ? (double *)hs.out_dev(o_pts) : nullptr, src ? (uint32_t *)hs.out_dev(o_src) : nullptr, capacity,
                                      (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    if ((rc = ndtgpu_marker_count(h, n_segments, overflow, flags)) != NDTGPU_OK) return rc;
    const size_t m = std::min(*n_segments, capacity);
    if (m) memcpy(points, hs.out_host(o_pts), m * 6 * sizeof(double));
    if (m && src) memcpy(src, hs.out_host(o_src), m * 2 * sizeof(uint32_t));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_links_device(ndtgpu_marker *h, const double *T16_nodes_dev, size_t n_nodes, const uint32_t *ref_dev,
                                         const uint32_t *mov_dev, const double *score_dev, size_t n_links, const ndtgpu_marker_params *prm,
                                         double *points_dev, size_t capacity, ndtgpu_stream stream)
{
    const char *who = "marker_links_device";
    const ndtgpu_marker_params p = marker_params(prm);
    ndtgpu_status rc = marker_links_args(who, T16_nodes_dev, n_nodes, ref_dev, mov_dev, n_links, p, points_dev, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (n_links > h->max_links) return fail_in(NDTGPU_ERR_CAPACITY, who, "more links than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    NdtMarkerLinks l{};
    l.T16_nodes = T16_nodes_dev;
    l.ref = ref_dev;
    l.mov = mov_dev;
    l.score = score_dev;
    l.n_nodes = (uint32_t)n_nodes;
    l.n_links = (uint32_t)n_links;
    l.skip_negative = p.skip_negative;
    l.points = points_dev;
    NdtMarkerSel sel{};
    if ((rc = marker_selection(h, who, ndt_marker_tiles(n_links), capacity, st, sel)) != NDTGPU_OK) return rc;
    const hipError_t e = ndt_marker_links_launch(l, sel, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "marker_links_device: launch", e);
    h->counted = true;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_marker_links(ndtgpu_marker *h, const double *T16_nodes, size_t n_nodes, const uint32_t *ref, const uint32_t *mov,
                                  const double *score, size_t n_links, const ndtgpu_marker_params *prm, double *points, size_t capacity,
                                  size_t *n_segments, int32_t *overflow)
{
    const char *who = "marker_links";
    const ndtgpu_marker_params p = marker_params(prm);
    ndtgpu_status rc = marker_links_args(who, T16_nodes, n_nodes, ref, mov, n_links, p, points, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!n_segments) return fail_in(NDTGPU_ERR_INVALID, who, "null n_segments");
    for (size_t i = 0; i < n_links; i++)            // (the links the device form would flag: a skipped link's indices are never read)
        if (ndt_marker_link_kept(score, i, p.skip_negative) && ndt_marker_link_bad(ref[i], mov[i], (uint32_t)n_nodes)) return fail_in(NDTGPU_ERR_INVALID, who, "a node index is not one of the n_nodes nodes");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    StageLayout in, outl;
    in.take(sizeof(double));               // (never an empty block)
    outl.take(sizeof(double));
    const size_t o_T = in.take(n_nodes * 16 * sizeof(double)), o_ref = in.take(n_links * sizeof(uint32_t)), o_mov = in.take(n_links * sizeof(uint32_t)),
                 o_sc = in.take(score ? n_links * sizeof(double) : 0);
    const size_t o_pts = outl.take(capacity * 6 * sizeof(double));
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    if (n_nodes) memcpy(hs.in_host(o_T), T16_nodes, n_nodes * 16 * sizeof(double));
    if (n_links) {
        memcpy(hs.in_host(o_ref), ref, n_links * sizeof(uint32_t));
        memcpy(hs.in_host(o_mov), mov, n_links * sizeof(uint32_t));
        if (score) memcpy(hs.in_host(o_sc), score, n_links * sizeof(double));
    }
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_marker_links_device(h, n_nodes ? (const double *)hs.in_dev(o_T) : nullptr, n_nodes, n_links ? (const uint32_t *)hs.in_dev(o_ref) : nullptr,
                                    n_links ? (const uint32_t *)hs.in_dev(o_mov) : nullptr, score ? (const double *)hs.in_dev(o_sc) : nullptr, n_links,
                                    &p, capacity ? (double *)hs.out_dev(o_pts) : nullptr, capacity, (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    if ((rc = ndtgpu_marker_count(h, n_segments, overflow, nullptr)) != NDTGPU_OK) return rc;
    const size_t m = std::min(*n_segments, capacity);
    if (m) memcpy(points, hs.out_host(o_pts), m * 6 * sizeof(double));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_markers_device(ndtgpu_mcl *mcl, size_t first, size_t count, const ndtgpu_marker_params *prm, double *points_dev,
                                        ndtgpu_stream stream)
{
    const char *who = "mcl_markers_device";
    const ndtgpu_marker_params p = marker_params(prm);
    if (const char *bad = ndt_marker_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!points_dev) return fail_in(NDTGPU_ERR_INVALID, who, "null points_dev");
    MclParticles v;
    const ndtgpu_status rc = mcl_particles_view(mcl, first, count, who, v);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(v.used->order(st));            // (behind the bank's last call, whatever stream it ran on)
    const hipError_t e = ndt_marker_particles_launch((const double *)v.T, v.n, p.particle_length, points_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "mcl_markers_device: launch", e);
    HIP_TRY(v.used->record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mcl_markers(ndtgpu_mcl *mcl, size_t first, size_t count, const ndtgpu_marker_params *prm, double *points)
{
    const char *who = "mcl_markers";
    const ndtgpu_marker_params p = marker_params(prm);
    if (const char *bad = ndt_marker_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!points) return fail_in(NDTGPU_ERR_INVALID, who, "null points");
    MclParticles v;
    ndtgpu_status rc = mcl_particles_view(mcl, first, count, who, v);
    if (rc != NDTGPU_OK) return rc;
    DeviceBuffer<double> out;              // (a local of the owning type: gone on return)
    if (out.alloc(v.n * 6) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "device buffer");
    if ((rc = ndtgpu_mcl_markers_device(mcl, first, count, &p, out.get(), (ndtgpu_stream)v.hst)) != NDTGPU_OK) return rc;
    HIP_TRY(hipMemcpyAsync(points, out.get(), v.n * 6 * sizeof(double), hipMemcpyDeviceToHost, v.hst));
    HIP_TRY(hipStreamSynchronize(v.hst));
    return NDTGPU_OK;
}

}   // extern "C"
