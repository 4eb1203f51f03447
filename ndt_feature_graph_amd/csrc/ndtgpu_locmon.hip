// ndtgpu_locmon.hip -- C-ABI (include/ndtgpu.h "localisation monitor") of the scan-pose evaluator of flirtlib_ros
// (localization_monitor.cpp:41-120) and the relocalisation pick of localization_monitor_node.cpp:348-372.  Host side only: the
// handle, the argument checks, the beam table, the upload of the origins and the lattice tables, the staging of the host forms
// and the pure host entries; the work runs in csrc/ndt_locmon.hip.
#include "ndtgpu_host.h"
#include "ndt_locmon.h"

#include <limits>

struct ndtgpu_locmon {
    size_t max_grids = 0, max_pixels = 0, max_beams = 0, max_candidates = 0, chunk = 0;
    // what is installed
    size_t n_grids = 0, width = 0, height = 0, n_beams = 0;
    double resolution = 0.0, max_dist = 0.0;
    DeviceBuffer<uint16_t> field;          // [max_pixels]
    DeviceBuffer<uint8_t> rowdist;         // [max_pixels]: the row pass's output
    DeviceBuffer<double> origin;           // [max_grids][2]
    DeviceBuffer<double> beams;            // [max_beams][2]
    DeviceBuffer<uint32_t> cand_key;       // [chunk]
    DeviceBuffer<unsigned long long> tile_word;
    PinnedBuffer<double> origin_pin, beams_pin;
    LatticeTables lattice;                 // the lattice tables of a search
    HostStage host;                        // the host forms' staging
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the host forms' stream (last: ndtgpu_resource.h)
};

static ndtgpu_locmon_params locmon_params(const ndtgpu_locmon_params *prm) { return params_or_default(prm, ndtgpu_default_locmon_params); }

static NdtLocmonMap locmon_map(const ndtgpu_locmon *h)
{
    NdtLocmonMap m{};
    m.field = h->field.get();
    m.origin = h->origin.get();
    m.beams = h->beams.get();
    m.n_grids = (uint32_t)h->n_grids;
    m.width = (uint32_t)h->width;
    m.height = (uint32_t)h->height;
    m.n_beams = (uint32_t)h->n_beams;
    m.resolution = h->resolution;
    m.max_dist = h->max_dist;
    return m;
}

static ndtgpu_status locmon_installed(const char *who, const ndtgpu_locmon *h)
{
    if (h->n_grids == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no grids are installed (set_grids)");
    if (h->n_beams == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no beam table is installed (set_beams)");
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_locmon_params(ndtgpu_locmon_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_dist = 0.375;                   // localization_monitor_node.cpp:214, :324: badness_threshold_ 0.25 * 1.5
    p->r_min = 0.0;
    p->r_max = std::numeric_limits<double>::infinity();
    p->post_x = -0.275;                    // common.cpp:58
    p->post_y = 0.0;
    p->occupied_min = 55;
    p->min_num_matches = 8;                // localization_monitor_node.cpp:209
}

uint32_t ndtgpu_locmon_tile(void) { return NDT_LOCMON_TILE; }

ndtgpu_status ndtgpu_locmon_check(size_t n_grids, size_t width, size_t height, double resolution, size_t n_beams, double angle_min,
                                  double angle_increment, size_t n_scans, size_t n_queries, const ndtgpu_locmon_params *prm)
{
    const char *bad = ndt_locmon_check_grids(n_grids, width, height, resolution, locmon_params(prm));
    if (!bad) bad = ndt_locmon_check_beams(n_beams, angle_min, angle_increment);
    if (!bad) bad = ndt_locmon_check_counts(n_scans, n_queries);
    return bad ? fail_in(NDTGPU_ERR_INVALID, "locmon_check", bad) : NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_radius(double max_dist, double resolution, int32_t *R)
{
    if (!R) return fail(NDTGPU_ERR_INVALID, "locmon_radius: R is NULL");
    *R = 0;
    if (!(max_dist > 0.0 && max_dist < 1e150)) return fail(NDTGPU_ERR_INVALID, "locmon_radius: max_dist must be finite and > 0");
    if (!(resolution > 0.0 && resolution < 1e150)) return fail(NDTGPU_ERR_INVALID, "locmon_radius: resolution must be finite and > 0");
    *R = ndt_locmon_radius(max_dist, resolution);
    if (*R == 0) return fail(NDTGPU_ERR_INVALID, "locmon_radius: max_dist / resolution: the radius must be 1 .. 254 pixels");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_beam_table(size_t n_beams, double angle_min, double angle_increment, double *cb, double *sb)
{
    if (const char *bad = ndt_locmon_check_beams(n_beams, angle_min, angle_increment)) return fail_in(NDTGPU_ERR_INVALID, "locmon_beam_table", bad);
    if (!cb || !sb) return fail(NDTGPU_ERR_INVALID, "locmon_beam_table: null cb or sb");
    for (size_t i = 0; i < n_beams; i++) {
        const double a = angle_min + (double)i * angle_increment;
        cb[i] = cos(a);
        sb[i] = sin(a);
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_pixel(const double pose4[4], double cb, double sb, double r, const double origin2[2], double resolution,
                                  uint32_t width, uint32_t height, int32_t cell2[2], int32_t *in_bounds)
{
    if (!pose4 || !origin2 || !cell2 || !in_bounds) return fail(NDTGPU_ERR_INVALID, "locmon_pixel: null pose4, origin2, cell2 or in_bounds");
    *in_bounds = 0;
    if (!(resolution > 0.0 && resolution < 1e150)) return fail(NDTGPU_ERR_INVALID, "locmon_pixel: resolution must be finite and > 0");
    if (width == 0 || width > NDT_LOCMON_MAX_SIDE) return fail(NDTGPU_ERR_INVALID, "locmon_pixel: width must be 1 .. 2^15");
    if (height == 0 || height > NDT_LOCMON_MAX_SIDE) return fail(NDTGPU_ERR_INVALID, "locmon_pixel: height must be 1 .. 2^15");
    uint32_t fi = 0, fj = 0;
    if (ndt_locmon_pixel(pose4[0], pose4[1], pose4[2], pose4[3], cb, sb, r, origin2[0], origin2[1], resolution, width, height, fi, fj)) {
        *in_bounds = 1;
        cell2[0] = (int32_t)fi;
        cell2[1] = (int32_t)fj;
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_metres(uint32_t key, double resolution, double max_dist, double *badness)
{
    if (!badness) return fail(NDTGPU_ERR_INVALID, "locmon_metres: badness is NULL");
    *badness = ndt_locmon_metres(key, resolution, max_dist);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_compose(const double ref_pose4[4], const double match4[4], const double post2[2], double out4[4])
{
    if (!ref_pose4 || !match4 || !post2 || !out4) return fail(NDTGPU_ERR_INVALID, "locmon_compose: null ref_pose4, match4, post2 or out4");
    double out[4];
    ndt_locmon_compose(ref_pose4, match4, post2[0], post2[1], out);
    memcpy(out4, out, sizeof out);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_create(size_t max_grids, size_t max_pixels, size_t max_beams, size_t max_candidates, ndtgpu_locmon **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "locmon_create: out is NULL");
    *out = nullptr;
    if (const char *bad = ndt_locmon_check_capacity(max_grids, max_pixels, max_beams, max_candidates))
        return fail_in(NDTGPU_ERR_INVALID, "locmon_create", bad);
    ndtgpu_locmon *h;
    const ndtgpu_status rc = handle_new("locmon_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->max_grids = max_grids;
    h->max_pixels = max_pixels;
    h->max_beams = max_beams;
    h->max_candidates = max_candidates;
    h->chunk = ndt_locmon_handle_chunk(max_beams, max_candidates);
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "locmon_create: device buffers", expr)
    TRY(h->field.alloc(max_pixels));
    TRY(h->rowdist.alloc(max_pixels));
    TRY(h->origin.alloc(max_grids * 2));
    TRY(h->beams.alloc(max_beams * 2));
    TRY(h->cand_key.alloc(h->chunk));
    TRY(h->tile_word.alloc(ndt_locmon_tiles(max_candidates)));
    TRY(h->origin_pin.alloc(max_grids * 2));
    TRY(h->beams_pin.alloc(max_beams * 2));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_destroy(ndtgpu_locmon *h) { return handle_destroy(h, "locmon_destroy"); }

ndtgpu_status ndtgpu_locmon_set_beams(ndtgpu_locmon *h, size_t n_beams, double angle_min, double angle_increment, ndtgpu_stream stream)
{
    if (const char *bad = ndt_locmon_check_beams(n_beams, angle_min, angle_increment)) return fail_in(NDTGPU_ERR_INVALID, "locmon_set_beams", bad);
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_set_beams: null handle");
    if (n_beams > h->max_beams) return fail(NDTGPU_ERR_CAPACITY, "locmon_set_beams: more beams than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.sync());               // (the pinned table is overwritten: the previous call's work must have ended)
    double *pin = h->beams_pin.get();
    for (size_t i = 0; i < n_beams; i++) {
        const double a = angle_min + (double)i * angle_increment;
        pin[2 * i] = cos(a);
        pin[2 * i + 1] = sin(a);
    }
    HIP_TRY(hipMemcpyAsync(h->beams.get(), pin, 2 * n_beams * sizeof(double), hipMemcpyHostToDevice, st));
    h->n_beams = n_beams;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_set_grids_device(ndtgpu_locmon *h, const int8_t *grids_dev, size_t n_grids, size_t width, size_t height,
                                             double resolution, const double *origins2, const ndtgpu_locmon_params *prm,
                                             ndtgpu_stream stream)
{
    const char *who = "locmon_set_grids_device";
    const ndtgpu_locmon_params p = locmon_params(prm);
    if (const char *bad = ndt_locmon_check_grids(n_grids, width, height, resolution, p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!grids_dev || !origins2) return fail(NDTGPU_ERR_INVALID, "locmon_set_grids_device: null grids_dev or origins2");
    for (size_t k = 0; k < 2 * n_grids; k++)
        if (!(std::fabs(origins2[k]) < 1e150)) return fail_in(NDTGPU_ERR_INVALID, who, "origins2 must be finite");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_set_grids_device: null handle");
    if (n_grids > h->max_grids) return fail_in(NDTGPU_ERR_CAPACITY, who, "more grids than the handle was created for");
    if (n_grids * width * height > h->max_pixels) return fail_in(NDTGPU_ERR_CAPACITY, who, "more pixels than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.sync());               // (the pinned origins and the fields are overwritten: the previous call's work must have ended)
    memcpy(h->origin_pin.get(), origins2, 2 * n_grids * sizeof(double));
    HIP_TRY(hipMemcpyAsync(h->origin.get(), h->origin_pin.get(), 2 * n_grids * sizeof(double), hipMemcpyHostToDevice, st));
    const int R = ndt_locmon_radius(p.max_dist, resolution);
    const hipError_t e = ndt_locmon_field_launch(grids_dev, h->rowdist.get(), h->field.get(), (uint32_t)n_grids, (uint32_t)width, (uint32_t)height,
                                                 R, p.occupied_min, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "locmon_set_grids_device: launch", e);
    h->n_grids = n_grids;
    h->width = width;
    h->height = height;
    h->resolution = resolution;
    h->max_dist = p.max_dist;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_set_grids(ndtgpu_locmon *h, const int8_t *grids, size_t n_grids, size_t width, size_t height, double resolution,
                                      const double *origins2, const ndtgpu_locmon_params *prm)
{
    const char *who = "locmon_set_grids";
    const ndtgpu_locmon_params p = locmon_params(prm);
    if (const char *bad = ndt_locmon_check_grids(n_grids, width, height, resolution, p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!grids || !origins2) return fail(NDTGPU_ERR_INVALID, "locmon_set_grids: null grids or origins2");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_set_grids: null handle");
    const size_t bytes = n_grids * width * height;
    if (n_grids > h->max_grids) return fail_in(NDTGPU_ERR_CAPACITY, who, "more grids than the handle was created for");
    if (bytes > h->max_pixels) return fail_in(NDTGPU_ERR_CAPACITY, who, "more pixels than the handle was created for");
    hipStream_t st = h->hst.get();
    // only the device block of the staging: the grids travel from the caller's pageable memory
    DeviceBuffer<char> &stage = h->host.stage;
    HIP_TRY(h->used.sync());               // (the staging block may be replaced below)
    if (stage.reserve(bytes) != hipSuccess) return fail(NDTGPU_ERR_ALLOC, "locmon_set_grids: staging buffer");
    const hipError_t e = hipMemcpyAsync(stage.get(), grids, bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "hipMemcpyAsync(h->stage.get(), grids, bytes, hipMemcpyHostToDevice, st)", e);
    HIP_TRY(hipStreamSynchronize(st));     // (the copy read pageable memory of the caller's)
    const ndtgpu_status rc = ndtgpu_locmon_set_grids_device(h, (const int8_t *)stage.get(), n_grids, width, height, resolution, origins2, &p,
                                                            (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_field_get(ndtgpu_locmon *h, size_t grid, uint16_t *field)
{
    if (!field) return fail(NDTGPU_ERR_INVALID, "locmon_field_get: field is NULL");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_field_get: null handle");
    if (grid >= h->n_grids) return fail(NDTGPU_ERR_INVALID, "locmon_field_get: grid is not one of the installed grids");
    HIP_TRY(h->used.sync());
    const size_t wh = h->width * h->height;
    HIP_TRY(hipMemcpyAsync(field, h->field.get() + grid * wh, wh * sizeof(uint16_t), hipMemcpyDeviceToHost, h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_evaluate_device(ndtgpu_locmon *h, const double *ranges_dev, size_t n_scans, const ndtgpu_locmon_query *queries_dev,
                                            size_t n_queries, const ndtgpu_locmon_params *prm, ndtgpu_locmon_result *results_dev,
                                            ndtgpu_stream stream)
{
    const char *who = "locmon_evaluate_device";
    const ndtgpu_locmon_params p = locmon_params(prm);
    const char *bad = ndt_locmon_check_counts(n_scans, n_queries);
    if (!bad) bad = ndt_locmon_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!ranges_dev || (n_queries && (!queries_dev || !results_dev)))
        return fail(NDTGPU_ERR_INVALID, "locmon_evaluate_device: null ranges_dev, queries_dev or results_dev");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_evaluate_device: null handle");
    ndtgpu_status rc = locmon_installed(who, h);
    if (rc != NDTGPU_OK) return rc;
    if (n_queries == 0) return NDTGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));            // (behind the field build and the table upload, whatever stream they ran on)
    const hipError_t e = ndt_locmon_evaluate_launch(locmon_map(h), ranges_dev, (uint32_t)n_scans, queries_dev, (uint32_t)n_queries, p.r_min, p.r_max,
                                                    results_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "locmon_evaluate_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_evaluate(ndtgpu_locmon *h, const double *ranges, size_t n_scans, const ndtgpu_locmon_query *queries,
                                     size_t n_queries, const ndtgpu_locmon_params *prm, ndtgpu_locmon_result *results)
{
    const char *who = "locmon_evaluate";
    const ndtgpu_locmon_params p = locmon_params(prm);
    const char *bad = ndt_locmon_check_counts(n_scans, n_queries);
    if (!bad) bad = ndt_locmon_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!ranges || (n_queries && (!queries || !results))) return fail(NDTGPU_ERR_INVALID, "locmon_evaluate: null ranges, queries or results");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_evaluate: null handle");
    ndtgpu_status rc = locmon_installed(who, h);
    if (rc != NDTGPU_OK) return rc;
    if (n_queries == 0) return NDTGPU_OK;
    StageLayout in, outl;
    const size_t o_ranges = in.take(n_scans * h->n_beams * sizeof(double)), o_q = in.take(n_queries * sizeof(ndtgpu_locmon_query));
    const size_t o_res = outl.take(n_queries * sizeof(ndtgpu_locmon_result));
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    memcpy(hs.in_host(o_ranges), ranges, n_scans * h->n_beams * sizeof(double));
    memcpy(hs.in_host(o_q), queries, n_queries * sizeof(ndtgpu_locmon_query));
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_locmon_evaluate_device(h, (const double *)hs.in_dev(o_ranges), n_scans, (const ndtgpu_locmon_query *)hs.in_dev(o_q), n_queries, &p,
                                       (ndtgpu_locmon_result *)hs.out_dev(o_res), (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(results, hs.out_host(o_res), n_queries * sizeof(ndtgpu_locmon_result));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_adjust_device(ndtgpu_locmon *h, const double *ranges_dev, size_t n_scans, uint32_t scan, uint32_t grid,
                                          const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn,
                                          size_t nyaw, const ndtgpu_locmon_params *prm, ndtgpu_locmon_adjust_result *result_dev,
                                          uint32_t *volume_dev, ndtgpu_stream stream)
{
    const char *who = "locmon_adjust_device";
    const ndtgpu_locmon_params p = locmon_params(prm);
    const char *bad = ndt_locmon_check_counts(n_scans, 0);
    if (!bad) bad = ndt_locmon_check_lattice(nx, ny, nyaw);
    if (!bad) bad = ndt_locmon_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!ranges_dev || !result_dev) return fail(NDTGPU_ERR_INVALID, "locmon_adjust_device: null ranges_dev or result_dev");
    ndtgpu_status rc = LatticeTables::check(who, xs, nx, ys, ny, cs, sn, nyaw);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_adjust_device: null handle");
    const size_t n_candidates = nx * ny * nyaw;
    if (n_candidates > h->max_candidates) return fail_in(NDTGPU_ERR_CAPACITY, who, "more candidates than the handle was created for");
    if ((rc = locmon_installed(who, h)) != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    LatticeTables::Dev t;
    if ((rc = h->lattice.upload(h, who, xs, nx, ys, ny, cs, sn, nyaw, st, t)) != NDTGPU_OK) return rc;
    NdtLocmonSearch s{};
    s.xs = t.xs;
    s.ys = t.ys;
    s.cs = t.cs;
    s.sn = t.sn;
    s.ny = (uint32_t)ny;
    s.nyaw = (uint32_t)nyaw;
    s.n_candidates = (uint32_t)n_candidates;
    s.scan = scan;
    s.grid = grid;
    s.cand_key = h->cand_key.get();
    s.tile_word = h->tile_word.get();
    s.volume = volume_dev;
    s.result = result_dev;
    const hipError_t e = ndt_locmon_adjust_launch(locmon_map(h), ranges_dev, (uint32_t)n_scans, s, (uint32_t)h->chunk, p.r_min, p.r_max, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "locmon_adjust_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_adjust(ndtgpu_locmon *h, const double *ranges, size_t n_scans, uint32_t scan, uint32_t grid, const double *xs,
                                   size_t nx, const double *ys, size_t ny, const double *cs, const double *sn, size_t nyaw,
                                   const ndtgpu_locmon_params *prm, ndtgpu_locmon_adjust_result *result, uint32_t *volume)
{
    const char *who = "locmon_adjust";
    const ndtgpu_locmon_params p = locmon_params(prm);
    const char *bad = ndt_locmon_check_counts(n_scans, 0);
    if (!bad) bad = ndt_locmon_check_lattice(nx, ny, nyaw);
    if (!bad) bad = ndt_locmon_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!ranges || !result) return fail(NDTGPU_ERR_INVALID, "locmon_adjust: null ranges or result");
    ndtgpu_status rc = LatticeTables::check(who, xs, nx, ys, ny, cs, sn, nyaw);
    if (rc != NDTGPU_OK) return rc;
    if (scan >= n_scans) return fail_in(NDTGPU_ERR_INVALID, who, "scan must be < n_scans");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_adjust: null handle");
    const size_t n_candidates = nx * ny * nyaw;
    if (n_candidates > h->max_candidates) return fail_in(NDTGPU_ERR_CAPACITY, who, "more candidates than the handle was created for");
    if ((rc = locmon_installed(who, h)) != NDTGPU_OK) return rc;
    // only the scan that is searched travels
    StageLayout in, outl;
    const size_t o_ranges = in.take(h->n_beams * sizeof(double));
    const size_t o_res = outl.take(sizeof(ndtgpu_locmon_adjust_result)), o_vol = outl.take(volume ? n_candidates * sizeof(uint32_t) : 0);
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    memcpy(hs.in_host(o_ranges), ranges + (size_t)scan * h->n_beams, h->n_beams * sizeof(double));
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_locmon_adjust_device(h, (const double *)hs.in_dev(o_ranges), 1, 0, grid, xs, nx, ys, ny, cs, sn, nyaw, &p,
                                     (ndtgpu_locmon_adjust_result *)hs.out_dev(o_res), volume ? (uint32_t *)hs.out_dev(o_vol) : nullptr,
                                     (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(result, hs.out_host(o_res), sizeof *result);
    if (volume) memcpy(volume, hs.out_host(o_vol), n_candidates * sizeof(uint32_t));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_locmon_pick_device(ndtgpu_locmon *h, const ndtgpu_featmatch_result *matches_dev, const double *ref_poses_dev,
                                        size_t n_pairs, uint32_t scan, uint32_t grid, const ndtgpu_locmon_params *prm,
                                        ndtgpu_locmon_query *query_dev, ndtgpu_locmon_pick *pick_dev, ndtgpu_stream stream)
{
    const char *who = "locmon_pick_device";
    const ndtgpu_locmon_params p = locmon_params(prm);
    if (n_pairs > NDT_LOCMON_MAX_PAIRS) return fail_in(NDTGPU_ERR_INVALID, who, "n_pairs: more than 2^20");
    if (const char *bad = ndt_locmon_check_params(p)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if ((n_pairs && (!matches_dev || !ref_poses_dev)) || !query_dev || !pick_dev)
        return fail(NDTGPU_ERR_INVALID, "locmon_pick_device: null matches_dev, ref_poses_dev, query_dev or pick_dev");
    if (!h) return fail(NDTGPU_ERR_INVALID, "locmon_pick_device: null handle");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));
    const hipError_t e = ndt_locmon_pick_launch(matches_dev, ref_poses_dev, (uint32_t)n_pairs, scan, grid, p.min_num_matches, p.post_x, p.post_y,
                                                query_dev, pick_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "locmon_pick_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

}   // extern "C"
