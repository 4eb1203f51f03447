// ndtgpu_scansim.hip -- C-ABI (include/ndtgpu.h "scan simulation") of occupancy_grid_utils::simulateRangeScan as flirtlib_ros calls it
// (place_rec_test.cpp:242, simulate_scans.cpp:131) and of the pose lattice of generateRefScans (place_rec_test.cpp:218-237).  Host
// side only: the handle, the argument checks, the beam table, the upload of the origins and the heading tables, the staging of the
// host forms and the pure host entries; the work runs in csrc/ndt_scansim.hip.
#include "ndtgpu_host.h"
#include "ndt_scansim.h"

#include <limits>

struct ndtgpu_scansim {
    size_t max_grids = 0, max_beams = 0, max_poses = 0;
    // what is installed
    size_t n_grids = 0, width = 0, height = 0, n_beams = 0;
    double resolution = 0.0;
    const int8_t *grids = nullptr;         // the caller's bytes (set_grids_device: borrowed until the next set or destroy) or `owned`
    DeviceBuffer<int8_t> owned;            // set_grids: the host form's copy
    DeviceBuffer<double> origin;           // [max_grids][2]
    DeviceBuffer<double> beams;            // [max_beams][2]
    DeviceBuffer<uint32_t> tile;           // the lattice's tile counts: made by the first lattice, grown by later ones
    PinnedBuffer<double> origin_pin, beams_pin;
    LatticeTables lattice;                 // the heading tables of a lattice
    HostStage host;                        // the host forms' staging
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the host forms' stream (last: ndtgpu_resource.h)
};

static ndtgpu_scansim_params scansim_params(const ndtgpu_scansim_params *prm) { return params_or_default(prm, ndtgpu_default_scansim_params); }

static NdtScansimMap scansim_map(const ndtgpu_scansim *h)
{
    NdtScansimMap m{};
    m.grids = h->grids;
    m.origin = h->origin.get();
    m.beams = h->beams.get();
    m.n_grids = (uint32_t)h->n_grids;
    m.width = (uint32_t)h->width;
    m.height = (uint32_t)h->height;
    m.n_beams = (uint32_t)h->n_beams;
    m.resolution = h->resolution;
    return m;
}

static const double SCANSIM_NO_BOX[4] = {-std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                                         std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()};

// what both forms of the lattice check before they read the handle
static ndtgpu_status scansim_lattice_args(const char *who, size_t skip, const double *cs, const double *sn, size_t nyaw, const double *box4,
                                          size_t capacity)
{
    // (the grid's sides are the handle's: the node count is checked behind it)
    if (const char *bad = ndt_scansim_check_lattice(1, 1, skip, nyaw, box4, capacity)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!cs || !sn) return fail_in(NDTGPU_ERR_INVALID, who, "null cs or sn");
    if (const char *bad = ndt_lattice_check_tables(cs, 0, cs, 0, cs, sn, nyaw)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_scansim_params(ndtgpu_scansim_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->range_max = 10.0;                   // place_rec_test.cpp: the scanner of generateRefScans
    p->miss = 11.0;                        // range_max + 1: upstream's out-of-range value
    p->occupied_min = 55;
    p->unknown_is_obstacle = 1;            // every call site passes true
}

uint32_t ndtgpu_scansim_tile(void) { return NDT_SCANSIM_TILE; }

ndtgpu_status ndtgpu_scansim_check(size_t n_grids, size_t width, size_t height, double resolution, size_t n_beams, double angle_min,
                                   double angle_increment, size_t n_poses, const ndtgpu_scansim_params *prm)
{
    const char *bad = ndt_scansim_check_grids(n_grids, width, height, resolution);
    if (!bad) bad = ndt_scansim_check_beams(n_beams, angle_min, angle_increment);
    if (!bad) bad = ndt_scansim_check_poses(n_poses);
    if (!bad) bad = ndt_scansim_check_reach(resolution, scansim_params(prm));
    return bad ? fail_in(NDTGPU_ERR_INVALID, "scansim_check", bad) : NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_reach(double range_max, double resolution, int32_t *R)
{
    if (!R) return fail(NDTGPU_ERR_INVALID, "scansim_reach: R is NULL");
    *R = 0;
    if (!(range_max > 0.0 && range_max < 1e150)) return fail(NDTGPU_ERR_INVALID, "scansim_reach: range_max must be finite and > 0");
    if (!(resolution > 0.0 && resolution < 1e150)) return fail(NDTGPU_ERR_INVALID, "scansim_reach: resolution must be finite and > 0");
    *R = ndt_scansim_reach(range_max, resolution);
    if (*R == 0) return fail(NDTGPU_ERR_INVALID, "scansim_reach: range_max / resolution: the reach must be 1 .. 4094 cells");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_skip(double ref_pos_resolution, double resolution, uint32_t *skip)
{
    if (!skip) return fail(NDTGPU_ERR_INVALID, "scansim_skip: skip is NULL");
    *skip = 0;
    if (!(ref_pos_resolution > 0.0 && ref_pos_resolution < 1e150))
        return fail(NDTGPU_ERR_INVALID, "scansim_skip: ref_pos_resolution must be finite and > 0");
    if (!(resolution > 0.0 && resolution < 1e150)) return fail(NDTGPU_ERR_INVALID, "scansim_skip: resolution must be finite and > 0");
    *skip = ndt_scansim_skip(ref_pos_resolution, resolution);
    if (*skip == 0) return fail(NDTGPU_ERR_INVALID, "scansim_skip: ref_pos_resolution / resolution: skip must be 1 .. 2^15 (0 is refused)");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_cell(int32_t di, int32_t dj, int32_t k, int32_t cell2[2])
{
    if (!cell2) return fail(NDTGPU_ERR_INVALID, "scansim_cell: cell2 is NULL");
    if (di < -32768 || di > 32768) return fail(NDTGPU_ERR_INVALID, "scansim_cell: di must be -2^15 .. 2^15");
    if (dj < -32768 || dj > 32768) return fail(NDTGPU_ERR_INVALID, "scansim_cell: dj must be -2^15 .. 2^15");
    const NdtScansimRay r = ndt_scansim_ray_of(di, dj);
    if (k < 0 || k > r.n) return fail(NDTGPU_ERR_INVALID, "scansim_cell: k must be 0 .. max(|di|, |dj|)");
    ndt_scansim_step_cell(r, k, cell2[0], cell2[1]);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_beam(const int8_t *grid, size_t width, size_t height, const double origin2[2], double resolution,
                                  const double pose4[4], double cb, double sb, const ndtgpu_scansim_params *prm, double *range, int32_t *hit,
                                  uint32_t *flags)
{
    const char *who = "scansim_beam";
    const ndtgpu_scansim_params p = scansim_params(prm);
    const char *bad = ndt_scansim_check_grids(1, width, height, resolution);
    if (!bad) bad = ndt_scansim_check_reach(resolution, p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!grid || !origin2 || !pose4 || !range || !hit || !flags)
        return fail_in(NDTGPU_ERR_INVALID, who, "null grid, origin2, pose4, range, hit or flags");
    *range = p.miss;
    *hit = 0;
    *flags = 0;
    int32_t i0, j0;
    if (!ndt_scansim_point_cell(pose4[0], pose4[1], origin2[0], origin2[1], resolution, (uint32_t)width, (uint32_t)height, i0, j0)) {
        *flags = NDTGPU_SCANSIM_OFFMAP;
        return NDTGPU_OK;
    }
    NdtScansimRay ray;
    uint32_t d2 = 0;
    if (ndt_scansim_beam_ray(pose4[0], pose4[1], pose4[2], pose4[3], cb, sb, p.range_max, origin2[0], origin2[1], resolution, i0, j0, ray) &&
        ndt_scansim_walk(grid, (uint32_t)width, (uint32_t)height, i0, j0, ray, ndt_scansim_reach(p.range_max, resolution), p.occupied_min,
                         p.unknown_is_obstacle, d2)) {
        *range = ndt_scansim_metres(d2, resolution);
        *hit = 1;
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_headings(double angle_step, size_t *count, double *cs, double *sn, size_t room)
{
    if (!count) return fail(NDTGPU_ERR_INVALID, "scansim_headings: count is NULL");
    *count = 0;
    if (!(angle_step > 0.0 && angle_step < 1e150)) return fail(NDTGPU_ERR_INVALID, "scansim_headings: angle_step must be finite and > 0");
    const size_t n = ndt_scansim_headings(angle_step, nullptr, nullptr, 0);
    if (n > NDT_SCANSIM_MAX_POSES) return fail(NDTGPU_ERR_INVALID, "scansim_headings: angle_step: more than 2^24 headings");
    *count = n;
    if ((cs || sn) && n > room) return fail(NDTGPU_ERR_CAPACITY, "scansim_headings: more headings than room");
    ndt_scansim_headings(angle_step, cs, sn, room);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_create(size_t max_grids, size_t max_beams, size_t max_poses, ndtgpu_scansim **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "scansim_create: out is NULL");
    *out = nullptr;
    if (const char *bad = ndt_scansim_check_capacity(max_grids, max_beams, max_poses)) return fail_in(NDTGPU_ERR_INVALID, "scansim_create", bad);
    ndtgpu_scansim *h;
    const ndtgpu_status rc = handle_new("scansim_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->max_grids = max_grids;
    h->max_beams = max_beams;
    h->max_poses = max_poses;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "scansim_create: device buffers", expr)
    TRY(h->origin.alloc(max_grids * 2));
    TRY(h->beams.alloc(max_beams * 2));
    TRY(h->origin_pin.alloc(max_grids * 2));
    TRY(h->beams_pin.alloc(max_beams * 2));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_destroy(ndtgpu_scansim *h) { return handle_destroy(h, "scansim_destroy"); }

ndtgpu_status ndtgpu_scansim_set_beams(ndtgpu_scansim *h, size_t n_beams, double angle_min, double angle_increment, ndtgpu_stream stream)
{
    if (const char *bad = ndt_scansim_check_beams(n_beams, angle_min, angle_increment)) return fail_in(NDTGPU_ERR_INVALID, "scansim_set_beams", bad);
    if (!h) return fail(NDTGPU_ERR_INVALID, "scansim_set_beams: null handle");
    if (n_beams > h->max_beams) return fail(NDTGPU_ERR_CAPACITY, "scansim_set_beams: more beams than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.sync());               // (the pinned table is overwritten: the previous call's work must have ended)
    double *pin = h->beams_pin.get();
    for (size_t i = 0; i < n_beams; i++) {  // (the table of ndtgpu_locmon_beam_table)
        const double a = angle_min + (double)i * angle_increment;
        pin[2 * i] = cos(a);
        pin[2 * i + 1] = sin(a);
    }
    HIP_TRY(hipMemcpyAsync(h->beams.get(), pin, 2 * n_beams * sizeof(double), hipMemcpyHostToDevice, st));
    h->n_beams = n_beams;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_set_grids_device(ndtgpu_scansim *h, const int8_t *grids_dev, size_t n_grids, size_t width, size_t height,
                                              double resolution, const double *origins2, ndtgpu_stream stream)
{
    const char *who = "scansim_set_grids_device";
    if (const char *bad = ndt_scansim_check_grids(n_grids, width, height, resolution)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!grids_dev || !origins2) return fail_in(NDTGPU_ERR_INVALID, who, "null grids_dev or origins2");
    for (size_t k = 0; k < 2 * n_grids; k++)
        if (!(std::fabs(origins2[k]) < 1e150)) return fail_in(NDTGPU_ERR_INVALID, who, "origins2 must be finite");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (n_grids > h->max_grids) return fail_in(NDTGPU_ERR_CAPACITY, who, "more grids than the handle was created for");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.sync());               // (the pinned origins are overwritten: the previous call's work must have ended)
    memcpy(h->origin_pin.get(), origins2, 2 * n_grids * sizeof(double));
    HIP_TRY(hipMemcpyAsync(h->origin.get(), h->origin_pin.get(), 2 * n_grids * sizeof(double), hipMemcpyHostToDevice, st));
    h->grids = grids_dev;
    h->n_grids = n_grids;
    h->width = width;
    h->height = height;
    h->resolution = resolution;
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_set_grids(ndtgpu_scansim *h, const int8_t *grids, size_t n_grids, size_t width, size_t height, double resolution,
                                       const double *origins2)
{
    const char *who = "scansim_set_grids";
    if (const char *bad = ndt_scansim_check_grids(n_grids, width, height, resolution)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!grids || !origins2) return fail_in(NDTGPU_ERR_INVALID, who, "null grids or origins2");
    for (size_t k = 0; k < 2 * n_grids; k++)
        if (!(std::fabs(origins2[k]) < 1e150)) return fail_in(NDTGPU_ERR_INVALID, who, "origins2 must be finite");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (n_grids > h->max_grids) return fail_in(NDTGPU_ERR_CAPACITY, who, "more grids than the handle was created for");
    const size_t bytes = n_grids * width * height;
    hipStream_t st = h->hst.get();
    HIP_TRY(h->used.sync());               // (the owned block may be replaced below, and is overwritten)
    if (h->owned.reserve(bytes) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "the grids' device buffer");
    int8_t *dev = h->owned.get();
    HIP_TRY(hipMemcpyAsync(dev, grids, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));     // (the copy read pageable memory of the caller's)
    const ndtgpu_status rc = ndtgpu_scansim_set_grids_device(h, dev, n_grids, width, height, resolution, origins2, (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_lattice_device(ndtgpu_scansim *h, uint32_t grid, uint32_t skip, const double *cs, const double *sn, size_t nyaw,
                                            const double *box4, size_t capacity, double *poses_dev, uint32_t *index_dev, uint32_t *count_dev,
                                            ndtgpu_stream stream)
{
    const char *who = "scansim_lattice_device";
    ndtgpu_status rc = scansim_lattice_args(who, skip, cs, sn, nyaw, box4, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!poses_dev || !count_dev) return fail_in(NDTGPU_ERR_INVALID, who, "null poses_dev or count_dev");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (h->n_grids == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no grids are installed (set_grids)");
    if (grid >= h->n_grids) return fail_in(NDTGPU_ERR_INVALID, who, "grid is not one of the installed grids");
    if (const char *bad = ndt_scansim_check_lattice(h->width, h->height, skip, nyaw, box4, capacity)) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    hipStream_t st = (hipStream_t)stream;
    LatticeTables::Dev t;
    if ((rc = h->lattice.upload(h, who, cs, 0, cs, 0, cs, sn, nyaw, st, t)) != NDTGPU_OK) return rc;   // (no xs, ys: the positions are pixels)
    NdtScansimLattice l{};
    l.cs = t.cs;
    l.sn = t.sn;
    l.grid = grid;
    l.skip = skip;
    l.npx = ndt_scansim_axis_nodes((uint32_t)h->width, skip);
    l.npy = ndt_scansim_axis_nodes((uint32_t)h->height, skip);
    l.nyaw = (uint32_t)nyaw;
    memcpy(l.box4, box4 ? box4 : SCANSIM_NO_BOX, sizeof l.box4);
    // (the host has waited for the handle's previous call in the upload: the tile counts may be replaced)
    if (h->tile.reserve(ndt_scansim_tiles((size_t)l.npx * l.npy)) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "tile counts");
    l.tile = h->tile.get();
    l.capacity = capacity;
    l.poses = poses_dev;
    l.index = index_dev;
    l.count = count_dev;
    const hipError_t e = ndt_scansim_lattice_launch(scansim_map(h), l, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "scansim_lattice_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_lattice(ndtgpu_scansim *h, uint32_t grid, uint32_t skip, const double *cs, const double *sn, size_t nyaw,
                                     const double *box4, size_t capacity, double *poses, uint32_t *index, uint32_t counts2[2])
{
    const char *who = "scansim_lattice";
    ndtgpu_status rc = scansim_lattice_args(who, skip, cs, sn, nyaw, box4, capacity);
    if (rc != NDTGPU_OK) return rc;
    if (!poses || !counts2) return fail_in(NDTGPU_ERR_INVALID, who, "null poses or counts2");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    StageLayout in, outl;
    const size_t o_cnt = outl.take(2 * sizeof(uint32_t)), o_poses = outl.take(capacity * 4 * sizeof(double)),
                 o_idx = outl.take(index ? capacity * sizeof(uint32_t) : 0);
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    rc = ndtgpu_scansim_lattice_device(h, grid, skip, cs, sn, nyaw, box4, capacity, (double *)hs.out_dev(o_poses),
                                       index ? (uint32_t *)hs.out_dev(o_idx) : nullptr, (uint32_t *)hs.out_dev(o_cnt), (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(counts2, hs.out_host(o_cnt), 2 * sizeof(uint32_t));
    memcpy(poses, hs.out_host(o_poses), (size_t)counts2[0] * 4 * sizeof(double));
    if (index) memcpy(index, hs.out_host(o_idx), (size_t)counts2[0] * sizeof(uint32_t));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_simulate_device(ndtgpu_scansim *h, const double *poses_dev, const uint32_t *grid_idx_dev, size_t n_poses,
                                             const uint32_t *count_dev, const ndtgpu_scansim_params *prm, double *ranges_dev,
                                             ndtgpu_scansim_result *results_dev, ndtgpu_stream stream)
{
    const char *who = "scansim_simulate_device";
    const ndtgpu_scansim_params p = scansim_params(prm);
    const char *bad = ndt_scansim_check_poses(n_poses);
    if (!bad) bad = ndt_scansim_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!poses_dev || !ranges_dev) return fail_in(NDTGPU_ERR_INVALID, who, "null poses_dev or ranges_dev");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (n_poses > h->max_poses) return fail_in(NDTGPU_ERR_CAPACITY, who, "more poses than the handle was created for");
    if (h->n_grids == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no grids are installed (set_grids)");
    if (h->n_beams == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no beam table is installed (set_beams)");
    if ((bad = ndt_scansim_check_reach(h->resolution, p))) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    NdtScansimCast c{};
    c.range_max = p.range_max;
    c.miss = p.miss;
    c.R = ndt_scansim_reach(p.range_max, h->resolution);
    c.occupied_min = p.occupied_min;
    c.unknown_is_obstacle = p.unknown_is_obstacle;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));            // (behind the uploads of the origins and the beam table, whatever stream they ran on)
    const hipError_t e = ndt_scansim_cast_launch(scansim_map(h), c, poses_dev, grid_idx_dev, (uint32_t)n_poses, count_dev, ranges_dev, results_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "scansim_simulate_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scansim_simulate(ndtgpu_scansim *h, const double *poses, const uint32_t *grid_idx, size_t n_poses,
                                      const ndtgpu_scansim_params *prm, double *ranges, ndtgpu_scansim_result *results)
{
    const char *who = "scansim_simulate";
    const ndtgpu_scansim_params p = scansim_params(prm);
    const char *bad = ndt_scansim_check_poses(n_poses);
    if (!bad) bad = ndt_scansim_check_params(p);
    if (bad) return fail_in(NDTGPU_ERR_INVALID, who, bad);
    if (!poses || !ranges) return fail_in(NDTGPU_ERR_INVALID, who, "null poses or ranges");
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (n_poses > h->max_poses) return fail_in(NDTGPU_ERR_CAPACITY, who, "more poses than the handle was created for");
    if (h->n_beams == 0) return fail_in(NDTGPU_ERR_INVALID, who, "no beam table is installed (set_beams)");
    StageLayout in, outl;
    const size_t o_poses = in.take(n_poses * 4 * sizeof(double)), o_gi = in.take(grid_idx ? n_poses * sizeof(uint32_t) : 0);
    const size_t o_ranges = outl.take(n_poses * h->n_beams * sizeof(double)),
                 o_res = outl.take(results ? n_poses * sizeof(ndtgpu_scansim_result) : 0);
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    ndtgpu_status rc;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    memcpy(hs.in_host(o_poses), poses, n_poses * 4 * sizeof(double));
    if (grid_idx) memcpy(hs.in_host(o_gi), grid_idx, n_poses * sizeof(uint32_t));
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_scansim_simulate_device(h, (const double *)hs.in_dev(o_poses), grid_idx ? (const uint32_t *)hs.in_dev(o_gi) : nullptr, n_poses,
                                        nullptr, &p, (double *)hs.out_dev(o_ranges),
                                        results ? (ndtgpu_scansim_result *)hs.out_dev(o_res) : nullptr, (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(ranges, hs.out_host(o_ranges), n_poses * h->n_beams * sizeof(double));
    if (results) memcpy(results, hs.out_host(o_res), n_poses * sizeof(ndtgpu_scansim_result));
    return NDTGPU_OK;
}

}   // extern "C"
