// ndtgpu_calib.hip -- C-ABI (include/ndtgpu.h "extrinsic calibration") of the laser-to-base calibration: the brute-force search over
// sensor offsets of laser2d_extrinsic_calibration.cpp:176-204 with the score of :85-122 and :146-152, and the pair selection of the
// callback (:312-349).  Host side only: the handle, the argument checks, the upload of the lattice tables, the staging of the host
// form and the pure host entries; the search runs in csrc/ndt_calib.hip.
#include "ndtgpu_host.h"
#include "ndt_calib.h"

struct ndtgpu_calib {
    size_t max_pairs = 0, max_points = 0, max_candidates = 0, chunk = 0;
    DeviceBuffer<double> a3, b3, motion, partial, tile_score;
    DeviceBuffer<uint32_t> counts, tile_index;
    LatticeTables lattice;                 // the lattice tables of a call
    HostStage host;                        // the host form's staging (clouds | counts | poses | pairs in, result | volume out)
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the host form's stream (last: ndtgpu_resource.h)
};

static ndtgpu_calib_params calib_params(const ndtgpu_calib_params *prm) { return params_or_default(prm, ndtgpu_default_calib_params); }

// the checks every entry makes before it reads the handle
static ndtgpu_status calib_check(const char *who, size_t n_scans, size_t n_points, size_t stride_bytes, size_t map_stride_bytes, size_t n_pairs,
                                 size_t nx, size_t ny, size_t nyaw, const ndtgpu_calib_params &p)
{
    const char *bad = ndt_calib_check_args(n_scans, n_points, stride_bytes, map_stride_bytes, n_pairs, nx, ny, nyaw);
    if (!bad) bad = ndt_calib_check_params(p);
    return bad ? fail_in(NDTGPU_ERR_INVALID, who, bad) : NDTGPU_OK;
}

static ndtgpu_status calib_fits(const char *who, const ndtgpu_calib *h, size_t n_points, size_t n_pairs, size_t n_candidates)
{
    if (n_pairs > h->max_pairs) return fail_in(NDTGPU_ERR_CAPACITY, who, "more pairs than the handle was created for");
    if (n_points > h->max_points) return fail_in(NDTGPU_ERR_CAPACITY, who, "more points than the handle was created for");
    if (n_candidates > h->max_candidates) return fail_in(NDTGPU_ERR_CAPACITY, who, "more candidates than the handle was created for");
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_calib_params(ndtgpu_calib_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_dist = 0.1;                     // laser2d_extrinsic_calibration.cpp:106: error_th = 0.1 * 0.1
}

uint32_t ndtgpu_calib_tile(void) { return NDT_CALIB_TILE; }

ndtgpu_status ndtgpu_calib_lattice(double ix, double iy, double iyaw, double x_s, double y_s, double yaw_s, double t_r, double yaw_r,
                                   size_t counts3[3], double *xs, double *ys, double *yaws, double *cs, double *sn, size_t room)
{
    if (!counts3) return fail(NDTGPU_ERR_INVALID, "calib_lattice: counts3 is NULL");
    counts3[0] = counts3[1] = counts3[2] = 0;
    if (const char *bad = ndt_calib_check_lattice(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r))
        return fail_in(NDTGPU_ERR_INVALID, "calib_lattice", bad);
    const size_t cap = NDT_CALIB_MAX_CANDIDATES;
    const size_t nx = ndt_calib_axis(ix, x_s, t_r, xs, room, cap);
    const size_t ny = ndt_calib_axis(iy, y_s, t_r, ys, room, cap);
    const size_t nyaw = ndt_calib_axis(iyaw, yaw_s, yaw_r, yaws, room, cap);
    if (nx > cap || ny > cap || nyaw > cap) return fail(NDTGPU_ERR_INVALID, "calib_lattice: more than 2^24 nodes on an axis (t_r / yaw_r too small)");
    counts3[0] = nx;
    counts3[1] = ny;
    counts3[2] = nyaw;
    if ((xs && nx > room) || (ys && ny > room) || ((yaws || cs || sn) && nyaw > room))
        return fail(NDTGPU_ERR_CAPACITY, "calib_lattice: an axis has more nodes than room");
    if (cs || sn) {
        double v = iyaw - yaw_s;               // (the walk again: yaws may be NULL)
        for (size_t k = 0; k < nyaw; k++, v += yaw_r) {
            if (cs) cs[k] = cos(v);
            if (sn) sn[k] = sin(v);
        }
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_calib_pair_motion(const double pose1[4], const double pose2[4], double D[4])
{
    if (!pose1 || !pose2 || !D) return fail(NDTGPU_ERR_INVALID, "calib_pair_motion: null pose1, pose2 or D");
    ndt_calib_pair_motion(pose1, pose2, D);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_calib_select_pairs(const double *poses4, size_t n, double max_translation, double min_yaw, uint32_t *pairs2,
                                        size_t room, size_t *n_pairs)
{
    if (!n_pairs) return fail(NDTGPU_ERR_INVALID, "calib_select_pairs: n_pairs is NULL");
    *n_pairs = 0;
    if (n && !poses4) return fail(NDTGPU_ERR_INVALID, "calib_select_pairs: null poses4");
    if (n > NDT_CALIB_MAX_SCANS) return fail(NDTGPU_ERR_INVALID, "calib_select_pairs: n: more than 2^20 poses");
    if (!(max_translation >= 0.0)) return fail(NDTGPU_ERR_INVALID, "calib_select_pairs: max_translation must be >= 0");
    if (!(min_yaw >= 0.0)) return fail(NDTGPU_ERR_INVALID, "calib_select_pairs: min_yaw must be >= 0");
    *n_pairs = ndt_calib_select_pairs(poses4, n, max_translation, min_yaw, pairs2, room);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_calib_check(size_t n_scans, size_t n_points, size_t stride_bytes, size_t map_stride_bytes, size_t n_pairs, size_t nx,
                                 size_t ny, size_t nyaw, const ndtgpu_calib_params *prm)
{
    return calib_check("calib_check", n_scans, n_points, stride_bytes, map_stride_bytes, n_pairs, nx, ny, nyaw, calib_params(prm));
}

ndtgpu_status ndtgpu_calib_create(size_t max_pairs, size_t max_points, size_t max_candidates, ndtgpu_calib **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "calib_create: out is NULL");
    *out = nullptr;
    if (const char *bad = ndt_calib_check_capacity(max_pairs, max_points, max_candidates)) return fail_in(NDTGPU_ERR_INVALID, "calib_create", bad);
    ndtgpu_calib *h;
    const ndtgpu_status rc = handle_new("calib_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->max_pairs = max_pairs;
    h->max_points = max_points;
    h->max_candidates = max_candidates;
    h->chunk = ndt_calib_handle_chunk(max_pairs, max_candidates);
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "calib_create: device buffers", expr)
    TRY(h->a3.alloc(max_pairs * max_points * 3));
    TRY(h->b3.alloc(max_pairs * max_points * 3));
    TRY(h->motion.alloc(max_pairs * 4));
    TRY(h->counts.alloc(max_pairs * 4));
    TRY(h->partial.alloc(max_pairs * h->chunk));
    TRY(h->tile_score.alloc(ndt_calib_tiles(max_candidates)));
    TRY(h->tile_index.alloc(ndt_calib_tiles(max_candidates)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_calib_destroy(ndtgpu_calib *h) { return handle_destroy(h, "calib_destroy"); }

ndtgpu_status ndtgpu_calib_search_device(ndtgpu_calib *h, const void *xyz_dev, size_t n_scans, size_t n_points, size_t stride_bytes,
                                         size_t map_stride_bytes, const uint32_t *n_kept_dev, const double *poses_dev,
                                         const uint32_t *pairs_dev, size_t n_pairs, const double *xs, size_t nx, const double *ys, size_t ny,
                                         const double *cs, const double *sn, size_t nyaw, const ndtgpu_calib_params *prm,
                                         ndtgpu_calib_result *result_dev, double *volume_dev, ndtgpu_stream stream)
{
    const char *who = "calib_search_device";
    const ndtgpu_calib_params p = calib_params(prm);
    ndtgpu_status rc = calib_check(who, n_scans, n_points, stride_bytes, map_stride_bytes, n_pairs, nx, ny, nyaw, p);
    if (rc != NDTGPU_OK) return rc;
    if (!xyz_dev || !n_kept_dev || !poses_dev || !pairs_dev || !result_dev)
        return fail(NDTGPU_ERR_INVALID, "calib_search_device: null xyz_dev, n_kept_dev, poses_dev, pairs_dev or result_dev");
    if ((rc = LatticeTables::check(who, xs, nx, ys, ny, cs, sn, nyaw)) != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "calib_search_device: null handle");
    const size_t n_candidates = nx * ny * nyaw;
    if ((rc = calib_fits(who, h, n_points, n_pairs, n_candidates)) != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    LatticeTables::Dev t;
    if ((rc = h->lattice.upload(h, who, xs, nx, ys, ny, cs, sn, nyaw, st, t)) != NDTGPU_OK) return rc;
    NdtCalibArgs a{};
    a.xyz = (const uint32_t *)xyz_dev;
    a.n_kept = n_kept_dev;
    a.poses = poses_dev;
    a.pairs = pairs_dev;
    a.xs = t.xs;
    a.ys = t.ys;
    a.cs = t.cs;
    a.sn = t.sn;
    a.stride_words = stride_bytes / 4;
    a.map_stride_words = map_stride_bytes / 4;
    a.n_scans = (uint32_t)n_scans;
    a.n_points = (uint32_t)n_points;
    a.n_pairs = (uint32_t)n_pairs;
    a.nx = (uint32_t)nx;
    a.ny = (uint32_t)ny;
    a.nyaw = (uint32_t)nyaw;
    a.n_candidates = (uint32_t)n_candidates;
    a.chunk = (uint32_t)h->chunk;
    a.th2 = p.max_dist * p.max_dist;
    a.a3 = h->a3.get();
    a.b3 = h->b3.get();
    a.motion = h->motion.get();
    a.counts = h->counts.get();
    a.partial = h->partial.get();
    a.tile_score = h->tile_score.get();
    a.tile_index = h->tile_index.get();
    a.result = result_dev;
    a.volume = volume_dev;
    const hipError_t e = ndt_calib_launch(a, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "calib_search_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_calib_search(ndtgpu_calib *h, const void *xyz, size_t n_scans, size_t n_points, size_t stride_bytes,
                                  size_t map_stride_bytes, const uint32_t *n_kept, const double *poses, const uint32_t *pairs, size_t n_pairs,
                                  const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn, size_t nyaw,
                                  const ndtgpu_calib_params *prm, ndtgpu_calib_result *result, double *volume)
{
    const char *who = "calib_search";
    const ndtgpu_calib_params p = calib_params(prm);
    ndtgpu_status rc = calib_check(who, n_scans, n_points, stride_bytes, map_stride_bytes, n_pairs, nx, ny, nyaw, p);
    if (rc != NDTGPU_OK) return rc;
    if (!xyz || !n_kept || !poses || !pairs || !result) return fail(NDTGPU_ERR_INVALID, "calib_search: null xyz, n_kept, poses, pairs or result");
    if ((rc = LatticeTables::check(who, xs, nx, ys, ny, cs, sn, nyaw)) != NDTGPU_OK) return rc;
    for (size_t k = 0; k < 2 * n_pairs; k++)
        if (pairs[k] >= n_scans) return fail(NDTGPU_ERR_INVALID, "calib_search: pairs names a scan >= n_scans");
    if (!h) return fail(NDTGPU_ERR_INVALID, "calib_search: null handle");
    const size_t n_candidates = nx * ny * nyaw;
    if ((rc = calib_fits(who, h, n_points, n_pairs, n_candidates)) != NDTGPU_OK) return rc;
    // only the scans that a pair names travel, packed (12 bytes a row), each once per use: scan 2k is pair k's cloud1, 2k + 1 its cloud2
    const size_t n_used = 2 * n_pairs, row = 12;
    StageLayout in, outl;
    const size_t o_rows = in.take(n_used * n_points * row), o_kept = in.take(n_used * sizeof(uint32_t)),
                 o_poses = in.take(n_used * 4 * sizeof(double)), o_pairs = in.take(n_used * sizeof(uint32_t));
    const size_t o_res = outl.take(sizeof(ndtgpu_calib_result)), o_vol = outl.take(volume ? n_candidates * sizeof(double) : 0);
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, who, in, outl)) != NDTGPU_OK) return rc;
    for (size_t k = 0; k < n_used; k++) {
        const size_t s = pairs[k];
        const char *src = (const char *)xyz + s * map_stride_bytes;
        char *dst = hs.in_host(o_rows) + k * n_points * row;
        for (size_t i = 0; i < n_points; i++) memcpy(dst + i * row, src + i * stride_bytes, row);
        ((uint32_t *)hs.in_host(o_kept))[k] = n_kept[s];
        memcpy(hs.in_host(o_poses) + k * 4 * sizeof(double), poses + 4 * s, 4 * sizeof(double));
        ((uint32_t *)hs.in_host(o_pairs))[k] = (uint32_t)k;
    }
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_calib_search_device(h, hs.in_dev(o_rows), n_used, n_points, row, n_points * row, (const uint32_t *)hs.in_dev(o_kept),
                                    (const double *)hs.in_dev(o_poses), (const uint32_t *)hs.in_dev(o_pairs), n_pairs, xs, nx, ys, ny, cs, sn,
                                    nyaw, &p, (ndtgpu_calib_result *)hs.out_dev(o_res), volume ? (double *)hs.out_dev(o_vol) : nullptr,
                                    (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(result, hs.out_host(o_res), sizeof *result);
    if (volume) memcpy(volume, hs.out_host(o_vol), n_candidates * sizeof(double));
    return NDTGPU_OK;
}

}   // extern "C"
