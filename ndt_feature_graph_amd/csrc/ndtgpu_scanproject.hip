// ndtgpu_scanproject.hip -- C-ABI (include/ndtgpu.h "laser-scan projection") of the step at the head of the chain: a batch of laser
// scans to the point clouds in the sensor frame that the fuser bank and the registrar take (projectLaser, the range gate and the z
// jitter of ndt_feature2d_fuser.cpp:747-765 and the other call sites the header lists).  Host side only: the handle, the argument
// checks, the staging of the host form and the order of the launches; the projection runs in csrc/ndt_scanproject.hip.
#include "ndtgpu_host.h"
#include "ndt_scanproject.h"

struct ndtgpu_scanproj {
    size_t max_scans = 0, max_beams = 0;
    DeviceBuffer<uint32_t> tile;           // one count per tile of every scan: what the two launches of a call hand over
    HostStage host;                        // the host form's staging (ranges | scan ids in, rows | counts out)
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the host form's stream (last: ndtgpu_resource.h)
};

static ndtgpu_scanproject_params scanproject_params(const ndtgpu_scanproject_params *prm)
{
    return params_or_default(prm, ndtgpu_default_scanproject_params);
}

// the checks every entry makes before it reads the handle
static ndtgpu_status scanproj_check(const char *who, size_t n_scans, size_t n_beams, double angle_min, double angle_increment,
                                    size_t stride_bytes, size_t map_stride_bytes, const ndtgpu_scanproject_params &p)
{
    const char *bad = ndt_scanproject_check_args(n_scans, n_beams, angle_min, angle_increment, stride_bytes, map_stride_bytes);
    if (!bad) bad = ndt_scanproject_check_params(p);
    return bad ? fail_in(NDTGPU_ERR_INVALID, who, bad) : NDTGPU_OK;
}

static ndtgpu_status scanproj_fits(const char *who, const ndtgpu_scanproj *h, size_t n_scans, size_t n_beams)
{
    if (n_scans > h->max_scans) return fail_in(NDTGPU_ERR_CAPACITY, who, "more scans than the handle was created for");
    if (n_beams > h->max_beams) return fail_in(NDTGPU_ERR_CAPACITY, who, "more beams than the handle was created for");
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_scanproject_params(ndtgpu_scanproject_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->r_min = 0.5;                        // gustav_laser_tf.launch:20-23: min_laser_range
    p->r_max = 30.0;                       // ... sensor_range
    p->varz = 0.02;                        // ... laser_variance_z
    p->seed = 0;
}

uint32_t ndtgpu_scanproj_tile(void) { return NDT_SCANPROJECT_TILE; }

ndtgpu_status ndtgpu_scanproj_check(size_t n_scans, size_t n_beams, double angle_min, double angle_increment, size_t stride_bytes,
                                    size_t map_stride_bytes, const ndtgpu_scanproject_params *prm)
{
    return scanproj_check("scanproj_check", n_scans, n_beams, angle_min, angle_increment, stride_bytes, map_stride_bytes,
                          scanproject_params(prm));
}

int ndtgpu_scanproj_beam(const ndtgpu_scanproject_params *prm, double angle_min, double angle_increment, uint64_t scan_id, uint32_t i,
                         double r, float xyz[3])
{
    float p[3];
    if (!ndt_scanproject_beam(ndt_scanproject_params_dev(scanproject_params(prm)), angle_min, angle_increment, scan_id, i, r, p)) return 0;
    if (xyz) memcpy(xyz, p, sizeof p);
    return 1;
}

ndtgpu_status ndtgpu_scanproj_create(size_t max_scans, size_t max_beams, ndtgpu_scanproj **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "scanproj_create: out is NULL");
    *out = nullptr;
    if (const char *bad = ndt_scanproject_check_capacity(max_scans, max_beams)) return fail_in(NDTGPU_ERR_INVALID, "scanproj_create", bad);
    ndtgpu_scanproj *h;
    const ndtgpu_status rc = handle_new("scanproj_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->max_scans = max_scans;
    h->max_beams = max_beams;
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "scanproj_create: device buffers", expr)
    TRY(h->tile.alloc(max_scans * ndt_scanproject_tiles(max_beams)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scanproj_destroy(ndtgpu_scanproj *h) { return handle_destroy(h, "scanproj_destroy"); }

ndtgpu_status ndtgpu_scanproj_project_device(ndtgpu_scanproj *h, const double *ranges_dev, const uint64_t *scan_id_dev, size_t n_scans,
                                             size_t n_beams, double angle_min, double angle_increment,
                                             const ndtgpu_scanproject_params *prm, void *xyz_dev, size_t stride_bytes,
                                             size_t map_stride_bytes, uint32_t *n_kept_dev, ndtgpu_stream stream)
{
    const ndtgpu_scanproject_params p = scanproject_params(prm);
    ndtgpu_status rc = scanproj_check("scanproj_project_device", n_scans, n_beams, angle_min, angle_increment, stride_bytes,
                                      map_stride_bytes, p);
    if (rc != NDTGPU_OK) return rc;
    if (n_scans && (!ranges_dev || !xyz_dev)) return fail(NDTGPU_ERR_INVALID, "scanproj_project_device: null ranges_dev or xyz_dev");
    if (!h) return fail(NDTGPU_ERR_INVALID, "scanproj_project_device: null handle");
    if ((rc = scanproj_fits("scanproj_project_device", h, n_scans, n_beams)) != NDTGPU_OK) return rc;
    if (n_scans == 0) return NDTGPU_OK;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));            // (the previous call, which used the tile counts, may have run on another stream)
    const hipError_t e = ndt_scanproject_launch(ranges_dev, (const unsigned long long *)scan_id_dev, n_scans, n_beams, angle_min,
                                                angle_increment, ndt_scanproject_params_dev(p), h->tile.get(), (uint32_t *)xyz_dev,
                                                stride_bytes / 4, map_stride_bytes / 4, n_kept_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "scanproj_project_device: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_scanproj_project(ndtgpu_scanproj *h, const double *ranges, const uint64_t *scan_id, size_t n_scans, size_t n_beams,
                                      double angle_min, double angle_increment, const ndtgpu_scanproject_params *prm, void *xyz,
                                      size_t stride_bytes, size_t map_stride_bytes, uint32_t *n_kept)
{
    const ndtgpu_scanproject_params p = scanproject_params(prm);
    ndtgpu_status rc = scanproj_check("scanproj_project", n_scans, n_beams, angle_min, angle_increment, stride_bytes, map_stride_bytes, p);
    if (rc != NDTGPU_OK) return rc;
    if (n_scans && (!ranges || !xyz)) return fail(NDTGPU_ERR_INVALID, "scanproj_project: null ranges or xyz");
    if (!h) return fail(NDTGPU_ERR_INVALID, "scanproj_project: null handle");
    if ((rc = scanproj_fits("scanproj_project", h, n_scans, n_beams)) != NDTGPU_OK) return rc;
    if (n_scans == 0) return NDTGPU_OK;
    // the rows travel packed (12 or 16 bytes each) and are spread to the caller's strides on the host: every other byte of xyz
    // stays as it is
    const size_t row = stride_bytes >= 16 ? 16 : 12, beams = n_scans * n_beams;
    StageLayout in, outl;
    const size_t o_ranges = in.take(beams * sizeof(double)), o_ids = in.take(scan_id ? n_scans * sizeof(uint64_t) : 0);
    const size_t o_rows = outl.take(beams * row), o_kept = outl.take(n_scans * sizeof(uint32_t));
    hipStream_t st = h->hst.get();
    HostStage &hs = h->host;
    if ((rc = hs.open(h, "scanproj_project", in, outl)) != NDTGPU_OK) return rc;
    memcpy(hs.in_host(o_ranges), ranges, beams * sizeof(double));
    if (scan_id) memcpy(hs.in_host(o_ids), scan_id, n_scans * sizeof(uint64_t));
    if ((rc = hs.upload(st)) != NDTGPU_OK) return rc;
    rc = ndtgpu_scanproj_project_device(h, (const double *)hs.in_dev(o_ranges), scan_id ? (const uint64_t *)hs.in_dev(o_ids) : nullptr,
                                        n_scans, n_beams, angle_min, angle_increment, &p, hs.out_dev(o_rows), row, n_beams * row,
                                        (uint32_t *)hs.out_dev(o_kept), (ndtgpu_stream)st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = hs.finish(h, st)) != NDTGPU_OK) return rc;
    for (size_t b = 0; b < n_scans; b++) {
        const char *src = hs.out_host(o_rows) + b * n_beams * row;
        char *dst = (char *)xyz + b * map_stride_bytes;
        for (size_t i = 0; i < n_beams; i++) memcpy(dst + i * stride_bytes, src + i * row, row);
    }
    if (n_kept) memcpy(n_kept, hs.out_host(o_kept), n_scans * sizeof(uint32_t));
    return NDTGPU_OK;
}

}   // extern "C"
