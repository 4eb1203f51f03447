// ndtgpu_occgrid.hip -- C-ABI (include/ndtgpu.h) of the occupancy-grid export: maps of a set rasterised the way
// lslgeneric::toOccupancyGrid fills a nav_msgs::OccupancyGrid (ndt_feature2d_fuser.cpp:428-433, 450-454), and moveOccupancyMap
// (ros_utils.h:12-18).  Host side only: the geometry of a grid, the argument checks, the copy of the synchronous form and its
// counts; the kernel is in csrc/ndt_occgrid.hip.  No handle: the temporary of the synchronous form is a local of the owning
// type and is gone on return.
#include "ndtgpu_host.h"
#include "ndt_occgrid.h"

namespace {

const double OCCGRID_MAX_BYTES = 1099511627776.0;      // 2^40 per call

// what both forms check before any device work; fills the call's shape
ndtgpu_status occgrid_prepare(const char *who, ndtgpu_mapset *s, size_t first, size_t count, double occ_resolution,
                              const ndtgpu_occgrid_params *prm, const void *out, NdtOccGridCall &call)
{
    char msg[160];
    // what needs no handle first: a map set only exists where a device does
    if (!(occ_resolution > 0.0) || !std::isfinite(occ_resolution)) {
        snprintf(msg, sizeof msg, "%s: occ_resolution must be positive and finite", who);
        return fail(NDTGPU_ERR_INVALID, msg);
    }
    if (!out) {
        snprintf(msg, sizeof msg, "%s: null output", who);
        return fail(NDTGPU_ERR_INVALID, msg);
    }
    if (!s) {
        snprintf(msg, sizeof msg, "%s: null map set", who);
        return fail(NDTGPU_ERR_INVALID, msg);
    }
    const ndtgpu_occgrid_params p = params_or_default(prm, ndtgpu_default_occgrid_params);
    if (std::isnan(p.z) || p.occupied_no_gaussian < -128 || p.occupied_no_gaussian > 127) {
        snprintf(msg, sizeof msg, "%s: params.z must be a number, params.occupied_no_gaussian an int8", who);
        return fail(NDTGPU_ERR_INVALID, msg);
    }
    double origin[3];
    const double c0[3] = {0., 0., 0.};
    const ndtgpu_status rc = ndtgpu_occgrid_dims(s->v.grid.res, s->v.grid.size, c0, occ_resolution, &call.width, &call.height, origin);
    if (rc != NDTGPU_OK) return rc;
    const ndtgpu_status rc2 = ndtgpu_occgrid_check(s->n_maps, first, count, call.width, call.height);
    if (rc2 != NDTGPU_OK) return rc2;
    call.r = occ_resolution;
    call.z = p.z;
    call.occupied_no_gaussian = p.occupied_no_gaussian;
    return NDTGPU_OK;
}

}  // namespace

extern "C" {

void ndtgpu_default_occgrid_params(ndtgpu_occgrid_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->z = 0.0;                       // upstream probes pcl::PointXYZ(px, py, 0)
    p->occupied_no_gaussian = 100;
}

ndtgpu_status ndtgpu_occgrid_dims(double res, const int32_t cells_per_axis[3], const double centre[3], double occ_resolution,
                                  int32_t *width, int32_t *height, double origin[3])
{
    if (!cells_per_axis || !centre || !width || !height || !origin) return fail(NDTGPU_ERR_INVALID, "occgrid_dims: null argument");
    if (!(res > 0.0) || !std::isfinite(res) || !(occ_resolution > 0.0) || !std::isfinite(occ_resolution))
        return fail(NDTGPU_ERR_INVALID, "occgrid_dims: res and occ_resolution must be positive and finite");
    if (cells_per_axis[0] <= 0 || cells_per_axis[1] <= 0 || cells_per_axis[2] <= 0)
        return fail(NDTGPU_ERR_INVALID, "occgrid_dims: empty grid axis");
    int32_t wh[2];
    for (int a = 0; a < 2; a++) {
        const double size_m = cells_per_axis[a] * res;
        const double n = size_m / occ_resolution;
        if (!(n < 1073741824.0)) return fail(NDTGPU_ERR_INVALID, "occgrid_dims: 2^30 pixels or more along an axis");
        wh[a] = (int32_t)n;
        if (wh[a] <= 0) return fail(NDTGPU_ERR_INVALID, "occgrid_dims: width or height 0 (occ_resolution larger than the map)");
    }
    *width = wh[0];
    *height = wh[1];
    origin[0] = ndt_occgrid_origin(centre[0], cells_per_axis[0], res);
    origin[1] = ndt_occgrid_origin(centre[1], cells_per_axis[1], res);
    origin[2] = 0.0;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_occgrid_check(size_t n_maps, size_t first, size_t count, int32_t width, int32_t height)
{
    if (first > n_maps || count > n_maps - first) return fail(NDTGPU_ERR_INVALID, "occupancy_grid: maps [first, first + count) out of range");
    if (width <= 0 || height <= 0) return fail(NDTGPU_ERR_INVALID, "occupancy_grid: width or height 0");
    if ((double)count * (double)width * (double)height > OCCGRID_MAX_BYTES)
        return fail(NDTGPU_ERR_INVALID, "occupancy_grid: count * width * height beyond 2^40 bytes");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset_occupancy_grid_device(ndtgpu_mapset *s, size_t first, size_t count, double occ_resolution,
                                                  const ndtgpu_occgrid_params *prm, int8_t *out_dev, ndtgpu_stream stream)
{
    NdtOccGridCall call;
    ndtgpu_status rc = occgrid_prepare("occupancy_grid_device", s, first, count, occ_resolution, prm, out_dev, call);
    if (rc != NDTGPU_OK) return rc;
    if (count == 0) return NDTGPU_OK;
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "occupancy_grid_device: no HIP device");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = s->wait_all_on(st)) != NDTGPU_OK) return rc;         // (builds on other streams)
    const hipError_t e = ndt_launch_occgrid(s->v, first, count, call, out_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "occupancy_grid_device: launch", e);
    return s->touch(st);
}

ndtgpu_status ndtgpu_mapset_occupancy_grid(ndtgpu_mapset *s, size_t first, size_t count, double occ_resolution,
                                           const ndtgpu_occgrid_params *prm, int8_t *out_host, ndtgpu_occgrid_info *info,
                                           ndtgpu_stream stream)
{
    NdtOccGridCall call;
    ndtgpu_status rc = occgrid_prepare("occupancy_grid", s, first, count, occ_resolution, prm, out_host, call);
    if (rc != NDTGPU_OK) return rc;
    if (count == 0) return NDTGPU_OK;
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "occupancy_grid: no HIP device");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = s->wait_all_on(st)) != NDTGPU_OK) return rc;
    std::vector<NdtMapCounters> ctr(count);
    HIP_TRY(hipMemcpyAsync(ctr.data(), s->v.counters + first, count * sizeof(NdtMapCounters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < count; k++)
        if (ctr[k].overflow) return fail(NDTGPU_ERR_CAPACITY, "occupancy_grid: a map needs more cells than max_cells");
    const size_t per_map = (size_t)call.width * (size_t)call.height, bytes = count * per_map;
    DeviceBuffer<int8_t> grid_dev;
    if (grid_dev.alloc(bytes) != hipSuccess) return fail(NDTGPU_ERR_ALLOC, "occupancy_grid: device buffer");
    const hipError_t e = ndt_launch_occgrid(s->v, first, count, call, grid_dev.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "occupancy_grid: launch", e);
    HIP_TRY(hipMemcpyAsync(out_host, grid_dev.get(), bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info)
        for (size_t k = 0; k < count; k++) {
            ndtgpu_occgrid_info &o = info[k];
            memset(&o, 0, sizeof o);
            (void)ndtgpu_occgrid_dims(s->v.grid.res, s->v.grid.size, &s->centres_host[(first + k) * 3], occ_resolution, &o.width, &o.height,
                                      o.origin);
            o.resolution = occ_resolution;
            const int8_t *d = out_host + k * per_map;
            for (size_t i = 0; i < per_map; i++) {
                if (d[i] < 0) o.n_unknown++;
                else if (d[i] == 0) o.n_free++;
                else o.n_occupied++;
            }
        }
    return NDTGPU_OK;
}

void ndtgpu_occgrid_move(const double T16[16], const double origin_pose16[16], double moved16[16])
{
    if (!T16 || !origin_pose16 || !moved16) return;
    double m[16];
    for (int c = 0; c < 4; c++)                     // column-major 4 x 4, like every T16 of this interface
        for (int r = 0; r < 4; r++) {
            double sum = 0.0;
            for (int k = 0; k < 4; k++) sum += T16[4 * k + r] * origin_pose16[4 * c + k];
            m[4 * c + r] = sum;
        }
    memcpy(moved16, m, sizeof m);
}

}   // extern "C"
