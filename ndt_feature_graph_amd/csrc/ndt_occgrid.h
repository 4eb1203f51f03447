// ndt_occgrid.h -- what csrc/ndt_occgrid.hip (kernel) and csrc/ndtgpu_occgrid.hip (C-ABI) share of the occupancy-grid export
// (include/ndtgpu.h "occupancy-grid export"): the geometry of a grid, the value of a pixel and the launcher.
#pragma once
#include "ndt_common.h"
#include "ndt_math.h"

// what the kernel needs of a call besides the map set
struct NdtOccGridCall {
    int width, height;             // pixels per row, rows
    double r;                      // pixel size
    double z;                      // the probed height (ndtgpu_occgrid_params::z)
    int occupied_no_gaussian;      // value of a cell with occ > 0 and no Gaussian
};

// lower corner of a map's grid along one axis: centre - (cells * res) / 2, and the centre of pixel i: origin + (i + 0.5) r.
// fp64, not contracted: the host (ndtgpu_occgrid_dims), the kernel and tests/occgrid_model.py evaluate the same roundings.
NDT_HD double ndt_occgrid_origin(double centre, int cells, double res)
{
#pragma clang fp contract(off)
    const double size_m = cells * res;
    return centre - size_m / 2;
}
NDT_HD double ndt_occgrid_pixel(double origin, int i, double r)
{
#pragma clang fp contract(off)
    return origin + (i + 0.5) * r;
}

// Sigma^-1 of a stored cell covariance (xx xy xz yy yz zz) by the adjugate.  Refuses only det <= 0 and a determinant that is not
// finite: a single cell's covariance is legitimately tiny (a wall cell at 0.5 m with eigenvalues 0.02, 2e-5, 2e-5 has det 8e-12),
// so the |det| > 1e-12 gate that inverse_check (csrc/ndt_math.h) applies to C_i + C_j has no place here.
NDT_HD bool ndt_occgrid_inverse(const double c[6], double inv[6])
{
    const double c00 = c[3] * c[5] - c[4] * c[4];
    const double c01 = c[4] * c[2] - c[1] * c[5];
    const double c02 = c[1] * c[4] - c[3] * c[2];
    const double det = c[0] * c00 + c[1] * c01 + c[2] * c02;
    if (!(det > 0.0 && det < __builtin_inf())) return false;
    const double id = 1.0 / det;
    inv[0] = c00 * id;
    inv[1] = c01 * id;
    inv[2] = c02 * id;
    inv[3] = (c[0] * c[5] - c[2] * c[2]) * id;
    inv[4] = (c[1] * c[2] - c[0] * c[4]) * id;
    inv[5] = (c[0] * c[3] - c[1] * c[1]) * id;
    return true;
}

// the value of a pixel at p in a cell with occ > 0 and the Gaussian (mean, cov): 55..100, -1 where the likelihood is not a number
NDT_HD int ndt_occgrid_gaussian_value(const double p[3], const double mean[3], const double cov[6])
{
    double inv[6];
    if (!ndt_occgrid_inverse(cov, inv)) return -1;
    const double dx = p[0] - mean[0], dy = p[1] - mean[1], dz = p[2] - mean[2];
    const double l = dx * (inv[0] * dx + inv[1] * dy + inv[2] * dz) + dy * (inv[1] * dx + inv[3] * dy + inv[4] * dz) +
                     dz * (inv[2] * dx + inv[4] * dy + inv[5] * dz);
    if (!(l - l == 0.0)) return -1;                  // NaN or infinite
    const double v = 0.5 + 0.5 * (exp(-l / 2) + 0.1);
    return v > 1.0 ? 100 : (int)(v * 100);
}

// maps [first, first + count) -> count grids of width * height bytes back to back at out_dev; asynchronous on `stream`
hipError_t ndt_launch_occgrid(const NdtSetView &set, size_t first, size_t count, const NdtOccGridCall &call, int8_t *out_dev,
                              hipStream_t stream);
