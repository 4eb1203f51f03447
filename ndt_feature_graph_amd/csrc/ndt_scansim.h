// ndt_scansim.h -- what the scan simulator's kernels (csrc/ndt_scansim.hip), its C-ABI (csrc/ndtgpu_scansim.hip) and host programs
// share (include/ndtgpu.h "scan simulation"): the reach of a ray, the cell of a point, the ray of a beam, the cell of a step, the
// walk of a ray through a grid, the lattice of reference poses and the checks of a call's arguments.  Plain C++ for host and
// device: NDT_HD is __host__ __device__ under hipcc and `inline` elsewhere, so tests/native/scansim_checks.cpp compiles this file
// with g++ alone (under the address and undefined-behaviour sanitizers).  tests/scansim_model.py restates all of it in NumPy.
//
// THE ORDER OF OPERATIONS, part of the contract: every fp64 expression below is evaluated as written, NOT contracted (no fused
// multiply-add); everything behind the two cells of a ray is integer.  A pose is (x, y, c, s); beam i has the table entry
// (cb, sb) = (cos a_i, sin a_i), a_i = angle_min + (double)i * angle_increment, made on the host (ndtgpu_locmon_beam_table).
//   reach      R = (int)floor(range_max / resolution)
//   cell       of a point (px, py): (floor((px - ox) / resolution), floor((py - oy) / resolution)), in the grid iff 0 <= . < width,
//              height as doubles (a NaN is off the map)
//   direction  ex = c * cb - s * sb,  ey = s * cb + c * sb   (the order of ndt_locmon_pixel)
//   ray        c0 = cell(x, y), c1 = cell(x + ex * range_max, y + ey * range_max), (di, dj) = c1 - c0, n = max(|di|, |dj|).  A ray with
//              |di| or |dj| above 2^15, or not a number -- a direction that is no unit vector -- is a miss without a walk.
//   step k     1 .. n: sign * k on the major axis (x where |di| == |dj|), sign * floor((2 * k * dmin + n) / (2 * n)) on the minor one
//   stop       per visited cell, in this order: outside the grid: miss; d2 = di_k^2 + dj_k^2 > R * R: miss; an obstacle (v >=
//              occupied_min), or an unknown pixel (v < 0) where unknown_is_obstacle: hit, range = resolution * sqrt((double)d2);
//              behind step n: miss.  The start cell is never tested.
//   lattice    position (ix, iy) = (px * skip, py * skip), px < npx = ceil(width / skip), py < npy likewise, px outermost; kept iff
//              its pixel == 0 and its centre (ox + ((double)ix + 0.5) * resolution, oy + ((double)iy + 0.5) * resolution) lies in
//              [x0, x1] x [y0, y1]; the linear index of heading t at a position is (px * npy + py) * nyaw + t.
#pragma once
#include "../../include/ndtgpu.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "ndt_common.h"   // NDT_HD
#elif !defined(NDT_HD)
#define NDT_HD inline
#endif

#define NDT_SCANSIM_THREADS 256                   // a workgroup of every kernel
#define NDT_SCANSIM_WAVES (NDT_SCANSIM_THREADS / 64)
#define NDT_SCANSIM_TILE NDT_SCANSIM_THREADS      // beams of one pass of a cast workgroup, positions of a lattice workgroup
#define NDT_SCANSIM_MAX_BEAMS 8192u
#define NDT_SCANSIM_MAX_REACH 4094
#define NDT_SCANSIM_MAX_SIDE (1u << 15)           // width, height
#define NDT_SCANSIM_MAX_GRIDS 1024u
#define NDT_SCANSIM_MAX_POSES (1u << 24)
#define NDT_SCANSIM_MAX_DELTA 32768.0             // |di|, |dj| of a ray
#define NDT_SCANSIM_MAX_NODES 0xFFFFFFFFull       // of a lattice: the linear index is a uint32
#define NDT_SCANSIM_LAUNCH_POSES (1u << 22)       // poses of one launch of the cast

// R of (range_max, resolution); 0 where it is not 1 .. 4094
NDT_HD int ndt_scansim_reach(double range_max, double resolution)
{
    const double q = floor(range_max / resolution);
    return q >= 1.0 && q <= (double)NDT_SCANSIM_MAX_REACH ? (int)q : 0;
}

// skip = (unsigned)(ref_pos_resolution / resolution); 0 where it is not 1 .. 2^15
NDT_HD uint32_t ndt_scansim_skip(double ref_pos_resolution, double resolution)
{
    const double q = ref_pos_resolution / resolution;
    return q >= 1.0 && q < (double)NDT_SCANSIM_MAX_SIDE + 1.0 ? (uint32_t)q : 0u;
}

// the cell of a point: true and (i, j) iff it is in the grid
NDT_HD bool ndt_scansim_point_cell(double px, double py, double ox, double oy, double resolution, uint32_t width, uint32_t height, int32_t &i,
                                   int32_t &j)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double fi = floor((px - ox) / resolution), fj = floor((py - oy) / resolution);
    if (!(fi >= 0.0 && fi < (double)width && fj >= 0.0 && fj < (double)height)) return false;
    i = (int32_t)fi;
    j = (int32_t)fj;
    return true;
}

// a ray in cells: n steps, |minor| = dmin at the end, the signs of the two axes
struct NdtScansimRay {
    int32_t si, sj;                               // -1, 0, 1
    int32_t n, dmin;
    int32_t xmajor;                               // the x axis advances a cell a step
};

NDT_HD NdtScansimRay ndt_scansim_ray_of(int32_t di, int32_t dj)
{
    NdtScansimRay r;
    const int32_t ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj;
    r.si = di > 0 ? 1 : (di < 0 ? -1 : 0);
    r.sj = dj > 0 ? 1 : (dj < 0 ? -1 : 0);
    r.xmajor = ai >= aj ? 1 : 0;
    r.n = r.xmajor ? ai : aj;
    r.dmin = r.xmajor ? aj : ai;
    return r;
}

// the ray of a beam from the pose (x, y, c, s) whose cell is (i0, j0): false where it is a miss without a walk
NDT_HD bool ndt_scansim_beam_ray(double x, double y, double c, double s, double cb, double sb, double range_max, double ox, double oy,
                                 double resolution, int32_t i0, int32_t j0, NdtScansimRay &ray)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ex = c * cb - s * sb, ey = s * cb + c * sb;
    const double px = x + ex * range_max, py = y + ey * range_max;
    const double di = floor((px - ox) / resolution) - (double)i0, dj = floor((py - oy) / resolution) - (double)j0;
    if (!(fabs(di) <= NDT_SCANSIM_MAX_DELTA && fabs(dj) <= NDT_SCANSIM_MAX_DELTA)) return false;
    ray = ndt_scansim_ray_of((int32_t)di, (int32_t)dj);
    return true;
}

// the closed form, the specification: the cell of step k of the ray, relative to its start
NDT_HD void ndt_scansim_step_cell(const NdtScansimRay &r, int32_t k, int32_t &a, int32_t &b)
{
    const int32_t m = r.n > 0 ? (int32_t)((2 * (int64_t)k * r.dmin + r.n) / (2 * (int64_t)r.n)) : 0;   // (2^31 and more at |di| = |dj| = 2^15)
    a = r.xmajor ? r.si * k : r.si * m;
    b = r.xmajor ? r.sj * m : r.sj * k;
}

NDT_HD bool ndt_scansim_blocked(int8_t v, int occupied_min, int unknown_is_obstacle)
{
    return (int)v >= occupied_min || (unknown_is_obstacle && v < 0);
}

// The walk of a ray from (i0, j0) through one grid: true and d2 at a hit.  The minor axis by the accumulator that equals the closed
// form (tests/test_scansim_model.py compares the two for every |di|, |dj| <= 40; scansim_checks.cpp again).
// AT MOST R + 2 STEPS: the major axis is k cells from the start at step k, so d2 >= k * k, and k = R + 1 fails the reach test; a
// ray of a unit direction has n <= R + 2 by its construction anyway.
NDT_HD bool ndt_scansim_walk(const int8_t *grid, uint32_t width, uint32_t height, int32_t i0, int32_t j0, const NdtScansimRay &r, int32_t R,
                             int occupied_min, int unknown_is_obstacle, uint32_t &d2_out)
{
    const int32_t R2 = R * R, two_n = 2 * r.n, two_d = 2 * r.dmin;
    int32_t acc = r.n, m = 0;
    for (int32_t k = 1; k <= r.n; k++) {
        acc += two_d;
        if (acc >= two_n) { acc -= two_n; m++; }
        const int32_t a = r.xmajor ? r.si * k : r.si * m, b = r.xmajor ? r.sj * m : r.sj * k;
        const int32_t i = i0 + a, j = j0 + b;
        if (i < 0 || j < 0 || i >= (int32_t)width || j >= (int32_t)height) return false;
        const int32_t d2 = k * k + m * m;
        if (d2 > R2) return false;
        if (ndt_scansim_blocked(grid[(size_t)j * width + (size_t)i], occupied_min, unknown_is_obstacle)) {
            d2_out = (uint32_t)d2;
            return true;
        }
    }
    return false;
}

NDT_HD double ndt_scansim_metres(uint32_t d2, double resolution)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return resolution * sqrt((double)d2);
}

// ---- the lattice ---------------------------------------------------------------------------------------------------------------
NDT_HD uint32_t ndt_scansim_axis_nodes(uint32_t side, uint32_t skip) { return (side + skip - 1u) / skip; }

// position (px, py) of the lattice: kept iff its pixel is free and its centre lies in the box; the centre in (cx, cy)
NDT_HD bool ndt_scansim_position(const int8_t *grid, uint32_t width, uint32_t px, uint32_t py, uint32_t skip, double ox, double oy,
                                 double resolution, const double box4[4], double &cx, double &cy)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t ix = px * skip, iy = py * skip;
    cx = ox + ((double)ix + 0.5) * resolution;
    cy = oy + ((double)iy + 0.5) * resolution;
    if (grid[(size_t)iy * width + ix] != 0) return false;
    return cx >= box4[0] && cx <= box4[2] && cy >= box4[1] && cy <= box4[3];
}

// the headings of generateRefScans: theta = 0, then theta += angle_step while theta < 6.28; the count, and cs / sn where not NULL
// (up to room)
inline size_t ndt_scansim_headings(double angle_step, double *cs, double *sn, size_t room)
{
    size_t n = 0;
    for (double theta = 0.0; theta < 6.28 && n <= NDT_SCANSIM_MAX_POSES; theta += angle_step, n++) {
        if (n < room) {
            if (cs) cs[n] = cos(theta);
            if (sn) sn[n] = sin(theta);
        }
    }
    return n;
}

NDT_HD size_t ndt_scansim_tiles(size_t n) { return (n + NDT_SCANSIM_TILE - 1) / NDT_SCANSIM_TILE; }

// ---- checks: NULL: fine, else the message (it names the argument) ---------------------------------------------------------------
inline const char *ndt_scansim_check_params(const ndtgpu_scansim_params &p)
{
    if (!(p.range_max > 0.0 && p.range_max < 1e150)) return "range_max must be finite and > 0";
    if (!(std::fabs(p.miss) < 1e150)) return "miss must be finite";
    if (p.occupied_min < -128 || p.occupied_min > 127) return "occupied_min must be -128 .. 127";
    if (p.unknown_is_obstacle != 0 && p.unknown_is_obstacle != 1) return "unknown_is_obstacle must be 0 or 1";
    return nullptr;
}
inline const char *ndt_scansim_check_grids(size_t n_grids, size_t width, size_t height, double resolution)
{
    if (n_grids == 0 || n_grids > NDT_SCANSIM_MAX_GRIDS) return "n_grids must be 1 .. 1024";
    if (width == 0 || width > NDT_SCANSIM_MAX_SIDE) return "width must be 1 .. 2^15";
    if (height == 0 || height > NDT_SCANSIM_MAX_SIDE) return "height must be 1 .. 2^15";
    if (!(resolution > 0.0 && resolution < 1e150)) return "resolution must be finite and > 0";
    return nullptr;
}
inline const char *ndt_scansim_check_reach(double resolution, const ndtgpu_scansim_params &p)
{
    if (const char *bad = ndt_scansim_check_params(p)) return bad;
    if (ndt_scansim_reach(p.range_max, resolution) == 0) return "range_max / resolution: the reach must be 1 .. 4094 cells";
    return nullptr;
}
inline const char *ndt_scansim_check_beams(size_t n_beams, double angle_min, double angle_increment)
{
    if (n_beams == 0 || n_beams > NDT_SCANSIM_MAX_BEAMS) return "n_beams must be 1 .. 8192";
    if (!(std::fabs(angle_min) < 1e150)) return "angle_min must be finite";
    if (!(std::fabs(angle_increment) < 1e150)) return "angle_increment must be finite";
    return nullptr;
}
inline const char *ndt_scansim_check_poses(size_t n_poses)
{
    if (n_poses == 0 || n_poses > NDT_SCANSIM_MAX_POSES) return "n_poses must be 1 .. 2^24";
    return nullptr;
}
inline const char *ndt_scansim_check_lattice(size_t width, size_t height, size_t skip, size_t nyaw, const double *box4, size_t capacity)
{
    if (skip == 0 || skip > NDT_SCANSIM_MAX_SIDE) return "skip must be 1 .. 2^15";
    if (nyaw == 0 || nyaw > NDT_SCANSIM_MAX_POSES) return "nyaw must be 1 .. 2^24";
    if (capacity == 0 || capacity > NDT_SCANSIM_MAX_POSES) return "capacity must be 1 .. 2^24";
    if (box4) {
        for (int k = 0; k < 4; k++)
            if (box4[k] != box4[k]) return "box4 must not hold a NaN";
    }
    const unsigned long long nodes = (unsigned long long)((width + skip - 1) / skip) * ((height + skip - 1) / skip);
    if (nodes > NDT_SCANSIM_MAX_NODES / nyaw) return "the lattice: more than 2^32 - 1 nodes";
    return nullptr;
}
inline const char *ndt_scansim_check_capacity(size_t max_grids, size_t max_beams, size_t max_poses)
{
    if (max_grids == 0 || max_grids > NDT_SCANSIM_MAX_GRIDS) return "max_grids must be 1 .. 1024";
    if (max_beams == 0 || max_beams > NDT_SCANSIM_MAX_BEAMS) return "max_beams must be 1 .. 8192";
    if (max_poses == 0 || max_poses > NDT_SCANSIM_MAX_POSES) return "max_poses must be 1 .. 2^24";
    return nullptr;
}

#if defined(__HIPCC__)
// what the handle holds on the device: the installed grids (borrowed or owned), their origins and the beam table
struct NdtScansimMap {
    const int8_t *grids;                          // [n_grids][height][width]
    const double *origin;                         // [n_grids][2]
    const double *beams;                          // [n_beams][2] = (cb, sb)
    uint32_t n_grids, width, height, n_beams;
    double resolution;
};
struct NdtScansimCast {
    double range_max, miss;
    int32_t R, occupied_min, unknown_is_obstacle;
};
struct NdtScansimLattice {
    const double *cs, *sn;                        // [nyaw], device copies
    uint32_t grid, skip, npx, npy, nyaw;
    double box4[4];
    uint32_t *tile;                               // [tiles of the positions]: counts, then the kept before each tile
    unsigned long long capacity;
    double *poses;                                // [capacity][4]
    uint32_t *index;                              // [capacity] or NULL
    uint32_t *count;                              // [2]: written, passed
};
// host launchers: plain launches on `st`
hipError_t ndt_scansim_cast_launch(const NdtScansimMap &m, const NdtScansimCast &c, const double *poses, const uint32_t *grid_idx, uint32_t n_poses,
                                   const uint32_t *count, double *ranges, ndtgpu_scansim_result *results, hipStream_t st);
hipError_t ndt_scansim_lattice_launch(const NdtScansimMap &m, const NdtScansimLattice &l, hipStream_t st);
#endif
