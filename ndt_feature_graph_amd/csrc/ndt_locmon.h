// ndt_locmon.h -- what the localisation monitor's kernels (csrc/ndt_locmon.hip), its C-ABI (csrc/ndtgpu_locmon.hip) and host
// programs share (include/ndtgpu.h "localisation monitor"): the radius of the distance field, the beam table, the pixel of a
// beam's endpoint, the key of a beam, the badness of a key, the composition of a picked pose, the rules of the two ordered
// selections and the checks of a call's arguments.  Plain C++ for host and device: NDT_HD is __host__ __device__ under hipcc and
// `inline` elsewhere, so tests/native/locmon_checks.cpp compiles this file with g++ alone (under the address and
// undefined-behaviour sanitizers).  tests/locmon_model.py restates all of it in NumPy.
//
// THE ORDER OF OPERATIONS, part of the contract: every expression below is evaluated as written in fp64, NOT contracted (no fused
// multiply-add).  A pose is (x, y, c, s) with c = cos(yaw), s = sin(yaw); beam i has the table entry (cb, sb) = (cos a_i, sin a_i),
// a_i = angle_min + (double)i * angle_increment, made on the host.
//   radius    R = (int)floor(max_dist / resolution)
//   kept      r is finite and r_min < r < r_max
//   endpoint  ex = c * cb - s * sb,  ey = s * cb + c * sb,  px = x + ex * r,  py = y + ey * r
//   pixel     fi = floor((px - ox) / resolution),  fj = floor((py - oy) / resolution)
//             in bounds iff 0 <= fi < width and 0 <= fj < height as doubles (a NaN is off the map)
//   key       the field's value k (dx^2 + dy^2 in pixels) | 0x10000 where the field says far | 0x10001 off the map
//   median    the element at index n_kept / 2 of the ascending keys of the kept beams
//   badness   resolution * sqrt((double)k) | max_dist for far | 1e9 off the map
//   compose   ref o match:  ax = xr + (cr * xm - sr * ym),  ay = yr + (sr * xm + cr * ym),  ac = cr * cm - sr * sm,  as = sr * cm + cr * sm
//             ... o post:   x = ax + (ac * px - as * py),  y = ay + (as * px + ac * py),  c = ac,  s = as
// The field itself is integer: row pass g = the smallest |dx| <= R to an obstacle pixel of the same row (255: none); column pass
// k = the smallest dy^2 + g^2 over |dy| <= R with k <= R^2 (0xFFFF: none).
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

#define NDT_LOCMON_THREADS 256                    // a workgroup of every pass
#define NDT_LOCMON_WAVES (NDT_LOCMON_THREADS / 64)
#define NDT_LOCMON_TILE NDT_LOCMON_THREADS        // candidates of an arg-min workgroup, pixels of a field workgroup
#define NDT_LOCMON_MAX_BEAMS 8192u
#define NDT_LOCMON_MAX_RADIUS 254
#define NDT_LOCMON_MAX_SIDE (1u << 15)            // width, height
#define NDT_LOCMON_MAX_GRIDS 1024u
#define NDT_LOCMON_MAX_PIXELS ((size_t)1 << 31)   // of all grids of a handle
#define NDT_LOCMON_MAX_SCANS (1u << 24)
#define NDT_LOCMON_MAX_QUERIES (1u << 24)
#define NDT_LOCMON_MAX_CANDIDATES (1u << 24)      // nx * ny * nyaw
#define NDT_LOCMON_MAX_PAIRS (1u << 20)
#define NDT_LOCMON_CHUNK_BEAMS ((size_t)1 << 23)  // beam evaluations of one launch of a search

#define NDT_LOCMON_ROW_NONE 255u                  // the row pass: no obstacle within R along the row
#define NDT_LOCMON_FIELD_FAR 0xFFFFu              // the field: no obstacle within R
#define NDT_LOCMON_KEY_FAR 0x10000u
#define NDT_LOCMON_KEY_OFFMAP 0x10001u
#define NDT_LOCMON_KEY_BITS 17                    // keys are below 2^17
#define NDT_LOCMON_NO_SCAN 0xFFFFFFFFu            // a query's scan: no query
#define NDT_LOCMON_OFFMAP_BADNESS 1e9             // localization_monitor.cpp:112
#define NDT_LOCMON_NO_RESULT_BADNESS 1e8          // localization_monitor.cpp:83

// ---- the field -----------------------------------------------------------------------------------------------------------------
// R of (max_dist, resolution); 0 where it is not 1 .. 254
NDT_HD int ndt_locmon_radius(double max_dist, double resolution)
{
    const double q = floor(max_dist / resolution);
    return q >= 1.0 && q <= (double)NDT_LOCMON_MAX_RADIUS ? (int)q : 0;
}

NDT_HD bool ndt_locmon_obstacle(int8_t v, int occupied_min) { return (int)v >= occupied_min; }

// the row pass at pixel x of a row of `width` pixels
NDT_HD uint32_t ndt_locmon_row_dist(const int8_t *row, uint32_t x, uint32_t width, int R, int occupied_min)
{
    for (int d = 0; d <= R; d++) {
        if ((uint32_t)d <= x && ndt_locmon_obstacle(row[x - (uint32_t)d], occupied_min)) return (uint32_t)d;
        if (x + (uint32_t)d < width && ndt_locmon_obstacle(row[x + (uint32_t)d], occupied_min)) return (uint32_t)d;
    }
    return NDT_LOCMON_ROW_NONE;
}

// the column pass at pixel (x, y): g is the row pass's output of the grid, [height][width]
NDT_HD uint32_t ndt_locmon_col_dist(const uint8_t *g, uint32_t x, uint32_t y, uint32_t width, uint32_t height, int R)
{
    const uint32_t R2 = (uint32_t)(R * R);
    uint32_t best = NDT_LOCMON_FIELD_FAR;
    const uint32_t y0 = y > (uint32_t)R ? y - (uint32_t)R : 0u, y1 = y + (uint32_t)R < height ? y + (uint32_t)R : height - 1u;
    for (uint32_t yy = y0; yy <= y1; yy++) {
        const uint32_t gv = g[(size_t)yy * width + x];
        if (gv == NDT_LOCMON_ROW_NONE) continue;
        const uint32_t dy = yy > y ? yy - y : y - yy, k = dy * dy + gv * gv;
        if (k <= R2 && k < best) best = k;
    }
    return best;
}

// ---- a beam ------------------------------------------------------------------------------------------------------------------------
NDT_HD bool ndt_locmon_kept(double r, double r_min, double r_max)
{
    return r >= -1.7976931348623157e308 && r <= 1.7976931348623157e308 && r > r_min && r < r_max;   // (a NaN fails every comparison)
}

// the pixel of the endpoint of a beam: true and (fi, fj) iff it is in bounds
NDT_HD bool ndt_locmon_pixel(double x, double y, double c, double s, double cb, double sb, double r, double ox, double oy, double resolution,
                             uint32_t width, uint32_t height, uint32_t &fi, uint32_t &fj)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ex = c * cb - s * sb, ey = s * cb + c * sb;
    const double px = x + ex * r, py = y + ey * r;
    const double di = floor((px - ox) / resolution), dj = floor((py - oy) / resolution);
    if (!(di >= 0.0 && di < (double)width && dj >= 0.0 && dj < (double)height)) return false;
    fi = (uint32_t)di;
    fj = (uint32_t)dj;
    return true;
}

NDT_HD uint32_t ndt_locmon_key_of_field(uint32_t field) { return field == NDT_LOCMON_FIELD_FAR ? NDT_LOCMON_KEY_FAR : field; }

NDT_HD double ndt_locmon_metres(uint32_t key, double resolution, double max_dist)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (key >= NDT_LOCMON_KEY_OFFMAP) return NDT_LOCMON_OFFMAP_BADNESS;
    if (key == NDT_LOCMON_KEY_FAR) return max_dist;
    return resolution * sqrt((double)key);
}

// ---- the picked pose: ref o match o post, poses as (x, y, c, s), post a translation ------------------------------------------------
NDT_HD void ndt_locmon_compose(const double ref[4], const double m[4], double post_x, double post_y, double out[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = ref[0] + (ref[2] * m[0] - ref[3] * m[1]);
    const double ay = ref[1] + (ref[3] * m[0] + ref[2] * m[1]);
    const double ac = ref[2] * m[2] - ref[3] * m[3];
    const double as = ref[3] * m[2] + ref[2] * m[3];
    out[0] = ax + (ac * post_x - as * post_y);
    out[1] = ay + (as * post_x + ac * post_y);
    out[2] = ac;
    out[3] = as;
}

// ---- the two ordered selections as one unsigned comparison ------------------------------------------------------------------------
// adjustPose: the smallest key, ties to the lowest candidate index -> the smallest word
NDT_HD unsigned long long ndt_locmon_min_word(uint32_t key, uint32_t index) { return ((unsigned long long)key << 32) | index; }
// updateUnlocalized: the most inliers, ties to the lowest pair -> the largest word; 0: the pair does not qualify
NDT_HD unsigned long long ndt_locmon_pick_word(int32_t status, int32_t n_inliers, int32_t min_num_matches, uint32_t pair)
{
    if (status != 0 || n_inliers <= min_num_matches || n_inliers <= 0) return 0ull;
    return ((unsigned long long)(uint32_t)n_inliers << 32) | (0xFFFFFFFFu - pair);
}

// ---- chunks of a search: the candidates of one launch, a multiple of the tile -------------------------------------------------------
NDT_HD size_t ndt_locmon_tiles(size_t n) { return (n + NDT_LOCMON_TILE - 1) / NDT_LOCMON_TILE; }
NDT_HD size_t ndt_locmon_handle_chunk(size_t max_beams, size_t max_candidates)
{
    const size_t per = NDT_LOCMON_CHUNK_BEAMS / (max_beams ? max_beams : 1) / NDT_LOCMON_TILE;
    const size_t chunk = (per ? per : 1) * NDT_LOCMON_TILE, all = ndt_locmon_tiles(max_candidates) * NDT_LOCMON_TILE;
    return chunk < all ? chunk : all;
}

// ---- checks: NULL: fine, else the message (it names the argument) ---------------------------------------------------------------
inline const char *ndt_locmon_check_params(const ndtgpu_locmon_params &p)
{
    if (!(p.max_dist > 0.0 && p.max_dist < 1e150)) return "max_dist must be finite and > 0";
    if (!(p.r_min >= 0.0 && p.r_min < 1e150)) return "r_min must be finite and >= 0";
    if (!(p.r_max > p.r_min)) return "r_max must be > r_min (+inf allowed)";
    if (!(std::fabs(p.post_x) < 1e150) || !(std::fabs(p.post_y) < 1e150)) return "post_x and post_y must be finite";
    if (p.occupied_min < -128 || p.occupied_min > 127) return "occupied_min must be -128 .. 127";
    if (p.min_num_matches < 0) return "min_num_matches must be >= 0";
    return nullptr;
}
inline const char *ndt_locmon_check_grids(size_t n_grids, size_t width, size_t height, double resolution, const ndtgpu_locmon_params &p)
{
    if (n_grids == 0 || n_grids > NDT_LOCMON_MAX_GRIDS) return "n_grids must be 1 .. 1024";
    if (width == 0 || width > NDT_LOCMON_MAX_SIDE) return "width must be 1 .. 2^15";
    if (height == 0 || height > NDT_LOCMON_MAX_SIDE) return "height must be 1 .. 2^15";
    if (n_grids * width * height > NDT_LOCMON_MAX_PIXELS) return "n_grids * width * height: more than 2^31 pixels";
    if (!(resolution > 0.0 && resolution < 1e150)) return "resolution must be finite and > 0";
    if (const char *bad = ndt_locmon_check_params(p)) return bad;
    if (ndt_locmon_radius(p.max_dist, resolution) == 0) return "max_dist / resolution: the radius must be 1 .. 254 pixels";
    return nullptr;
}
inline const char *ndt_locmon_check_beams(size_t n_beams, double angle_min, double angle_increment)
{
    if (n_beams == 0 || n_beams > NDT_LOCMON_MAX_BEAMS) return "n_beams must be 1 .. 8192";
    if (!(std::fabs(angle_min) < 1e150)) return "angle_min must be finite";
    if (!(std::fabs(angle_increment) < 1e150)) return "angle_increment must be finite";
    return nullptr;
}
inline const char *ndt_locmon_check_counts(size_t n_scans, size_t n_queries)
{
    if (n_scans == 0 || n_scans > NDT_LOCMON_MAX_SCANS) return "n_scans must be 1 .. 2^24";
    if (n_queries > NDT_LOCMON_MAX_QUERIES) return "n_queries: more than 2^24";
    return nullptr;
}
inline const char *ndt_locmon_check_lattice(size_t nx, size_t ny, size_t nyaw)
{
    if (nx == 0 || nx > NDT_LOCMON_MAX_CANDIDATES) return "nx must be 1 .. 2^24";
    if (ny == 0 || ny > NDT_LOCMON_MAX_CANDIDATES) return "ny must be 1 .. 2^24";
    if (nyaw == 0 || nyaw > NDT_LOCMON_MAX_CANDIDATES) return "nyaw must be 1 .. 2^24";
    if (nx * ny > NDT_LOCMON_MAX_CANDIDATES || nx * ny * nyaw > NDT_LOCMON_MAX_CANDIDATES) return "nx * ny * nyaw: more than 2^24 candidates";
    return nullptr;
}
// (the lattice tables of a call: csrc/ndt_lattice.h)
inline const char *ndt_locmon_check_capacity(size_t max_grids, size_t max_pixels, size_t max_beams, size_t max_candidates)
{
    if (max_grids == 0 || max_grids > NDT_LOCMON_MAX_GRIDS) return "max_grids must be 1 .. 1024";
    if (max_pixels == 0 || max_pixels > NDT_LOCMON_MAX_PIXELS) return "max_pixels must be 1 .. 2^31";
    if (max_beams == 0 || max_beams > NDT_LOCMON_MAX_BEAMS) return "max_beams must be 1 .. 8192";
    if (max_candidates == 0 || max_candidates > NDT_LOCMON_MAX_CANDIDATES) return "max_candidates must be 1 .. 2^24";
    return nullptr;
}

#if defined(__HIPCC__)
// what the handle holds on the device: the fields of the installed grids and the beam table
struct NdtLocmonMap {
    const uint16_t *field;                        // [n_grids][height][width]
    const double *origin;                         // [n_grids][2]
    const double *beams;                          // [n_beams][2] = (cb, sb)
    uint32_t n_grids, width, height, n_beams;
    double resolution, max_dist;
};
struct NdtLocmonSearch {
    const double *xs, *ys, *cs, *sn;              // the lattice tables, device copies
    uint32_t ny, nyaw, n_candidates, scan, grid;
    uint32_t *cand_key;                           // [chunk]
    unsigned long long *tile_word;                // [tiles of the lattice]
    uint32_t *volume;                             // [n_candidates] or NULL
    ndtgpu_locmon_adjust_result *result;
};
// host launchers: plain launches on `st`
hipError_t ndt_locmon_field_launch(const int8_t *grids, uint8_t *rowdist, uint16_t *field, uint32_t n_grids, uint32_t width, uint32_t height, int R,
                                   int occupied_min, hipStream_t st);
hipError_t ndt_locmon_evaluate_launch(const NdtLocmonMap &m, const double *ranges, uint32_t n_scans, const ndtgpu_locmon_query *queries,
                                      uint32_t n_queries, double r_min, double r_max, ndtgpu_locmon_result *results, hipStream_t st);
hipError_t ndt_locmon_adjust_launch(const NdtLocmonMap &m, const double *ranges, uint32_t n_scans, const NdtLocmonSearch &s, uint32_t chunk,
                                    double r_min, double r_max, hipStream_t st);
hipError_t ndt_locmon_pick_launch(const ndtgpu_featmatch_result *matches, const double *ref_poses, uint32_t n_pairs, uint32_t scan, uint32_t grid,
                                  int32_t min_num_matches, double post_x, double post_y, ndtgpu_locmon_query *query, ndtgpu_locmon_pick *pick,
                                  hipStream_t st);
#endif
