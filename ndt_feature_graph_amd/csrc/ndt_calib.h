// ndt_calib.h -- what the laser-to-base extrinsic calibration's kernels (csrc/ndt_calib.hip), its C-ABI (csrc/ndtgpu_calib.hip) and
// host programs share (include/ndtgpu.h "extrinsic calibration"): the lattice of candidates, the motion of a pair, the score's
// arithmetic, the winner's rule, the pair selection and the checks of a call's arguments.  Plain C++ for host and device: NDT_HD is
// __host__ __device__ under hipcc and `inline` elsewhere, so tests/native/calib_checks.cpp compiles this file with g++ alone (under
// the address and undefined-behaviour sanitizers).  tests/calib_model.py restates all of it in NumPy.
//
// THE ORDER OF OPERATIONS, part of the contract: every expression below is evaluated as written in fp64, NOT contracted (no fused
// multiply-add), on the float32 coordinates widened to double.  A pair is (cloud1 = a, pose1, cloud2 = b, pose2), a pose is
// (x, y, c, s) with c = cos(yaw), s = sin(yaw); a candidate is (xs, ys, c, s) with c / s from the host's tables.
//   pair      ex = x2 - x1, ey = y2 - y1
//             dx = c1 * ex + s1 * ey,  dy = c1 * ey - s1 * ex,  cd = c1 * c2 + s1 * s2,  sd = c1 * s2 - s1 * c2      (D = pose1^-1 pose2)
//   row of b  brx = cd * bx - sd * by,  bry = sd * bx + cd * by                                        (once per pair)
//   candidate ux = dx + (cd * xs - sd * ys) - xs,  uy = dy + (sd * xs + cd * ys) - ys                  (left to right)
//             tx = c * ux + s * uy,  ty = c * uy - s * ux
//   point     b' = (brx + tx, bry + ty, bz)
//             d2 = ((ax - b'x)^2 + (ay - b'y)^2) + (az - b'z)^2,  m = the minimum of d2 over the rows of a
//             term = m > th2 ? th2 : m,  th2 = max_dist * max_dist
//   pair      the terms added one after another in ascending row order of b, starting from 0.0
//   score     the pairs' sums added one after another in ascending pair order, starting from 0.0
// Rows at or beyond n_kept are ignored; a row in front of n_kept with a non-finite coordinate is skipped and counted; a pair whose
// cloud1 has no usable row contributes 0.0, and so does one whose cloud2 has none.  The winner is the smallest score, ties to the
// lowest linear index (ix * ny + iy) * nyaw + iyaw.
#pragma once
#include "../../include/ndtgpu.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "ndt_common.h"   // NDT_HD
#else
#define NDT_HD inline
#endif

#define NDT_CALIB_THREADS 256                     // a workgroup of every pass
#define NDT_CALIB_WAVES (NDT_CALIB_THREADS / 64)
#define NDT_CALIB_TILE NDT_CALIB_THREADS          // candidates of a workgroup: a lane per candidate
#define NDT_CALIB_MAX_POINTS (1u << 16)           // rows of a scan
#define NDT_CALIB_MAX_PAIRS 1024u                 // (the second dimension of the score pass's grid)
#define NDT_CALIB_MAX_SCANS (1u << 20)
#define NDT_CALIB_MAX_CANDIDATES (1u << 24)       // nx * ny * nyaw
#define NDT_CALIB_PARTIAL_DOUBLES ((size_t)1 << 22)   // the (pair, candidate) sums of one chunk: 32 MiB
#define NDT_CALIB_CAP 1e6                         // the reference's min_score at the start of bruteForceOptimization

#define NDT_CALIB_FLAG_NO_RESULT 1u               // the winner's score is >= NDT_CALIB_CAP: the reference would report nothing
#define NDT_CALIB_FLAG_BAD_PAIR 2u                // a pair names a scan >= n_scans: it contributed 0.0

// ---- the lattice ---------------------------------------------------------------------------------------------------------------
// the nodes of `for (double v = centre - span; v < centre + span; v += step)`: their count, and the first `room` of them in out
// (out may be NULL).  More than `cap` nodes: cap + 1 (the walk stops there).
inline size_t ndt_calib_axis(double centre, double span, double step, double *out, size_t room, size_t cap)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    size_t n = 0;
    const double end = centre + span;
    for (double v = centre - span; v < end; v += step) {
        if (n >= cap) return cap + 1;
        if (out && n < room) out[n] = v;
        n++;
    }
    return n;
}

inline const char *ndt_calib_check_lattice(double ix, double iy, double iyaw, double x_s, double y_s, double yaw_s, double t_r, double yaw_r)
{
    if (!(std::fabs(ix) < 1e300) || !(std::fabs(iy) < 1e300) || !(std::fabs(iyaw) < 1e300)) return "ix, iy and iyaw must be finite";
    if (!(x_s > 0.0 && x_s < 1e300)) return "x_s must be finite and > 0";
    if (!(y_s > 0.0 && y_s < 1e300)) return "y_s must be finite and > 0";
    if (!(yaw_s > 0.0 && yaw_s < 1e300)) return "yaw_s must be finite and > 0";
    if (!(t_r > 0.0 && t_r < 1e300)) return "t_r must be finite and > 0";
    if (!(yaw_r > 0.0 && yaw_r < 1e300)) return "yaw_r must be finite and > 0";
    return nullptr;
}

// ---- the motion of a pair --------------------------------------------------------------------------------------------------------
// D = pose1^-1 pose2 as (dx, dy, cd, sd) of two poses (x, y, c, s)
NDT_HD void ndt_calib_pair_motion(const double p1[4], const double p2[4], double D[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ex = p2[0] - p1[0], ey = p2[1] - p1[1];
    D[0] = p1[2] * ex + p1[3] * ey;
    D[1] = p1[2] * ey - p1[3] * ex;
    D[2] = p1[2] * p2[2] + p1[3] * p2[3];
    D[3] = p1[2] * p2[3] - p1[3] * p2[2];
}

// ---- the score ---------------------------------------------------------------------------------------------------------------------
NDT_HD bool ndt_calib_usable(float x, float y, float z)
{
    const float big = 3.4028234663852886e38f;     // (a NaN fails every comparison)
    return x >= -big && x <= big && y >= -big && y <= big && z >= -big && z <= big;
}

// a row of cloud2 under the pair's rotation
NDT_HD void ndt_calib_rotate(double cd, double sd, double bx, double by, double &brx, double &bry)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    brx = cd * bx - sd * by;
    bry = sd * bx + cd * by;
}

// the translation of M = Ts^-1 D Ts for the candidate Ts = (xs, ys, c, s)
NDT_HD void ndt_calib_translation(const double D[4], double xs, double ys, double c, double s, double &tx, double &ty)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ux = D[0] + (D[2] * xs - D[3] * ys) - xs;
    const double uy = D[1] + (D[3] * xs + D[2] * ys) - ys;
    tx = c * ux + s * uy;
    ty = c * uy - s * ux;
}

NDT_HD double ndt_calib_d2(double ax, double ay, double az, double bx, double by, double bz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ex = ax - bx, ey = ay - by, ez = az - bz;
    return (ex * ex + ey * ey) + ez * ez;
}

NDT_HD double ndt_calib_term(double m, double th2) { return m > th2 ? th2 : m; }

// ---- the winner: does (score, idx) beat (best, best_idx)? ---------------------------------------------------------------------------
NDT_HD bool ndt_calib_better(double score, uint32_t idx, double best, uint32_t best_idx)
{
    return score < best || (score == best && idx < best_idx);
}

// ---- chunks: the candidates whose (pair, candidate) sums the scratch holds at once, a multiple of the tile -----------------------
NDT_HD size_t ndt_calib_tiles(size_t n_candidates) { return (n_candidates + NDT_CALIB_TILE - 1) / NDT_CALIB_TILE; }
NDT_HD size_t ndt_calib_chunk(size_t pairs)
{
    const size_t per = NDT_CALIB_PARTIAL_DOUBLES / (pairs ? pairs : 1) / NDT_CALIB_TILE;
    return (per ? per : 1) * NDT_CALIB_TILE;
}
// ... of a handle made for (max_pairs, max_candidates): every call on it uses this chunk, so max_pairs x chunk doubles hold its sums
NDT_HD size_t ndt_calib_handle_chunk(size_t max_pairs, size_t max_candidates)
{
    const size_t chunk = ndt_calib_chunk(max_pairs), all = ndt_calib_tiles(max_candidates) * NDT_CALIB_TILE;
    return chunk < all ? chunk : all;
}

// ---- pair selection: the callback's anchor and gate walk (laser2d_extrinsic_calibration.cpp:312-349), host only -------------------
// |yaw| of D's rotation: the arc cosine of its cosine brought into [-1, 1] (getRobustYawFromAffine3d's form; the sign is not needed)
inline double ndt_calib_abs_yaw(double cd) { return std::acos(cd > 1.0 ? 1.0 : (cd < -1.0 ? -1.0 : cd)); }

// poses4: n poses (x, y, c, s).  Writes the first `room` pairs (anchor, current) into pairs2 (may be NULL) and returns their count.
inline size_t ndt_calib_select_pairs(const double *poses4, size_t n, double max_translation, double min_yaw, uint32_t *pairs2, size_t room)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    size_t anchor = 0, count = 0;
    for (size_t k = 1; k < n; k++) {
        double D[4];
        ndt_calib_pair_motion(poses4 + 4 * anchor, poses4 + 4 * k, D);
        if (std::sqrt(D[0] * D[0] + D[1] * D[1]) > max_translation) { anchor = k; continue; }
        if (ndt_calib_abs_yaw(D[2]) < min_yaw) continue;
        if (pairs2 && count < room) { pairs2[2 * count] = (uint32_t)anchor; pairs2[2 * count + 1] = (uint32_t)k; }
        count++;
        anchor = k;
    }
    return count;
}

// ---- checks: NULL: fine, else the message (it names the argument) ---------------------------------------------------------------
inline const char *ndt_calib_check_args(size_t n_scans, size_t n_points, size_t stride_bytes, size_t map_stride_bytes, size_t n_pairs,
                                        size_t nx, size_t ny, size_t nyaw)
{
    if (n_scans == 0 || n_scans > NDT_CALIB_MAX_SCANS) return "n_scans must be 1 .. 2^20";
    if (n_points == 0 || n_points > NDT_CALIB_MAX_POINTS) return "n_points must be 1 .. 2^16";
    if (stride_bytes < 12 || stride_bytes % 4 != 0 || stride_bytes > ((size_t)1 << 30)) return "stride_bytes must be 12 .. 2^30 and a multiple of 4";
    if (map_stride_bytes < n_points * stride_bytes || map_stride_bytes % 4 != 0)
        return "map_stride_bytes must be >= n_points * stride_bytes and a multiple of 4";
    if (n_pairs == 0 || n_pairs > NDT_CALIB_MAX_PAIRS) return "n_pairs must be 1 .. 1024";
    if (nx == 0 || nx > NDT_CALIB_MAX_CANDIDATES) return "nx must be 1 .. 2^24";
    if (ny == 0 || ny > NDT_CALIB_MAX_CANDIDATES) return "ny must be 1 .. 2^24";
    if (nyaw == 0 || nyaw > NDT_CALIB_MAX_CANDIDATES) return "nyaw must be 1 .. 2^24";
    if (nx * ny > NDT_CALIB_MAX_CANDIDATES || nx * ny * nyaw > NDT_CALIB_MAX_CANDIDATES) return "nx * ny * nyaw: more than 2^24 candidates";
    return nullptr;
}
inline const char *ndt_calib_check_params(const ndtgpu_calib_params &p)
{
    if (!(p.max_dist > 0.0 && p.max_dist < 1e150)) return "max_dist must be finite and > 0";
    return nullptr;
}
// (the lattice tables of a call: csrc/ndt_lattice.h)
inline const char *ndt_calib_check_capacity(size_t max_pairs, size_t max_points, size_t max_candidates)
{
    if (max_pairs == 0 || max_pairs > NDT_CALIB_MAX_PAIRS) return "max_pairs must be 1 .. 1024";
    if (max_points == 0 || max_points > NDT_CALIB_MAX_POINTS) return "max_points must be 1 .. 2^16";
    if (max_candidates == 0 || max_candidates > NDT_CALIB_MAX_CANDIDATES) return "max_candidates must be 1 .. 2^24";
    return nullptr;
}

#if defined(__HIPCC__)
// what a search reads and writes on the device (csrc/ndt_calib.hip)
struct NdtCalibArgs {
    const uint32_t *xyz;                          // the bank as 4-byte words
    const uint32_t *n_kept;                       // [n_scans]
    const double *poses;                          // [n_scans][4]
    const uint32_t *pairs;                        // [n_pairs][2]
    const double *xs, *ys, *cs, *sn;              // the lattice tables, device copies
    unsigned long long stride_words, map_stride_words;
    uint32_t n_scans, n_points, n_pairs, nx, ny, nyaw, n_candidates;
    uint32_t chunk;                               // candidates per chunk, a multiple of the tile
    double th2;
    // the handle's scratch
    double *a3, *b3;                              // [n_pairs][n_points][3] usable rows of cloud1; of cloud2, rotated
    double *motion;                               // [n_pairs][4]
    uint32_t *counts;                             // [n_pairs][4]: rows of a3, rows of b3, skipped rows, 1 where an index is out of range
    double *partial;                              // [n_pairs][chunk]
    double *tile_score;                           // [tiles]
    uint32_t *tile_index;                         // [tiles]
    // the results
    ndtgpu_calib_result *result;
    double *volume;                               // [n_candidates] or NULL
};
// host launcher: prepare, then per chunk of candidates score and finish, then the winner; plain launches on `st`
hipError_t ndt_calib_launch(const NdtCalibArgs &a, hipStream_t st);
#endif
