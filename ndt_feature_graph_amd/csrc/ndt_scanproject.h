// ndt_scanproject.h -- what the laser-scan projection's kernels (csrc/ndt_scanproject.hip), its C-ABI (csrc/ndtgpu_scanproject.hip)
// and host programs share (include/ndtgpu.h "laser-scan projection"): the gate and the point of one beam, the checks of a call's
// arguments and parameters, and the tile arithmetic of the launches.  Plain C++ for host and device: NDT_HD is
// __host__ __device__ under hipcc and `inline` elsewhere, so tests/native/scanproject_checks.cpp compiles this file with g++ alone
// (under the address and undefined-behaviour sanitizers).  The z draw (ndt_hash_uniform, csrc/ndt_mcl.h) needs the HIP headers,
// so the one function that makes it, ndt_scanproject_beam, is declared for HIP translation units only; the gate and the point
// take the draw as an argument.  tests/scanproject_model.py restates all of it in NumPy.
//
// THE ORDER OF OPERATIONS, part of the contract: every expression below is evaluated as written in fp64, NOT contracted (no fused
// multiply-add), and rounded to float once:
//   a = angle_min + (double)i * angle_increment          (the expression of ndt_featextract_kernel: one ranges buffer serves both)
//   x = (float)(r * cos(a)),  y = (float)(r * sin(a)),  z = (float)(varz * u)
#pragma once
#include "../../include/ndtgpu.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include "ndt_mcl.h"   // NDT_HD; ndt_hash_uniform: the counter-based uniform of the z jitter
#else
#define NDT_HD inline
#endif

#define NDT_SCANPROJECT_THREADS 256               // a workgroup of the count and emit passes
#define NDT_SCANPROJECT_WAVES (NDT_SCANPROJECT_THREADS / 64)
#define NDT_SCANPROJECT_SUBTILES 4                // ... works through this many runs of NDT_SCANPROJECT_THREADS consecutive beams
#define NDT_SCANPROJECT_TILE (NDT_SCANPROJECT_THREADS * NDT_SCANPROJECT_SUBTILES)      // T
#define NDT_SCANPROJECT_MAX_BEAMS (1u << 20)
#define NDT_SCANPROJECT_MAX_SCANS (1u << 24)
#define NDT_SCANPROJECT_MAX_GRID 0x7FFFFFFFull    // workgroups of one launch

// the parameters as the kernels take them
struct NdtScanProjectParamsDev {
    double r_min, r_max, varz;
    unsigned long long seed;
};

// ---- tile arithmetic ---------------------------------------------------------------------------------------------------------
// tiles of a scan of n_beams beams
NDT_HD uint32_t ndt_scanproject_tiles(size_t n_beams) { return (uint32_t)((n_beams + NDT_SCANPROJECT_TILE - 1) / NDT_SCANPROJECT_TILE); }
// the beams [begin, end) of tile t
NDT_HD void ndt_scanproject_tile_range(uint32_t t, size_t n_beams, uint32_t &begin, uint32_t &end)
{
    const size_t b = (size_t)t * NDT_SCANPROJECT_TILE;
    begin = (uint32_t)(b < n_beams ? b : n_beams);
    end = (uint32_t)(b + NDT_SCANPROJECT_TILE < n_beams ? b + NDT_SCANPROJECT_TILE : n_beams);
}
// The pad rows [begin, end) that tile t writes: the rows of its own beam range that lie at or beyond n_kept.  n_kept <= n_beams, so
// every pad row belongs to exactly one tile, and no pad row is a kept row of any tile.
NDT_HD void ndt_scanproject_pad_range(uint32_t t, size_t n_beams, uint32_t n_kept, uint32_t &begin, uint32_t &end)
{
    ndt_scanproject_tile_range(t, n_beams, begin, end);
    if (begin < n_kept) begin = n_kept < end ? n_kept : end;
}
// scans of one launch: the grid of a launch is (scans) x (tiles of a scan) workgroups, at most NDT_SCANPROJECT_MAX_GRID
NDT_HD size_t ndt_scanproject_scans_per_launch(size_t n_beams)
{
    return (size_t)(NDT_SCANPROJECT_MAX_GRID / ndt_scanproject_tiles(n_beams ? n_beams : 1));
}

// ---- the beam ----------------------------------------------------------------------------------------------------------------
// kept iff r is finite and r_min < r < r_max, both strict.  A NaN fails both comparisons, -inf the first (r_min >= 0), +inf the
// second also where r_max is +inf.
NDT_HD bool ndt_scanproject_kept(double r, double r_min, double r_max) { return r > r_min && r < r_max; }

// the point of kept beam i with range r and z draw u (see the head of this file)
NDT_HD void ndt_scanproject_point(double angle_min, double angle_increment, uint32_t i, double r, double varz, double u, float xyz[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = angle_min + (double)i * angle_increment;
    xyz[0] = (float)(r * cos(a));
    xyz[1] = (float)(r * sin(a));
    xyz[2] = (float)(varz * u);
}

#if defined(__HIPCC__)
// gate and point of beam i of scan scan_id: true and xyz written iff kept.  u is drawn by the BEAM index, not by the rank among
// the kept points: a beam's point does not depend on the other beams.
NDT_HD bool ndt_scanproject_beam(const NdtScanProjectParamsDev &prm, double angle_min, double angle_increment, unsigned long long scan_id,
                                 uint32_t i, double r, float xyz[3])
{
    if (!ndt_scanproject_kept(r, prm.r_min, prm.r_max)) return false;
    ndt_scanproject_point(angle_min, angle_increment, i, r, prm.varz, ndt_hash_uniform(prm.seed, scan_id, i), xyz);
    return true;
}
#endif

// ---- checks: NULL: fine, else the message (it names the argument) ---------------------------------------------------------------
inline const char *ndt_scanproject_check_args(size_t n_scans, size_t n_beams, double angle_min, double angle_increment, size_t stride_bytes,
                                              size_t map_stride_bytes)
{
    if (n_beams == 0 || n_beams > NDT_SCANPROJECT_MAX_BEAMS) return "n_beams must be 1 .. 2^20";
    if (n_scans > NDT_SCANPROJECT_MAX_SCANS) return "n_scans: more than 2^24 scans";
    if (!(std::fabs(angle_min) < 1e300) || !(std::fabs(angle_increment) < 1e300)) return "angle_min and angle_increment must be finite";
    if (stride_bytes < 12 || stride_bytes % 4 != 0 || stride_bytes > ((size_t)1 << 40))       // (n_beams * stride_bytes cannot wrap)
        return "stride_bytes must be 12 .. 2^40 and a multiple of 4";
    if (map_stride_bytes < n_beams * stride_bytes || map_stride_bytes % 4 != 0)
        return "map_stride_bytes must be >= n_beams * stride_bytes and a multiple of 4";
    return nullptr;
}
inline const char *ndt_scanproject_check_params(const ndtgpu_scanproject_params &p)
{
    if (!(p.r_min >= 0.0 && p.r_min < 1e300)) return "r_min must be finite and >= 0";
    if (!(p.r_max > p.r_min)) return "r_max must be > r_min (+inf allowed)";                       // (NaN fails)
    if (!(p.varz >= 0.0 && p.varz < 1e300)) return "varz must be finite and >= 0";
    return nullptr;
}
// what a handle made for (max_scans, max_beams) holds: one count per tile
inline const char *ndt_scanproject_check_capacity(size_t max_scans, size_t max_beams)
{
    if (max_scans == 0 || max_scans > NDT_SCANPROJECT_MAX_SCANS) return "max_scans must be 1 .. 2^24";
    if (max_beams == 0 || max_beams > NDT_SCANPROJECT_MAX_BEAMS) return "max_beams must be 1 .. 2^20";
    return nullptr;
}

inline NdtScanProjectParamsDev ndt_scanproject_params_dev(const ndtgpu_scanproject_params &p)
{
    NdtScanProjectParamsDev d;
    d.r_min = p.r_min;
    d.r_max = p.r_max;
    d.varz = p.varz;
    d.seed = p.seed;
    return d;
}

#if defined(__HIPCC__)
// host launcher (csrc/ndt_scanproject.hip): two launches on `st` per chunk of scans.  tile_dev: room for n_scans x tiles counts.
// scan_id_dev NULL: scan b has id b; n_kept_dev may be NULL.  stride_words / map_stride_words: the strides in 4-byte words.
hipError_t ndt_scanproject_launch(const double *ranges_dev, const unsigned long long *scan_id_dev, size_t n_scans, size_t n_beams,
                                  double angle_min, double angle_increment, const NdtScanProjectParamsDev &prm, uint32_t *tile_dev,
                                  uint32_t *xyz_dev, size_t stride_words, size_t map_stride_words, uint32_t *n_kept_dev, hipStream_t st);
#endif
