// ndt_scansim.hip -- scan simulation in occupancy grids on CDNA4 (gfx950): the ranges a laser at a pose would measure in a grid, and
// the lattice of reference poses over a grid's free cells (include/ndtgpu.h "scan simulation").
//
// Replaces (reference, flirtlib_ros): occupancy_grid_utils::simulateRangeScan as place_rec_test.cpp:242 and simulate_scans.cpp:131
// call it, and the three loops of generateRefScans (place_rec_test.cpp:218-237).
//
// Design.  Everything behind the two cells of a ray is integer; the order of the fp64 operations that lead to them is
// in csrc/ndt_scansim.h.  Plain launches in stream order, no atomics, no workgroup waits on another:
//   cast      ndt_scansim_cast_kernel, ONE WORKGROUP of 256 lanes per pose, a lane per beam, tiles of 256 beams in turn.  All lanes
//             walk step k together (ndt_scansim_walk): neighbouring beams of one pose load neighbouring bytes in the same iteration,
//             and a wave leaves the loop once its last lane has stopped.  Plain byte loads through L2: poses arrive in lattice order,
//             so neighbouring workgroups walk the same pixels.  n_hits by one ndt_block_count behind the last tile.
//   lattice   the ordered selection of the link gate (ndt_linkgate.hip), three launches: ndt_scansim_flag_kernel, a lane per
//             position, leaves the kept positions of each tile of 256; ndt_scansim_scan_kernel, one workgroup, turns the counts into
//             the kept before each tile and writes count[2]; ndt_scansim_emit_kernel tests the positions again, ranks the kept ones by
//             ndt_block_rank and writes nyaw poses a position, in loop order, up to the capacity.
// A scan depends on its own pose and grid alone: the same bytes in any batch, at any row, on any run.
#include "ndt_scansim.h"
#include "ndt_block.h"

// poses [pose0, pose0 + gridDim.x) of the call
extern "C" __global__ __launch_bounds__(NDT_SCANSIM_THREADS) void ndt_scansim_cast_kernel(NdtScansimMap m, NdtScansimCast cp, const double *poses,
                                                                                         const uint32_t *grid_idx, uint32_t pose0,
                                                                                         const uint32_t *count, double *ranges,
                                                                                         ndtgpu_scansim_result *results)
{
    __shared__ NdtBlockCounts<NDT_SCANSIM_WAVES> cnt;
    int par = 0;
    const uint32_t row = pose0 + blockIdx.x;
    double *out = ranges + (size_t)row * m.n_beams;
    uint32_t flags = 0, grid = 0;
    int32_t i0 = 0, j0 = 0;
    double x = 0.0, y = 0.0, c = 1.0, s = 0.0, ox = 0.0, oy = 0.0;
    // (the flags are the same in every thread of the workgroup: so is the barrier below)
    if (count && row >= count[0]) {
        flags = NDTGPU_SCANSIM_NO_POSE;
    } else {
        grid = grid_idx ? grid_idx[row] : 0u;
        if (grid >= m.n_grids) {
            flags = NDTGPU_SCANSIM_BAD_INDEX;
        } else {
            x = poses[4 * (size_t)row];
            y = poses[4 * (size_t)row + 1];
            c = poses[4 * (size_t)row + 2];
            s = poses[4 * (size_t)row + 3];
            ox = m.origin[2 * grid];
            oy = m.origin[2 * grid + 1];
            if (!ndt_scansim_point_cell(x, y, ox, oy, m.resolution, m.width, m.height, i0, j0)) flags = NDTGPU_SCANSIM_OFFMAP;
        }
    }
    unsigned hits = 0;
    if (flags) {
        for (uint32_t b = threadIdx.x; b < m.n_beams; b += NDT_SCANSIM_THREADS) out[b] = cp.miss;
    } else {
        const int8_t *g = m.grids + (size_t)grid * m.width * m.height;
        for (uint32_t b = threadIdx.x; b < m.n_beams; b += NDT_SCANSIM_THREADS) {
            NdtScansimRay ray;
            uint32_t d2 = 0;
            // (at most R + 2 steps a beam: csrc/ndt_scansim.h)
            const bool hit = ndt_scansim_beam_ray(x, y, c, s, m.beams[2 * b], m.beams[2 * b + 1], cp.range_max, ox, oy, m.resolution, i0, j0, ray) &&
                             ndt_scansim_walk(g, m.width, m.height, i0, j0, ray, cp.R, cp.occupied_min, cp.unknown_is_obstacle, d2);
            out[b] = hit ? ndt_scansim_metres(d2, m.resolution) : cp.miss;
            hits += hit ? 1u : 0u;
        }
    }
    if (!results) return;
    const unsigned n_hits = ndt_block_count(hits, cnt, par);
    if (threadIdx.x == 0) {
        results[row].n_hits = n_hits;
        results[row].flags = flags;
    }
}

// position `pos` of the lattice: kept, and its centre
NDT_D bool ndt_scansim_flag(const NdtScansimMap &m, const NdtScansimLattice &l, unsigned long long pos, double &cx, double &cy)
{
    if (pos >= (unsigned long long)l.npx * l.npy) return false;
    const uint32_t px = (uint32_t)(pos / l.npy), py = (uint32_t)(pos - (unsigned long long)px * l.npy);
    return ndt_scansim_position(m.grids + (size_t)l.grid * m.width * m.height, m.width, px, py, l.skip, m.origin[2 * l.grid],
                                m.origin[2 * l.grid + 1], m.resolution, l.box4, cx, cy);
}

extern "C" __global__ __launch_bounds__(NDT_SCANSIM_THREADS) void ndt_scansim_flag_kernel(NdtScansimMap m, NdtScansimLattice l)
{
    __shared__ NdtBlockCounts<NDT_SCANSIM_WAVES> cnt;
    int par = 0;
    double cx, cy;
    const bool keep = ndt_scansim_flag(m, l, (unsigned long long)blockIdx.x * NDT_SCANSIM_TILE + threadIdx.x, cx, cy);
    const unsigned n = ndt_block_count(keep ? 1u : 0u, cnt, par);
    if (threadIdx.x == 0) l.tile[blockIdx.x] = n;
}

// tile[t] <- the sum of tile[0 .. t); count[1] <- the poses that passed, count[0] <- those written: one workgroup, chunks of 256
// tiles with a running carry
extern "C" __global__ __launch_bounds__(NDT_SCANSIM_THREADS) void ndt_scansim_scan_kernel(NdtScansimLattice l, unsigned n_tiles)
{
    __shared__ NdtBlockCounts<NDT_SCANSIM_WAVES> cnt;
    int par = 0;
    unsigned carry = 0;
    for (unsigned at = 0; at < n_tiles; at += NDT_SCANSIM_THREADS) {
        const unsigned t = at + threadIdx.x;
        const unsigned c = t < n_tiles ? l.tile[t] : 0u;
        unsigned all;
        const unsigned below = ndt_block_scan(c, cnt, par, all);
        if (t < n_tiles) l.tile[t] = carry + below;
        carry += all;
    }
    if (threadIdx.x == 0) {
        const unsigned long long passed = (unsigned long long)carry * l.nyaw;
        l.count[1] = (uint32_t)passed;
        l.count[0] = (uint32_t)(passed < l.capacity ? passed : l.capacity);
    }
}

extern "C" __global__ __launch_bounds__(NDT_SCANSIM_THREADS) void ndt_scansim_emit_kernel(NdtScansimMap m, NdtScansimLattice l)
{
    __shared__ NdtBlockCounts<NDT_SCANSIM_WAVES> cnt;
    int par = 0;
    const unsigned long long pos = (unsigned long long)blockIdx.x * NDT_SCANSIM_TILE + threadIdx.x;
    double cx = 0.0, cy = 0.0;
    const bool keep = ndt_scansim_flag(m, l, pos, cx, cy);
    unsigned run;
    const unsigned long long rank = (unsigned long long)l.tile[blockIdx.x] + ndt_block_rank(keep, cnt, par, run);
    if (!keep) return;
    for (uint32_t t = 0; t < l.nyaw; t++) {
        const unsigned long long row = rank * l.nyaw + t;
        if (row >= l.capacity) return;
        double *p = l.poses + 4 * row;
        p[0] = cx;
        p[1] = cy;
        p[2] = l.cs[t];
        p[3] = l.sn[t];
        if (l.index) l.index[row] = (uint32_t)(pos * l.nyaw + t);
    }
}

hipError_t ndt_scansim_cast_launch(const NdtScansimMap &m, const NdtScansimCast &c, const double *poses, const uint32_t *grid_idx, uint32_t n_poses,
                                   const uint32_t *count, double *ranges, ndtgpu_scansim_result *results, hipStream_t st)
{
    for (uint32_t first = 0; first < n_poses; first += NDT_SCANSIM_LAUNCH_POSES) {
        const uint32_t n = n_poses - first < NDT_SCANSIM_LAUNCH_POSES ? n_poses - first : NDT_SCANSIM_LAUNCH_POSES;
        hipLaunchKernelGGL(ndt_scansim_cast_kernel, dim3(n), dim3(NDT_SCANSIM_THREADS), 0, st, m, c, poses, grid_idx, first, count, ranges, results);
    }
    return hipGetLastError();
}

hipError_t ndt_scansim_lattice_launch(const NdtScansimMap &m, const NdtScansimLattice &l, hipStream_t st)
{
    const unsigned n_tiles = (unsigned)ndt_scansim_tiles((size_t)l.npx * l.npy);
    const dim3 threads(NDT_SCANSIM_THREADS);
    hipLaunchKernelGGL(ndt_scansim_flag_kernel, dim3(n_tiles), threads, 0, st, m, l);
    hipLaunchKernelGGL(ndt_scansim_scan_kernel, dim3(1), threads, 0, st, l, n_tiles);
    hipLaunchKernelGGL(ndt_scansim_emit_kernel, dim3(n_tiles), threads, 0, st, m, l);
    return hipGetLastError();
}
