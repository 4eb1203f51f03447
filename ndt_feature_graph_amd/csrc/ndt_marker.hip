// ndt_marker.hip -- marker export on CDNA4 (gfx950): the axis segments of the Gaussian cells of maps under their poses, the segments
// of the links of a pose graph and of the particles of a filter bank, as the points of a LINE_LIST (include/ndtgpu.h "marker export").
//
// Replaces (reference): ndt_visualisation::markerNDTCells (ndt_rviz.h:1090-1153, 1163-1233; called from ndt_feature2d_fuser.cpp:425,
// 448, ndt_feature_fuser.cpp:253, ndt_feature_mcl_node.cpp:287), markerParticlesNDTMCL3D (ndt_rviz.h:1277-1297) and
// ndt_feature::markerNDTFeatureLinks (ndt_feature_rviz.h:282-313).
//
// Design.  The order of every fp64 operation is in csrc/ndt_marker.h.  Plain launches in stream order, no atomics, no
// workgroup waits on another:
//   cells      an ordered selection with 0 .. 3 items a lane, three launches.  ndt_marker_count_kernel, grid (tiles of 256 cells of a
//              map) x (maps of the call), a lane per cell: the 3 x 3 Jacobi of the cell's covariance in registers, the axes at or above
//              min_eval counted, the tile's sum by ndt_block_count.  ndt_marker_scan_kernel, one workgroup (a run of tiles a thread,
//              one block scan of the runs' sums), turns the tile words into the segments before each tile in (map, tile) order
//              and writes the count words.  ndt_marker_emit_kernel, the same lanes:
//              the eigen-pairs AGAIN by the same function (the count and the emit agree by construction; no 144-byte record per cell
//              travels through memory), ndt_block_scan of the lanes' counts plus the tile's base, the lane's segments contiguous from
//              there, up to the capacity.
//   links      the same three launches with a flag per lane and ndt_block_rank.
//   particles  one launch, a lane per particle, reading the filter bank's poses in place.
// A segment depends on its own cell and its map's pose alone, its row on the cells before it in the call: the same bytes in any batch,
// at any `first`, with any other maps in the call, on any run.
#include "ndt_marker.h"
#include "ndt_block.h"

#include <algorithm>

// the lane's cell: false where the lane has none.  A map whose build overflowed has ranks beyond its cell array: it is empty here.
NDT_D bool ndt_marker_lane_cell(const NdtSetView &set, uint32_t map, uint32_t rank, NdtCell &c)
{
    const NdtMapCounters *ctr = set.counters + map;
    const uint32_t n_cells = ctr->overflow ? 0u : min(ctr->n_cells, set.grid.max_cells);
    if (rank >= n_cells) return false;
    c = ndt_cells_of(set, map, set.cell_sel ? set.cell_sel[map] : 0u)[rank];
    return true;
}

// maps [map0, map0 + gridDim.y) of the call
extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_count_kernel(NdtSetView set, NdtMarkerCells mc, NdtMarkerSel sel,
                                                                                        uint32_t map0)
{
    __shared__ NdtBlockCounts<NDT_MARKER_WAVES> cnt;
    int par = 0;
    const uint32_t local = map0 + blockIdx.y, rank = blockIdx.x * NDT_MARKER_TILE + threadIdx.x;
    NdtCell c;
    uint32_t n = 0, flags = 0;
    if (ndt_marker_lane_cell(set, mc.first + local, rank, c)) n = ndt_marker_cell_count(c.cov, mc.min_eval, flags);
    const unsigned word = ndt_block_count(n | (flags ? 1u << 16 : 0u), cnt, par);
    if (threadIdx.x == 0) sel.tile[(size_t)local * mc.tiles_per_map + blockIdx.x] = word;
}

// tile[t] <- the segments of tiles [0, t); count <- {written, total, overflow, flags}: one workgroup.  A tile word is (items of the
// tile) | (its lanes that raised `flag`) << 16.  Thread i owns the run of tiles [i * per, (i + 1) * per): it adds its run up, ONE block
// scan orders the runs' sums, and it walks its run again writing the running sum -- two barriers whatever the number of tiles (a
// block scan per chunk of 256 tiles, the link gate's form, is 313 chunks for 5000 maps of 16 tiles).  Integer sums: the order is free.
extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_scan_kernel(NdtMarkerSel sel, unsigned n_tiles, uint32_t flag)
{
    __shared__ NdtBlockCounts<NDT_MARKER_WAVES> cnt;
    int par = 0;
    const unsigned per = (n_tiles + NDT_MARKER_THREADS - 1) / NDT_MARKER_THREADS;
    const unsigned begin = min(threadIdx.x * per, n_tiles), end = min(begin + per, n_tiles);
    unsigned sum = 0, raised = 0;
    for (unsigned t = begin; t < end; t++) {
        const unsigned w = sel.tile[t];
        sum += w & 0xFFFFu;
        raised += w >> 16;
    }
    unsigned all;
    unsigned run = ndt_block_scan(sum, cnt, par, all);
    raised = ndt_block_count(raised, cnt, par);
    for (unsigned t = begin; t < end; t++) {
        const unsigned w = sel.tile[t];
        sel.tile[t] = run;
        run += w & 0xFFFFu;
    }
    if (threadIdx.x == 0) {
        sel.count[0] = (uint32_t)((unsigned long long)all < sel.capacity ? all : sel.capacity);
        sel.count[1] = all;
        sel.count[2] = (unsigned long long)all > sel.capacity ? 1u : 0u;
        sel.count[3] = raised ? flag : 0u;
    }
}

extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_emit_kernel(NdtSetView set, NdtMarkerCells mc, NdtMarkerSel sel,
                                                                                       uint32_t map0)
{
    __shared__ NdtBlockCounts<NDT_MARKER_WAVES> cnt;
    int par = 0;
    const uint32_t local = map0 + blockIdx.y, map = mc.first + local, rank = blockIdx.x * NDT_MARKER_TILE + threadIdx.x;
    NdtCell c;
    double seg[3][2][3], evals[3], T12[12];
    uint32_t n = 0, flags = 0;
    if (ndt_marker_lane_cell(set, map, rank, c)) {
        if (mc.T16) ndt_marker_pose12(mc.T16 + 16 * (size_t)local, T12);
        n = ndt_marker_cell(c.mean, c.cov, mc.T16 != nullptr, T12, mc.min_eval, seg, flags, evals);
    }
    unsigned all;
    const unsigned long long row0 = (unsigned long long)sel.tile[(size_t)local * mc.tiles_per_map + blockIdx.x] + ndt_block_scan(n, cnt, par, all);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const unsigned long long row = row0 + k;
        if (k < n && row < sel.capacity) {
            double *p = mc.points + 6 * row;
#pragma unroll
            for (int e = 0; e < 3; e++) {
                p[e] = seg[k][0][e];
                p[3 + e] = seg[k][1][e];
            }
            if (mc.src) {
                mc.src[2 * row] = map;
                mc.src[2 * row + 1] = rank;
            }
        }
    }
}

// link `i`: kept, or raised as a bad index
NDT_D bool ndt_marker_lane_link(const NdtMarkerLinks &l, size_t i, bool &bad)
{
    bad = false;
    if (i >= l.n_links) return false;
    if (!ndt_marker_link_kept(l.score, i, l.skip_negative)) return false;
    bad = ndt_marker_link_bad(l.ref[i], l.mov[i], l.n_nodes);
    return !bad;
}

extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_link_flag_kernel(NdtMarkerLinks l, NdtMarkerSel sel)
{
    __shared__ NdtBlockCounts<NDT_MARKER_WAVES> cnt;
    int par = 0;
    bool bad;
    const bool keep = ndt_marker_lane_link(l, (size_t)blockIdx.x * NDT_MARKER_TILE + threadIdx.x, bad);
    const unsigned word = ndt_block_count((keep ? 1u : 0u) | (bad ? 1u << 16 : 0u), cnt, par);
    if (threadIdx.x == 0) sel.tile[blockIdx.x] = word;
}

extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_link_emit_kernel(NdtMarkerLinks l, NdtMarkerSel sel)
{
    __shared__ NdtBlockCounts<NDT_MARKER_WAVES> cnt;
    int par = 0;
    const size_t i = (size_t)blockIdx.x * NDT_MARKER_TILE + threadIdx.x;
    bool bad;
    const bool keep = ndt_marker_lane_link(l, i, bad);
    unsigned all;
    const unsigned long long row = (unsigned long long)sel.tile[blockIdx.x] + ndt_block_rank(keep, cnt, par, all);
    if (!keep || row >= sel.capacity) return;
    ndt_marker_link(l.T16_nodes, l.ref[i], l.mov[i], l.points + 6 * row);
}

extern "C" __global__ __launch_bounds__(NDT_MARKER_THREADS) void ndt_marker_particle_kernel(const double *T12, unsigned long long n, double length,
                                                                                           double *points)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * NDT_MARKER_TILE + threadIdx.x;
    if (i >= n) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = T12[12 * i + k];
    ndt_marker_particle(T, length, points + 6 * i);
}

hipError_t ndt_marker_cells_launch(const NdtSetView &set, const NdtMarkerCells &c, const NdtMarkerSel &sel, hipStream_t st)
{
    const dim3 threads(NDT_MARKER_THREADS);
    const unsigned n_tiles = c.count * c.tiles_per_map;
    for (uint32_t m0 = 0; m0 < c.count; m0 += 65535u)
        hipLaunchKernelGGL(ndt_marker_count_kernel, dim3(c.tiles_per_map, std::min(65535u, c.count - m0)), threads, 0, st, set, c, sel, m0);
    hipLaunchKernelGGL(ndt_marker_scan_kernel, dim3(1), threads, 0, st, sel, n_tiles, (uint32_t)NDTGPU_MARKER_NONFINITE);
    for (uint32_t m0 = 0; m0 < c.count; m0 += 65535u)
        hipLaunchKernelGGL(ndt_marker_emit_kernel, dim3(c.tiles_per_map, std::min(65535u, c.count - m0)), threads, 0, st, set, c, sel, m0);
    return hipGetLastError();
}

hipError_t ndt_marker_links_launch(const NdtMarkerLinks &l, const NdtMarkerSel &sel, hipStream_t st)
{
    const dim3 threads(NDT_MARKER_THREADS);
    const unsigned n_tiles = (unsigned)ndt_marker_tiles(l.n_links);
    if (n_tiles) hipLaunchKernelGGL(ndt_marker_link_flag_kernel, dim3(n_tiles), threads, 0, st, l, sel);
    hipLaunchKernelGGL(ndt_marker_scan_kernel, dim3(1), threads, 0, st, sel, n_tiles, (uint32_t)NDTGPU_MARKER_BAD_INDEX);
    if (n_tiles) hipLaunchKernelGGL(ndt_marker_link_emit_kernel, dim3(n_tiles), threads, 0, st, l, sel);
    return hipGetLastError();
}

hipError_t ndt_marker_particles_launch(const double *T12, size_t n, double length, double *points, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ndt_marker_particle_kernel, dim3((unsigned)ndt_marker_tiles(n)), dim3(NDT_MARKER_THREADS), 0, st, T12,
                       (unsigned long long)n, length, points);
    return hipGetLastError();
}
