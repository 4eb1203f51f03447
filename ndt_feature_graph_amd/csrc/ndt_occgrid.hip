// ndt_occgrid.hip -- occupancy-grid export on CDNA4 (gfx950): maps of a set rasterised into int8 grids the way
// lslgeneric::toOccupancyGrid fills a nav_msgs::OccupancyGrid (include/ndtgpu.h "occupancy-grid export").
//
// Replaces (reference call sites): lslgeneric::toOccupancyGrid(map, omap, occ_map_resolution_, frame)
//   ndt_feature/src/ndt_feature2d_fuser.cpp:428-433, 450-454
//
// Design (DESIGN.md "Occupancy-grid export"):
//   * grid (tiles of 256 x 4 pixels in row-major order, map of the call).  One lane owns 4 pixels consecutive in x of one row and
//     writes them as one 32-bit store where the byte address is 4-aligned (a wave then writes 256 contiguous bytes per store
//     instruction), with byte stores otherwise: the tail of a row, the unaligned rows of a width that is no multiple of 4, a
//     map or a buffer whose first byte is not aligned.
//   * per pixel: LazyGrid::getIndexForPoint (lazygrid_index_half, fp64), one 8-byte rank-map word (ndt_rank_of), the occupancy
//     where the set has one, and only where a Gaussian is present the 80-byte NdtCell, the adjugate inverse, the quadratic form
//     and one exp.  Neighbouring lanes share their cell (~100 pixels per cell at 0.05 m in 0.5 m cells): the cell reads come out
//     of the cache.  No LDS staging of per-cell inverses (DESIGN.md records why).
//   * plain launches in stream order: no atomics, no barriers, nothing shared between lanes.  A pixel is a function of its map
//     and the call's numbers only, so a map's bytes are the same in any batch and on any call.
#include "ndt_occgrid.h"
#include <algorithm>

#define NDT_OCCGRID_THREADS 256

extern "C" __global__ __launch_bounds__(NDT_OCCGRID_THREADS) void ndt_occgrid_kernel(NdtSetView set, unsigned first, unsigned map0,
                                                                                      NdtOccGridCall call, int quads_per_row,
                                                                                      int8_t *__restrict__ out)
{
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * NDT_OCCGRID_THREADS + threadIdx.x;       // the lane's quad of pixels
    if (q >= (long long)quads_per_row * call.height) return;
    const int j = (int)(q / quads_per_row), i0 = (int)(q - (long long)j * quads_per_row) * 4;
    const unsigned local = map0 + blockIdx.y, map = first + local;
    const NdtGrid g = set.grid;
    const double cx = set.centres[map * 3 + 0], cy = set.centres[map * 3 + 1], cz = set.centres[map * 3 + 2];
    const double ox = ndt_occgrid_origin(cx, g.size[0], g.res), oy = ndt_occgrid_origin(cy, g.size[1], g.res);
    const NdtMapCounters *ctr = set.counters + map;
    // (a map whose build overflowed has ranks beyond its cell array: nothing of it is read, its whole grid is unknown)
    const bool usable = ctr->overflow == 0u;
    const unsigned n_cells = min(ctr->n_cells, g.max_cells);
    const uint2 *rankmap = set.rankmap + (size_t)map * ndt_rm_stride(g);
    const NdtCell *cells = ndt_cells_of(set, map, set.cell_sel ? set.cell_sel[map] : 0u);
    const float *occ = set.occ ? set.occ + (size_t)map * g.slots : nullptr;

    double p[3];
    p[1] = ndt_occgrid_pixel(oy, j, call.r);
    p[2] = call.z;
    const int iy = lazygrid_index_half(p[1], cy, g.res, g.half[1]), iz = lazygrid_index_half(p[2], cz, g.res, g.half[2]);
    const bool row_inside = usable && (unsigned)iy < (unsigned)g.size[1] && (unsigned)iz < (unsigned)g.size[2];
    int val[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = i0 + k;
        int v = -1;
        p[0] = ndt_occgrid_pixel(ox, i, call.r);
        const int ix = lazygrid_index_half(p[0], cx, g.res, g.half[0]);
        if (row_inside && i < call.width && (unsigned)ix < (unsigned)g.size[0]) {
            const unsigned slot = ((unsigned)ix * (unsigned)g.size[1] + (unsigned)iy) * (unsigned)g.size[2] + (unsigned)iz;
            int rank = ndt_rank_of(rankmap, slot);
            if ((unsigned)rank >= n_cells) rank = -1;
            const float o = occ ? occ[slot] : (rank >= 0 ? 1.0f : 0.0f);
            if (o < 0.0f) v = 0;
            else if (o > 0.0f) {
                if (rank >= 0) {
                    const NdtCell c = cells[rank];
                    v = ndt_occgrid_gaussian_value(p, c.mean, c.cov);
                } else {
                    v = call.occupied_no_gaussian;
                }
            }
        }
        val[k] = v;
    }
    int8_t *dst = out + (size_t)local * ((size_t)call.width * (size_t)call.height) + (size_t)j * (size_t)call.width + (size_t)i0;
    if (i0 + 3 < call.width && ((uintptr_t)dst & 3u) == 0u) {
        *reinterpret_cast<uint32_t *>(dst) = ((uint32_t)val[0] & 0xFFu) | (((uint32_t)val[1] & 0xFFu) << 8) | (((uint32_t)val[2] & 0xFFu) << 16) |
                                             (((uint32_t)val[3] & 0xFFu) << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + k < call.width) dst[k] = (int8_t)val[k];
    }
}

hipError_t ndt_launch_occgrid(const NdtSetView &set, size_t first, size_t count, const NdtOccGridCall &call, int8_t *out_dev,
                              hipStream_t stream)
{
    if (count == 0 || call.width <= 0 || call.height <= 0) return hipSuccess;
    const int quads_per_row = (call.width + 3) / 4;
    const long long quads = (long long)quads_per_row * call.height;
    const unsigned blocks = (unsigned)((quads + NDT_OCCGRID_THREADS - 1) / NDT_OCCGRID_THREADS);     // (the C-ABI bounds a call's pixels by 2^40)
    for (size_t m0 = 0; m0 < count; m0 += 65535u) {
        const unsigned ny = (unsigned)std::min<size_t>(65535u, count - m0);
        hipLaunchKernelGGL(ndt_occgrid_kernel, dim3(blocks, ny), dim3(NDT_OCCGRID_THREADS), 0, stream, set, (unsigned)first, (unsigned)m0,
                           call, quads_per_row, out_dev);
    }
    return hipGetLastError();
}
