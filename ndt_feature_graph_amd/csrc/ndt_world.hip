// ndt_world.hip -- world-map assembly on CDNA4 (gfx950): the Gaussian cells of many node maps, moved by their nodes' graph
// poses, are merged into the cells of one destination map per world (include/ndtgpu.h "world-map assembly").
//
// Replaces (reference call sites): NDTMap::pseudoTransformNDTMap + the empty NDTFeatureGraph::fuse()
//   ndt_feature/include/ndt_feature/ndt_feature_graph.h:149-152, ndt_feature/src/ndt_feature2d_fuser.cpp:425-432, :471,
//   ndt_feature/src/ndt_feature_graph_opt.cpp:178-185
//
// Design (DESIGN.md "World-map assembly"):
//   * a contribution (mu', Sigma', n) to a world cell is, in the cell's own units u = (mu' - cell origin) / res, the virtual
//     point set with  sum u = n u  and  sum u u^T = (n - 1) Sigma' / res^2 + n u u^T.  ndt_world_scatter_kernel writes exactly
//     these sums into the destination map's BUILD SCRATCH in the build's own format (NdtAcc 64-bit fixed point, each partial
//     rounded once with ndt_fixed_from_double and added with integer atomics; work table / bitmap / acc_slot / n_alloc
//     allocated like phase A of ndt_build_kernel).  The unmodified finaliser of csrc/ndt_build.hip (ndt_launch_finalise)
//     then turns them into pooled mean / sample covariance, rescales, ranks and cleans the scratch.
//   * integer sums are associative: a world's cells do not depend on the order of its nodes, of the workgroups or of the
//     atomics.  The shifts are a function of the world's own nodes (ndt_world_count_kernel: sum of the listed cells' n).
//   * one lane per source cell, grid (chunks of a node's cells, listed node).  A wave stages its 64 records in LDS and adds
//     them as (record, word) items: 80 contiguous bytes per record and atomic instruction, not one lane per record.
//   * plain launches in stream order: no grid barrier, no spin, no persistent kernel.
#include "ndt_math.h"
#include "ndt_binning.h"
#include "ndt_world.h"
#include <algorithm>

#define NDT_WORLD_THREADS 256
#define NDT_WORLD_EMPTY (-1)

namespace {

// a source cell's point count as the merge sees it: a Gaussian stands for at least two points (ndtgpu_mapset_set_cells
// installs n = 1)
NDT_D unsigned world_n(unsigned n) { return n < 2u ? 2u : n; }

// slot -> accumulator id of the destination map, allocating on first touch: phase A of ndt_build_kernel (get_or_assign)
// without its per-wave cache.  A racing loser wastes one id (left with n == 0, skipped by the finaliser).
NDT_D int world_get_or_assign(int32_t *wtable, uint32_t *bitmap, uint32_t *acc_slot, NdtMapCounters *ctr, uint32_t cap, int slot)
{
    int id = __hip_atomic_load(&wtable[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (id != NDT_WORLD_EMPTY) return id;
    int expected = NDT_WORLD_EMPTY;
    const unsigned nid = __hip_atomic_fetch_add(&ctr->n_alloc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_compare_exchange_strong(&wtable[slot], &expected, (int)nid, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_fetch_or(&bitmap[slot >> 5], 1u << (slot & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nid < cap) acc_slot[nid] = (uint32_t)slot;
        else __hip_atomic_store(&ctr->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (int)nid;
    }
    return expected;   // somebody else assigned it first
}

}  // namespace

// First pass: the bound of a world's largest per-cell N -- the sum of n over ALL cells of its listed nodes (n < 2 counts as
// 2), dropped and rejected ones included: an integer sum, the same whatever the order.
extern "C" __global__ __launch_bounds__(NDT_WORLD_THREADS) void ndt_world_count_kernel(NdtSetView src, const NdtWorldItem *__restrict__ items,
                                                                                        NdtWorldStats *stats, unsigned item0)
{
    const NdtWorldItem *it = items + item0 + blockIdx.y;
    const unsigned n_cells = it->n_cells, i = blockIdx.x * NDT_WORLD_THREADS + threadIdx.x;
    if (blockIdx.x * NDT_WORLD_THREADS >= n_cells) return;
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    const NdtCell *cells = ndt_cells_of(src, it->src_map, src.cell_sel ? src.cell_sel[it->src_map] : 0u);
    if (i < n_cells) atomicAdd(&s_sum, (unsigned long long)world_n(cells[i].n));
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[it->world].n_bound), s_sum);
}

// Second pass: every listed cell -> one record of the destination map's build scratch.
extern "C" __global__ __launch_bounds__(NDT_WORLD_THREADS) void ndt_world_scatter_kernel(NdtSetView dst, NdtSetView src,
                                                                                          const NdtWorldItem *__restrict__ items,
                                                                                          NdtWorldStats *stats, unsigned item0)
{
#pragma clang fp contract(off)
    const NdtWorldItem *it = items + item0 + blockIdx.y;
    const unsigned n_cells = it->n_cells, tid = threadIdx.x, i = blockIdx.x * NDT_WORLD_THREADS + tid;
    if (blockIdx.x * NDT_WORLD_THREADS >= n_cells) return;            // (the whole workgroup)
    __shared__ long long s_rec[NDT_WORLD_THREADS * 10];
    __shared__ int s_id[NDT_WORLD_THREADS];
    __shared__ unsigned s_dropped, s_rejected;
    __shared__ unsigned long long s_points;
    if (tid == 0) { s_dropped = 0u; s_rejected = 0u; s_points = 0ull; }
    __syncthreads();
    const unsigned lane = tid & 63u, wave = tid >> 6;
    const unsigned map = it->dst_map, world = it->world;
    const NdtGrid g = dst.grid;
    const uint32_t cap = g.max_cells;
    const int s1_shift = stats[world].s1_shift, s2_shift = stats[world].s2_shift;
    const double res = g.res, inv_res = 1.0 / g.res;
    const double q1 = ldexp(1.0, s1_shift), q2 = ldexp(1.0, s2_shift);
    const bool odd = ((g.size[0] | g.size[1] | g.size[2]) & 1) != 0;
    // what ndt_build_shifts leaves room for: |u| <= 1/2 and a second moment of one cell^2 per point on even grids, |u| < 2 and
    // sixteen on odd ones; n u_k^2 takes 1/4 (4) of it, (n - 1) |Sigma'_kl| / res^2 may take the rest
    const double u_max = odd ? 2.0 : 0.5 + 1e-9, cov_room = odd ? 12.0 : 0.75;
    int id = -1;
    long long rec[10];
#pragma unroll
    for (int k = 0; k < 10; k++) rec[k] = 0;
    if (i < n_cells) {
        const NdtCell c = ndt_cells_of(src, it->src_map, src.cell_sel ? src.cell_sel[it->src_map] : 0u)[i];
        const double *R = it->R, *t = it->t;                         // R row-major
        const double n = (double)world_n(c.n);
        double m[3];
#pragma unroll
        for (int r = 0; r < 3; r++) m[r] = R[3 * r] * c.mean[0] + R[3 * r + 1] * c.mean[1] + R[3 * r + 2] * c.mean[2] + t[r];
        // Sigma' = R Sigma R^T (pseudoTransformNDT)
        const double S[3][3] = {{c.cov[0], c.cov[1], c.cov[2]}, {c.cov[1], c.cov[3], c.cov[4]}, {c.cov[2], c.cov[4], c.cov[5]}};
        double RS[3][3], P[6];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) RS[r][q] = R[3 * r] * S[0][q] + R[3 * r + 1] * S[1][q] + R[3 * r + 2] * S[2][q];
        {
            int k = 0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int q = r; q < 3; q++) P[k++] = RS[r][0] * R[3 * q] + RS[r][1] * R[3 * q + 1] + RS[r][2] * R[3 * q + 2];
        }
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; k++) finite = finite && isfinite(m[k]);
#pragma unroll
        for (int k = 0; k < 6; k++) finite = finite && isfinite(P[k]);
        const double cx = dst.centres[map * 3 + 0], cy = dst.centres[map * 3 + 1], cz = dst.centres[map * 3 + 2];
        // LazyGrid::getIndexForPoint(mu') of the destination grid
        const int ix = lazygrid_index_half(m[0], cx, res, g.half[0]), iy = lazygrid_index_half(m[1], cy, res, g.half[1]),
                  iz = lazygrid_index_half(m[2], cz, res, g.half[2]);
        const bool inside = (unsigned)ix < (unsigned)g.size[0] && (unsigned)iy < (unsigned)g.size[1] && (unsigned)iz < (unsigned)g.size[2];
        if (!finite) {
            atomicAdd(&s_rejected, 1u);
        } else if (!inside) {
            atomicAdd(&s_dropped, 1u);
        } else {
            // offset from the cell's origin as the finaliser defines it: centre + (index - size / 2) res
            const double u[3] = {(m[0] - (cx + (ix - g.half[0]) * res)) * inv_res, (m[1] - (cy + (iy - g.half[1]) * res)) * inv_res,
                                 (m[2] - (cz + (iz - g.half[2]) * res)) * inv_res};
            const double w = (n - 1.0) * inv_res * inv_res;
            bool fits = fabs(u[0]) <= u_max && fabs(u[1]) <= u_max && fabs(u[2]) <= u_max;
#pragma unroll
            for (int k = 0; k < 6; k++) fits = fits && w * fabs(P[k]) <= cov_room * n;
            if (!fits) {
                atomicAdd(&s_rejected, 1u);
            } else {
                const int slot = (int)(((unsigned)ix * (unsigned)g.size[1] + (unsigned)iy) * (unsigned)g.size[2] + (unsigned)iz);
                const int a = world_get_or_assign(dst.wtable + (size_t)map * g.slots, dst.bitmap + (size_t)map * ((g.slots + 31) >> 5),
                                                  dst.acc_slot + (size_t)map * cap, dst.counters + map, cap, slot);
                if (a >= 0 && (uint32_t)a < cap) {                 // (past the capacity: the map overflows, like a build)
                    id = a;
                    rec[0] = (long long)world_n(c.n);
#pragma unroll
                    for (int k = 0; k < 3; k++) rec[1 + k] = ndt_fixed_from_double(n * u[k] * q1);
                    rec[4] = ndt_fixed_from_double((w * P[0] + n * u[0] * u[0]) * q2);
                    rec[5] = ndt_fixed_from_double((w * P[1] + n * u[0] * u[1]) * q2);
                    rec[6] = ndt_fixed_from_double((w * P[2] + n * u[0] * u[2]) * q2);
                    rec[7] = ndt_fixed_from_double((w * P[3] + n * u[1] * u[1]) * q2);
                    rec[8] = ndt_fixed_from_double((w * P[4] + n * u[1] * u[2]) * q2);
                    rec[9] = ndt_fixed_from_double((w * P[5] + n * u[2] * u[2]) * q2);
                    atomicAdd(&s_points, (unsigned long long)world_n(c.n));
                }
            }
        }
    }
    // the wave's 64 records, then 640 (record, word) items: consecutive lanes add consecutive words of a record
    long long *wrec = s_rec + wave * 640u;
    int *wid = s_id + wave * 64u;
    wid[lane] = id;
#pragma unroll
    for (int k = 0; k < 10; k++) wrec[lane * 10u + k] = rec[k];
    ndt_wave_sync();
    NdtAcc *acc = dst.acc + (size_t)map * cap;
    for (unsigned item = lane; item < 640u; item += 64u) {
        const unsigned e = item / 10u, k = item - 10u * e;
        const int a = wid[e];
        const long long v = wrec[item];
        if (a >= 0 && v != 0)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(acc + a) + k, (unsigned long long)v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid == 0) {
        NdtWorldStats *s = stats + world;
        if (s_dropped) atomicAdd(reinterpret_cast<unsigned long long *>(&s->n_dropped), (unsigned long long)s_dropped);
        if (s_rejected) atomicAdd(reinterpret_cast<unsigned long long *>(&s->n_rejected), (unsigned long long)s_rejected);
        if (s_points) atomicAdd(reinterpret_cast<unsigned long long *>(&s->n_points), s_points);
    }
}

// After the finaliser: the end-of-chain saturation of the stored n (mean and covariance do not change with it), the
// occupancy limit where it is below the build's 255, and the map's n_dropped counter (the finaliser derives it from a point
// count, which an assembly does not have).
extern "C" __global__ __launch_bounds__(NDT_WORLD_THREADS) void ndt_world_finish_kernel(NdtSetView dst, unsigned first,
                                                                                         const NdtWorldStats *__restrict__ stats,
                                                                                         double maxnumpoints, double occupancy_limit)
{
    const unsigned map = first + blockIdx.y, tid = blockIdx.x * NDT_WORLD_THREADS + threadIdx.x, step = gridDim.x * NDT_WORLD_THREADS;
    const NdtGrid g = dst.grid;
    NdtMapCounters *ctr = dst.counters + map;
    unsigned n_cells = ctr->n_cells;
    if (n_cells > g.max_cells) n_cells = g.max_cells;
    NdtCell *cells = dst.cells + (size_t)map * g.max_cells;            // (a finalised map lives in the first cell array)
    if (maxnumpoints > 0.0) {
        const uint32_t lim = maxnumpoints >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)maxnumpoints;
        for (unsigned i = tid; i < n_cells; i += step)
            if (cells[i].n > lim) cells[i].n = lim;
    }
    if (dst.occ && occupancy_limit < 255.0) {
        const float lim = (float)occupancy_limit;
        float *occ = dst.occ + (size_t)map * g.slots;
        for (unsigned s = tid; s < (unsigned)g.slots; s += step)
            if (occ[s] > lim) occ[s] = lim;
    }
    if (tid == 0) {
        const long long lost = stats[blockIdx.y].n_dropped + stats[blockIdx.y].n_rejected;
        ctr->n_dropped = lost > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)lost;
    }
}

hipError_t ndt_launch_world_count(const NdtSetView &src, const NdtWorldItem *items_dev, size_t n_items, unsigned max_item_cells,
                                  NdtWorldStats *stats_dev, hipStream_t stream)
{
    const unsigned chunks = (max_item_cells + NDT_WORLD_THREADS - 1) / NDT_WORLD_THREADS;
    for (size_t i0 = 0; chunks && i0 < n_items; i0 += 65535u) {
        const unsigned ny = (unsigned)std::min<size_t>(65535u, n_items - i0);
        hipLaunchKernelGGL(ndt_world_count_kernel, dim3(chunks, ny), dim3(NDT_WORLD_THREADS), 0, stream, src, items_dev, stats_dev,
                           (unsigned)i0);
    }
    return hipGetLastError();
}

hipError_t ndt_launch_world_scatter(const NdtSetView &dst, const NdtSetView &src, const NdtWorldItem *items_dev, size_t n_items,
                                    unsigned max_item_cells, NdtWorldStats *stats_dev, hipStream_t stream)
{
    const unsigned chunks = (max_item_cells + NDT_WORLD_THREADS - 1) / NDT_WORLD_THREADS;
    for (size_t i0 = 0; chunks && i0 < n_items; i0 += 65535u) {
        const unsigned ny = (unsigned)std::min<size_t>(65535u, n_items - i0);
        hipLaunchKernelGGL(ndt_world_scatter_kernel, dim3(chunks, ny), dim3(NDT_WORLD_THREADS), 0, stream, dst, src, items_dev,
                           stats_dev, (unsigned)i0);
    }
    return hipGetLastError();
}

hipError_t ndt_launch_world_finish(const NdtSetView &dst, size_t first, size_t count, const NdtWorldStats *stats_dev,
                                   double maxnumpoints, double occupancy_limit, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    const bool occ_pass = dst.occ && occupancy_limit < 255.0;
    const unsigned work = occ_pass ? (unsigned)dst.grid.slots : dst.grid.max_cells;
    unsigned blocks = (work + NDT_WORLD_THREADS * 8u - 1) / (NDT_WORLD_THREADS * 8u);
    blocks = std::max(1u, std::min(blocks, 64u));
    hipLaunchKernelGGL(ndt_world_finish_kernel, dim3(blocks, (unsigned)count), dim3(NDT_WORLD_THREADS), 0, stream, dst, (unsigned)first,
                       stats_dev, maxnumpoints, occupancy_limit);
    return hipGetLastError();
}
