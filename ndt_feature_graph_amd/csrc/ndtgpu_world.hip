// ndtgpu_world.hip -- C-ABI (include/ndtgpu.h) of the world-map assembly: the node maps of a pose graph, under the graph's
// poses, merged into one map per world (graph->getMap() moved by getT(), ndt_feature2d_fuser.cpp:425-432; the declared but empty
// NDTFeatureGraph::fuse(), ndt_feature_graph.h:149-152).  Host side only: the argument checks, the table of listed nodes, the
// shifts of every world and the order of the launches; the kernels are in csrc/ndt_world.hip, the finaliser in csrc/ndt_build.hip.
// No handle: the temporaries are locals of the owning types and are gone on return.
#include "ndtgpu_host.h"
#include "ndt_world.h"

extern "C" {

void ndtgpu_default_world_params(ndtgpu_world_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->maxnumpoints = 1e5;        // fuser_hmt.cpp:486
    p->eval_factor = 1000.0;      // NDTCell::rescaleCovariance's EVAL_FACTOR default, as ndtgpu_default_cell_params
    p->occupancy_limit = 255.0;
}

ndtgpu_status ndtgpu_world_check(size_t dst_n_maps, double dst_res, size_t dst_first, size_t count, size_t src_n_maps, double src_res,
                                 int same_set, const uint32_t *node_offsets, const uint32_t *node_idx)
{
    if (count == 0) return NDTGPU_OK;
    if (!node_offsets) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_offsets is required");
    for (size_t w = 0; w < count; w++)
        if (node_offsets[w + 1] < node_offsets[w]) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_offsets must be non-decreasing");
    const size_t n0 = node_offsets[0], n1 = node_offsets[count];
    if (n1 > n0 && !node_idx) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_idx is required");
    if (dst_first >= dst_n_maps || count > dst_n_maps - dst_first || count > 65535)
        return fail(NDTGPU_ERR_INVALID, "world_assemble: destination maps [dst_first, dst_first + count) out of range (count <= 65535)");
    for (size_t k = n0; k < n1; k++) {
        if (node_idx[k] >= src_n_maps) return fail(NDTGPU_ERR_INVALID, "world_assemble: node index out of range");
        if (same_set && node_idx[k] >= dst_first && node_idx[k] - dst_first < count)
            return fail(NDTGPU_ERR_INVALID, "world_assemble: a destination map is among the listed nodes");
    }
    if (!(dst_res >= src_res))
        return fail(NDTGPU_ERR_INVALID, "world_assemble: the destination res must not be smaller than the source res");
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_world_assemble(ndtgpu_mapset *dst, size_t dst_first, size_t count, ndtgpu_mapset *src,
                                    const uint32_t *node_offsets, const uint32_t *node_idx, const double *T16,
                                    const ndtgpu_world_params *prm, ndtgpu_world_result *results, ndtgpu_stream stream)
{
    if (!dst || !src) return fail(NDTGPU_ERR_INVALID, "world_assemble: null map set");
    if (count == 0) return NDTGPU_OK;
    // what can be checked without reading a handle comes first: a map set only exists where a device does
    if (!node_offsets) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_offsets is required");
    for (size_t w = 0; w < count; w++)
        if (node_offsets[w + 1] < node_offsets[w]) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_offsets must be non-decreasing");
    const size_t n0 = node_offsets[0], n_items = node_offsets[count] - n0;
    if (n_items && (!node_idx || !T16)) return fail(NDTGPU_ERR_INVALID, "world_assemble: node_idx and T16 are required");
    if (dst == src)
        for (size_t k = n0; k < n0 + n_items; k++)
            if (node_idx[k] >= dst_first && node_idx[k] - dst_first < count)
                return fail(NDTGPU_ERR_INVALID, "world_assemble: a destination map is among the listed nodes");
    const ndtgpu_world_params p = params_or_default(prm, ndtgpu_default_world_params);
    if (!(p.eval_factor > 0.0) || !std::isfinite(p.eval_factor) || !(p.occupancy_limit > 0.0) || std::isnan(p.maxnumpoints))
        return fail(NDTGPU_ERR_INVALID, "world_assemble: eval_factor and occupancy_limit must be positive, maxnumpoints a number");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "world_assemble: no HIP device");
    ndtgpu_status rc = ndtgpu_world_check(dst->n_maps, dst->v.grid.res, dst_first, count, src->n_maps, src->v.grid.res, dst == src,
                                          node_offsets, node_idx);
    if (rc != NDTGPU_OK) return rc;

    hipStream_t st = (hipStream_t)stream;
    if ((rc = dst->wait_all_on(st)) != NDTGPU_OK) return rc;
    if (src != dst && (rc = src->wait_all_on(st)) != NDTGPU_OK) return rc;
    // the listed nodes' cell counts (the launch shape, n_contributions)
    std::vector<NdtMapCounters> sc(src->n_maps);
    HIP_TRY(hipMemcpyAsync(sc.data(), src->v.counters, sc.size() * sizeof(NdtMapCounters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<NdtWorldItem> items(n_items);
    std::vector<ndtgpu_world_result> res(count);
    memset(res.data(), 0, count * sizeof(ndtgpu_world_result));
    unsigned max_item_cells = 0;
    for (size_t w = 0; w < count; w++) {
        res[w].n_nodes = (int32_t)(node_offsets[w + 1] - node_offsets[w]);
        for (size_t k = node_offsets[w]; k < node_offsets[w + 1]; k++) {
            NdtWorldItem &it = items[k - n0];
            const double *T = T16 + 16 * (k - n0);               // column-major
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) it.R[3 * r + c] = T[4 * c + r];
                it.t[r] = T[12 + r];
            }
            it.dst_map = (uint32_t)(dst_first + w);
            it.src_map = node_idx[k];
            it.world = (uint32_t)w;
            it.n_cells = std::min(sc[node_idx[k]].n_cells, src->v.grid.max_cells);
            max_item_cells = std::max(max_item_cells, it.n_cells);
            res[w].n_contributions += it.n_cells;
        }
    }
    DeviceBuffer<NdtWorldItem> items_dev;
    DeviceBuffer<NdtWorldStats> stats_dev;
    if (items_dev.alloc(std::max<size_t>(n_items, 1)) != hipSuccess || stats_dev.alloc(count) != hipSuccess)
        return fail(NDTGPU_ERR_ALLOC, "world_assemble: device buffers");
    std::vector<NdtWorldStats> stats(count);
    if (n_items) HIP_TRY(hipMemcpyAsync(items_dev.get(), items.data(), n_items * sizeof(NdtWorldItem), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(stats_dev.get(), 0, count * sizeof(NdtWorldStats), st));
    // pass 1: the bound of every world's per-cell N, then its shifts (the same function of the world's own nodes in any batch)
    hipError_t e = ndt_launch_world_count(src->v, items_dev.get(), n_items, max_item_cells, stats_dev.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "world_assemble: count launch", e);
    HIP_TRY(hipMemcpyAsync(stats.data(), stats_dev.get(), count * sizeof(NdtWorldStats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t w = 0; w < count; w++) {
        if (stats[w].n_bound > 0xFFFFFFFFll) return fail(NDTGPU_ERR_CAPACITY, "world_assemble: a world's nodes hold 2^32 points or more");
        ndt_build_shifts(dst->v.grid, (size_t)stats[w].n_bound, &stats[w].s1_shift, &stats[w].s2_shift);
        res[w].s1_shift = stats[w].s1_shift;
        res[w].s2_shift = stats[w].s2_shift;
    }
    HIP_TRY(hipMemcpyAsync(stats_dev.get(), stats.data(), count * sizeof(NdtWorldStats), hipMemcpyHostToDevice, st));
    // the destination maps start like rebuilt maps: no readings, {overflow, n_dropped} reset (mapset_build_core, ndt_launch_build)
    const NdtSetView &dv = dst->v;
    if (dv.occ) HIP_TRY(hipMemsetAsync(dv.occ + dst_first * (size_t)dv.grid.slots, 0, count * (size_t)dv.grid.slots * sizeof(float), st));
    HIP_TRY(hipMemset2DAsync(&dv.counters[dst_first].overflow, sizeof(NdtMapCounters), 0, 2 * sizeof(uint32_t), count, st));
    // pass 2: the scatter into the destination maps' build scratch
    e = ndt_launch_world_scatter(dv, src->v, items_dev.get(), n_items, max_item_cells, stats_dev.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "world_assemble: scatter launch", e);
    // scratch -> cells: one set of launches per run of worlds with the same shifts (n_min 2: every contribution is a Gaussian)
    for (size_t w0 = 0; w0 < count;) {
        size_t w1 = w0 + 1;
        while (w1 < count && stats[w1].s1_shift == stats[w0].s1_shift && stats[w1].s2_shift == stats[w0].s2_shift) w1++;
        e = ndt_launch_finalise(dv, dst_first + w0, w1 - w0, 2, p.eval_factor, stats[w0].s1_shift, stats[w0].s2_shift, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "world_assemble: finalise launch", e);
        w0 = w1;
    }
    e = ndt_launch_world_finish(dv, dst_first, count, stats_dev.get(), p.maxnumpoints, p.occupancy_limit, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "world_assemble: finish launch", e);
    std::vector<NdtMapCounters> dc(count);
    HIP_TRY(hipMemcpyAsync(stats.data(), stats_dev.get(), count * sizeof(NdtWorldStats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dc.data(), dv.counters + dst_first, count * sizeof(NdtMapCounters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (results)
        for (size_t w = 0; w < count; w++) {
            ndtgpu_world_result &r = res[w];
            r.n_cells = (int32_t)dc[w].n_cells;
            r.n_dropped = stats[w].n_dropped;
            r.n_rejected = stats[w].n_rejected;
            r.n_points = stats[w].n_points;
            r.overflow = (int32_t)dc[w].overflow;
            results[w] = r;
        }
    return NDTGPU_OK;
}

}   // extern "C"
