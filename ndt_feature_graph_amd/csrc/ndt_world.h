// ndt_world.h -- what csrc/ndt_world.hip (kernels) and csrc/ndtgpu_world.hip (C-ABI) share of the world-map assembly.
#pragma once
#include "ndt_common.h"

struct NdtWorldItem {          // one listed node of one world
    double R[9];               // node frame -> world frame, row-major
    double t[3];
    uint32_t dst_map;          // map of the destination set
    uint32_t src_map;          // node map of the source set
    uint32_t world;            // index of the world in the call (its NdtWorldStats record)
    uint32_t n_cells;          // Gaussian cells of the node map
};
static_assert(sizeof(NdtWorldItem) == 112, "NdtWorldItem layout");

struct NdtWorldStats {         // per world of a call, device resident while it runs
    long long n_bound;         // sum of n over all listed cells (n < 2 as 2): the bound of a cell's N that sizes the shifts
    long long n_dropped;       // contributions whose mean left the destination grid
    long long n_rejected;      // not finite, or a second moment beyond the accumulator's room
    long long n_points;        // sum of n over the merged contributions
    int s1_shift, s2_shift;    // written by the host between the two passes
};

hipError_t ndt_launch_world_count(const NdtSetView &src, const NdtWorldItem *items_dev, size_t n_items, unsigned max_item_cells,
                                  NdtWorldStats *stats_dev, hipStream_t stream);
hipError_t ndt_launch_world_scatter(const NdtSetView &dst, const NdtSetView &src, const NdtWorldItem *items_dev, size_t n_items,
                                    unsigned max_item_cells, NdtWorldStats *stats_dev, hipStream_t stream);
// stats_dev: the record of map `first`
hipError_t ndt_launch_world_finish(const NdtSetView &dst, size_t first, size_t count, const NdtWorldStats *stats_dev,
                                   double maxnumpoints, double occupancy_limit, hipStream_t stream);
// csrc/ndt_build.hip: build scratch -> cells of maps [first, first + count) with explicit shifts and n_min (the second half of
// ndt_launch_build's few-maps path); {overflow, n_dropped} of the maps were reset before the scratch was filled
hipError_t ndt_launch_finalise(const NdtSetView &set, size_t first, size_t count, int n_min, double eval_factor, int s1_shift,
                               int s2_shift, hipStream_t stream);
