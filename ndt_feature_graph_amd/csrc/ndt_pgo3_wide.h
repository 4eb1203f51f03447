// ndt_pgo3_wide.h -- what the chip-wide form of the SE(3) pose-graph optimiser (csrc/ndt_pgo3_wide.hip: ONE graph spread over
// the device, one plain launch per pass) shares with its C-ABI (csrc/ndtgpu_pgo3.hip, ndtgpu_pgo3_optimize_wide): the launch
// argument and the launcher.  The tile, the control block, the passes and the steering loop are those of
// csrc/ndt_pgo_wide_core.h, the same copy the SE(2) form uses.
#pragma once
#include "ndt_pgo3.h"
#include "ndt_pgo_wide_core.h"

// a launch's argument
struct NdtPgo3Wide {
    Pgo3Graph G;
    NdtPgo3ParamsDev prm;
    const NdtPgoWideCtl *src;
    NdtPgoWideCtl *dst;
    unsigned node_tiles, link_tiles;              // ceil(N / TILE), ceil((E + 1) / TILE) -- the prior is the link behind the last, so
                                                  // link_tiles is never 0: the graph's own, never the handle's capacity
    double *part_dot;                             // [2][node_tiles]  per-tile r.z and r.r
    double *part_pap;                             // [node_tiles]     per-tile p.Ap
    double *part_step;                            // [node_tiles]     per-tile largest |x|
    double *part_cost;                            // [2][link_tiles]  per-tile sum e^T W e, and the tile's number of half turns
    ndtgpu_pgo_result *out;                       // the graph's record in the bank
};

inline size_t ndt_pgo3_wide_link_tiles(size_t n_edges) { return ndt_pgo_wide_tiles(n_edges + 1); }
// doubles of per-tile partial sums a graph of this size needs
inline size_t ndt_pgo3_wide_partials(size_t n_nodes, size_t n_edges) { return 4 * ndt_pgo_wide_tiles(n_nodes) + 2 * ndt_pgo3_wide_link_tiles(n_edges); }

// host launcher (csrc/ndt_pgo3_wide.hip), one plain launch; src / dst of W as the caller set them
hipError_t ndt_pgo3_wide_launch(NdtPgoWidePass pass, const NdtPgo3Wide &W, hipStream_t st);
