// ndt_pgo_wide.h -- what the chip-wide form of the SE(2) pose-graph optimiser (csrc/ndt_pgo_wide.hip: ONE graph spread over the
// device, one plain launch per pass) shares with its C-ABI (csrc/ndtgpu_pgo.hip, ndtgpu_pgo_optimize_wide): the launch
// argument and the launcher.  The tile, the control block and the passes are those of csrc/ndt_pgo_wide_core.h.
#pragma once
#include "ndt_pgo.h"
#include "ndt_pgo_wide_core.h"                    // the tile, the control block, the passes, the steering loop: shared with the SE(3) form

// a launch's argument
struct NdtPgoWide {
    PgoGraph G;
    NdtPgoParamsDev prm;
    const NdtPgoWideCtl *src;
    NdtPgoWideCtl *dst;
    unsigned node_tiles, edge_tiles;              // ceil(N / TILE), ceil(E / TILE): the graph's own, never the handle's capacity
    double *part_dot;                             // [2][node_tiles]  per-tile r.z and r.r
    double *part_pap;                             // [node_tiles]     per-tile p.Ap
    double *part_step;                            // [node_tiles]     per-tile largest |x|
    double *part_cost;                            // [edge_tiles]     per-tile sum e^T W e
    ndtgpu_pgo_result *out;                       // the graph's record in the bank
};

// doubles of per-tile partial sums a graph of this size needs
inline size_t ndt_pgo_wide_partials(size_t n_nodes, size_t n_edges) { return 4 * ndt_pgo_wide_tiles(n_nodes) + ndt_pgo_wide_tiles(n_edges); }

// host launcher (csrc/ndt_pgo_wide.hip), one plain launch; src / dst of W as the caller set them.  The link passes (LINEARISE,
// LINK) are not launched for a graph without links: a grid of no workgroups is an error.
hipError_t ndt_pgo_wide_launch(NdtPgoWidePass pass, const NdtPgoWide &W, hipStream_t st);
