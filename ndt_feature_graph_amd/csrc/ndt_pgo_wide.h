// ndt_pgo_wide.h -- what the chip-wide form of the SE(2) pose-graph optimiser (csrc/ndt_pgo_wide.hip: ONE graph spread over the
// device, one plain launch per pass) shares with its C-ABI (csrc/ndtgpu_pgo.hip, ndtgpu_pgo_optimize_wide): the tile, the control
// block that carries the run's scalars from launch to launch, the launch argument and the launchers.
#pragma once
#include "ndt_pgo.h"

#define NDT_PGO_WIDE_TILE 256                     // items (links or nodes) per tile = threads per workgroup: part of the summation order
#define NDT_PGO_WIDE_WAVES (NDT_PGO_WIDE_TILE / 64)

// The run's scalars, counters and flags.  There are TWO in device memory: a launch reads one (src) and, where it is a node
// pass, one lane of its workgroup 0 writes the other (dst) IN FULL -- a launch whose phase is over copies src to dst -- and the
// host swaps the two after every node pass.  So no word is written by a launch in which any workgroup reads it.  The link
// passes write no control word: they read the src of the node pass behind them and come to the same decisions from the same
// partial sums.
struct NdtPgoWideCtl {
    int32_t run_done;                             // the Gauss-Newton loop has ended: exit_code holds, the result record is written
    int32_t solve_done;                           // the inner solve of this update has stopped: x is the step
    int32_t exit_code, iterations, linear;        // as ndtgpu_pgo_result; linear: inner iterations TAKEN, all updates together
    int32_t any_capped;                           // an inner solve of the run stopped at max_linear_iterations
    int32_t k;                                    // inner iterations of this solve
    int32_t pad_;
    double rz, tol2;                              // r.z of the iterate, eps_linear^2 * r.r of the solve's start
    double cost, cost_initial, max_step;
    double prior_cost;                            // the prior's term at the updated poses (written by the pose update)
};

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

inline size_t ndt_pgo_wide_tiles(size_t n) { return (n + NDT_PGO_WIDE_TILE - 1) / NDT_PGO_WIDE_TILE; }
// doubles of per-tile partial sums a graph of this size needs
inline size_t ndt_pgo_wide_partials(size_t n_nodes, size_t n_edges) { return 4 * ndt_pgo_wide_tiles(n_nodes) + ndt_pgo_wide_tiles(n_edges); }

// host launchers (csrc/ndt_pgo_wide.hip), one plain launch each; src / dst of W as the caller set them
enum NdtPgoWidePass {
    NDT_PGO_WIDE_LINEARISE,       // link pass: jac, te, per-tile cost                                   (not with E == 0)
    NDT_PGO_WIDE_ASSESS_FIRST,    // node pass: the cost at the poses as set; ends the run where it must
    NDT_PGO_WIDE_ASSESS,          // node pass: the cost after an update, the roll-back, the stop rule, the result record
    NDT_PGO_WIDE_START,           // node pass: gather b and the block inverses, x = 0, r = b, z = p = D^-1 r
    NDT_PGO_WIDE_LINK,            // link pass: t_e = W (J_ref p_ref + J_mov p_mov), p = z + beta p formed on the fly  (not with E == 0)
    NDT_PGO_WIDE_NODE,            // node pass: the solve's break rules, p = z + beta p stored, A p, per-tile p.Ap
    NDT_PGO_WIDE_STEP,            // node pass: alpha, x, r, z, per-tile r.z and r.r
    NDT_PGO_WIDE_UPDATE           // node pass: prev = pose, pose += x, per-tile largest |x|
};
inline bool ndt_pgo_wide_is_link_pass(NdtPgoWidePass p) { return p == NDT_PGO_WIDE_LINEARISE || p == NDT_PGO_WIDE_LINK; }
hipError_t ndt_pgo_wide_launch(NdtPgoWidePass pass, const NdtPgoWide &W, hipStream_t st);
