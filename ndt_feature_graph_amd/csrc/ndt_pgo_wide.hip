// ndt_pgo_wide.hip -- the chip-wide form of the SE(2) pose-graph optimiser (include/ndtgpu.h, ndtgpu_pgo_optimize_wide): ONE
// graph, a lane per link or per node over the whole grid, ONE PLAIN LAUNCH PER PASS on one stream.  The algorithm is that of
// ndt_pgo.hip operation for operation (the per-link and per-node bodies are the same inlines of ndt_pgo.h); what orders the
// passes is the boundary between two launches, nothing else: no grid barrier, no cooperative launch, no workgroup that waits for
// another, no spin on memory, no atomics.
//
// SUMS.  Items are cut into tiles of NDT_PGO_WIDE_TILE consecutive items, one workgroup per tile.  A tile's sum is taken in the
// order of ndt_block.h and written to partial[tile] by one lane.  Every workgroup of the launch that needs the graph's sum
// combines the partials itself, in one fixed order: thread t adds partials t, t + TILE, ... ascending from 0.0, then
// ndt_block_sum.  The tiling follows n_nodes and n_edges alone, so the bits do not depend on the bank's capacity, the other
// graphs, the CU count or the run.  A node's incident links are summed in ascending link order by one lane.
//
// CONTROL.  Every launch begins by reading the control block (ndt_pgo_wide_core.h: two copies, read one, write the other) and does
// nothing where its phase is over -- the solve has stopped, or the run has ended -- so the host may enqueue more inner
// iterations than the solve takes and the result is the same bits.
//
// An inner iteration is THREE launches:
//   LINK  per link: combines the per-tile r.z / r.r of the step before, applies the break rules (all workgroups come to the same
//         answer), beta = r.z' / r.z, and t_e = W (J_ref p_ref + J_mov p_mov) with p = z + beta p of its two end nodes formed on
//         the fly -- the fourth launch that would store the new search direction first is saved;
//   NODE  per node: the same head (it is the one that records it), p = z + beta p stored, (A p)_i gathered, per-tile p.Ap;
//   STEP  per node: combines p.Ap, alpha, x += alpha p, r -= alpha A p, z = D^-1 r, per-tile r.z and r.r.
// The combiners of the per-tile sums, the control block's store and the head of an inner iteration are csrc/ndt_pgo_wide_core.h's.
#include "ndt_pgo_wide.h"
#include "ndt_block.h"

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_linearise_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) return;
    const unsigned e = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double cost = 0.0;
    if (e < W.G.E) cost = pgo_linearise_link(W.G, e);
    cost = ndt_block_sum(cost, red, par);
    if (threadIdx.x == 0) W.part_cost[blockIdx.x] = cost;
}

// the cost at the current poses and what follows from it: FIRST at the poses as set, otherwise after an update
template <bool FIRST>
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_assess_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    double sum[1];
    wide_combine(W.part_cost, W.edge_tiles, sum, red, par);
    // (FIRST: no launch has moved the poses yet and this one does not; otherwise the roll-back below writes node 0's pose, so the
    //  prior's term comes from the pose update that computed it)
    const double cost = (FIRST ? pgo_prior_cost(W.G, W.prm) : c.prior_cost) + sum[0];
    const bool finite = cost - cost == 0.0;
    NdtPgoWideCtl n = c;
    if (FIRST) {
        n.cost_initial = n.cost = cost;
        if (!finite) {
            n.exit_code = NDTGPU_PGO_NOT_FINITE;
            n.run_done = 1;
        } else if (n.iterations >= W.prm.max_iterations) {
            n.exit_code = NDTGPU_PGO_MAX_ITERATIONS;
            n.run_done = 1;
        }
    } else {
        n.max_step = wide_combine_max(W.part_step, W.node_tiles, red, par);
        n.iterations = c.iterations + 1;
        if (!finite) {                               // the step left the finite numbers: back to the last iterate
            const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
            if (i < W.G.N)
                for (int d = 0; d < 3; d++) W.G.pose[3 * (size_t)i + d] = W.G.prev[3 * (size_t)i + d];
            n.exit_code = NDTGPU_PGO_NOT_FINITE;
            n.run_done = 1;
        } else {
            n.cost = cost;
            if (n.max_step <= W.prm.eps_step) {
                n.run_done = 1;
            } else if (n.iterations >= W.prm.max_iterations) {
                n.exit_code = NDTGPU_PGO_MAX_ITERATIONS;
                n.run_done = 1;
            }
        }
    }
    if (n.run_done) {
        if (n.exit_code != NDTGPU_PGO_NOT_FINITE && n.any_capped) n.exit_code = NDTGPU_PGO_LINEAR_CAP;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            W.out->exit_code = n.exit_code;
            W.out->iterations = n.iterations;
            W.out->linear_iterations = n.linear;
            W.out->cost_initial = n.cost_initial;
            W.out->cost_final = n.cost;
            W.out->max_step = n.max_step;
        }
    }
    wide_store(W, n);
}

// per node: gather b and the block inverse, then the solve's start: x = 0, r = b, z = p = D^-1 r, per-tile r.z and r.r
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_start_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    const PgoGraph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double dot[2] = {0.0, 0.0};
    if (i < G.N) {
        pgo_gather_node(G, W.prm, i);
        const size_t o = 3 * (size_t)i;
        const double r0 = G.b[o], r1 = G.b[o + 1], r2 = G.b[o + 2];
        double z0, z1, z2;
        pgo_symv(G.dinv + 6 * (size_t)i, r0, r1, r2, z0, z1, z2);
        G.x[o] = G.x[o + 1] = G.x[o + 2] = 0.0;
        G.r[o] = r0; G.r[o + 1] = r1; G.r[o + 2] = r2;
        G.p[o] = z0; G.p[o + 1] = z1; G.p[o + 2] = z2;
        dot[0] = r0 * z0 + r1 * z1 + r2 * z2;
        dot[1] = r0 * r0 + r1 * r1 + r2 * r2;
    }
    ndt_block_sum(dot, red, par);
    if (threadIdx.x == 0) {
        W.part_dot[blockIdx.x] = dot[0];
        W.part_dot[(size_t)W.node_tiles + blockIdx.x] = dot[1];
    }
    NdtPgoWideCtl n = c;
    n.k = 0;
    n.solve_done = 0;
    wide_store(W, n);
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_link_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done || c.solve_done) return;
    const WideHead h = wide_head(W, c, red, par);
    if (h.stop) return;
    const PgoGraph &G = W.G;
    const unsigned e = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    if (e >= G.E) return;
    const size_t oi = 3 * (size_t)G.ref[e], oj = 3 * (size_t)G.mov[e];
    double pi[3], pj[3];
    for (int d = 0; d < 3; d++) {
        pi[d] = G.p[oi + d];
        pj[d] = G.p[oj + d];
    }
    if (c.k > 0)
        for (int d = 0; d < 3; d++) {
            pi[d] = wide_direction(G.z[oi + d], h.beta, pi[d]);
            pj[d] = wide_direction(G.z[oj + d], h.beta, pj[d]);
        }
    pgo_link_product(G, e, pi, pj);
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_node_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done || c.solve_done) {
        wide_store(W, c);
        return;
    }
    const WideHead h = wide_head(W, c, red, par);
    NdtPgoWideCtl n = c;
    if (h.stop) {
        n.solve_done = 1;
        if (h.capped) n.any_capped = 1;
        wide_store(W, n);
        return;
    }
    const PgoGraph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double pap = 0.0;
    if (i < G.N) {
        const size_t o = 3 * (size_t)i;
        double p[3];
        for (int d = 0; d < 3; d++) p[d] = G.p[o + d];
        if (c.k > 0)
            for (int d = 0; d < 3; d++) {
                p[d] = wide_direction(G.z[o + d], h.beta, p[d]);
                G.p[o + d] = p[d];
            }
        double a0, a1, a2;
        pgo_node_product(G, W.prm, i, p[0], p[1], p[2], a0, a1, a2);
        G.ap[o] = a0; G.ap[o + 1] = a1; G.ap[o + 2] = a2;
        pap = p[0] * a0 + p[1] * a1 + p[2] * a2;
    }
    pap = ndt_block_sum(pap, red, par);
    if (threadIdx.x == 0) W.part_pap[blockIdx.x] = pap;
    n.rz = h.rz;
    n.tol2 = h.tol2;
    wide_store(W, n);
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_step_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done || c.solve_done) {
        wide_store(W, c);
        return;
    }
    double sum[1];
    wide_combine(W.part_pap, W.node_tiles, sum, red, par);
    const double pap = sum[0];
    NdtPgoWideCtl n = c;
    if (!(pap > 0.0)) {                                  // (not positive definite, or not finite: the iterate so far is the step)
        n.solve_done = 1;
        wide_store(W, n);
        return;
    }
    const double alpha = c.rz / pap;
    const PgoGraph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double dot[2] = {0.0, 0.0};
    if (i < G.N) {
        const size_t o = 3 * (size_t)i;
        double r[3], z[3];
        for (int d = 0; d < 3; d++) {
            G.x[o + d] += alpha * G.p[o + d];
            r[d] = G.r[o + d] - alpha * G.ap[o + d];
            G.r[o + d] = r[d];
        }
        pgo_symv(G.dinv + 6 * (size_t)i, r[0], r[1], r[2], z[0], z[1], z[2]);
        for (int d = 0; d < 3; d++) G.z[o + d] = z[d];
        dot[0] = r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
        dot[1] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
    ndt_block_sum(dot, red, par);
    if (threadIdx.x == 0) {
        W.part_dot[blockIdx.x] = dot[0];
        W.part_dot[(size_t)W.node_tiles + blockIdx.x] = dot[1];
    }
    n.k = c.k + 1;
    n.linear = c.linear + 1;
    wide_store(W, n);
}

// the pose update behind a solve that has stopped
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo_wide_update_kernel(NdtPgoWide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    const PgoGraph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double step = 0.0;
    if (i < G.N) {
        const size_t o = 3 * (size_t)i;
        for (int d = 0; d < 3; d++) {
            G.prev[o + d] = G.pose[o + d];
            step = fmax(step, fabs(G.x[o + d]));
        }
        G.pose[o] += G.x[o];
        G.pose[o + 1] += G.x[o + 1];
        G.pose[o + 2] = ndt_pgo_wrap(G.pose[o + 2] + G.x[o + 2]);
    }
    step = ndt_block_max(step, red, par);
    if (threadIdx.x == 0) W.part_step[blockIdx.x] = step;
    NdtPgoWideCtl n = c;
    if (blockIdx.x == 0 && threadIdx.x == 0) n.prior_cost = pgo_prior_cost(G, W.prm);   // (the lane that has just moved node 0)
    wide_store(W, n);
}

hipError_t ndt_pgo_wide_launch(NdtPgoWidePass pass, const NdtPgoWide &W, hipStream_t st)
{
    const unsigned tiles = ndt_pgo_wide_is_link_pass(pass) ? W.edge_tiles : W.node_tiles;
    if (!tiles) return hipErrorInvalidValue;             // (a grid of no workgroups: the caller skips the link passes of a graph without links)
    const dim3 grid(tiles), block(NDT_PGO_WIDE_TILE);
    switch (pass) {
    case NDT_PGO_WIDE_LINEARISE: hipLaunchKernelGGL(ndt_pgo_wide_linearise_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_ASSESS_FIRST: hipLaunchKernelGGL(ndt_pgo_wide_assess_kernel<true>, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_ASSESS: hipLaunchKernelGGL(ndt_pgo_wide_assess_kernel<false>, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_START: hipLaunchKernelGGL(ndt_pgo_wide_start_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_LINK: hipLaunchKernelGGL(ndt_pgo_wide_link_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_NODE: hipLaunchKernelGGL(ndt_pgo_wide_node_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_STEP: hipLaunchKernelGGL(ndt_pgo_wide_step_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_UPDATE: hipLaunchKernelGGL(ndt_pgo_wide_update_kernel, grid, block, 0, st, W); break;
    }
    return hipGetLastError();
}
