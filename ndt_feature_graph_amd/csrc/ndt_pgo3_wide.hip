// ndt_pgo3_wide.hip -- the chip-wide form of the SE(3) pose-graph optimiser (include/ndtgpu.h, ndtgpu_pgo3_optimize_wide): ONE
// graph, a lane per link or per node over the whole grid, ONE PLAIN LAUNCH PER PASS on one stream.  The algorithm is that of
// ndt_pgo3.hip operation for operation (the per-link and per-node bodies are the same inlines of ndt_pgo3.h, unchanged); the
// structure is that of ndt_pgo_wide.hip, and what the two wide forms have in common -- the tile, the control block, the combiners
// of the per-tile sums, the head of an inner iteration, the host's steering loop -- is csrc/ndt_pgo_wide_core.h, once.  What
// orders the passes is the boundary between two launches, nothing else: no grid barrier, no cooperative launch, no workgroup
// that waits for another, no spin on memory, no atomics.
//
// ITEMS.  The node passes run over N items.  The link passes run over E + 1: the prior is the link behind the last, item E, as in
// ndt_pgo3.h, so a link pass always has a workgroup, also for a graph without links.  The linearisation treats item E like any
// link (pgo3_linearise_link); the product pass does nothing for it -- the prior's J^T W J p stays in node 0's lane
// (pgo3_node_product).
//
// SUMS.  Items are cut into tiles of NDT_PGO_WIDE_TILE consecutive items, one workgroup per tile.  A tile's sum is taken in the
// order of ndt_block.h and written to partial[tile] by one lane.  Every workgroup of the launch that needs the graph's sum
// combines the partials itself, in one fixed order: thread t adds partials t, t + TILE, ... ascending from 0.0, then
// ndt_block_sum.  The tiling follows n_nodes and n_edges alone, so the bits do not depend on the bank's capacity, the other
// graphs, the CU count or the run.  A node's incident links are summed in ascending link order by one lane.  A half turn is a
// per-tile count summed the same way beside the cost.
//
// CONTROL.  Every launch begins by reading the control block (two copies, read one, write the other) and does nothing where its
// phase is over, so the host may enqueue more inner iterations than the solve takes and the result is the same bits.
//
// An inner iteration is THREE launches, LINK, NODE and STEP as in ndt_pgo_wide.hip.  The search direction p = z + beta p is one
// fma (wide_direction) in the link pass that uses it and in the node pass that stores it: the same bits in both.  (The
// one-workgroup kernel leaves the contraction of z + beta * p to the compiler; the two forms differ in their summation order
// anyway.)
//
// REGISTERS.  Every pass is its own kernel of 256 threads, one wave per SIMD, so the linearisation and the gather have the
// whole register file and START holds the gather and the solve's start in ONE launch; include/ndtgpu.h quotes the figures of
// tools/kernel_resources.py pgo3_wide (no VGPR spill, no scratch in any of them).
#include "ndt_pgo3_wide.h"
#include "ndt_block.h"

// pgo3_link_product with the two end nodes' search directions in registers instead of G.p, the same operations in the same order
__device__ __forceinline__ void pgo3_wide_link_product(const Pgo3Graph &G, unsigned e, const double (&pi)[6], const double (&pj)[6])
{
    const double *jac = G.jac + NDT_PGO3_JAC * (size_t)e;
    double u[6], v[6], t[6];
    pgo3_j(0, jac, pi, u);
    pgo3_j(1, jac, pj, v);
    for (int k = 0; k < 6; k++) u[k] += v[k];
    pgo3_symv(G.info + 21 * (size_t)e, u, t);
    double *te = G.te + 6 * (size_t)e;
    for (int k = 0; k < 6; k++) te[k] = t[k];
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_linearise_kernel(NdtPgo3Wide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) return;
    const unsigned e = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    bool half = false;
    double s[2] = {0.0, 0.0};
    if (e <= W.G.E) s[0] = pgo3_linearise_link(W.G, W.prm, e, half);
    s[1] = half ? 1.0 : 0.0;
    ndt_block_sum(s, red, par);
    if (threadIdx.x == 0) {
        W.part_cost[blockIdx.x] = s[0];
        W.part_cost[(size_t)W.link_tiles + blockIdx.x] = s[1];
    }
}

// the cost at the current poses and what follows from it: FIRST at the poses as set, otherwise after an update
template <bool FIRST>
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_assess_kernel(NdtPgo3Wide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    double sum[2];
    wide_combine(W.part_cost, W.link_tiles, sum, red, par);
    const double cost = sum[0];                      // (the prior's term is item E's)
    const bool half = sum[1] > 0.0, finite = cost - cost == 0.0;
    NdtPgoWideCtl n = c;
    if (FIRST) {
        n.cost_initial = n.cost = cost;
        if (half) {                                  // (tested before the cost, which a half turn makes NaN)
            n.exit_code = NDTGPU_PGO3_HALF_TURN;
            n.run_done = 1;
        } else if (!finite) {
            n.exit_code = NDTGPU_PGO_NOT_FINITE;
            n.run_done = 1;
        } else if (n.iterations >= W.prm.max_iterations) {
            n.exit_code = NDTGPU_PGO_MAX_ITERATIONS;
            n.run_done = 1;
        }
    } else {
        n.max_step = wide_combine_max(W.part_step, W.node_tiles, red, par);
        n.iterations = c.iterations + 1;
        if (!finite) {                               // the step left the finite numbers (or met a half turn): back to the last iterate
            const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
            if (i < W.G.N)
                for (int d = 0; d < 12; d++) W.G.pose[12 * (size_t)i + d] = W.G.prev[12 * (size_t)i + d];
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
        if (n.exit_code != NDTGPU_PGO_NOT_FINITE && n.exit_code != NDTGPU_PGO3_HALF_TURN && n.any_capped) n.exit_code = NDTGPU_PGO_LINEAR_CAP;
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

// per node: gather b and factor the diagonal block, then the solve's start: x = 0, r = b, z = p = M^-1 r, per-tile r.z and r.r
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_start_kernel(NdtPgo3Wide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    const Pgo3Graph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double dot[2] = {0.0, 0.0};
    if (i < G.N) {
        pgo3_gather_node(G, W.prm, i);
        const size_t o = 6 * (size_t)i;
        double r[6], z[6];
        for (int d = 0; d < 6; d++) r[d] = G.b[o + d];
        pgo3_precondition(G, i, r, z);
        for (int d = 0; d < 6; d++) {
            G.x[o + d] = 0.0;
            G.r[o + d] = r[d];
            G.p[o + d] = z[d];
        }
        dot[0] = pgo3_dot6(r, z);
        dot[1] = pgo3_dot6(r, r);
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

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_link_kernel(NdtPgo3Wide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done || c.solve_done) return;
    const WideHead h = wide_head(W, c, red, par);
    if (h.stop) return;
    const Pgo3Graph &G = W.G;
    const unsigned e = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    if (e >= G.E) return;                                // (item E, the prior, is node 0's in the node pass)
    const size_t oi = 6 * (size_t)G.ref[e], oj = 6 * (size_t)G.mov[e];
    double pi[6], pj[6];
    for (int d = 0; d < 6; d++) {
        pi[d] = G.p[oi + d];
        pj[d] = G.p[oj + d];
    }
    if (c.k > 0)
        for (int d = 0; d < 6; d++) {
            pi[d] = wide_direction(G.z[oi + d], h.beta, pi[d]);
            pj[d] = wide_direction(G.z[oj + d], h.beta, pj[d]);
        }
    pgo3_wide_link_product(G, e, pi, pj);
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_node_kernel(NdtPgo3Wide W)
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
    const Pgo3Graph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double pap = 0.0;
    if (i < G.N) {
        const size_t o = 6 * (size_t)i;
        double p[6], ap[6];
        for (int d = 0; d < 6; d++) p[d] = G.p[o + d];
        if (c.k > 0)
            for (int d = 0; d < 6; d++) {
                p[d] = wide_direction(G.z[o + d], h.beta, p[d]);
                G.p[o + d] = p[d];
            }
        pgo3_node_product(G, W.prm, i, p, ap);
        for (int d = 0; d < 6; d++) G.ap[o + d] = ap[d];
        pap = pgo3_dot6(p, ap);
    }
    pap = ndt_block_sum(pap, red, par);
    if (threadIdx.x == 0) W.part_pap[blockIdx.x] = pap;
    n.rz = h.rz;
    n.tol2 = h.tol2;
    wide_store(W, n);
}

__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_step_kernel(NdtPgo3Wide W)
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
    const Pgo3Graph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double dot[2] = {0.0, 0.0};
    if (i < G.N) {
        const size_t o = 6 * (size_t)i;
        double r[6], z[6];
        for (int d = 0; d < 6; d++) {
            G.x[o + d] += alpha * G.p[o + d];
            r[d] = G.r[o + d] - alpha * G.ap[o + d];
            G.r[o + d] = r[d];
        }
        pgo3_precondition(G, i, r, z);
        for (int d = 0; d < 6; d++) G.z[o + d] = z[d];
        dot[0] = pgo3_dot6(r, z);
        dot[1] = pgo3_dot6(r, r);
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
__global__ __launch_bounds__(NDT_PGO_WIDE_TILE) void ndt_pgo3_wide_update_kernel(NdtPgo3Wide W)
{
    __shared__ WideRed red;
    int par = 0;
    const NdtPgoWideCtl c = *W.src;
    if (c.run_done) {
        wide_store(W, c);
        return;
    }
    const Pgo3Graph &G = W.G;
    const unsigned i = blockIdx.x * NDT_PGO_WIDE_TILE + threadIdx.x;
    double step = 0.0;
    if (i < G.N) {
        double *P = G.pose + 12 * (size_t)i, *prev = G.prev + 12 * (size_t)i;
        double d[6];
        for (int k = 0; k < 6; k++) {
            d[k] = G.x[6 * (size_t)i + k];
            step = fmax(step, fabs(d[k]));
        }
        for (int k = 0; k < 12; k++) prev[k] = P[k];
        pgo3_retract(prev, d, P);
    }
    step = ndt_block_max(step, red, par);
    if (threadIdx.x == 0) W.part_step[blockIdx.x] = step;
    wide_store(W, c);
}

hipError_t ndt_pgo3_wide_launch(NdtPgoWidePass pass, const NdtPgo3Wide &W, hipStream_t st)
{
    const unsigned tiles = ndt_pgo_wide_is_link_pass(pass) ? W.link_tiles : W.node_tiles;
    if (!tiles) return hipErrorInvalidValue;
    const dim3 grid(tiles), block(NDT_PGO_WIDE_TILE);
    switch (pass) {
    case NDT_PGO_WIDE_LINEARISE: hipLaunchKernelGGL(ndt_pgo3_wide_linearise_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_ASSESS_FIRST: hipLaunchKernelGGL(ndt_pgo3_wide_assess_kernel<true>, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_ASSESS: hipLaunchKernelGGL(ndt_pgo3_wide_assess_kernel<false>, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_START: hipLaunchKernelGGL(ndt_pgo3_wide_start_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_LINK: hipLaunchKernelGGL(ndt_pgo3_wide_link_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_NODE: hipLaunchKernelGGL(ndt_pgo3_wide_node_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_STEP: hipLaunchKernelGGL(ndt_pgo3_wide_step_kernel, grid, block, 0, st, W); break;
    case NDT_PGO_WIDE_UPDATE: hipLaunchKernelGGL(ndt_pgo3_wide_update_kernel, grid, block, 0, st, W); break;
    }
    return hipGetLastError();
}
