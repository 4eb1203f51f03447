// ndt_pgo.hip -- batched SE(2) pose-graph optimisation (include/ndtgpu.h, ndtgpu_pgo_*): Gauss-Newton on the prior and the
// Pose2d_Pose2d factors of optimizeGraphUsingISAM (ndt_offline_mapper.h:40-107), each linear system by conjugate gradients
// preconditioned with the inverses of the 3x3 diagonal blocks.
//
// ndt_pgo_kernel: ONE workgroup of NDT_PGO_THREADS optimises ONE graph from start to finish; `count` graphs are `count`
// workgroups that never look at each other.  Inside a workgroup only __syncthreads orders the passes: no grid barrier, no
// queue, no spin on memory, no atomics.  Every sum is taken in one fixed order -- a thread's strided items in ascending order,
// then over the workgroup in the order of ndt_block.h; a node's incident edges in ascending edge order -- so a
// graph's result is the same bits whichever batch it runs in.
//   linearisation (once per Gauss-Newton iteration): a thread per edge (strided) writes c, s, lx, ly -- all that both 3x3
//     Jacobian blocks hold -- and W e; a thread per node gathers its gradient and its 3x3 diagonal block over the node's
//     incident edges (CSR adjacency built by the host) and inverts the block.
//   matrix-vector product: a per-edge pass t_e = W (J_ref p_ref + J_mov p_mov), then a per-node gather sum J^T t_e.
// A node is always handled by the same thread, so the vector updates between the passes need no barrier.  The vectors live in a
// per-graph scratch area in device memory (27 doubles per node, 7 per edge), LDS holds the reductions' partial sums.
// The per-link and per-node bodies are inlines of ndt_pgo.h, shared with the chip-wide form for one large graph (ndt_pgo_wide.hip).
#include "ndt_pgo.h"
#include "ndt_pgo_marginals.h"
#include "ndt_block.h"

typedef NdtBlockSums<NDT_PGO_WAVES, 2> PgoRed;

// per edge: error, Jacobian numbers, W e.  Returns the graph's cost sum e^T W e (prior included) in every thread; its barrier
// is the one that makes jac / te visible to the gather.
__device__ double pgo_linearise(const PgoGraph &G, const NdtPgoParamsDev &prm, PgoRed &red, int &par)
{
    double cost = 0.0;
    if (threadIdx.x == 0) cost = pgo_prior_cost(G, prm);
    for (unsigned e = threadIdx.x; e < G.E; e += NDT_PGO_THREADS) cost += pgo_linearise_link(G, e);
    return ndt_block_sum(cost, red, par);
}

// per node: b = -gradient and the inverse of the 3x3 diagonal block of J^T W J, over the node's incident edges
__device__ void pgo_gather(const PgoGraph &G, const NdtPgoParamsDev &prm)
{
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) pgo_gather_node(G, prm, i);
}

// Solves (J^T W J) x = b by preconditioned conjugate gradients from x = 0; returns the iterations taken, `capped` where it
// stopped at max_linear_iterations with the relative residual still above eps_linear.
__device__ int pgo_solve(const PgoGraph &G, const NdtPgoParamsDev &prm, PgoRed &red, int &par, bool &capped)
{
    double dot[2] = {0.0, 0.0};                          // r.z and r.r
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
        const size_t o = 3 * (size_t)i;
        const double r0 = G.b[o], r1 = G.b[o + 1], r2 = G.b[o + 2];
        double z0, z1, z2;
        pgo_symv(G.dinv + 6 * (size_t)i, r0, r1, r2, z0, z1, z2);
        G.x[o] = G.x[o + 1] = G.x[o + 2] = 0.0;
        G.r[o] = r0; G.r[o + 1] = r1; G.r[o + 2] = r2;
        G.p[o] = z0; G.p[o + 1] = z1; G.p[o + 2] = z2;
        dot[0] += r0 * z0 + r1 * z1 + r2 * z2;
        dot[1] += r0 * r0 + r1 * r1 + r2 * r2;
    }
    ndt_block_sum(dot, red, par);                        // (its barrier: p is visible to the edge pass)
    double rz = dot[0];
    const double tol2 = prm.eps_linear * prm.eps_linear * dot[1];
    int k = 0;
    capped = false;
    while (dot[1] > tol2) {
        if (k >= prm.max_linear_iterations) {
            capped = true;
            break;
        }
        for (unsigned e = threadIdx.x; e < G.E; e += NDT_PGO_THREADS)
            pgo_link_product(G, e, G.p + 3 * (size_t)G.ref[e], G.p + 3 * (size_t)G.mov[e]);
        __syncthreads();
        double pap = 0.0;
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
            const size_t o = 3 * (size_t)i;
            const double p0 = G.p[o], p1 = G.p[o + 1], p2 = G.p[o + 2];
            double a0, a1, a2;
            pgo_node_product(G, prm, i, p0, p1, p2, a0, a1, a2);
            G.ap[o] = a0; G.ap[o + 1] = a1; G.ap[o + 2] = a2;
            pap += p0 * a0 + p1 * a1 + p2 * a2;
        }
        pap = ndt_block_sum(pap, red, par);
        if (!(pap > 0.0)) break;                         // (not positive definite, or not finite: the iterate so far is the step)
        const double alpha = rz / pap;
        dot[0] = dot[1] = 0.0;
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
            const size_t o = 3 * (size_t)i;
            double r[3], z[3];
            for (int d = 0; d < 3; d++) {
                G.x[o + d] += alpha * G.p[o + d];
                r[d] = G.r[o + d] - alpha * G.ap[o + d];
                G.r[o + d] = r[d];
            }
            pgo_symv(G.dinv + 6 * (size_t)i, r[0], r[1], r[2], z[0], z[1], z[2]);
            for (int d = 0; d < 3; d++) G.z[o + d] = z[d];
            dot[0] += r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
            dot[1] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        }
        ndt_block_sum(dot, red, par);                    // (its barrier: every edge has read the old p)
        const double beta = dot[0] / rz;
        rz = dot[0];
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
            const size_t o = 3 * (size_t)i;
            for (int d = 0; d < 3; d++) G.p[o + d] = G.z[o + d] + beta * G.p[o + d];
        }
        __syncthreads();
        k++;
    }
    return k;
}

__global__ __launch_bounds__(NDT_PGO_THREADS) void ndt_pgo_kernel(NdtPgoView v, size_t first, NdtPgoParamsDev prm)
{
    __shared__ PgoRed red;
    int par = 0;
    const size_t g = first + blockIdx.x;
    ndtgpu_pgo_result *out = v.state + g;
    const PgoGraph G = ndt_pgo_graph(v, g, (unsigned)out->n_nodes, (unsigned)out->n_edges);

    int exit_code = NDTGPU_PGO_CONVERGED, iterations = 0, linear = 0;
    bool any_capped = false;
    double max_step = 0.0;
    double cost = pgo_linearise(G, prm, red, par);
    const double cost_initial = cost;
    if (!(cost - cost == 0.0)) {
        exit_code = NDTGPU_PGO_NOT_FINITE;
    } else {
        for (;;) {
            if (iterations >= prm.max_iterations) {
                exit_code = NDTGPU_PGO_MAX_ITERATIONS;
                break;
            }
            pgo_gather(G, prm);
            bool capped;
            linear += pgo_solve(G, prm, red, par, capped);
            any_capped = any_capped || capped;
            double step = 0.0;
            for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
                const size_t o = 3 * (size_t)i;
                for (int d = 0; d < 3; d++) {
                    G.prev[o + d] = G.pose[o + d];
                    step = fmax(step, fabs(G.x[o + d]));
                }
                G.pose[o] += G.x[o];
                G.pose[o + 1] += G.x[o + 1];
                G.pose[o + 2] = ndt_pgo_wrap(G.pose[o + 2] + G.x[o + 2]);
            }
            max_step = ndt_block_max(step, red, par);    // (its barrier: the new poses are visible to the edge pass)
            iterations++;
            const double cost_new = pgo_linearise(G, prm, red, par);
            if (!(cost_new - cost_new == 0.0)) {         // the step left the finite numbers: back to the last iterate
                for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS)
                    for (int d = 0; d < 3; d++) G.pose[3 * (size_t)i + d] = G.prev[3 * (size_t)i + d];
                exit_code = NDTGPU_PGO_NOT_FINITE;
                break;
            }
            cost = cost_new;
            if (max_step <= prm.eps_step) break;
        }
        if (exit_code != NDTGPU_PGO_NOT_FINITE && any_capped) exit_code = NDTGPU_PGO_LINEAR_CAP;
    }
    if (threadIdx.x == 0) {
        out->exit_code = exit_code;
        out->iterations = iterations;
        out->linear_iterations = linear;
        out->cost_initial = cost_initial;
        out->cost_final = cost;
        out->max_step = max_step;
    }
}

__global__ void ndt_pgo_links_kernel(NdtPgoView v, size_t g, unsigned n_edges, const double *T16, const double *cov36, const int32_t *flags)
{
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    ndt_pgo_link_from_registration(T16 + 16 * (size_t)e, cov36 ? cov36 + 36 * (size_t)e : nullptr, (cov36 && flags) ? flags[e] : 0,
                                   v.meas + (g * v.max_edges + e) * 3, v.info + (g * v.max_edges + e) * 6);
}

// ---- marginal covariances (include/ndtgpu.h, ndtgpu_pgo_marginals): three plain launches that drive the passes above ----
// Column k of block column q of H^-1 is the solution of H x = e_(q,k), and the columns of a call are independent: prepare
// linearises each graph named once, into the marginals' own workspace; solve gives every column a workgroup and a slot and calls
// pgo_solve as it is; finish symmetrises a lane per query.  Nothing is shared between workgroups except what prepare wrote, and
// a workgroup's slot is its position in the launch: no atomics, no waiting, and a column's bits do not depend on what runs beside it.

__global__ __launch_bounds__(NDT_PGO_THREADS) void ndt_pgo_marginal_prepare_kernel(NdtPgoView v, NdtPgoMarginalWork w, NdtPgoParamsDev prm)
{
    __shared__ PgoRed red;
    int par = 0;
    const size_t g = (size_t)w.area_graph[blockIdx.x];
    const ndtgpu_pgo_result *st = v.state + g;
    PgoGraph G = ndt_pgo_graph(v, g, (unsigned)st->n_nodes, (unsigned)st->n_edges);
    ndt_pgo_marginal_area(G, w.areas + blockIdx.x * w.area_doubles, v.max_nodes, v.max_edges);
    const double cost = pgo_linearise(G, prm, red, par);
    pgo_gather(G, prm);
    if (threadIdx.x == 0) w.verdict[blockIdx.x] = (cost - cost == 0.0) ? NDTGPU_PGO_CONVERGED : NDTGPU_PGO_NOT_FINITE;
}

__global__ __launch_bounds__(NDT_PGO_THREADS) void ndt_pgo_marginal_solve_kernel(NdtPgoView v, NdtPgoMarginalWork w, unsigned first,
                                                                                 NdtPgoParamsDev prm)
{
    __shared__ PgoRed red;
    int par = 0;
    const unsigned col = first + blockIdx.x, q = col / 3, k = col % 3;
    const NdtPgoMarginalQuery Q = w.query[q];
    if (w.verdict[Q.area] != NDTGPU_PGO_CONVERGED) return;       // (the whole workgroup: finish writes NaN)
    const ndtgpu_pgo_result *st = v.state + Q.graph;
    PgoGraph G = ndt_pgo_graph(v, (size_t)Q.graph, (unsigned)st->n_nodes, (unsigned)st->n_edges);
    ndt_pgo_marginal_slot(G, w.areas + Q.area * w.area_doubles, w.slots + blockIdx.x * w.slot_doubles, v.max_nodes, v.max_edges);
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS)
        for (unsigned d = 0; d < 3; d++) G.b[3 * (size_t)i + d] = (i == (unsigned)Q.node && d == k) ? 1.0 : 0.0;
    bool capped;
    const int iterations = pgo_solve(G, prm, red, par, capped);  // (a node's b is read by the thread that wrote it)
    __syncthreads();
    double *raw = w.raw + 18 * (size_t)q;
    if (threadIdx.x < 3) raw[3 * threadIdx.x + k] = G.x[3 * (size_t)Q.node + threadIdx.x];
    else if (threadIdx.x < 6 && Q.other >= 0) raw[9 + 3 * (threadIdx.x - 3) + k] = G.x[3 * (size_t)Q.other + threadIdx.x - 3];
    if (threadIdx.x == 0) w.col[col] = NdtPgoMarginalCol{iterations, capped ? 1 : 0};
}

// a lane per query (both banks: DOF is 3 or 6): the symmetric part of the raw diagonal block, its asymmetry, the raw cross block
// and the record; NaN for a graph whose linearisation was not finite or met a half turn
template <int DOF>
__global__ void ndt_pgo_marginal_finish_kernel(NdtPgoMarginalWork w, double *cov, double *cross, ndtgpu_pgo_marginal_result *results)
{
    const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= w.n_queries) return;
    constexpr int NN = DOF * DOF;
    const NdtPgoMarginalQuery Q = w.query[q];
    const int verdict = w.verdict[Q.area];
    const double *B = w.raw + 2 * NN * (size_t)q;
    double *C = cov + NN * (size_t)q, *X = (cross && Q.other >= 0) ? cross + NN * (size_t)q : nullptr;
    ndtgpu_pgo_marginal_result r;
    r.exit_code = verdict;
    r.linear_iterations = r.max_column_iterations = r.capped_columns = 0;
    r.asymmetry = 0.0;
    if (verdict != NDTGPU_PGO_CONVERGED) {
        for (int k = 0; k < NN; k++) C[k] = NAN;
        if (X)
            for (int k = 0; k < NN; k++) X[k] = NAN;
        r.asymmetry = NAN;
    } else {
#pragma unroll 1
        for (int i = 0; i < DOF; i++)                    // (rolled: unrolled, the 6x6 block's 36 loads set the kernel's registers)
            for (int j = 0; j < DOF; j++) {
                C[DOF * i + j] = 0.5 * (B[DOF * i + j] + B[DOF * j + i]);
                r.asymmetry = fmax(r.asymmetry, fabs(B[DOF * i + j] - B[DOF * j + i]));
            }
        if (X)
            for (int k = 0; k < NN; k++) X[k] = B[NN + k];
        for (int k = 0; k < DOF; k++) {
            const NdtPgoMarginalCol c = w.col[DOF * (size_t)q + k];
            r.linear_iterations += c.iterations;
            r.max_column_iterations = c.iterations > r.max_column_iterations ? c.iterations : r.max_column_iterations;
            r.capped_columns += c.capped;
        }
        if (r.capped_columns) r.exit_code = NDTGPU_PGO_LINEAR_CAP;
    }
    results[q] = r;
}

hipError_t ndt_pgo_marginal_launch_prepare(const NdtPgoView &v, const NdtPgoMarginalWork &w, size_t n_areas, const NdtPgoParamsDev &prm, hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo_marginal_prepare_kernel, dim3((unsigned)n_areas), dim3(NDT_PGO_THREADS), 0, st, v, w, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo_marginal_launch_solve(const NdtPgoView &v, const NdtPgoMarginalWork &w, size_t first, size_t count, const NdtPgoParamsDev &prm,
                                         hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo_marginal_solve_kernel, dim3((unsigned)count), dim3(NDT_PGO_THREADS), 0, st, v, w, (unsigned)first, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo_marginal_launch_finish(const NdtPgoMarginalWork &w, int dof, double *cov_dev, double *cross_dev,
                                          ndtgpu_pgo_marginal_result *results_dev, hipStream_t st)
{
    const dim3 grid((w.n_queries + 255) / 256), block(256);
    if (dof == 3) hipLaunchKernelGGL(ndt_pgo_marginal_finish_kernel<3>, grid, block, 0, st, w, cov_dev, cross_dev, results_dev);
    else hipLaunchKernelGGL(ndt_pgo_marginal_finish_kernel<6>, grid, block, 0, st, w, cov_dev, cross_dev, results_dev);
    return hipGetLastError();
}

hipError_t ndt_pgo_launch(const NdtPgoView &v, size_t first, size_t count, const NdtPgoParamsDev &prm, hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo_kernel, dim3((unsigned)count), dim3(NDT_PGO_THREADS), 0, st, v, first, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo_launch_links(const NdtPgoView &v, size_t g, size_t n_edges, const double *T16_dev, const double *cov36_dev,
                                const int32_t *cov_flags_dev, hipStream_t st)
{
    if (!n_edges) return hipSuccess;
    hipLaunchKernelGGL(ndt_pgo_links_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st, v, g, (unsigned)n_edges, T16_dev,
                       cov36_dev, cov_flags_dev);
    return hipGetLastError();
}
