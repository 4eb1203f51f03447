// ndt_pgo3.hip -- batched SE(3) pose-graph optimisation (include/ndtgpu.h, ndtgpu_pgo3_*): Gauss-Newton on the prior and the
// 6-DoF link factors e = (t_E, Log R_E), E = T_ref^-1 T_mov Z^-1, each linear system by conjugate gradients preconditioned with
// the Cholesky factors of the 6x6 diagonal blocks.  The SE(2) bank's algorithm (csrc/ndt_pgo.hip) with 6x6 blocks.
//
// ndt_pgo3_kernel: ONE workgroup of NDT_PGO3_THREADS optimises ONE graph from start to finish; `count` graphs are `count`
// workgroups that never look at each other.  Inside a workgroup only __syncthreads orders the passes: no grid barrier, no
// queue, no spin on memory, no atomics.  Every sum is taken in one fixed order -- a thread's strided items in ascending order,
// then over the workgroup in the order of ndt_block.h; a node's incident edges in ascending edge order -- so a graph's result
// is the same bits whichever batch it runs in.
//   linearisation (once per Gauss-Newton iteration): a thread per edge (strided; the prior is the edge behind the last) writes
//     the 39 numbers both Jacobian blocks are made of and W e; a thread per node gathers its gradient and its 6x6 diagonal block
//     over the node's incident edges (CSR adjacency built by the host) and factors the block.
//   matrix-vector product: a per-edge pass t_e = W (J_ref p_ref + J_mov p_mov), then a per-node gather sum J^T t_e.
// A node is always handled by the same thread, so the vector updates between the passes need no barrier.  The vectors live in a
// per-graph scratch area in device memory (69 doubles per node, 45 per edge), LDS holds the reductions' partial sums.
//
// 512 threads, not the SE(2) kernel's 1024: the linearisation holds four 3x3 matrices beside the poses and the measurement, the
// gather a column of J^T W J and then the 6x6 Cholesky factor, and with 1024 threads -- 128 VGPRs a thread -- the compiler spills
// 204 VGPRs to scratch memory; with 512 threads (up to 256 VGPRs) the kernel takes 228, has no VGPR spill and no private segment
// (tools/kernel_resources.py pgo3 prints the figures).  The gather sums its block in the node's scratch, not in registers, and
// the linearisation stores each Jacobian block as soon as it is known, for the same reason.
#include "ndt_pgo3.h"
#include "ndt_pgo_marginals.h"
#include "ndt_block.h"

typedef NdtBlockSums<NDT_PGO3_WAVES, 2> Pgo3Red;

// per edge: error, Jacobian numbers, W e.  Returns the graph's cost sum e^T W e (prior included) in every thread, `half` where
// a factor's residual rotation is a half turn; its barrier is the one that makes jac / te visible to the gather.
__device__ double pgo3_linearise(const Pgo3Graph &G, const NdtPgo3ParamsDev &prm, Pgo3Red &red, int &par, bool &half)
{
    bool mine = false;
    double s[2] = {0.0, 0.0};
    for (unsigned e = threadIdx.x; e <= G.E; e += NDT_PGO3_THREADS) s[0] += pgo3_linearise_link(G, prm, e, mine);
    s[1] = mine ? 1.0 : 0.0;
    ndt_block_sum(s, red, par);
    half = s[1] > 0.0;
    return s[0];
}

// Solves (J^T W J) x = b by preconditioned conjugate gradients from x = 0; returns the iterations taken, `capped` where it
// stopped at max_linear_iterations with the relative residual still above eps_linear.
__device__ int pgo3_solve(const Pgo3Graph &G, const NdtPgo3ParamsDev &prm, Pgo3Red &red, int &par, bool &capped)
{
    double dot[2] = {0.0, 0.0};                          // r.z and r.r
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) {
        const size_t o = 6 * (size_t)i;
        double r[6], z[6];
        for (int d = 0; d < 6; d++) r[d] = G.b[o + d];
        pgo3_precondition(G, i, r, z);
        for (int d = 0; d < 6; d++) {
            G.x[o + d] = 0.0;
            G.r[o + d] = r[d];
            G.p[o + d] = z[d];
        }
        dot[0] += pgo3_dot6(r, z);
        dot[1] += pgo3_dot6(r, r);
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
        for (unsigned e = threadIdx.x; e < G.E; e += NDT_PGO3_THREADS) pgo3_link_product(G, e);
        __syncthreads();
        double pap = 0.0;
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) {
            const size_t o = 6 * (size_t)i;
            double p[6], ap[6];
            for (int d = 0; d < 6; d++) p[d] = G.p[o + d];
            pgo3_node_product(G, prm, i, p, ap);
            for (int d = 0; d < 6; d++) G.ap[o + d] = ap[d];
            pap += pgo3_dot6(p, ap);
        }
        pap = ndt_block_sum(pap, red, par);
        if (!(pap > 0.0)) break;                         // (not positive definite, or not finite: the iterate so far is the step)
        const double alpha = rz / pap;
        dot[0] = dot[1] = 0.0;
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) {
            const size_t o = 6 * (size_t)i;
            double r[6], z[6];
            for (int d = 0; d < 6; d++) {
                G.x[o + d] += alpha * G.p[o + d];
                r[d] = G.r[o + d] - alpha * G.ap[o + d];
                G.r[o + d] = r[d];
            }
            pgo3_precondition(G, i, r, z);
            for (int d = 0; d < 6; d++) G.z[o + d] = z[d];
            dot[0] += pgo3_dot6(r, z);
            dot[1] += pgo3_dot6(r, r);
        }
        ndt_block_sum(dot, red, par);                    // (its barrier: every edge has read the old p)
        const double beta = dot[0] / rz;
        rz = dot[0];
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) {
            const size_t o = 6 * (size_t)i;
            for (int d = 0; d < 6; d++) G.p[o + d] = G.z[o + d] + beta * G.p[o + d];
        }
        __syncthreads();
        k++;
    }
    return k;
}

__global__ __launch_bounds__(NDT_PGO3_THREADS) void ndt_pgo3_kernel(NdtPgo3View v, size_t first, NdtPgo3ParamsDev prm)
{
    __shared__ Pgo3Red red;
    int par = 0;
    const size_t g = first + blockIdx.x;
    ndtgpu_pgo_result *out = v.state + g;
    const Pgo3Graph G = ndt_pgo3_graph(v, g, (unsigned)out->n_nodes, (unsigned)out->n_edges);

    int exit_code = NDTGPU_PGO_CONVERGED, iterations = 0, linear = 0;
    bool any_capped = false, half;
    double max_step = 0.0;
    double cost = pgo3_linearise(G, prm, red, par, half);
    const double cost_initial = cost;
    if (half) {
        exit_code = NDTGPU_PGO3_HALF_TURN;
    } else if (!(cost - cost == 0.0)) {
        exit_code = NDTGPU_PGO_NOT_FINITE;
    } else {
        for (;;) {
            if (iterations >= prm.max_iterations) {
                exit_code = NDTGPU_PGO_MAX_ITERATIONS;
                break;
            }
            for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) pgo3_gather_node(G, prm, i);
            bool capped;
            linear += pgo3_solve(G, prm, red, par, capped);
            any_capped = any_capped || capped;
            double step = 0.0;
            for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) {
                double *P = G.pose + 12 * (size_t)i, *prev = G.prev + 12 * (size_t)i;
                double d[6];
                for (int k = 0; k < 6; k++) {
                    d[k] = G.x[6 * (size_t)i + k];
                    step = fmax(step, fabs(d[k]));
                }
                for (int k = 0; k < 12; k++) prev[k] = P[k];
                pgo3_retract(prev, d, P);
            }
            max_step = ndt_block_max(step, red, par);    // (its barrier: the new poses are visible to the edge pass)
            iterations++;
            const double cost_new = pgo3_linearise(G, prm, red, par, half);
            if (!(cost_new - cost_new == 0.0)) {         // the step left the finite numbers (or met a half turn): back to the last iterate
                for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS)
                    for (int k = 0; k < 12; k++) G.pose[12 * (size_t)i + k] = G.prev[12 * (size_t)i + k];
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

__global__ void ndt_pgo3_links_kernel(NdtPgo3View v, size_t g, unsigned n_edges, const double *T16, const double *cov36, const int32_t *flags)
{
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    double Z16[16], W36[36];
    ndt_pgo3_link_from_registration(T16 + 16 * (size_t)e, cov36 ? cov36 + 36 * (size_t)e : nullptr, (cov36 && flags) ? flags[e] : 0, Z16, W36);
    pgo3_from_T16(Z16, v.meas + (g * v.max_edges + e) * 12);
    pgo3_sym21(W36, v.info + (g * v.max_edges + e) * 21);
}

// ---- marginal covariances (include/ndtgpu.h, ndtgpu_pgo3_marginals): the structure of csrc/ndt_pgo.hip's, with 6x6 blocks ----
// prepare: one workgroup per graph named linearises it at the held poses into the marginals' own workspace; solve: one workgroup
// and one slot per column, pgo3_solve as it is on the unit vector; finish: ndt_pgo_marginal_finish_kernel<6> (csrc/ndt_pgo.hip).

__global__ __launch_bounds__(NDT_PGO3_THREADS) void ndt_pgo3_marginal_prepare_kernel(NdtPgo3View v, NdtPgoMarginalWork w, NdtPgo3ParamsDev prm)
{
    __shared__ Pgo3Red red;
    int par = 0;
    const size_t g = (size_t)w.area_graph[blockIdx.x];
    const ndtgpu_pgo_result *st = v.state + g;
    Pgo3Graph G = ndt_pgo3_graph(v, g, (unsigned)st->n_nodes, (unsigned)st->n_edges);
    ndt_pgo3_marginal_area(G, w.areas + blockIdx.x * w.area_doubles, v.max_nodes, v.max_edges);
    bool half;
    const double cost = pgo3_linearise(G, prm, red, par, half);
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS) pgo3_gather_node(G, prm, i);
    if (threadIdx.x == 0)
        w.verdict[blockIdx.x] = half ? NDTGPU_PGO3_HALF_TURN : (cost - cost == 0.0) ? NDTGPU_PGO_CONVERGED : NDTGPU_PGO_NOT_FINITE;
}

__global__ __launch_bounds__(NDT_PGO3_THREADS) void ndt_pgo3_marginal_solve_kernel(NdtPgo3View v, NdtPgoMarginalWork w, unsigned first,
                                                                                   NdtPgo3ParamsDev prm)
{
    __shared__ Pgo3Red red;
    int par = 0;
    const unsigned col = first + blockIdx.x, q = col / 6, k = col % 6;
    const NdtPgoMarginalQuery Q = w.query[q];
    if (w.verdict[Q.area] != NDTGPU_PGO_CONVERGED) return;       // (the whole workgroup: finish writes NaN)
    const ndtgpu_pgo_result *st = v.state + Q.graph;
    Pgo3Graph G = ndt_pgo3_graph(v, (size_t)Q.graph, (unsigned)st->n_nodes, (unsigned)st->n_edges);
    ndt_pgo3_marginal_slot(G, w.areas + Q.area * w.area_doubles, w.slots + blockIdx.x * w.slot_doubles, v.max_nodes, v.max_edges);
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO3_THREADS)
        for (unsigned d = 0; d < 6; d++) G.b[6 * (size_t)i + d] = (i == (unsigned)Q.node && d == k) ? 1.0 : 0.0;
    bool capped;
    const int iterations = pgo3_solve(G, prm, red, par, capped); // (a node's b is read by the thread that wrote it)
    __syncthreads();
    double *raw = w.raw + 72 * (size_t)q;
    if (threadIdx.x < 6) raw[6 * threadIdx.x + k] = G.x[6 * (size_t)Q.node + threadIdx.x];
    else if (threadIdx.x < 12 && Q.other >= 0) raw[36 + 6 * (threadIdx.x - 6) + k] = G.x[6 * (size_t)Q.other + threadIdx.x - 6];
    if (threadIdx.x == 0) w.col[col] = NdtPgoMarginalCol{iterations, capped ? 1 : 0};
}

hipError_t ndt_pgo3_marginal_launch_prepare(const NdtPgo3View &v, const NdtPgoMarginalWork &w, size_t n_areas, const NdtPgo3ParamsDev &prm, hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo3_marginal_prepare_kernel, dim3((unsigned)n_areas), dim3(NDT_PGO3_THREADS), 0, st, v, w, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo3_marginal_launch_solve(const NdtPgo3View &v, const NdtPgoMarginalWork &w, size_t first, size_t count,
                                          const NdtPgo3ParamsDev &prm, hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo3_marginal_solve_kernel, dim3((unsigned)count), dim3(NDT_PGO3_THREADS), 0, st, v, w, (unsigned)first, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo3_launch(const NdtPgo3View &v, size_t first, size_t count, const NdtPgo3ParamsDev &prm, hipStream_t st)
{
    hipLaunchKernelGGL(ndt_pgo3_kernel, dim3((unsigned)count), dim3(NDT_PGO3_THREADS), 0, st, v, first, prm);
    return hipGetLastError();
}

hipError_t ndt_pgo3_launch_links(const NdtPgo3View &v, size_t g, size_t n_edges, const double *T16_dev, const double *cov36_dev,
                                 const int32_t *cov_flags_dev, hipStream_t st)
{
    if (!n_edges) return hipSuccess;
    hipLaunchKernelGGL(ndt_pgo3_links_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st, v, g, (unsigned)n_edges, T16_dev,
                       cov36_dev, cov_flags_dev);
    return hipGetLastError();
}
