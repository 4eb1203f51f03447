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
#include "ndt_pgo.h"
#include "ndt_block.h"

typedef NdtBlockSums<NDT_PGO_WAVES, 2> PgoRed;

// y = W x, W symmetric as 6 numbers
__device__ __forceinline__ void pgo_symv(const double *W, double x0, double x1, double x2, double &y0, double &y1, double &y2)
{
    y0 = W[0] * x0 + W[1] * x1 + W[2] * x2;
    y1 = W[1] * x0 + W[3] * x1 + W[4] * x2;
    y2 = W[2] * x0 + W[4] * x1 + W[5] * x2;
}

// The factor's error is e = (p_mov ominus p_ref) - z.  With c, s of t_ref and (lx, ly) = p_mov ominus p_ref's translation:
//   J_ref = [[-c, -s, ly], [s, -c, -lx], [0, 0, -1]]      J_mov = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
// J^T w for the side of the edge the node is on
__device__ __forceinline__ void pgo_jt(int side, double c, double s, double lx, double ly, double w0, double w1, double w2, double &g0,
                                       double &g1, double &g2)
{
    if (side == 0) {
        g0 = -c * w0 + s * w1;
        g1 = -s * w0 - c * w1;
        g2 = ly * w0 - lx * w1 - w2;
    } else {
        g0 = c * w0 - s * w1;
        g1 = s * w0 + c * w1;
        g2 = w2;
    }
}

struct PgoGraph {
    unsigned N, E;
    double *pose;
    const double *origin;
    const int32_t *ref, *mov;
    const double *meas, *info;
    const uint32_t *adj_off, *adj;
    double *jac, *te;
    double *prev, *b, *x, *r, *z, *p, *ap, *dinv;
};

// the prior's error on node 0
__device__ __forceinline__ void pgo_prior_error(const PgoGraph &G, double &e0, double &e1, double &e2)
{
    e0 = G.pose[0] - G.origin[0];
    e1 = G.pose[1] - G.origin[1];
    e2 = ndt_pgo_wrap(G.pose[2] - G.origin[2]);
}

// per edge: error, Jacobian numbers, W e.  Returns the graph's cost sum e^T W e (prior included) in every thread; its barrier
// is the one that makes jac / te visible to the gather.
__device__ double pgo_linearise(const PgoGraph &G, const NdtPgoParamsDev &prm, PgoRed &red, int &par)
{
    double cost = 0.0;
    if (threadIdx.x == 0) {
        double e0, e1, e2, w0, w1, w2;
        pgo_prior_error(G, e0, e1, e2);
        pgo_symv(prm.prior, e0, e1, e2, w0, w1, w2);
        cost = e0 * w0 + e1 * w1 + e2 * w2;
    }
    for (unsigned e = threadIdx.x; e < G.E; e += NDT_PGO_THREADS) {
        const double *pi = G.pose + 3 * (size_t)G.ref[e], *pj = G.pose + 3 * (size_t)G.mov[e];
        double s, c;
        sincos(pi[2], &s, &c);
        const double dx = pj[0] - pi[0], dy = pj[1] - pi[1];
        const double lx = c * dx + s * dy, ly = -s * dx + c * dy;
        const double *zm = G.meas + 3 * (size_t)e;
        const double e0 = lx - zm[0], e1 = ly - zm[1], e2 = ndt_pgo_wrap(ndt_pgo_wrap(pj[2] - pi[2]) - zm[2]);
        double w0, w1, w2;
        pgo_symv(G.info + 6 * (size_t)e, e0, e1, e2, w0, w1, w2);
        double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e;
        j[0] = c; j[1] = s; j[2] = lx; j[3] = ly;
        t[0] = w0; t[1] = w1; t[2] = w2;
        cost += e0 * w0 + e1 * w1 + e2 * w2;
    }
    return ndt_block_sum(cost, red, par);
}

// per node: b = -gradient and the inverse of the 3x3 diagonal block of J^T W J, over the node's incident edges
__device__ void pgo_gather(const PgoGraph &G, const NdtPgoParamsDev &prm)
{
    for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
        double g0 = 0.0, g1 = 0.0, g2 = 0.0, D[6] = {0, 0, 0, 0, 0, 0};
        for (unsigned k = G.adj_off[i]; k < G.adj_off[i + 1]; k++) {
            const unsigned a = G.adj[k], e = a >> 1;
            const int side = (int)(a & 1u);
            const double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e, *W = G.info + 6 * (size_t)e;
            double h0, h1, h2;
            pgo_jt(side, j[0], j[1], j[2], j[3], t[0], t[1], t[2], h0, h1, h2);
            g0 += h0; g1 += h1; g2 += h2;
            // J^T W J: column q of W J, then J^T of it
            const double c = j[0], s = j[1], lx = j[2], ly = j[3];
            const double Jc[3][3] = {{side ? c : -c, side ? -s : s, 0.0}, {side ? s : -s, side ? c : -c, 0.0},
                                     {side ? 0.0 : ly, side ? 0.0 : -lx, side ? 1.0 : -1.0}};   // Jc[q] = column q of J
            double M[3][3];
            for (int q = 0; q < 3; q++) {
                double u0, u1, u2;
                pgo_symv(W, Jc[q][0], Jc[q][1], Jc[q][2], u0, u1, u2);
                pgo_jt(side, c, s, lx, ly, u0, u1, u2, M[0][q], M[1][q], M[2][q]);
            }
            D[0] += M[0][0]; D[1] += M[0][1]; D[2] += M[0][2]; D[3] += M[1][1]; D[4] += M[1][2]; D[5] += M[2][2];
        }
        if (i == 0) {
            double e0, e1, e2, w0, w1, w2;
            pgo_prior_error(G, e0, e1, e2);
            pgo_symv(prm.prior, e0, e1, e2, w0, w1, w2);
            g0 += w0; g1 += w1; g2 += w2;
            for (int k = 0; k < 6; k++) D[k] += prm.prior[k];
        }
        double *b = G.b + 3 * (size_t)i, *di = G.dinv + 6 * (size_t)i;
        b[0] = -g0; b[1] = -g1; b[2] = -g2;
        if (!ndt_pgo_inv_sym3(D[0], D[1], D[2], D[3], D[4], D[5], di)) {      // (an information matrix that is not positive definite)
            di[0] = di[3] = di[5] = 1.0;
            di[1] = di[2] = di[4] = 0.0;
        }
    }
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
        for (unsigned e = threadIdx.x; e < G.E; e += NDT_PGO_THREADS) {
            const double *pi = G.p + 3 * (size_t)G.ref[e], *pj = G.p + 3 * (size_t)G.mov[e], *j = G.jac + 4 * (size_t)e;
            const double c = j[0], s = j[1], lx = j[2], ly = j[3];
            const double u0 = -c * pi[0] - s * pi[1] + ly * pi[2] + c * pj[0] + s * pj[1];
            const double u1 = s * pi[0] - c * pi[1] - lx * pi[2] - s * pj[0] + c * pj[1];
            const double u2 = pj[2] - pi[2];
            double *t = G.te + 3 * (size_t)e;
            pgo_symv(G.info + 6 * (size_t)e, u0, u1, u2, t[0], t[1], t[2]);
        }
        __syncthreads();
        double pap = 0.0;
        for (unsigned i = threadIdx.x; i < G.N; i += NDT_PGO_THREADS) {
            const size_t o = 3 * (size_t)i;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (unsigned q = G.adj_off[i]; q < G.adj_off[i + 1]; q++) {
                const unsigned a = G.adj[q], e = a >> 1;
                const double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e;
                double h0, h1, h2;
                pgo_jt((int)(a & 1u), j[0], j[1], j[2], j[3], t[0], t[1], t[2], h0, h1, h2);
                a0 += h0; a1 += h1; a2 += h2;
            }
            const double p0 = G.p[o], p1 = G.p[o + 1], p2 = G.p[o + 2];
            if (i == 0) {
                double w0, w1, w2;
                pgo_symv(prm.prior, p0, p1, p2, w0, w1, w2);
                a0 += w0; a1 += w1; a2 += w2;
            }
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
    PgoGraph G;
    G.N = (unsigned)out->n_nodes;
    G.E = (unsigned)out->n_edges;
    G.pose = v.pose + g * 3 * v.max_nodes;
    G.origin = v.origin + g * 3;
    G.ref = v.ref + g * v.max_edges;
    G.mov = v.mov + g * v.max_edges;
    G.meas = v.meas + g * 3 * v.max_edges;
    G.info = v.info + g * 6 * v.max_edges;
    G.adj_off = v.adj_off + g * (v.max_nodes + 1);
    G.adj = v.adj + g * 2 * v.max_edges;
    G.jac = v.jac + g * 4 * v.max_edges;
    G.te = v.te + g * 3 * v.max_edges;
    double *nb = v.node + g * NDT_PGO_NODE_DOUBLES * v.max_nodes;
    G.prev = nb;
    G.b = nb + 3 * v.max_nodes;
    G.x = nb + 6 * v.max_nodes;
    G.r = nb + 9 * v.max_nodes;
    G.z = nb + 12 * v.max_nodes;
    G.p = nb + 15 * v.max_nodes;
    G.ap = nb + 18 * v.max_nodes;
    G.dinv = nb + 21 * v.max_nodes;

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
