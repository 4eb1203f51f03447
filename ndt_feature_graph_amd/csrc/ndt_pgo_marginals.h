// ndt_pgo_marginals.h -- what the marginal-covariance kernels of the two pose-graph banks (csrc/ndt_pgo.hip, csrc/ndt_pgo3.hip:
// ndt_pgo_marginal_* / ndt_pgo3_marginal_*) and their C-ABI (csrc/ndtgpu_pgo.hip, csrc/ndtgpu_pgo3.hip through
// csrc/ndtgpu_pgo_marginals.h) share: the query and column records, the layout of the marginals' own workspace, the plan that cuts
// a call into launches, and the covariance of a link's error from two nodes' marginals.  include/ndtgpu.h ("Marginal covariances
// of the pose-graph banks") states the semantics.
//
// The workspace has two parts, both sized by the bank's capacity as the optimiser's scratch is:
//   an AREA per distinct graph a call names: the linearisation at the held poses (jac), the preconditioner (the inverses of the
//     diagonal blocks, SE(3): their Cholesky factors) and the throw-away te / b of that linearisation.  Written by the prepare
//     launch, read-only afterwards.
//   a SLOT per workgroup of a solve launch: b, x, r, z, p, Ap and t_e of ONE column's conjugate gradients.  The slot is the
//     workgroup's position in its launch; the next launch of the same stream reuses the slots.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_pgo3.h"

// one query of a call, as the kernels read it
struct NdtPgoMarginalQuery {
    int32_t area;                                 // which of the call's areas holds the graph's linearisation
    int32_t graph;                                // the graph, in the bank
    int32_t node;                                 // q
    int32_t other;                                // o, -1: no cross block
};

// what the solve of one column leaves for the finish launch
struct NdtPgoMarginalCol {
    int32_t iterations, capped;
};

// the device side of one call
struct NdtPgoMarginalWork {
    const NdtPgoMarginalQuery *query;             // [n_queries]
    const int32_t *area_graph;                    // [n_areas]  the graph an area is for
    int32_t *verdict;                             // [n_areas]  NDTGPU_PGO_CONVERGED, NDTGPU_PGO_NOT_FINITE or NDTGPU_PGO3_HALF_TURN
    double *areas;                                // [n_areas][area_doubles]
    double *slots;                                // [slots][slot_doubles]
    double *raw;                                  // [n_queries][2 dof dof]  the raw blocks [q, q] and [o, q], row-major
    NdtPgoMarginalCol *col;                       // [n_queries][dof]
    size_t area_doubles, slot_doubles;
    unsigned n_queries;
};

// (the SE(3) arrays jac and te have one more entry than the graph has links: the prior's)
NDT_HD size_t ndt_pgo_marginal_slot_doubles(int dof, size_t max_nodes, size_t max_edges)
{
    return dof == 3 ? 18 * max_nodes + 3 * max_edges : 36 * max_nodes + 6 * (max_edges + 1);
}
NDT_HD size_t ndt_pgo_marginal_area_doubles(int dof, size_t max_nodes, size_t max_edges)
{
    return dof == 3 ? 9 * max_nodes + 7 * max_edges : 27 * max_nodes + (NDT_PGO3_JAC + 6) * (max_edges + 1);
}

// The views.  Both redirect every pointer the linearisation, the gather and the solve WRITE through; pose, origin, ref, mov, meas,
// info and the adjacency stay the bank's, which these passes only read.  What a pass does not use is NULL.
NDT_HD void ndt_pgo_marginal_area(PgoGraph &G, double *a, size_t max_nodes, size_t max_edges)
{
    G.jac = a;
    G.dinv = a + 4 * max_edges;
    G.te = G.dinv + 6 * max_nodes;
    G.b = G.te + 3 * max_edges;
    G.prev = G.x = G.r = G.z = G.p = G.ap = nullptr;
}
NDT_HD void ndt_pgo_marginal_slot(PgoGraph &G, const double *a, double *s, size_t max_nodes, size_t max_edges)
{
    G.jac = const_cast<double *>(a);              // (read by the solve)
    G.dinv = const_cast<double *>(a) + 4 * max_edges;
    G.b = s;
    G.x = s + 3 * max_nodes;
    G.r = s + 6 * max_nodes;
    G.z = s + 9 * max_nodes;
    G.p = s + 12 * max_nodes;
    G.ap = s + 15 * max_nodes;
    G.te = s + 18 * max_nodes;
    G.prev = nullptr;
}
NDT_HD void ndt_pgo3_marginal_area(Pgo3Graph &G, double *a, size_t max_nodes, size_t max_edges)
{
    G.jac = a;
    G.chol = a + NDT_PGO3_JAC * (max_edges + 1);
    G.te = G.chol + 21 * max_nodes;
    G.b = G.te + 6 * (max_edges + 1);
    G.prev = G.x = G.r = G.z = G.p = G.ap = nullptr;
}
NDT_HD void ndt_pgo3_marginal_slot(Pgo3Graph &G, const double *a, double *s, size_t max_nodes, size_t max_edges)
{
    G.jac = const_cast<double *>(a);
    G.chol = const_cast<double *>(a) + NDT_PGO3_JAC * (max_edges + 1);
    G.b = s;
    G.x = s + 6 * max_nodes;
    G.r = s + 12 * max_nodes;
    G.z = s + 18 * max_nodes;
    G.p = s + 24 * max_nodes;
    G.ap = s + 30 * max_nodes;
    G.te = s + 36 * max_nodes;
    G.prev = nullptr;
}

// The plan: how many slots a budget buys (at least one, at most one per column) and how many solve launches the call takes.
// false beyond the limits of ndtgpu_pgo_create or for a dof other than 3 and 6.
inline bool ndt_pgo_marginal_plan(size_t max_nodes, size_t max_edges, size_t n_queries, int dof, uint64_t max_workspace_bytes,
                                  size_t &slot_bytes, size_t &slots, size_t &launches)
{
    if ((dof != 3 && dof != 6) || max_nodes == 0 || max_nodes > (1u << 24) || max_edges > (1u << 27) || n_queries > (1u << 27)) return false;
    slot_bytes = ndt_pgo_marginal_slot_doubles(dof, max_nodes, max_edges) * sizeof(double);
    const size_t columns = n_queries * (size_t)dof;
    uint64_t n = max_workspace_bytes / slot_bytes;
    if (n > columns) n = columns;
    if (n < 1) n = 1;
    slots = (size_t)n;
    launches = (columns + slots - 1) / slots;
    return true;
}

// ---- the covariance of a link's error from the marginals of its two nodes (pure host; the Jacobians are the kernels') ----

// out = J S J^T for J = [J_ref J_mov] (N x 2N, row-major) and S = [[S_rr, S_mr^T], [S_mr, S_mm]]: the four terms
// J_ref S_rr J_ref^T + J_ref S_rm J_mov^T + J_mov S_mr J_ref^T + J_mov S_mm J_mov^T summed in the order of the stacked product,
// every sum from 0.0 in ascending index order, without contraction (tests/pgo_marginals_model.py restates it)
template <int N>
inline void ndt_pgo_jsjt(const double *J, const double *Srr, const double *Smm, const double *Smr, double *out)
{
#pragma clang fp contract(off)
    double S[2 * N][2 * N], M[N][2 * N];
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) {
            S[r][c] = Srr[N * r + c];
            S[N + r][N + c] = Smm[N * r + c];
            S[N + r][c] = Smr[N * r + c];
            S[c][N + r] = Smr[N * r + c];
        }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < 2 * N; j++) {
            double s = 0.0;
            for (int k = 0; k < 2 * N; k++) s = s + J[2 * N * i + k] * S[k][j];
            M[i][j] = s;
        }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            double s = 0.0;
            for (int k = 0; k < 2 * N; k++) s = s + M[i][k] * J[2 * N * j + k];
            out[N * i + j] = s;
        }
}

// SE(2): the Jacobians of pgo_jt's comment at the poses given
inline void ndt_pgo_relative_covariance(const double *pr, const double *pm, const double *Srr, const double *Smm, const double *Smr, double *out9)
{
#pragma clang fp contract(off)
    const double c = cos(pr[2]), s = sin(pr[2]);
    const double dx = pm[0] - pr[0], dy = pm[1] - pr[1];
    const double lx = c * dx + s * dy, ly = -s * dx + c * dy;
    const double J[18] = {-c, -s, ly, c, s, 0.0, s, -c, -lx, -s, c, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 1.0};
    ndt_pgo_jsjt<3>(J, Srr, Smm, Smr, out9);
}

// SE(3): pgo3_link_error's Jacobians with Z = T_ref^-1 T_mov, the current relative pose; false at a half turn (which Z = the
// relative pose itself cannot give short of poses that are not finite)
inline bool ndt_pgo3_relative_covariance(const double *Pr, const double *Pm, const double *Srr, const double *Smm, const double *Smr,
                                         double *out36)
{
    double Z[12], d[3], e[6], jac[NDT_PGO3_JAC], J[72];
    pgo3_mtm(Pr, Pm, Z);
    for (int k = 0; k < 3; k++) d[k] = Pm[9 + k] - Pr[9 + k];
    pgo3_mtv(Pr, d, Z + 9);
    if (!pgo3_link_error(Pr, Pm, Z, e, jac)) return false;
    for (int side = 0; side < 2; side++)
        for (int q = 0; q < 6; q++) {
            double col[6];
            pgo3_j_column(side, jac, q, col);
            for (int r = 0; r < 6; r++) J[12 * r + 6 * side + q] = col[r];
        }
    ndt_pgo_jsjt<6>(J, Srr, Smm, Smr, out36);
    return true;
}

// host launchers (csrc/ndt_pgo.hip, csrc/ndt_pgo3.hip), all plain launches on `st`
// one workgroup per area: the linearisation and the preconditioner at the held poses, and the verdict
hipError_t ndt_pgo_marginal_launch_prepare(const NdtPgoView &v, const NdtPgoMarginalWork &w, size_t n_areas, const NdtPgoParamsDev &prm, hipStream_t st);
hipError_t ndt_pgo3_marginal_launch_prepare(const NdtPgo3View &v, const NdtPgoMarginalWork &w, size_t n_areas, const NdtPgo3ParamsDev &prm, hipStream_t st);
// columns [first, first + count) of the call -- column c is component c % dof of query c / dof --, one workgroup and one slot each
hipError_t ndt_pgo_marginal_launch_solve(const NdtPgoView &v, const NdtPgoMarginalWork &w, size_t first, size_t count, const NdtPgoParamsDev &prm,
                                         hipStream_t st);
hipError_t ndt_pgo3_marginal_launch_solve(const NdtPgo3View &v, const NdtPgoMarginalWork &w, size_t first, size_t count,
                                          const NdtPgo3ParamsDev &prm, hipStream_t st);
// a lane per query: cov, cross (NULL: none) and the result records
hipError_t ndt_pgo_marginal_launch_finish(const NdtPgoMarginalWork &w, int dof, double *cov_dev, double *cross_dev,
                                          ndtgpu_pgo_marginal_result *results_dev, hipStream_t st);
