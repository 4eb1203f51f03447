// ndtgpu_pgo3.hip -- C-ABI (include/ndtgpu.h) of the SE(3) pose-graph optimiser: the back end of the 6-DoF links
// (link.T and link.cov_3d, ndt_feature_graph.cpp:296-330) for a bank of independent graphs.  Host side only: the handle, the
// checks of a graph (csrc/ndtgpu_pgo_graph.h, shared with the SE(2) bank), the adjacency and the order of the launches; the
// optimisation runs in csrc/ndt_pgo3.hip and, for one large graph spread over the device with the host steering the phases
// (ndtgpu_pgo3_optimize_wide), in csrc/ndt_pgo3_wide.hip.  The three pure host entries call the same inlines of csrc/ndt_pgo3.h
// as the kernels.
#include "ndtgpu_host.h"
#include "ndt_pgo3.h"
#include "ndt_pgo3_wide.h"
#include "ndtgpu_pgo_graph.h"
#include "ndtgpu_pgo_marginals.h"
#include "ndtgpu_pgo_bank.h"           // the handle, the device form of the parameters

extern "C" {

void ndtgpu_default_pgo3_params(ndtgpu_pgo3_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // the stop rule is that of ndtgpu_default_pgo_params
    p->max_iterations = 50;
    p->max_linear_iterations = 2000;
    p->eps_step = 1e-8;
    p->eps_linear = 1e-8;
    for (int k = 0; k < 6; k++) p->prior_information[7 * k] = 100.0;      // the analogue of ndt_offline_mapper.h:45, :61
}

ndtgpu_status ndtgpu_pgo3_link_error(const double *Ti16, const double *Tj16, const double *Z16, double *e6, double *Jref36, double *Jmov36)
{
    if (!Ti16 || !Tj16 || !Z16 || !e6) return fail(NDTGPU_ERR_INVALID, "pgo3_link_error: Ti16, Tj16, Z16 and e6 are required");
    double Pi[12], Pj[12], Z[12], jac[NDT_PGO3_JAC];
    pgo3_from_T16(Ti16, Pi);
    pgo3_from_T16(Tj16, Pj);
    pgo3_from_T16(Z16, Z);
    if (!pgo3_link_error(Pi, Pj, Z, e6, jac)) return fail(NDTGPU_ERR_INVALID, "pgo3_link_error: the residual rotation is a half turn");
    for (int side = 0; side < 2; side++) {
        double *J = side ? Jmov36 : Jref36;
        if (!J) continue;
        for (int q = 0; q < 6; q++) {
            double col[6];
            pgo3_j_column(side, jac, q, col);
            for (int r = 0; r < 6; r++) J[6 * r + q] = col[r];
        }
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_retract(const double *T16, const double *d6, double *T16_out)
{
    if (!T16 || !d6 || !T16_out) return fail(NDTGPU_ERR_INVALID, "pgo3_retract: null argument");
    double P[12], Q[12];
    pgo3_from_T16(T16, P);
    pgo3_retract(P, d6, Q);
    pgo3_to_T16(Q, T16_out);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_link_from_registration(const double *T16, const double *cov36, int32_t flags, double *Z16, double *W36)
{
    if (!T16 || !Z16 || !W36) return fail(NDTGPU_ERR_INVALID, "pgo3_link_from_registration: T16, Z16 and W36 are required");
    ndt_pgo3_link_from_registration(T16, cov36, flags, Z16, W36);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_destroy(ndtgpu_pgo3 *h) { return handle_destroy(h, "pgo3_destroy"); }

ndtgpu_status ndtgpu_pgo3_create(size_t n_graphs, size_t max_nodes, size_t max_edges, ndtgpu_pgo3 **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "pgo3_create: out is NULL");
    *out = nullptr;
    if (n_graphs == 0 || n_graphs > (1u << 24) || max_nodes == 0 || max_nodes > (1u << 24) || max_edges > (1u << 27))
        return fail(NDTGPU_ERR_INVALID, "pgo3_create: n_graphs and max_nodes must be 1 .. 2^24, max_edges <= 2^27");
    ndtgpu_pgo3 *h;
    const ndtgpu_status rc = handle_new("pgo3_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->G = n_graphs;
    h->n_nodes.assign(n_graphs, 0);
    h->n_edges.assign(n_graphs, 0);
    NdtPgo3View &v = h->v;
    v.max_nodes = max_nodes;
    v.max_edges = max_edges;
    const size_t G = n_graphs, E = std::max<size_t>(max_edges, 1);     // (no zero-byte allocations)
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "pgo3_create: device buffers", expr)
    TRY(h->state.alloc(G, &v.state));
    TRY(h->pose.alloc(G * 12 * max_nodes, &v.pose));
    TRY(h->origin.alloc(G * 24, &v.origin));
    TRY(h->ref.alloc(G * E, &v.ref));
    TRY(h->mov.alloc(G * E, &v.mov));
    TRY(h->meas.alloc(G * 12 * E, &v.meas));
    TRY(h->info.alloc(G * 21 * E, &v.info));
    TRY(h->adj_off.alloc(G * (max_nodes + 1), &v.adj_off));
    TRY(h->adj.alloc(G * 2 * E, &v.adj));
    TRY(h->jac.alloc(G * NDT_PGO3_JAC * (max_edges + 1), &v.jac));
    TRY(h->te.alloc(G * 6 * (max_edges + 1), &v.te));
    TRY(h->node.alloc(G * NDT_PGO3_NODE_DOUBLES * max_nodes, &v.node));
    TRY(hipMemset(v.state, 0, G * sizeof(ndtgpu_pgo_result)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

// poses, indices and the adjacency of graph g onto the device, on the handle's stream behind its previous call; meas / info are
// the caller's to fill on the same stream before pgo3_installed
static ndtgpu_status pgo3_install(ndtgpu_pgo3 *h, const char *what, size_t g, size_t n_nodes, const double *T16_nodes, size_t n_edges,
                                  const uint32_t *ref_idx, const uint32_t *mov_idx)
{
    if (g >= h->G) return fail_in(NDTGPU_ERR_INVALID, what, "graph index out of range");
    if (n_nodes > h->v.max_nodes || n_edges > h->v.max_edges)
        return fail_in(NDTGPU_ERR_CAPACITY, what, "more nodes or links than the handle was created for");
    // (values that are not finite are not refused here: the kernel reports NDTGPU_PGO_NOT_FINITE for that graph)
    std::vector<uint32_t> off, adj;
    pgo_adjacency(n_nodes, n_edges, ref_idx, mov_idx, off, adj);
    std::vector<int32_t> ri(ref_idx, ref_idx + n_edges), mi(mov_idx, mov_idx + n_edges);
    std::vector<double> P(12 * n_nodes);
    for (size_t i = 0; i < n_nodes; i++) pgo3_from_T16(T16_nodes + 16 * i, &P[12 * i]);
    double origin[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    memcpy(origin, P.data(), 12 * sizeof(double));
    ndtgpu_pgo_result st{};
    st.n_nodes = (int32_t)n_nodes;
    st.n_edges = (int32_t)n_edges;
    const NdtPgo3View &v = h->v;
    h->n_nodes[g] = 0;
    h->n_edges[g] = (uint32_t)n_edges;
    h->robust.invalidate(g);               // (the robust calls' copy of the information as set)
    HIP_TRY(h->used.order(h->hst.get()));
    HIP_TRY(hipMemcpyAsync(v.pose + g * 12 * v.max_nodes, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(hipMemcpyAsync(v.origin + g * 24, origin, sizeof origin, hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(hipMemcpyAsync(v.adj_off + g * (v.max_nodes + 1), off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->hst.get()));
    if (n_edges) {
        HIP_TRY(hipMemcpyAsync(v.ref + g * v.max_edges, ri.data(), n_edges * sizeof(int32_t), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipMemcpyAsync(v.mov + g * v.max_edges, mi.data(), n_edges * sizeof(int32_t), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipMemcpyAsync(v.adj + g * 2 * v.max_edges, adj.data(), adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->hst.get()));
    }
    HIP_TRY(hipMemcpyAsync(v.state + g, &st, sizeof st, hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));               // (the staging vectors above end with this function)
    return NDTGPU_OK;
}

static ndtgpu_status pgo3_installed(ndtgpu_pgo3 *h, size_t g, size_t n_nodes)
{
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    h->n_nodes[g] = (uint32_t)n_nodes;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_set_graph(ndtgpu_pgo3 *h, size_t g, size_t n_nodes, const double *T16_nodes, size_t n_edges,
                                    const uint32_t *ref_idx, const uint32_t *mov_idx, const double *Z16, const double *info36)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_set_graph: null handle");
    if (n_edges && !Z16) return fail(NDTGPU_ERR_INVALID, "pgo3_set_graph: Z16 is required");
    ndtgpu_status rc = pgo_check_graph("pgo3_set_graph", n_nodes, T16_nodes, n_edges, ref_idx, mov_idx);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = pgo3_install(h, "pgo3_set_graph", g, n_nodes, T16_nodes, n_edges, ref_idx, mov_idx)) != NDTGPU_OK) return rc;
    if (n_edges) {
        std::vector<double> Z(12 * n_edges), W(21 * n_edges);
        double I100[36] = {};
        for (int k = 0; k < 6; k++) I100[7 * k] = 100.0;
        for (size_t e = 0; e < n_edges; e++) {
            pgo3_from_T16(Z16 + 16 * e, &Z[12 * e]);
            pgo3_sym21(info36 ? info36 + 36 * e : I100, &W[21 * e]);
        }
        const NdtPgo3View &v = h->v;
        HIP_TRY(hipMemcpyAsync(v.meas + g * 12 * v.max_edges, Z.data(), Z.size() * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipMemcpyAsync(v.info + g * 21 * v.max_edges, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipStreamSynchronize(h->hst.get()));
    }
    return pgo3_installed(h, g, n_nodes);
}

ndtgpu_status ndtgpu_pgo3_set_links_device(ndtgpu_pgo3 *h, size_t g, size_t n_nodes, const double *T16_nodes, size_t n_edges,
                                           const uint32_t *ref_idx, const uint32_t *mov_idx, const double *T16_dev,
                                           const double *cov36_dev, const int32_t *cov_flags_dev)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_set_links_device: null handle");
    if (n_edges && (!T16_dev || (cov36_dev && !cov_flags_dev)))
        return fail(NDTGPU_ERR_INVALID, "pgo3_set_links_device: T16_dev is required, and cov_flags_dev with cov36_dev");
    ndtgpu_status rc = pgo_check_graph("pgo3_set_links_device", n_nodes, T16_nodes, n_edges, ref_idx, mov_idx);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = pgo3_install(h, "pgo3_set_links_device", g, n_nodes, T16_nodes, n_edges, ref_idx, mov_idx)) != NDTGPU_OK) return rc;
    hipError_t e = ndt_pgo3_launch_links(h->v, g, n_edges, T16_dev, cov36_dev, cov_flags_dev, h->hst.get());
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pgo3_set_links_device: launch", e);
    return pgo3_installed(h, g, n_nodes);
}

ndtgpu_status ndtgpu_pgo3_optimize(ndtgpu_pgo3 *h, size_t first, size_t count, const ndtgpu_pgo3_params *prm, ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize: null handle");
    if (count == 0 || first >= h->G || count > h->G - first)
        return fail(NDTGPU_ERR_INVALID, "pgo3_optimize: graphs [first, first + count) out of range");
    NdtPgo3ParamsDev d;
    if (!pgo3_params_dev(prm, d)) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize: bad parameter (caps and tolerances >= 0, a finite prior)");
    for (size_t g = first; g < first + count; g++)
        if (!h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize: a graph of the range has not been set");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));   // (the previous call may have run on another stream)
    hipError_t e = ndt_pgo3_launch(h->v, first, count, d, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pgo3_optimize: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_poses(ndtgpu_pgo3 *h, size_t g, double *T16_out, ndtgpu_pgo_result *result)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_poses: null handle");
    if (g >= h->G || !h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo3_poses: no such graph, or it has not been set");
    HIP_TRY(h->used.sync());
    const size_t n = h->n_nodes[g];
    if (T16_out) {
        std::vector<double> P(12 * n);
        HIP_TRY(hipMemcpy(P.data(), h->v.pose + g * 12 * h->v.max_nodes, P.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) pgo3_to_T16(&P[12 * i], T16_out + 16 * i);
    }
    if (result) HIP_TRY(hipMemcpy(result, h->v.state + g, sizeof *result, hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo3_wide_plan(size_t n_nodes, size_t n_edges, uint32_t *tile, size_t *node_tiles, size_t *link_tiles, size_t *extra_bytes)
{
    if (n_nodes == 0 || n_nodes > (1u << 24) || n_edges > (1u << 27))
        return fail(NDTGPU_ERR_INVALID, "pgo3_wide_plan: n_nodes must be 1 .. 2^24, n_edges <= 2^27");
    if (tile) *tile = NDT_PGO_WIDE_TILE;
    if (node_tiles) *node_tiles = ndt_pgo_wide_tiles(n_nodes);
    if (link_tiles) *link_tiles = ndt_pgo3_wide_link_tiles(n_edges);
    if (extra_bytes) *extra_bytes = ndt_pgo3_wide_partials(n_nodes, n_edges) * sizeof(double) + 2 * sizeof(NdtPgoWideCtl);
    return NDTGPU_OK;
}

// The host steers the phases with the SE(2) wide form's loop (ndt_pgo_wide_steer, csrc/ndt_pgo_wide_core.h) over the passes of
// ndt_pgo3_wide.hip.  Every pass is launched for every graph: the link passes run over E + 1 items, the prior included.
ndtgpu_status ndtgpu_pgo3_optimize_wide(ndtgpu_pgo3 *h, size_t g, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_wide_params *wide,
                                        ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_wide: null handle");
    const ndtgpu_pgo_wide_params wp = params_or_default(wide, ndtgpu_default_pgo_wide_params);
    NdtPgo3Wide W{};
    if (!pgo3_params_dev(prm, W.prm))
        return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_wide: bad parameter (caps and tolerances >= 0, a finite prior)");
    if (wp.check_every < 1) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_wide: check_every must be >= 1");
    if (g >= h->G || !h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_wide: no such graph, or it has not been set");
    const NdtPgo3View &v = h->v;
    hipStream_t st = (hipStream_t)stream;
    if (!h->wide_ctl.get()) {
        HIP_TRY(h->wide_part.alloc(ndt_pgo3_wide_partials(v.max_nodes, v.max_edges)));
        HIP_TRY(h->wide_mirror.alloc(1));
        HIP_TRY(h->wide_ctl.alloc(2));
    }
    const size_t N = h->n_nodes[g], E = h->n_edges[g];
    W.G = ndt_pgo3_graph(v, g, (unsigned)N, (unsigned)E);
    W.node_tiles = (unsigned)ndt_pgo_wide_tiles(N);
    W.link_tiles = (unsigned)ndt_pgo3_wide_link_tiles(E);
    W.part_dot = h->wide_part.get();
    W.part_pap = W.part_dot + 2 * (size_t)W.node_tiles;
    W.part_step = W.part_pap + W.node_tiles;
    W.part_cost = W.part_step + W.node_tiles;
    W.out = v.state + g;
    auto launch = [&](NdtPgoWidePass what, const NdtPgoWideCtl *src, NdtPgoWideCtl *dst) -> hipError_t {
        W.src = src;
        W.dst = dst;
        return ndt_pgo3_wide_launch(what, W, st);
    };
    HIP_TRY(h->used.order(st));            // (the previous call may have run on another stream)
    HIP_TRY(ndt_pgo_wide_steer(launch, h->wide_ctl.get(), h->wide_mirror.get(), wp.check_every, st));
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

// ---- marginal covariances (csrc/ndtgpu_pgo_marginals.h holds what the two banks share) ----

ndtgpu_status ndtgpu_pgo3_relative_covariance(const double *Tref16, const double *Tmov16, const double *cov_ref36, const double *cov_mov36,
                                              const double *cross36, double *out36)
{
    if (!Tref16 || !Tmov16 || !cov_ref36 || !cov_mov36 || !cross36 || !out36)
        return fail(NDTGPU_ERR_INVALID, "pgo3_relative_covariance: null argument");
    double Pr[12], Pm[12];
    pgo3_from_T16(Tref16, Pr);
    pgo3_from_T16(Tmov16, Pm);
    if (!ndt_pgo3_relative_covariance(Pr, Pm, cov_ref36, cov_mov36, cross36, out36))
        return fail(NDTGPU_ERR_INVALID, "pgo3_relative_covariance: the relative pose's residual is a half turn (poses that are not finite)");
    return NDTGPU_OK;
}

// the checks of a marginals call that need no handle, and the device form of its parameters
static ndtgpu_status pgo3_marginal_args(const char *who, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                       const uint32_t *other_idx, const ndtgpu_pgo3_params *prm, const void *cov, const void *cross,
                                       const void *results, NdtPgo3ParamsDev &d)
{
    const ndtgpu_pgo3_params p = params_or_default(prm, ndtgpu_default_pgo3_params);
    (void)pgo3_params_dev(&p, d);          // (its verdict covers fields this call ignores: the three it reads are checked below)
    bool finite = true;
    for (double w : p.prior_information) finite = finite && std::isfinite(w);
    return pgo_marginal_check_args(who, n_queries, graph_idx, node_idx, other_idx, cov, cross, results, p.eps_linear, p.max_linear_iterations, finite);
}

ndtgpu_status ndtgpu_pgo3_marginals_device(ndtgpu_pgo3 *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                          const uint32_t *other_idx, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                          double *cov36_dev, double *cross36_dev, ndtgpu_pgo_marginal_result *results_dev, ndtgpu_stream stream)
{
    NdtPgo3ParamsDev d;
    const ndtgpu_status rc = pgo3_marginal_args("pgo3_marginals_device", n_queries, graph_idx, node_idx, other_idx, prm, cov36_dev, cross36_dev, results_dev, d);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_marginals_device: null handle");
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](int phase, const NdtPgoMarginalWork &w, size_t first, size_t count) -> hipError_t {
        return phase == 0 ? ndt_pgo3_marginal_launch_prepare(h->v, w, count, d, st) : ndt_pgo3_marginal_launch_solve(h->v, w, first, count, d, st);
    };
    HIP_TRY(h->used.order(st));            // (the previous call may have run on another stream)
    return pgo_marginals_device_core<6>(h, h->marginal, "pgo3_marginals_device", n_queries, graph_idx, node_idx, other_idx, mprm, cov36_dev,
                                        cross36_dev, results_dev, st, launch);
}

ndtgpu_status ndtgpu_pgo3_marginals(ndtgpu_pgo3 *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                   const uint32_t *other_idx, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                   double *cov36_out, double *cross36_out, ndtgpu_pgo_marginal_result *results_out)
{
    NdtPgo3ParamsDev d;
    const ndtgpu_status rc = pgo3_marginal_args("pgo3_marginals", n_queries, graph_idx, node_idx, other_idx, prm, cov36_out, cross36_out, results_out, d);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_marginals: null handle");
    return pgo_marginals_host_core<6>(h, h->marginal, "pgo3_marginals", n_queries, other_idx != nullptr, cov36_out, cross36_out, results_out,
                                      [&](double *cov_dev, double *cross_dev, ndtgpu_pgo_marginal_result *res_dev, hipStream_t st) {
                                          return ndtgpu_pgo3_marginals_device(h, n_queries, graph_idx, node_idx, other_idx, prm, mprm, cov_dev,
                                                                             cross_dev, res_dev, (ndtgpu_stream)st);
                                      });
}

}   // extern "C"
