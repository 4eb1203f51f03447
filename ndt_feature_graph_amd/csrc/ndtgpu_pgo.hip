// ndtgpu_pgo.hip -- C-ABI (include/ndtgpu.h) of the SE(2) pose-graph optimiser: optimizeGraphUsingISAM
// (ndt_feature/include/ndt_feature/ndt_offline_mapper.h:40-107; call site ndt_feature/src/ndt_feature_graph_opt.cpp:152-164) for
// a bank of independent graphs.  Host side only: the handle, the checks of a graph (index range, self links, connectivity by
// union-find), the node-to-edge adjacency and the order of the launches; the optimisation runs in csrc/ndt_pgo.hip and, for one
// large graph spread over the device with the host steering the phases (ndtgpu_pgo_optimize_wide), in csrc/ndt_pgo_wide.hip.
#include "ndtgpu_host.h"
#include "ndt_pgo.h"
#include "ndt_pgo_wide.h"
#include "ndtgpu_pgo_graph.h"
#include "ndtgpu_pgo_marginals.h"
#include "ndtgpu_pgo_bank.h"           // the handle, the device form of the parameters

extern "C" {

void ndtgpu_default_pgo_params(ndtgpu_pgo_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // the stop rule is ours, not iSAM's
    p->max_iterations = 50;
    p->max_linear_iterations = 2000;
    p->eps_step = 1e-8;
    p->eps_linear = 1e-8;
    p->prior_information[0] = p->prior_information[4] = p->prior_information[8] = 100.0;   // ndt_offline_mapper.h:45, :61
}

ndtgpu_status ndtgpu_pgo_destroy(ndtgpu_pgo *h) { return handle_destroy(h, "pgo_destroy"); }

ndtgpu_status ndtgpu_pgo_create(size_t n_graphs, size_t max_nodes, size_t max_edges, ndtgpu_pgo **out)
{
    if (!out) return fail(NDTGPU_ERR_INVALID, "pgo_create: out is NULL");
    *out = nullptr;
    if (n_graphs == 0 || n_graphs > (1u << 24) || max_nodes == 0 || max_nodes > (1u << 24) || max_edges > (1u << 27))
        return fail(NDTGPU_ERR_INVALID, "pgo_create: n_graphs and max_nodes must be 1 .. 2^24, max_edges <= 2^27");
    ndtgpu_pgo *h;
    const ndtgpu_status rc = handle_new("pgo_create", h);
    if (rc != NDTGPU_OK) return rc;
    h->G = n_graphs;
    h->n_nodes.assign(n_graphs, 0);
    h->n_edges.assign(n_graphs, 0);
    NdtPgoView &v = h->v;
    v.max_nodes = max_nodes;
    v.max_edges = max_edges;
    const size_t G = n_graphs, E = std::max<size_t>(max_edges, 1);     // (no zero-byte allocations)
#define TRY(expr) CREATE_TRY(h, NDTGPU_ERR_ALLOC, "pgo_create: device buffers", expr)
    TRY(h->state.alloc(G, &v.state));
    TRY(h->pose.alloc(G * 3 * max_nodes, &v.pose));
    TRY(h->origin.alloc(G * 3, &v.origin));
    TRY(h->ref.alloc(G * E, &v.ref));
    TRY(h->mov.alloc(G * E, &v.mov));
    TRY(h->meas.alloc(G * 3 * E, &v.meas));
    TRY(h->info.alloc(G * 6 * E, &v.info));
    TRY(h->adj_off.alloc(G * (max_nodes + 1), &v.adj_off));
    TRY(h->adj.alloc(G * 2 * E, &v.adj));
    TRY(h->jac.alloc(G * 4 * E, &v.jac));
    TRY(h->te.alloc(G * 3 * E, &v.te));
    TRY(h->node.alloc(G * NDT_PGO_NODE_DOUBLES * max_nodes, &v.node));
    TRY(hipMemset(v.state, 0, G * sizeof(ndtgpu_pgo_result)));
    TRY(h->used.create());
    TRY(h->hst.create(hipStreamNonBlocking));
#undef TRY
    *out = h;
    return NDTGPU_OK;
}

// poses, indices and the adjacency of graph g onto the device, on the handle's stream behind its previous call; meas / info are
// the caller's to fill on the same stream before pgo_installed
static ndtgpu_status pgo_install(ndtgpu_pgo *h, const char *what, size_t g, size_t n_nodes, const double *pose3, size_t n_edges,
                                 const uint32_t *ref_idx, const uint32_t *mov_idx)
{
    if (g >= h->G) return fail_in(NDTGPU_ERR_INVALID, what, "graph index out of range");
    if (n_nodes > h->v.max_nodes || n_edges > h->v.max_edges)
        return fail_in(NDTGPU_ERR_CAPACITY, what, "more nodes or links than the handle was created for");
    // (values that are not finite are not refused here: the kernel reports NDTGPU_PGO_NOT_FINITE for that graph)
    std::vector<uint32_t> off, adj;
    pgo_adjacency(n_nodes, n_edges, ref_idx, mov_idx, off, adj);
    std::vector<int32_t> ri(ref_idx, ref_idx + n_edges), mi(mov_idx, mov_idx + n_edges);
    ndtgpu_pgo_result st{};
    st.n_nodes = (int32_t)n_nodes;
    st.n_edges = (int32_t)n_edges;
    const NdtPgoView &v = h->v;
    h->n_nodes[g] = 0;
    h->n_edges[g] = (uint32_t)n_edges;
    h->robust.invalidate(g);               // (the robust calls' copy of the information as set)
    HIP_TRY(h->used.order(h->hst.get()));
    HIP_TRY(hipMemcpyAsync(v.pose + g * 3 * v.max_nodes, pose3, 3 * n_nodes * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
    HIP_TRY(hipMemcpyAsync(v.origin + g * 3, pose3, 3 * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
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

static ndtgpu_status pgo_installed(ndtgpu_pgo *h, size_t g, size_t n_nodes)
{
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    h->n_nodes[g] = (uint32_t)n_nodes;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo_set_graph(ndtgpu_pgo *h, size_t g, size_t n_nodes, const double *pose3, size_t n_edges,
                                   const uint32_t *ref_idx, const uint32_t *mov_idx, const double *meas3, const double *info9)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_set_graph: null handle");
    if (n_edges && !meas3) return fail(NDTGPU_ERR_INVALID, "pgo_set_graph: meas3 is required");
    ndtgpu_status rc = pgo_check_graph("pgo_set_graph", n_nodes, pose3, n_edges, ref_idx, mov_idx);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = pgo_install(h, "pgo_set_graph", g, n_nodes, pose3, n_edges, ref_idx, mov_idx)) != NDTGPU_OK) return rc;
    if (n_edges) {
        std::vector<double> W(6 * n_edges);
        static const double I100[9] = {100, 0, 0, 0, 100, 0, 0, 0, 100};
        for (size_t e = 0; e < n_edges; e++) sym6(info9 ? info9 + 9 * e : I100, &W[6 * e]);
        const NdtPgoView &v = h->v;
        HIP_TRY(hipMemcpyAsync(v.meas + g * 3 * v.max_edges, meas3, 3 * n_edges * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipMemcpyAsync(v.info + g * 6 * v.max_edges, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, h->hst.get()));
        HIP_TRY(hipStreamSynchronize(h->hst.get()));
    }
    return pgo_installed(h, g, n_nodes);
}

ndtgpu_status ndtgpu_pgo_set_links_device(ndtgpu_pgo *h, size_t g, size_t n_nodes, const double *pose3, size_t n_edges,
                                          const uint32_t *ref_idx, const uint32_t *mov_idx, const double *T16_dev,
                                          const double *cov36_dev, const int32_t *cov_flags_dev)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_set_links_device: null handle");
    if (n_edges && (!T16_dev || (cov36_dev && !cov_flags_dev)))
        return fail(NDTGPU_ERR_INVALID, "pgo_set_links_device: T16_dev is required, and cov_flags_dev with cov36_dev");
    ndtgpu_status rc = pgo_check_graph("pgo_set_links_device", n_nodes, pose3, n_edges, ref_idx, mov_idx);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = pgo_install(h, "pgo_set_links_device", g, n_nodes, pose3, n_edges, ref_idx, mov_idx)) != NDTGPU_OK) return rc;
    hipError_t e = ndt_pgo_launch_links(h->v, g, n_edges, T16_dev, cov36_dev, cov_flags_dev, h->hst.get());
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pgo_set_links_device: launch", e);
    return pgo_installed(h, g, n_nodes);
}

ndtgpu_status ndtgpu_pgo_optimize(ndtgpu_pgo *h, size_t first, size_t count, const ndtgpu_pgo_params *prm, ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_optimize: null handle");
    if (count == 0 || first >= h->G || count > h->G - first)
        return fail(NDTGPU_ERR_INVALID, "pgo_optimize: graphs [first, first + count) out of range");
    NdtPgoParamsDev d;
    if (!pgo_params_dev(prm, d)) return fail(NDTGPU_ERR_INVALID, "pgo_optimize: bad parameter (caps and tolerances >= 0, a finite prior)");
    for (size_t g = first; g < first + count; g++)
        if (!h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo_optimize: a graph of the range has not been set");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(h->used.order(st));   // (the previous call may have run on another stream)
    hipError_t e = ndt_pgo_launch(h->v, first, count, d, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "pgo_optimize: launch", e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo_poses(ndtgpu_pgo *h, size_t g, double *pose3_out, double *T16_out, ndtgpu_pgo_result *result)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_poses: null handle");
    if (g >= h->G || !h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo_poses: no such graph, or it has not been set");
    HIP_TRY(h->used.sync());
    const size_t n = h->n_nodes[g];
    std::vector<double> p(3 * n);
    HIP_TRY(hipMemcpy(p.data(), h->v.pose + g * 3 * h->v.max_nodes, p.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (pose3_out) memcpy(pose3_out, p.data(), p.size() * sizeof(double));
    if (T16_out)
        for (size_t i = 0; i < n; i++) {                 // convertIsamPose2dToEigenAffine3d: Translation(x, y, 0) * Rz(t)
            double *T = T16_out + 16 * i;
            const double c = std::cos(p[3 * i + 2]), s = std::sin(p[3 * i + 2]);
            for (int k = 0; k < 16; k++) T[k] = 0.0;
            T[0] = c; T[1] = s; T[4] = -s; T[5] = c; T[10] = 1.0;
            T[12] = p[3 * i]; T[13] = p[3 * i + 1]; T[15] = 1.0;
        }
    if (result) HIP_TRY(hipMemcpy(result, h->v.state + g, sizeof *result, hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

void ndtgpu_default_pgo_wide_params(ndtgpu_pgo_wide_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->check_every = 32;
}

ndtgpu_status ndtgpu_pgo_wide_plan(size_t n_nodes, size_t n_edges, uint32_t *tile, size_t *node_tiles, size_t *edge_tiles, size_t *extra_bytes)
{
    if (n_nodes == 0 || n_nodes > (1u << 24) || n_edges > (1u << 27))
        return fail(NDTGPU_ERR_INVALID, "pgo_wide_plan: n_nodes must be 1 .. 2^24, n_edges <= 2^27");
    if (tile) *tile = NDT_PGO_WIDE_TILE;
    if (node_tiles) *node_tiles = ndt_pgo_wide_tiles(n_nodes);
    if (edge_tiles) *edge_tiles = ndt_pgo_wide_tiles(n_edges);
    if (extra_bytes) *extra_bytes = ndt_pgo_wide_partials(n_nodes, n_edges) * sizeof(double) + 2 * sizeof(NdtPgoWideCtl);
    return NDTGPU_OK;
}

// The host steers the phases (ndt_pgo_wide_steer, csrc/ndt_pgo_wide_core.h): it enqueues the passes of ndt_pgo_wide.hip on
// `stream` one launch each, and after every chunk of check_every inner iterations -- and after every cost assessment -- copies
// the control block to pinned memory and waits for it.  Launches enqueued past a stop do nothing, so the result does not depend
// on check_every.
ndtgpu_status ndtgpu_pgo_optimize_wide(ndtgpu_pgo *h, size_t g, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_wide_params *wide,
                                       ndtgpu_stream stream)
{
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_wide: null handle");
    const ndtgpu_pgo_wide_params wp = params_or_default(wide, ndtgpu_default_pgo_wide_params);
    NdtPgoWide W{};
    if (!pgo_params_dev(prm, W.prm))
        return fail(NDTGPU_ERR_INVALID, "pgo_optimize_wide: bad parameter (caps and tolerances >= 0, a finite prior)");
    if (wp.check_every < 1) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_wide: check_every must be >= 1");
    if (g >= h->G || !h->n_nodes[g]) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_wide: no such graph, or it has not been set");
    const NdtPgoView &v = h->v;
    hipStream_t st = (hipStream_t)stream;
    if (!h->wide_ctl.get()) {
        HIP_TRY(h->wide_part.alloc(ndt_pgo_wide_partials(v.max_nodes, v.max_edges)));
        HIP_TRY(h->wide_mirror.alloc(1));
        HIP_TRY(h->wide_ctl.alloc(2));
    }
    const size_t N = h->n_nodes[g], E = h->n_edges[g];
    W.G = ndt_pgo_graph(v, g, (unsigned)N, (unsigned)E);
    W.node_tiles = (unsigned)ndt_pgo_wide_tiles(N);
    W.edge_tiles = (unsigned)ndt_pgo_wide_tiles(E);
    W.part_dot = h->wide_part.get();
    W.part_pap = W.part_dot + 2 * (size_t)W.node_tiles;
    W.part_step = W.part_pap + W.node_tiles;
    W.part_cost = W.part_step + W.node_tiles;
    W.out = v.state + g;
    // (a launch with a grid of no workgroups is an error: a graph without links has no link passes)
    auto launch = [&](NdtPgoWidePass what, const NdtPgoWideCtl *src, NdtPgoWideCtl *dst) -> hipError_t {
        if (ndt_pgo_wide_is_link_pass(what) && !E) return hipSuccess;
        W.src = src;
        W.dst = dst;
        return ndt_pgo_wide_launch(what, W, st);
    };
    HIP_TRY(h->used.order(st));            // (the previous call may have run on another stream)
    HIP_TRY(ndt_pgo_wide_steer(launch, h->wide_ctl.get(), h->wide_mirror.get(), wp.check_every, st));
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

// ---- marginal covariances (csrc/ndtgpu_pgo_marginals.h holds what the two banks share) ----

void ndtgpu_default_pgo_marginal_params(ndtgpu_pgo_marginal_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_workspace_bytes = (uint64_t)1 << 30;      // ours: every column of a 500-node graph of either bank in one launch
}

ndtgpu_status ndtgpu_pgo_marginal_plan(size_t max_nodes, size_t max_edges, size_t n_queries, int32_t dof, uint64_t max_workspace_bytes,
                                       size_t *slot_bytes, size_t *slots, size_t *launches)
{
    size_t sb, sl, la;
    if (!ndt_pgo_marginal_plan(max_nodes, max_edges, n_queries, dof, max_workspace_bytes, sb, sl, la))
        return fail(NDTGPU_ERR_INVALID, "pgo_marginal_plan: dof must be 3 or 6, max_nodes 1 .. 2^24, max_edges and n_queries <= 2^27");
    if (slot_bytes) *slot_bytes = sb;
    if (slots) *slots = sl;
    if (launches) *launches = la;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo_relative_covariance(const double *pose_ref3, const double *pose_mov3, const double *cov_ref9, const double *cov_mov9,
                                             const double *cross9, double *out9)
{
    if (!pose_ref3 || !pose_mov3 || !cov_ref9 || !cov_mov9 || !cross9 || !out9)
        return fail(NDTGPU_ERR_INVALID, "pgo_relative_covariance: null argument");
    ndt_pgo_relative_covariance(pose_ref3, pose_mov3, cov_ref9, cov_mov9, cross9, out9);
    return NDTGPU_OK;
}

// the checks of a marginals call that need no handle, and the device form of its parameters
static ndtgpu_status pgo_marginal_args(const char *who, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                       const uint32_t *other_idx, const ndtgpu_pgo_params *prm, const void *cov, const void *cross,
                                       const void *results, NdtPgoParamsDev &d)
{
    const ndtgpu_pgo_params p = params_or_default(prm, ndtgpu_default_pgo_params);
    (void)pgo_params_dev(&p, d);           // (its verdict covers fields this call ignores: the three it reads are checked below)
    bool finite = true;
    for (double w : p.prior_information) finite = finite && std::isfinite(w);
    return pgo_marginal_check_args(who, n_queries, graph_idx, node_idx, other_idx, cov, cross, results, p.eps_linear, p.max_linear_iterations, finite);
}

ndtgpu_status ndtgpu_pgo_marginals_device(ndtgpu_pgo *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                          const uint32_t *other_idx, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                          double *cov9_dev, double *cross9_dev, ndtgpu_pgo_marginal_result *results_dev, ndtgpu_stream stream)
{
    NdtPgoParamsDev d;
    const ndtgpu_status rc = pgo_marginal_args("pgo_marginals_device", n_queries, graph_idx, node_idx, other_idx, prm, cov9_dev, cross9_dev, results_dev, d);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_marginals_device: null handle");
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](int phase, const NdtPgoMarginalWork &w, size_t first, size_t count) -> hipError_t {
        return phase == 0 ? ndt_pgo_marginal_launch_prepare(h->v, w, count, d, st) : ndt_pgo_marginal_launch_solve(h->v, w, first, count, d, st);
    };
    HIP_TRY(h->used.order(st));            // (the previous call may have run on another stream)
    return pgo_marginals_device_core<3>(h, h->marginal, "pgo_marginals_device", n_queries, graph_idx, node_idx, other_idx, mprm, cov9_dev,
                                        cross9_dev, results_dev, st, launch);
}

ndtgpu_status ndtgpu_pgo_marginals(ndtgpu_pgo *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                   const uint32_t *other_idx, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                   double *cov9_out, double *cross9_out, ndtgpu_pgo_marginal_result *results_out)
{
    NdtPgoParamsDev d;
    const ndtgpu_status rc = pgo_marginal_args("pgo_marginals", n_queries, graph_idx, node_idx, other_idx, prm, cov9_out, cross9_out, results_out, d);
    if (rc != NDTGPU_OK) return rc;
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_marginals: null handle");
    return pgo_marginals_host_core<3>(h, h->marginal, "pgo_marginals", n_queries, other_idx != nullptr, cov9_out, cross9_out, results_out,
                                      [&](double *cov_dev, double *cross_dev, ndtgpu_pgo_marginal_result *res_dev, hipStream_t st) {
                                          return ndtgpu_pgo_marginals_device(h, n_queries, graph_idx, node_idx, other_idx, prm, mprm, cov_dev,
                                                                             cross_dev, res_dev, (ndtgpu_stream)st);
                                      });
}

}   // extern "C"
