// ndtgpu_pgo_marginals.h -- the host side of the marginal covariances that csrc/ndtgpu_pgo.hip and csrc/ndtgpu_pgo3.hip share
// (include/ndtgpu.h, "Marginal covariances of the pose-graph banks"): the workspace a handle owns, the checks of a call, the
// order of the three launches (csrc/ndt_pgo_marginals.h) and the staging of the host form.  Host side only, internal.
#pragma once
#include "ndtgpu_host.h"
#include "ndt_pgo_marginals.h"

#include <map>

#pragma GCC visibility push(hidden)

// What a bank's handle owns for its marginals calls: nothing until the first one.  It stands in front of the handle's `used` and
// `hst` (ndtgpu_resource.h: the stream goes first).
struct PgoMarginalSpace {
    DeviceBuffer<double> areas, slots, raw;
    DeviceBuffer<NdtPgoMarginalCol> col;
    DeviceBuffer<int32_t> idx;             // queries | area_graph | verdict
    PinnedBuffer<int32_t> idx_pin;         // queries | area_graph
    HostStage stage;                       // the host form's outputs
};

// the checks that need no handle: the outputs, the index arrays and the three parameters a marginals call reads
inline ndtgpu_status pgo_marginal_check_args(const char *who, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                             const uint32_t *other_idx, const void *cov, const void *cross, const void *results,
                                             double eps_linear, int max_linear_iterations, bool prior_finite)
{
    if (!cov || !results || (other_idx && !cross)) return fail_in(NDTGPU_ERR_INVALID, who, "NULL output (cov, results; cross with other_idx)");
    if (n_queries == 0 || n_queries > (1u << 27) || !graph_idx || !node_idx)
        return fail_in(NDTGPU_ERR_INVALID, who, "n_queries must be 1 .. 2^27, graph_idx and node_idx are required");
    if (!(eps_linear > 0.0) || !std::isfinite(eps_linear)) return fail_in(NDTGPU_ERR_INVALID, who, "eps_linear must be finite and positive");
    if (max_linear_iterations < 1) return fail_in(NDTGPU_ERR_INVALID, who, "max_linear_iterations must be >= 1");
    if (!prior_finite) return fail_in(NDTGPU_ERR_INVALID, who, "prior_information must be finite");
    return NDTGPU_OK;
}

// The _device form of both banks.  `launch(phase, work, first, count)` is the bank's: phase 0 prepare (count areas), 1 solve
// (columns [first, first + count)).  Outputs in device memory, asynchronous on `st`.
template <int DOF, class H, class Launch>
inline ndtgpu_status pgo_marginals_device_core(H *h, PgoMarginalSpace &m, const char *who, size_t n_queries, const uint32_t *graph_idx,
                                               const uint32_t *node_idx, const uint32_t *other_idx, const ndtgpu_pgo_marginal_params *mprm,
                                               double *cov_dev, double *cross_dev, ndtgpu_pgo_marginal_result *results_dev, hipStream_t st,
                                               Launch launch)
{
    const ndtgpu_pgo_marginal_params mp = params_or_default(mprm, ndtgpu_default_pgo_marginal_params);
    std::vector<NdtPgoMarginalQuery> query(n_queries);
    std::vector<int32_t> area_graph;
    std::map<uint32_t, int32_t> area_of;   // (areas in the order the call first names their graphs)
    for (size_t q = 0; q < n_queries; q++) {
        const uint32_t g = graph_idx[q];
        if (g >= h->G || !h->n_nodes[g]) return fail_in(NDTGPU_ERR_INVALID, who, "a query's graph is out of range or has not been set");
        if (node_idx[q] >= h->n_nodes[g] || (other_idx && other_idx[q] >= h->n_nodes[g]))
            return fail_in(NDTGPU_ERR_INVALID, who, "a query's node index is >= n_nodes");
        auto it = area_of.find(g);
        if (it == area_of.end()) {
            it = area_of.emplace(g, (int32_t)area_graph.size()).first;
            area_graph.push_back((int32_t)g);
        }
        query[q] = NdtPgoMarginalQuery{it->second, (int32_t)g, (int32_t)node_idx[q], other_idx ? (int32_t)other_idx[q] : -1};
    }
    const size_t max_nodes = h->v.max_nodes, max_edges = h->v.max_edges, n_areas = area_graph.size(), columns = n_queries * DOF;
    size_t slot_bytes, slots, launches;
    if (!ndt_pgo_marginal_plan(max_nodes, max_edges, n_queries, DOF, mp.max_workspace_bytes, slot_bytes, slots, launches))
        return fail_in(NDTGPU_ERR_INVALID, who, "the plan");
    // the workspace, once the handle's previous call has ended: the blocks may be replaced, and the pinned queries are overwritten
    HIP_TRY(h->used.sync());
    const size_t n_idx = 4 * n_queries + 2 * n_areas;
    NdtPgoMarginalWork w{};
    w.area_doubles = ndt_pgo_marginal_area_doubles(DOF, max_nodes, max_edges);
    w.slot_doubles = slot_bytes / sizeof(double);
    w.n_queries = (unsigned)n_queries;
    if (m.areas.reserve(n_areas * w.area_doubles) != hipSuccess || m.slots.reserve(slots * w.slot_doubles) != hipSuccess ||
        m.raw.reserve(2 * DOF * DOF * n_queries) != hipSuccess || m.col.reserve(columns) != hipSuccess ||
        m.idx.reserve(n_idx) != hipSuccess || m.idx_pin.reserve(n_idx) != hipSuccess)
        return fail_in(NDTGPU_ERR_ALLOC, who, "the marginals' workspace");
    memcpy(m.idx_pin.get(), query.data(), n_queries * sizeof(NdtPgoMarginalQuery));
    memcpy(m.idx_pin.get() + 4 * n_queries, area_graph.data(), n_areas * sizeof(int32_t));
    w.query = reinterpret_cast<const NdtPgoMarginalQuery *>(m.idx.get());
    w.area_graph = m.idx.get() + 4 * n_queries;
    w.verdict = m.idx.get() + 4 * n_queries + n_areas;
    w.areas = m.areas.get();
    w.slots = m.slots.get();
    w.raw = m.raw.get();
    w.col = m.col.get();
    HIP_TRY(hipMemcpyAsync(m.idx.get(), m.idx_pin.get(), (4 * n_queries + n_areas) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    // (a column whose query asks for no cross block leaves that half of raw unwritten: finish does not read it)
    hipError_t e = launch(0, w, (size_t)0, n_areas);
    for (size_t first = 0; e == hipSuccess && first < columns; first += slots) e = launch(1, w, first, std::min(slots, columns - first));
    if (e == hipSuccess) e = ndt_pgo_marginal_launch_finish(w, DOF, cov_dev, other_idx ? cross_dev : nullptr, results_dev, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, who, e);
    HIP_TRY(h->used.record(st));
    return NDTGPU_OK;
}

// The host form: the outputs staged through the handle's block and its pinned mirror, the _device form on the handle's stream.
template <int DOF, class H, class Device>
inline ndtgpu_status pgo_marginals_host_core(H *h, PgoMarginalSpace &m, const char *who, size_t n_queries, bool with_cross, double *cov_out,
                                             double *cross_out, ndtgpu_pgo_marginal_result *results_out, Device device)
{
    const size_t block = DOF * DOF * n_queries * sizeof(double);
    StageLayout in, out;
    const size_t o_cov = out.take(block), o_cross = out.take(with_cross ? block : 0), o_res = out.take(n_queries * sizeof(ndtgpu_pgo_marginal_result));
    ndtgpu_status rc = m.stage.open(h, who, in, out);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = h->hst.get();
    rc = device((double *)m.stage.out_dev(o_cov), with_cross ? (double *)m.stage.out_dev(o_cross) : nullptr,
                (ndtgpu_pgo_marginal_result *)m.stage.out_dev(o_res), st);
    if (rc != NDTGPU_OK) return rc;
    if ((rc = m.stage.finish(h, st)) != NDTGPU_OK) return rc;
    memcpy(cov_out, m.stage.out_host(o_cov), block);
    if (with_cross) memcpy(cross_out, m.stage.out_host(o_cross), block);
    memcpy(results_out, m.stage.out_host(o_res), n_queries * sizeof(ndtgpu_pgo_marginal_result));
    return NDTGPU_OK;
}

#pragma GCC visibility pop
