// ndtgpu_pgo_bank.h -- the handles of the two pose-graph banks (ndtgpu_pgo: SE(2), ndtgpu_pgo3: SE(3)) and the device form of their
// parameters, for the files of the C-ABI that work on them: csrc/ndtgpu_pgo.hip and csrc/ndtgpu_pgo3.hip (create, set, optimise,
// marginals) and csrc/ndtgpu_pgo_robust.hip (robust weighting, which steers rounds of the optimise entries of either bank).
#pragma once
#include "ndtgpu_host.h"
#include "ndt_pgo.h"
#include "ndt_pgo3.h"
#include "ndt_pgo_robust.h"
#include "ndt_pgo_wide_core.h"
#include "ndtgpu_pgo_marginals.h"

#pragma GCC visibility push(hidden)

// The robust calls' own (ndtgpu_pgo_optimize_robust / ndtgpu_pgo3_optimize_robust), allocated by a handle's first robust call for
// the handle's capacity: the copy of the information as the graphs were set, the per-link outputs, the per-tile sums and the
// graphs' sums.  saved[g]: w0 holds graph g's information as set; set_graph / set_links_device clear it.
struct PgoRobustSpace {
    NdtPgoRobustView v{};
    DeviceBuffer<double> w0, chi2, weight, part;
    DeviceBuffer<int32_t> inlier;
    DeviceBuffer<uint32_t> part_n;
    DeviceBuffer<NdtPgoRobustSum> sum;
    std::vector<uint8_t> saved;                  // per graph
    std::vector<uint8_t> weighed;                // per graph: a robust call has left chi2, weight, inlier and result
    std::vector<ndtgpu_pgo_robust_result> result;
    void invalidate(size_t g)
    {
        if (g < saved.size()) saved[g] = weighed[g] = 0;
    }
};

struct ndtgpu_pgo {
    size_t G = 0;
    NdtPgoView v{};                        // what the kernels receive: filled from the owners below at create
    DeviceBuffer<ndtgpu_pgo_result> state;
    DeviceBuffer<double> pose, origin, meas, info, jac, te, node;
    DeviceBuffer<int32_t> ref, mov;
    DeviceBuffer<uint32_t> adj_off, adj;
    std::vector<uint32_t> n_nodes;         // per graph, 0: not set
    std::vector<uint32_t> n_edges;         // per graph
    // the chip-wide form's own (ndtgpu_pgo_optimize_wide), allocated by the handle's first wide call for the handle's capacity:
    // per-tile partial sums, the two control blocks and their pinned mirror
    DeviceBuffer<double> wide_part;
    DeviceBuffer<NdtPgoWideCtl> wide_ctl;
    PinnedBuffer<NdtPgoWideCtl> wide_mirror;
    PgoMarginalSpace marginal;             // the marginals' own workspace, allocated by the handle's first marginals call
    PgoRobustSpace robust;                 // the robust calls' own, allocated by the handle's first robust call
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the synchronous entries' stream (last: ndtgpu_resource.h)
};

struct ndtgpu_pgo3 {
    size_t G = 0;
    NdtPgo3View v{};                       // what the kernels receive: filled from the owners below at create
    DeviceBuffer<ndtgpu_pgo_result> state;
    DeviceBuffer<double> pose, origin, meas, info, jac, te, node;
    DeviceBuffer<int32_t> ref, mov;
    DeviceBuffer<uint32_t> adj_off, adj;
    std::vector<uint32_t> n_nodes;         // per graph, 0: not set
    std::vector<uint32_t> n_edges;         // per graph
    // the chip-wide form's own (ndtgpu_pgo3_optimize_wide), allocated by the handle's first wide call for the handle's capacity:
    // per-tile partial sums, the two control blocks and their pinned mirror
    DeviceBuffer<double> wide_part;
    DeviceBuffer<NdtPgoWideCtl> wide_ctl;
    PinnedBuffer<NdtPgoWideCtl> wide_mirror;
    PgoMarginalSpace marginal;             // the marginals' own workspace, allocated by the handle's first marginals call
    PgoRobustSpace robust;                 // the robust calls' own, allocated by the handle's first robust call
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // the synchronous entries' stream (last: ndtgpu_resource.h)
};

inline void sym6(const double *W9, double *W6)
{
    W6[0] = W9[0]; W6[1] = 0.5 * (W9[1] + W9[3]); W6[2] = 0.5 * (W9[2] + W9[6]);
    W6[3] = W9[4]; W6[4] = 0.5 * (W9[5] + W9[7]); W6[5] = W9[8];
}

// the device form of a call's parameters (NULL: the defaults); false where one is out of range
inline bool pgo_params_dev(const ndtgpu_pgo_params *prm, NdtPgoParamsDev &d)
{
    const ndtgpu_pgo_params p = params_or_default(prm, ndtgpu_default_pgo_params);
    bool ok = p.max_iterations >= 0 && p.max_linear_iterations >= 0 && p.eps_step >= 0.0 && p.eps_linear >= 0.0;   // (NaN fails)
    for (double w : p.prior_information) ok = ok && std::isfinite(w);
    d.max_iterations = p.max_iterations;
    d.max_linear_iterations = p.max_linear_iterations;
    d.eps_step = p.eps_step;
    d.eps_linear = p.eps_linear;
    sym6(p.prior_information, d.prior);
    return ok;
}

inline bool pgo3_params_dev(const ndtgpu_pgo3_params *prm, NdtPgo3ParamsDev &d)
{
    const ndtgpu_pgo3_params p = params_or_default(prm, ndtgpu_default_pgo3_params);
    bool ok = p.max_iterations >= 0 && p.max_linear_iterations >= 0 && p.eps_step >= 0.0 && p.eps_linear >= 0.0;   // (NaN fails)
    for (double w : p.prior_information) ok = ok && std::isfinite(w);
    d.max_iterations = p.max_iterations;
    d.max_linear_iterations = p.max_linear_iterations;
    d.eps_step = p.eps_step;
    d.eps_linear = p.eps_linear;
    pgo3_sym21(p.prior_information, d.prior);
    return ok;
}

#pragma GCC visibility pop
