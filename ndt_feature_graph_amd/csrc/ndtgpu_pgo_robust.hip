// ndtgpu_pgo_robust.hip -- C-ABI (include/ndtgpu.h, "robust loop-closure weighting") of the robust form of the two pose-graph
// optimisers: iteratively re-weighted least squares round ndtgpu_pgo_optimize / _optimize_wide and the pgo3 pair as they are.
// Host side only: the parameter checks, the handle's robust buffers (csrc/ndtgpu_pgo_bank.h), the copy of the information as a
// graph was set, and the steering of the rounds -- weigh and finish (csrc/ndt_pgo_robust.hip) for the graphs still active, the
// existing optimise entry for contiguous runs of them, a look at the records.  One core serves both banks: what differs is the
// doubles of a link's information (6 or 21) and the entries called.
#include "ndtgpu_pgo_bank.h"

// the checks of a robust call's own parameters (NULL: the defaults), made before the handle is read
static bool robust_params_dev(const ndtgpu_pgo_robust_params *rp, ndtgpu_pgo_robust_params &p, NdtPgoRobustParamsDev &d)
{
    p = params_or_default(rp, ndtgpu_default_pgo_robust_params);
    const bool ok = (p.kind == NDTGPU_PGO_ROBUST_HUBER || p.kind == NDTGPU_PGO_ROBUST_CAUCHY || p.kind == NDTGPU_PGO_ROBUST_DCS) &&
                    std::isfinite(p.scale) && p.scale > 0.0 && p.max_rounds >= 0 && p.updates_per_round >= 1 && p.min_index_gap >= 1 &&
                    p.inlier_weight >= 0.0 && p.inlier_weight <= 1.0;                                    // (NaN fails)
    d.kind = p.kind;
    d.min_index_gap = p.min_index_gap;
    d.scale = p.scale;
    d.inlier_weight = p.inlier_weight;
    return ok;
}

static const char *const ROBUST_BAD = "bad robust parameter (kind HUBER, CAUCHY or DCS; scale finite and > 0; max_rounds >= 0; "
                                      "updates_per_round >= 1; min_index_gap >= 1; inlier_weight in [0, 1])";

// the handle's robust buffers, for its capacity; K: the doubles of a link's information.  `sum` is allocated last and is what says
// that all are there: after a failure part-way the next call allocates every buffer again, and Buffer::alloc (ndtgpu_resource.h)
// releases what it holds first, so nothing is leaked or counted twice.
template <class H>
static hipError_t robust_reserve(H *h, int K)
{
    PgoRobustSpace &s = h->robust;
    if (s.sum.get()) return hipSuccess;
    const size_t G = h->G, E = std::max<size_t>(h->v.max_edges, 1);
    const size_t tiles = (E + NDT_PGO_ROBUST_TILE - 1) / NDT_PGO_ROBUST_TILE;
    hipError_t e;
    if ((e = s.w0.alloc(G * K * E, &s.v.w0)) != hipSuccess) return e;
    if ((e = s.chi2.alloc(G * E, &s.v.chi2)) != hipSuccess) return e;
    if ((e = s.weight.alloc(G * E, &s.v.weight)) != hipSuccess) return e;
    if ((e = s.inlier.alloc(G * E, &s.v.inlier)) != hipSuccess) return e;
    if ((e = s.part.alloc(G * 2 * tiles, &s.v.part)) != hipSuccess) return e;
    if ((e = s.part_n.alloc(G * 3 * tiles, &s.v.part_n)) != hipSuccess) return e;
    s.v.tiles = (unsigned)tiles;
    s.saved.assign(G, 0);
    s.weighed.assign(G, 0);
    s.result.assign(G, ndtgpu_pgo_robust_result{});
    return s.sum.alloc(G, &s.v.sum);             // (last: what the first line tests)
}

// The rounds.  launch(first, count, max_links, apply): weigh + finish; optimise(first, count): the bank's optimise entry with
// max_iterations = updates_per_round, or its wide form on the one graph.  Both enqueue on st and keep the handle's calls ordered.
template <class H, class Launch, class Optimise>
static ndtgpu_status robust_core(const char *who, H *h, size_t first, size_t count, int K, const ndtgpu_pgo_robust_params &rp, double eps_step,
                                 hipStream_t st, Launch &&launch, Optimise &&optimise)
{
    if (count == 0 || first >= h->G || count > h->G - first) return fail_in(NDTGPU_ERR_INVALID, who, "graphs [first, first + count) out of range");
    for (size_t g = first; g < first + count; g++)
        if (!h->n_nodes[g]) return fail_in(NDTGPU_ERR_INVALID, who, "a graph of the range has not been set");
    HIP_TRY(robust_reserve(h, K));
    PgoRobustSpace &s = h->robust;
    const size_t Emax = h->v.max_edges;

    // the information as set, once per set_graph
    HIP_TRY(h->used.order(st));
    for (size_t g = first; g < first + count; g++) {
        if (s.saved[g]) continue;
        if (h->n_edges[g])
            HIP_TRY(hipMemcpyAsync(s.v.w0 + g * K * Emax, h->v.info + g * K * Emax, (size_t)K * h->n_edges[g] * sizeof(double),
                                   hipMemcpyDeviceToDevice, st));
        s.saved[g] = 1;
    }
    HIP_TRY(h->used.record(st));

    std::vector<NdtPgoRobustSum> sums(count);
    std::vector<ndtgpu_pgo_result> states(count);
    std::vector<size_t> active(count);
    for (size_t k = 0; k < count; k++) active[k] = first + k;
    // f(a, n): over the contiguous runs [a, a + n) of `list`, ascending
    auto runs = [](const std::vector<size_t> &list, auto &&f) -> ndtgpu_status {
        for (size_t i = 0; i < list.size();) {
            size_t j = i + 1;
            while (j < list.size() && list[j] == list[j - 1] + 1) j++;
            const ndtgpu_status rc = f(list[i], j - i);
            if (rc != NDTGPU_OK) return rc;
            i = j;
        }
        return NDTGPU_OK;
    };
    // weigh + finish of the listed graphs, then their sums on the host
    auto weigh = [&](const std::vector<size_t> &list, bool apply) -> ndtgpu_status {
        HIP_TRY(h->used.order(st));
        ndtgpu_status rc = runs(list, [&](size_t a, size_t n) -> ndtgpu_status {
            size_t max_links = 0;
            for (size_t g = a; g < a + n; g++) max_links = std::max<size_t>(max_links, h->n_edges[g]);
            HIP_TRY(launch(a, n, max_links, apply));
            HIP_TRY(hipMemcpyAsync(&sums[a - first], s.v.sum + a, n * sizeof(NdtPgoRobustSum), hipMemcpyDeviceToHost, st));
            return NDTGPU_OK;
        });
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(h->used.record(st));
        HIP_TRY(hipStreamSynchronize(st));
        return NDTGPU_OK;
    };

    const bool evaluate_only = rp.max_rounds == 0;
    ndtgpu_status rc = weigh(active, !evaluate_only);
    if (rc != NDTGPU_OK) return rc;
    std::vector<size_t> next;
    for (size_t g : active) {
        const NdtPgoRobustSum &u = sums[g - first];
        ndtgpu_pgo_robust_result r{};
        r.cost_initial = r.cost_final = u.cost;
        r.chi2_final = u.chi2;
        r.outliers = u.flagged;
        r.exit_code = u.status != NDTGPU_PGO_CONVERGED ? u.status : NDTGPU_PGO_MAX_ITERATIONS;   // (MAX_ROUNDS: all that max_rounds == 0 can end with)
        s.result[g] = r;
        s.weighed[g] = 1;
        if (u.status == NDTGPU_PGO_CONVERGED && !evaluate_only) next.push_back(g);
    }
    active.swap(next);

    for (int round = 1; !active.empty(); round++) {
        rc = runs(active, [&](size_t a, size_t n) -> ndtgpu_status {
            const ndtgpu_status orc = optimise(a, n);
            if (orc != NDTGPU_OK) return orc;
            HIP_TRY(hipMemcpyAsync(&states[a - first], h->v.state + a, n * sizeof(ndtgpu_pgo_result), hipMemcpyDeviceToHost, st));
            return NDTGPU_OK;
        });
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        // the verdicts of the round; every graph of it is weighed once more: a graph that goes on for its next round, one that
        // stops for the weights, flags and sums at the poses it ends with
        std::vector<uint8_t> stops(active.size(), 0);
        for (size_t k = 0; k < active.size(); k++) {
            const ndtgpu_pgo_result &o = states[active[k] - first];
            ndtgpu_pgo_robust_result &r = s.result[active[k]];
            r.rounds = round;
            r.updates += o.iterations;
            r.linear_iterations += o.linear_iterations;
            if (o.exit_code == NDTGPU_PGO_LINEAR_CAP || o.exit_code == NDTGPU_PGO_NOT_FINITE || o.exit_code == NDTGPU_PGO3_HALF_TURN) {
                r.exit_code = o.exit_code;
                stops[k] = 1;
            } else if (o.iterations <= 1 && o.max_step <= eps_step) {
                r.exit_code = NDTGPU_PGO_CONVERGED;
                stops[k] = 1;
            } else if (round >= rp.max_rounds) {
                r.exit_code = NDTGPU_PGO_MAX_ITERATIONS;
                stops[k] = 1;
            }
        }
        if ((rc = weigh(active, true)) != NDTGPU_OK) return rc;
        next.clear();
        for (size_t k = 0; k < active.size(); k++) {
            const size_t g = active[k];
            const NdtPgoRobustSum &u = sums[g - first];
            ndtgpu_pgo_robust_result &r = s.result[g];
            r.cost_final = u.cost;
            r.chi2_final = u.chi2;
            r.outliers = u.flagged;
            if (u.status != NDTGPU_PGO_CONVERGED) {
                if (!stops[k] || r.exit_code == NDTGPU_PGO_CONVERGED || r.exit_code == NDTGPU_PGO_MAX_ITERATIONS) r.exit_code = u.status;
            } else if (!stops[k]) {
                next.push_back(g);
            }
        }
        active.swap(next);
    }
    return NDTGPU_OK;
}

template <class H>
static ndtgpu_status robust_links(const char *who, H *h, size_t g, double *chi2, double *weight, int32_t *inlier, ndtgpu_pgo_robust_result *result)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (g >= h->G || !h->n_nodes[g] || g >= h->robust.weighed.size() || !h->robust.weighed[g])
        return fail_in(NDTGPU_ERR_INVALID, who, "no such graph, or no robust call since it was set");
    HIP_TRY(h->used.sync());
    const PgoRobustSpace &s = h->robust;
    const size_t n = h->n_edges[g], o = g * h->v.max_edges;
    if (n && chi2) HIP_TRY(hipMemcpy(chi2, s.v.chi2 + o, n * sizeof(double), hipMemcpyDeviceToHost));
    if (n && weight) HIP_TRY(hipMemcpy(weight, s.v.weight + o, n * sizeof(double), hipMemcpyDeviceToHost));
    if (n && inlier) HIP_TRY(hipMemcpy(inlier, s.v.inlier + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (result) *result = s.result[g];
    return NDTGPU_OK;
}

template <class H>
static ndtgpu_status robust_links_device(const char *who, H *h, size_t g, const double **chi2_dev, const double **weight_dev,
                                         const int32_t **inlier_dev)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (g >= h->G || !h->n_nodes[g] || g >= h->robust.weighed.size() || !h->robust.weighed[g])
        return fail_in(NDTGPU_ERR_INVALID, who, "no such graph, or no robust call since it was set");
    const PgoRobustSpace &s = h->robust;
    const size_t o = g * h->v.max_edges;
    if (chi2_dev) *chi2_dev = s.v.chi2 + o;
    if (weight_dev) *weight_dev = s.v.weight + o;
    if (inlier_dev) *inlier_dev = s.v.inlier + o;
    return NDTGPU_OK;
}

// the information as set back into the bank; nothing to do for a graph no robust call has weighed since it was set
template <class H>
static ndtgpu_status robust_restore(const char *who, H *h, size_t g, int K)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (g >= h->G || !h->n_nodes[g]) return fail_in(NDTGPU_ERR_INVALID, who, "no such graph, or it has not been set");
    PgoRobustSpace &s = h->robust;
    if (g >= s.saved.size() || !s.saved[g] || !h->n_edges[g]) return NDTGPU_OK;
    const size_t o = g * K * h->v.max_edges;
    HIP_TRY(h->used.order(h->hst.get()));
    HIP_TRY(hipMemcpyAsync(h->v.info + o, s.v.w0 + o, (size_t)K * h->n_edges[g] * sizeof(double), hipMemcpyDeviceToDevice, h->hst.get()));
    HIP_TRY(h->used.record(h->hst.get()));
    HIP_TRY(hipStreamSynchronize(h->hst.get()));
    return NDTGPU_OK;
}

// graph g's information as the bank holds it, K doubles a link
template <class H>
static ndtgpu_status link_information(const char *who, H *h, size_t g, int K, double *out)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null handle");
    if (!out) return fail_in(NDTGPU_ERR_INVALID, who, "the output is NULL");
    if (g >= h->G || !h->n_nodes[g]) return fail_in(NDTGPU_ERR_INVALID, who, "no such graph, or it has not been set");
    HIP_TRY(h->used.sync());
    if (h->n_edges[g])
        HIP_TRY(hipMemcpy(out, h->v.info + g * K * h->v.max_edges, (size_t)K * h->n_edges[g] * sizeof(double), hipMemcpyDeviceToHost));
    return NDTGPU_OK;
}

extern "C" {

void ndtgpu_default_pgo_robust_params(ndtgpu_pgo_robust_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // all OURS: the reference has no robust cost
    p->kind = NDTGPU_PGO_ROBUST_DCS;
    p->max_rounds = 50;
    p->updates_per_round = 1;
    p->min_index_gap = 2;
    p->scale = 1.0;
    p->inlier_weight = 0.5;
}

ndtgpu_status ndtgpu_pgo_robust_weight(int32_t kind, double scale, double chi2, double *weight)
{
    if (!weight) return fail(NDTGPU_ERR_INVALID, "pgo_robust_weight: weight is NULL");
    if ((kind != NDTGPU_PGO_ROBUST_HUBER && kind != NDTGPU_PGO_ROBUST_CAUCHY && kind != NDTGPU_PGO_ROBUST_DCS) || !std::isfinite(scale) || !(scale > 0.0))
        return fail(NDTGPU_ERR_INVALID, "pgo_robust_weight: kind HUBER, CAUCHY or DCS, scale finite and > 0");
    *weight = ndt_pgo_robust_weight(kind, scale, chi2);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_pgo_optimize_robust(ndtgpu_pgo *h, size_t first, size_t count, const ndtgpu_pgo_params *prm,
                                         const ndtgpu_pgo_robust_params *robust, const ndtgpu_pgo_wide_params *wide, ndtgpu_stream stream)
{
    ndtgpu_pgo_robust_params rp;
    NdtPgoRobustParamsDev d;
    NdtPgoParamsDev pd;
    if (!robust_params_dev(robust, rp, d)) return fail_in(NDTGPU_ERR_INVALID, "pgo_optimize_robust", ROBUST_BAD);
    if (!pgo_params_dev(prm, pd)) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_robust: bad parameter (caps and tolerances >= 0, a finite prior)");
    if (wide && wide->check_every < 1) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_robust: check_every must be >= 1");
    if (wide && count != 1) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_robust: the wide form takes one graph (count == 1)");
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo_optimize_robust: null handle");
    ndtgpu_pgo_params inner = params_or_default(prm, ndtgpu_default_pgo_params);
    inner.max_iterations = rp.updates_per_round;
    hipStream_t st = (hipStream_t)stream;
    return robust_core("pgo_optimize_robust", h, first, count, 6, rp, inner.eps_step, st,
                       [&](size_t a, size_t n, size_t max_links, bool apply) { return ndt_pgo_robust_launch(h->v, h->robust.v, a, n, max_links, d, apply, st); },
                       [&](size_t a, size_t n) {
                           return wide ? ndtgpu_pgo_optimize_wide(h, a, &inner, wide, stream) : ndtgpu_pgo_optimize(h, a, n, &inner, stream);
                       });
}

ndtgpu_status ndtgpu_pgo3_optimize_robust(ndtgpu_pgo3 *h, size_t first, size_t count, const ndtgpu_pgo3_params *prm,
                                          const ndtgpu_pgo_robust_params *robust, const ndtgpu_pgo_wide_params *wide, ndtgpu_stream stream)
{
    ndtgpu_pgo_robust_params rp;
    NdtPgoRobustParamsDev d;
    NdtPgo3ParamsDev pd;
    if (!robust_params_dev(robust, rp, d)) return fail_in(NDTGPU_ERR_INVALID, "pgo3_optimize_robust", ROBUST_BAD);
    if (!pgo3_params_dev(prm, pd)) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_robust: bad parameter (caps and tolerances >= 0, a finite prior)");
    if (wide && wide->check_every < 1) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_robust: check_every must be >= 1");
    if (wide && count != 1) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_robust: the wide form takes one graph (count == 1)");
    if (!h) return fail(NDTGPU_ERR_INVALID, "pgo3_optimize_robust: null handle");
    ndtgpu_pgo3_params inner = params_or_default(prm, ndtgpu_default_pgo3_params);
    inner.max_iterations = rp.updates_per_round;
    hipStream_t st = (hipStream_t)stream;
    return robust_core("pgo3_optimize_robust", h, first, count, 21, rp, inner.eps_step, st,
                       [&](size_t a, size_t n, size_t max_links, bool apply) { return ndt_pgo3_robust_launch(h->v, h->robust.v, a, n, max_links, d, apply, st); },
                       [&](size_t a, size_t n) {
                           return wide ? ndtgpu_pgo3_optimize_wide(h, a, &inner, wide, stream) : ndtgpu_pgo3_optimize(h, a, n, &inner, stream);
                       });
}

ndtgpu_status ndtgpu_pgo_robust_links(ndtgpu_pgo *h, size_t g, double *chi2, double *weight, int32_t *inlier, ndtgpu_pgo_robust_result *result)
{
    return robust_links("pgo_robust_links", h, g, chi2, weight, inlier, result);
}

ndtgpu_status ndtgpu_pgo3_robust_links(ndtgpu_pgo3 *h, size_t g, double *chi2, double *weight, int32_t *inlier, ndtgpu_pgo_robust_result *result)
{
    return robust_links("pgo3_robust_links", h, g, chi2, weight, inlier, result);
}

ndtgpu_status ndtgpu_pgo_robust_links_device(ndtgpu_pgo *h, size_t g, const double **chi2_dev, const double **weight_dev, const int32_t **inlier_dev)
{
    return robust_links_device("pgo_robust_links_device", h, g, chi2_dev, weight_dev, inlier_dev);
}

ndtgpu_status ndtgpu_pgo3_robust_links_device(ndtgpu_pgo3 *h, size_t g, const double **chi2_dev, const double **weight_dev,
                                              const int32_t **inlier_dev)
{
    return robust_links_device("pgo3_robust_links_device", h, g, chi2_dev, weight_dev, inlier_dev);
}

ndtgpu_status ndtgpu_pgo_link_information(ndtgpu_pgo *h, size_t g, double *W6_out) { return link_information("pgo_link_information", h, g, 6, W6_out); }

ndtgpu_status ndtgpu_pgo3_link_information(ndtgpu_pgo3 *h, size_t g, double *W21_out) { return link_information("pgo3_link_information", h, g, 21, W21_out); }

ndtgpu_status ndtgpu_pgo_robust_restore(ndtgpu_pgo *h, size_t g) { return robust_restore("pgo_robust_restore", h, g, 6); }

ndtgpu_status ndtgpu_pgo3_robust_restore(ndtgpu_pgo3 *h, size_t g) { return robust_restore("pgo3_robust_restore", h, g, 21); }

}   // extern "C"
