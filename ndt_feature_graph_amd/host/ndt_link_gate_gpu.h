// ndt_link_gate_gpu.h -- host front door of the step that decides which loop-closure links exist, over the ndtgpu_linkgate_*
// entries of libndtgpu.so (include/ndtgpu.h "link gating" gives the semantics, the NaN rule and what differs from upstream):
//   ndt_feature::computeCandidateLinks   the enumeration of computeAllPossibleLinks (ndt_feature_graph.cpp:395-405) gated by index
//                                        distance and by the nodes' own poses, before anything is matched
//   ndt_feature::getValidLinksGPU        NDTFeatureGraph::getValidLinks (ndt_feature_graph.cpp:527-556) in one device call
//   ndt_feature::optimizeGraphGated      the offline mapper's loop (ndt_feature_graph_opt.cpp:152-173): clearAllLinks,
//                                        appendLinks(incremental), getValidLinks, appendLinks(links), optimizeGraphUsingISAM, until
//                                        the number of links stops changing
// NDTFeatureGraph::getValidLinks, computeAllPossibleLinks and computeLink (host/ndt_feature_graph_gpu.h) are unchanged: the scalar
// getValidLinks stays the reference these are checked against (tests/native/linkgate_demo.cpp).  The graph is taken through
// NDTFeatureGraphInterface, so anything the iSAM layer accepts is accepted here.
#pragma once
#include "ndt_feature_graph_gpu.h"

#include <limits>

namespace ndt_feature {

// ndtgpu_linkgate_params with its defaults: 0.1, 1.0, 0.2, 2 (ndt_feature_graph_opt.cpp:49-52), clip_cosine 0 (upstream's NaN rule)
struct LinkGateParams : ndtgpu_linkgate_params {
    LinkGateParams() { ndtgpu_default_linkgate_params(this); }
    LinkGateParams(double maxScore, double maxDist, double maxAngularDist, int minIdxDist, bool clipCosine = false)
    {
        ndtgpu_default_linkgate_params(this);
        max_score = maxScore;
        max_dist = maxDist;
        max_angle = maxAngularDist;
        min_idx_dist = minIdxDist;
        clip_cosine = clipCosine ? 1 : 0;
    }
};

// a ndtgpu_linkgate handle holding a graph's node poses
class LinkGate {
public:
    LinkGate(size_t max_nodes, size_t max_links)
    {
        ndtgpu_host::check(ndtgpu_linkgate_create(std::max<size_t>(max_nodes, 1), max_links, &h_), "ndtgpu_linkgate_create");
    }
    ~LinkGate() { ndtgpu_linkgate_destroy(h_); }
    LinkGate(const LinkGate &) = delete;
    LinkGate &operator=(const LinkGate &) = delete;
    ndtgpu_linkgate *handle() const { return h_; }
    void setNodes(const NDTFeatureGraphInterface &graph)
    {
        const size_t n = graph.getNbNodes();
        std::vector<double> T(16 * std::max<size_t>(n, 1));
        for (size_t i = 0; i < n; i++) {
            const double *m = graph.getNodeInterface(i).getPose().data();
            for (int q = 0; q < 16; q++) T[16 * i + q] = m[q];
        }
        ndtgpu_host::check(ndtgpu_linkgate_set_nodes(h_, n, T.data()), "ndtgpu_linkgate_set_nodes");
    }
    // the indices of the links that stay, ascending
    std::vector<uint32_t> valid(const std::vector<NDTFeatureLink> &links, const ndtgpu_linkgate_params &prm, bool use_score = true)
    {
        const size_t n = links.size();
        std::vector<uint32_t> ref(n + 1), mov(n + 1);
        std::vector<double> T(16 * (n + 1)), score(n + 1);
        for (size_t k = 0; k < n; k++) {
            ref[k] = (uint32_t)links[k].getRefIdx();
            mov[k] = (uint32_t)links[k].getMovIdx();
            score[k] = links[k].getScore();
            const double *m = links[k].T.data();
            for (int q = 0; q < 16; q++) T[16 * k + q] = m[q];
        }
        ndtgpu_host::check(ndtgpu_linkgate_valid_host(h_, &prm, n, ref.data(), mov.data(), T.data(), use_score ? score.data() : nullptr),
                           "ndtgpu_linkgate_valid_host");
        size_t count = 0;
        ndtgpu_host::check(ndtgpu_linkgate_count(h_, &count, nullptr), "ndtgpu_linkgate_count");
        std::vector<uint32_t> keep(count + 1);
        ndtgpu_host::check(ndtgpu_linkgate_keep(h_, 0, count, keep.data()), "ndtgpu_linkgate_keep");
        keep.resize(count);
        return keep;
    }

private:
    ndtgpu_linkgate *h_ = nullptr;
};

// Every pair i < j of the graph's nodes, in computeAllPossibleLinks' order, that is worth matching: j - i >= min_idx_dist and
// distanceBetweenAffine3d(T_i, T_j) within max_dist / max_angle (max_score is not read).  The links carry ref = i, mov = j and
// T = T_i^-1 T_j -- the initial guess the matchers take -- and score 0; what computeLink would add (features, registration) is the
// caller's next step.
inline std::vector<NDTFeatureLink> computeCandidateLinks(const NDTFeatureGraphInterface &graph, const ndtgpu_linkgate_params &params = LinkGateParams())
{
    LinkGate gate(graph.getNbNodes(), 0);
    gate.setNodes(graph);
    // the count first, then arrays of that size
    ndtgpu_host::check(ndtgpu_linkgate_candidates_host(gate.handle(), &params, nullptr, nullptr, nullptr, 0), "ndtgpu_linkgate_candidates_host");
    size_t count = 0;
    ndtgpu_host::check(ndtgpu_linkgate_count(gate.handle(), &count, nullptr), "ndtgpu_linkgate_count");
    std::vector<uint32_t> ref(count + 1), mov(count + 1);
    std::vector<double> T(16 * (count + 1));
    ndtgpu_host::check(ndtgpu_linkgate_candidates_host(gate.handle(), &params, ref.data(), mov.data(), T.data(), count), "ndtgpu_linkgate_candidates_host");
    std::vector<NDTFeatureLink> links;
    links.reserve(count);
    for (size_t k = 0; k < count; k++) {
        NDTFeatureLink l(ref[k], mov[k]);
        double *m = l.T.data();
        for (int q = 0; q < 16; q++) m[q] = T[16 * k + q];
        links.push_back(l);
    }
    return links;
}

// getValidLinks (ndt_feature_graph.cpp:527-556) of `links` under the graph's node poses, in one device call
inline std::vector<NDTFeatureLink> getValidLinksGPU(const NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links,
                                                    const ndtgpu_linkgate_params &params = LinkGateParams(), std::vector<uint32_t> *kept = nullptr)
{
    LinkGate gate(graph.getNbNodes(), links.size());
    gate.setNodes(graph);
    const std::vector<uint32_t> keep = gate.valid(links, params);
    std::vector<NDTFeatureLink> ret;
    ret.reserve(keep.size());
    for (uint32_t k : keep) ret.push_back(links[k]);
    if (kept) *kept = keep;
    return ret;
}
inline std::vector<NDTFeatureLink> getValidLinksGPU(const NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links, double maxScore,
                                                    double maxDist, double maxAngularDist, int minIdxDist)
{
    return getValidLinksGPU(graph, links, LinkGateParams(maxScore, maxDist, maxAngularDist, minIdxDist));
}

// The loop of ndt_feature_graph_opt.cpp:152-173 on a graph that has clearAllLinks() and appendLinks() (NDTFeatureGraph): every
// round gates `matched` under the current node poses on the device, rebuilds the graph's links as incremental + kept and runs
// optimizeGraphUsingISAM.  It stops when nothing is kept, when the kept count repeats, or after max_rounds rounds -- max_rounds is
// OURS: upstream's loop has no cap and can oscillate between two link sets.  Returns the kept count of every round.
template <class Graph>
inline std::vector<size_t> optimizeGraphGated(Graph &graph, const std::vector<NDTFeatureLink> &incremental, const std::vector<NDTFeatureLink> &matched,
                                              const ndtgpu_linkgate_params &params = LinkGateParams(), int max_rounds = 10,
                                              const ndtgpu_pgo_params *pgo_params = nullptr)
{
    LinkGate gate(graph.getNbNodes(), matched.size());
    std::vector<size_t> rounds;
    size_t prev_nb_links = std::numeric_limits<size_t>::max();
    for (int round = 0; round < max_rounds; round++) {
        graph.clearAllLinks();
        graph.appendLinks(incremental);
        gate.setNodes(graph);
        const std::vector<uint32_t> keep = gate.valid(matched, params);
        rounds.push_back(keep.size());
        if (keep.empty()) break;
        std::vector<NDTFeatureLink> links;
        links.reserve(keep.size());
        for (uint32_t k : keep) links.push_back(matched[k]);
        graph.appendLinks(links);
        optimizeGraphUsingISAM(graph, pgo_params);
        if (prev_nb_links == keep.size()) break;
        prev_nb_links = keep.size();
    }
    return rounds;
}

}  // namespace ndt_feature
