// pgo_demo.cpp -- the host mirror's optimizeGraphUsingISAM (host/ndt_feature_graph_gpu.h) called the way ndt_feature_graph_opt.cpp
// does (:152-164: incremental links with score -1 and registered links appended, then optimizeGraphUsingISAM(graph)) on a graph
// of 12 nodes, against the ndtgpu_pgo_* calls it wraps given the same factors by hand -- the links with score < 0 twice, as
// ndt_offline_mapper.h:74-93 adds them: the node poses must be those of the C-ABI bit for bit.  Exit code 0 = every check
// passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// the part of NDTFeatureGraph that optimizeGraphUsingISAM sees (interfaces.h), without node maps
struct DemoGraph : NDTFeatureGraphInterface {
    std::vector<NDTFeatureNode> nodes;
    std::vector<NDTFeatureLink> links;
    size_t getNbNodes() const override { return nodes.size(); }
    NDTFeatureNodeInterface &getNodeInterface(size_t i) override { return nodes[i]; }
    const NDTFeatureNodeInterface &getNodeInterface(size_t i) const override { return nodes[i]; }
    size_t getNbLinks() const override { return links.size(); }
    NDTFeatureLinkInterface &getLinkInterface(size_t i) override { return links[i]; }
    const NDTFeatureLinkInterface &getLinkInterface(size_t i) const override { return links[i]; }
};

int main()
{
    const size_t n = 12;
    std::mt19937 rng(12);
    std::normal_distribution<double> nd(0.0, 1.0);
    // a loop of 12 nodes; the estimates have drifted from the truth
    std::vector<Eigen::Affine3d> truth(n);
    DemoGraph graph;
    graph.nodes.resize(n);
    for (size_t i = 0; i < n; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)n;
        truth[i] = ndtgpu_host::affine_from_pose(5.0 * std::cos(a), 4.0 * std::sin(a), 0, 0, 0, a + 2.2);
        graph.nodes[i].T = i == 0 ? truth[0]
                                  : truth[i] * ndtgpu_host::affine_from_pose(0.02 * (double)i * nd(rng), 0.02 * (double)i * nd(rng), 0, 0, 0, 0.01 * (double)i * nd(rng));
    }
    auto add = [&](size_t ref, size_t mov, double score) {
        NDTFeatureLink l(ref, mov);
        l.T = truth[ref].inverse() * truth[mov] * ndtgpu_host::affine_from_pose(0.01 * nd(rng), 0.01 * nd(rng), 0, 0, 0, 0.005 * nd(rng));
        l.score = score;
        graph.links.push_back(l);
    };
    for (size_t i = 0; i + 1 < n; i++) add(i, i + 1, -1.);        // getIncrementalLinks: score -1
    add(n - 1, 0, 0.3);                                           // registered links (getValidLinks)
    add(2, 9, 0.5);
    add(10, 4, 0.1);

    // the same factors by hand, for the C-ABI
    std::vector<double> pose(3 * n), meas;
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < n; i++) {
        pose[3 * i] = graph.nodes[i].T.translation()(0);
        pose[3 * i + 1] = graph.nodes[i].T.translation()(1);
        pose[3 * i + 2] = getRobustYawFromAffine3d(graph.nodes[i].T);
    }
    for (int pass = 0; pass < 2; pass++)
        for (const NDTFeatureLink &l : graph.links) {
            if (pass == 0 && l.score >= 0.) continue;
            ref.push_back((uint32_t)l.ref_idx);
            mov.push_back((uint32_t)l.mov_idx);
            meas.push_back(l.T.translation()(0));
            meas.push_back(l.T.translation()(1));
            meas.push_back(getRobustYawFromAffine3d(l.T));
        }
    CHECK(ref.size() == 2 * (n - 1) + 3, "%zu factors", ref.size());

    ndtgpu_pgo_result rm;
    try {
        optimizeGraphUsingISAM(graph, nullptr, &rm);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }

    // a bank of another shape, the graph in its last slot
    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(3, 40, 100, &h), "ndtgpu_pgo_create");
    ndtgpu_host::check(ndtgpu_pgo_set_graph(h, 2, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr), "ndtgpu_pgo_set_graph");
    ndtgpu_host::check(ndtgpu_pgo_optimize(h, 2, 1, nullptr, nullptr), "ndtgpu_pgo_optimize");
    std::vector<double> out(3 * n), T16(16 * n);
    ndtgpu_pgo_result rc;
    ndtgpu_host::check(ndtgpu_pgo_poses(h, 2, out.data(), T16.data(), &rc), "ndtgpu_pgo_poses");
    ndtgpu_pgo_destroy(h);

    int equal = 0;
    double worst = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) same = same && graph.nodes[i].T.data()[e] == T16[16 * i + e];
        CHECK(same, "node %zu: the mirror differs from the C-ABI", i);
        equal += same ? 1 : 0;
        const Eigen::Vector3d d = graph.nodes[i].T.translation() - truth[i].translation();
        worst = std::max(worst, d.norm());
    }
    CHECK(rm.exit_code == NDTGPU_PGO_CONVERGED && rc.exit_code == NDTGPU_PGO_CONVERGED, "exit codes %d / %d", rm.exit_code, rc.exit_code);
    CHECK(rm.iterations == rc.iterations && rm.linear_iterations == rc.linear_iterations && rm.cost_final == rc.cost_final &&
              rm.cost_initial == rc.cost_initial && rm.max_step == rc.max_step,
          "the reports differ");
    CHECK(rm.n_nodes == (int)n && rm.n_edges == (int)ref.size(), "%d nodes, %d factors", rm.n_nodes, rm.n_edges);
    CHECK(rm.cost_final < rm.cost_initial, "cost %.6g -> %.6g", rm.cost_initial, rm.cost_final);
    CHECK(worst < 0.1, "a node ends %.3f m from the truth", worst);
    std::printf("pgo_demo: %zu nodes, %d factors, %d equal to the C-ABI bit for bit, cost %.6g -> %.6g in %d updates, worst |dt| %.4f m, "
                "%d failures\n", n, rm.n_edges, equal, rm.cost_initial, rm.cost_final, rm.iterations, worst, g_fails);
    return g_fails ? 1 : 0;
}
