// pgo_robust_demo.cpp -- the host mirror's optimizeGraphUsingISAMRobust and optimizeGraph3DRobust (host/ndt_feature_graph_gpu.h) on
// the loop of 12 nodes of pgo_demo.cpp with one FALSE loop closure among its registered links, against the ndtgpu_pgo_optimize_robust
// / ndtgpu_pgo3_optimize_robust calls they wrap given the same factors by hand: the node poses must be those of the C-ABI bit for
// bit, the false closure must come back with a weight near 0 and every other link with weight 1 (DCS, the default).  Exit code 0
// = every check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// the part of NDTFeatureGraph that the optimisers see (interfaces.h), without node maps
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
    const size_t n = 12, false_link = n;                         // (the links' order below: 11 incremental, the closing one, then it)
    std::mt19937 rng(12);
    std::normal_distribution<double> nd(0.0, 1.0);
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
    graph.links.back().T = ndtgpu_host::affine_from_pose(0.4, -0.3, 0, 0, 0, 0.25);   // perceptual aliasing: nodes 2 and 9 are 8 m apart
    add(10, 4, 0.1);
    const std::vector<Eigen::Affine3d> start = [&] { std::vector<Eigen::Affine3d> s; for (auto &nd_ : graph.nodes) s.push_back(nd_.T); return s; }();

    // ---- SE(2): the factors by hand, the links with score < 0 twice ----
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
    std::vector<double> w2;
    ndtgpu_pgo_robust_result rm;
    try {
        optimizeGraphUsingISAMRobust(graph, nullptr, &w2, nullptr, &rm);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo_robust_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(3, 40, 100, &h), "ndtgpu_pgo_create");
    ndtgpu_host::check(ndtgpu_pgo_set_graph(h, 2, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr), "ndtgpu_pgo_set_graph");
    ndtgpu_host::check(ndtgpu_pgo_optimize_robust(h, 2, 1, nullptr, nullptr, nullptr, nullptr), "ndtgpu_pgo_optimize_robust");
    std::vector<double> out(3 * n), T16(16 * n), wc(ref.size());
    ndtgpu_pgo_robust_result rc;
    ndtgpu_host::check(ndtgpu_pgo_poses(h, 2, out.data(), T16.data(), nullptr), "ndtgpu_pgo_poses");
    ndtgpu_host::check(ndtgpu_pgo_robust_links(h, 2, nullptr, wc.data(), nullptr, &rc), "ndtgpu_pgo_robust_links");
    ndtgpu_pgo_destroy(h);
    int equal2 = 0;
    double worst2 = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) same = same && graph.nodes[i].T.data()[e] == T16[16 * i + e];
        CHECK(same, "SE(2) node %zu: the mirror differs from the C-ABI", i);
        equal2 += same ? 1 : 0;
        worst2 = std::max(worst2, (graph.nodes[i].T.translation() - truth[i].translation()).norm());
    }
    CHECK(w2.size() == graph.links.size(), "%zu weights", w2.size());
    for (size_t k = 0; k < w2.size(); k++) {
        CHECK(w2[k] == wc[n - 1 + k], "SE(2) link %zu: weight %.17g, C-ABI %.17g", k, w2[k], wc[n - 1 + k]);
        CHECK(k == false_link ? w2[k] < 1e-3 : w2[k] == 1.0, "SE(2) link %zu: weight %.6g", k, w2[k]);
    }
    CHECK(rm.exit_code == NDTGPU_PGO_CONVERGED && rm.exit_code == rc.exit_code && rm.rounds == rc.rounds && rm.updates == rc.updates &&
              rm.cost_final == rc.cost_final && rm.outliers == rc.outliers && rm.outliers == 1,
          "the reports: exit %d / %d, rounds %d / %d, outliers %d / %d", rm.exit_code, rc.exit_code, rm.rounds, rc.rounds, rm.outliers, rc.outliers);
    CHECK(worst2 < 0.1, "SE(2): a node ends %.3f m from the truth", worst2);

    // ---- SE(3): every link once, as optimizeGraph3D takes them (the information from cov_3d as the mirror converts it) ----
    for (size_t i = 0; i < n; i++) graph.nodes[i].T = start[i];
    std::vector<double> w3;
    ndtgpu_pgo_robust_result rm3, rc3;
    optimizeGraph3DRobust(graph, graph.links, nullptr, &w3, nullptr, &rm3);
    const size_t m = graph.links.size();
    std::vector<double> N16(16 * n), Z16(16 * m), W36(36 * m), wc3(m);
    std::vector<uint32_t> ref3(m), mov3(m);
    for (size_t i = 0; i < n; i++) std::copy_n(start[i].data(), 16, &N16[16 * i]);
    for (size_t k = 0; k < m; k++) {
        ref3[k] = (uint32_t)graph.links[k].ref_idx;
        mov3[k] = (uint32_t)graph.links[k].mov_idx;
        const NDTFeatureLink &l = graph.links[k];
        double cov[36];
        const bool has_cov = l.cov_3d.rows() == 6 && l.cov_3d.cols() == 6;
        if (has_cov)
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) cov[6 * a + b] = l.cov_3d(a, b);
        ndtgpu_host::check(ndtgpu_pgo3_link_from_registration(l.T.data(), has_cov ? cov : nullptr, 0, &Z16[16 * k], &W36[36 * k]),
                           "ndtgpu_pgo3_link_from_registration");
    }
    ndtgpu_pgo3 *h3 = nullptr;
    ndtgpu_host::check(ndtgpu_pgo3_create(2, 30, 60, &h3), "ndtgpu_pgo3_create");
    ndtgpu_host::check(ndtgpu_pgo3_set_graph(h3, 1, n, N16.data(), m, ref3.data(), mov3.data(), Z16.data(), W36.data()), "ndtgpu_pgo3_set_graph");
    ndtgpu_host::check(ndtgpu_pgo3_optimize_robust(h3, 1, 1, nullptr, nullptr, nullptr, nullptr), "ndtgpu_pgo3_optimize_robust");
    ndtgpu_host::check(ndtgpu_pgo3_poses(h3, 1, T16.data(), nullptr), "ndtgpu_pgo3_poses");
    ndtgpu_host::check(ndtgpu_pgo3_robust_links(h3, 1, nullptr, wc3.data(), nullptr, &rc3), "ndtgpu_pgo3_robust_links");
    ndtgpu_pgo3_destroy(h3);
    int equal3 = 0;
    double worst3 = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) same = same && graph.nodes[i].T.data()[e] == T16[16 * i + e];
        CHECK(same, "SE(3) node %zu: the mirror differs from the C-ABI", i);
        equal3 += same ? 1 : 0;
        worst3 = std::max(worst3, (graph.nodes[i].T.translation() - truth[i].translation()).norm());
    }
    CHECK(w3.size() == m, "%zu weights", w3.size());
    for (size_t k = 0; k < w3.size(); k++) {
        CHECK(w3[k] == wc3[k], "SE(3) link %zu: weight %.17g, C-ABI %.17g", k, w3[k], wc3[k]);
        CHECK(k == false_link ? w3[k] < 1e-3 : w3[k] == 1.0, "SE(3) link %zu: weight %.6g", k, w3[k]);
    }
    CHECK(rm3.exit_code == NDTGPU_PGO_CONVERGED && rm3.exit_code == rc3.exit_code && rm3.rounds == rc3.rounds && rm3.cost_final == rc3.cost_final &&
              rm3.outliers == 1 && rc3.outliers == 1,
          "the SE(3) reports: exit %d / %d, rounds %d / %d, outliers %d / %d", rm3.exit_code, rc3.exit_code, rm3.rounds, rc3.rounds, rm3.outliers, rc3.outliers);
    CHECK(worst3 < 0.1, "SE(3): a node ends %.3f m from the truth", worst3);
    std::printf("pgo_robust_demo: %zu nodes, %zu links, SE(2) %d and SE(3) %d equal to the C-ABI bit for bit, false closure weighted %.3g / %.3g, "
                "%d / %d rounds, worst |dt| %.4f / %.4f m, %d failures\n",
                n, m, equal2, equal3, w2[false_link], w3[false_link], rm.rounds, rm3.rounds, worst2, worst3, g_fails);
    return g_fails ? 1 : 0;
}
