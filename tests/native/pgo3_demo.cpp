// pgo3_demo.cpp -- the host mirror's optimizeGraph3D (host/ndt_feature_graph_gpu.h) on a climbing loop of 12 nodes with 6-DoF
// links and their cov_3d, without force2D, against the ndtgpu_pgo3_* calls it wraps given the same factors by hand: the node
// poses must be those of the C-ABI bit for bit.  Exit code 0 = every check passed; without a GPU the library fails loudly
// (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// the part of NDTFeatureGraph that optimizeGraph3D sees (interfaces.h), without node maps
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
    // a loop of 12 nodes that climbs and tilts; the estimates have drifted from the truth
    std::vector<Eigen::Affine3d> truth(n);
    DemoGraph graph;
    graph.nodes.resize(n);
    for (size_t i = 0; i < n; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)n;
        truth[i] = ndtgpu_host::affine_from_pose(5.0 * std::cos(a), 4.0 * std::sin(a), 0.3 * std::sin(2.0 * a), 0.1 * std::cos(a), -0.08 * std::sin(a), a + 2.2);
        const double s = 0.01 * (double)i;
        graph.nodes[i].T = i == 0 ? truth[0] : truth[i] * ndtgpu_host::affine_from_pose(s * nd(rng), s * nd(rng), s * nd(rng), 0.5 * s * nd(rng), 0.5 * s * nd(rng), 0.5 * s * nd(rng));
    }
    auto add = [&](size_t ref, size_t mov, int kind) {
        NDTFeatureLink l(ref, mov);
        l.T = truth[ref].inverse() * truth[mov] * ndtgpu_host::affine_from_pose(0.01 * nd(rng), 0.01 * nd(rng), 0.01 * nd(rng), 0.005 * nd(rng), 0.005 * nd(rng), 0.005 * nd(rng));
        // kind 0: a covariance of the registrar's kind (positive definite, not diagonal); 1: one that does not invert (0.02 I
        // stands in); 2: none (100 I)
        if (kind == 0) {
            double A[6][6];
            for (auto &row : A)
                for (double &v : row) v = 0.01 * nd(rng);
            for (int r = 0; r < 6; r++)
                for (int c = 0; c < 6; c++) {
                    double s = r == c ? 1e-4 : 0.0;
                    for (int k = 0; k < 6; k++) s += A[r][k] * A[c][k];
                    l.cov_3d(r, c) = s;
                }
        } else if (kind == 2) {
            l.cov_3d.resize(0, 0);
        }
        graph.links.push_back(l);
    };
    for (size_t i = 0; i + 1 < n; i++) add(i, i + 1, 0);
    add(n - 1, 0, 0);
    add(2, 9, 1);
    add(10, 4, 2);

    // the same factors by hand, for the C-ABI
    const size_t m = graph.links.size();
    std::vector<double> T16(16 * n), Z16(16 * m), W36(36 * m);
    std::vector<uint32_t> ref(m), mov(m);
    for (size_t i = 0; i < n; i++)
        for (int e = 0; e < 16; e++) T16[16 * i + e] = graph.nodes[i].T.data()[e];
    for (size_t k = 0; k < m; k++) {
        const NDTFeatureLink &l = graph.links[k];
        ref[k] = (uint32_t)l.ref_idx;
        mov[k] = (uint32_t)l.mov_idx;
        double cov[36];
        const bool has = l.cov_3d.rows() == 6;
        for (int r = 0; has && r < 6; r++)
            for (int c = 0; c < 6; c++) cov[6 * r + c] = l.cov_3d(r, c);
        ndtgpu_host::check(ndtgpu_pgo3_link_from_registration(l.T.data(), has ? cov : nullptr, 0, &Z16[16 * k], &W36[36 * k]), "link_from_registration");
    }
    CHECK(W36[36 * (m - 2)] == 50.0 && W36[36 * (m - 2) + 1] == 0.0, "the link without an inverse has W(0, 0) = %g", W36[36 * (m - 2)]);
    CHECK(W36[36 * (m - 1)] == 100.0, "the link without a covariance has W(0, 0) = %g", W36[36 * (m - 1)]);
    CHECK(W36[0] != 50.0 && W36[1] != 0.0, "a registered link's W is its own");

    ndtgpu_pgo_result rm;
    try {
        optimizeGraph3D(graph, graph.links, nullptr, &rm);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo3_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }

    // a bank of another shape, the graph in its last slot
    ndtgpu_pgo3 *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo3_create(3, 40, 100, &h), "ndtgpu_pgo3_create");
    ndtgpu_host::check(ndtgpu_pgo3_set_graph(h, 2, n, T16.data(), m, ref.data(), mov.data(), Z16.data(), W36.data()), "ndtgpu_pgo3_set_graph");
    ndtgpu_host::check(ndtgpu_pgo3_optimize(h, 2, 1, nullptr, nullptr), "ndtgpu_pgo3_optimize");
    std::vector<double> out(16 * n);
    ndtgpu_pgo_result rc;
    ndtgpu_host::check(ndtgpu_pgo3_poses(h, 2, out.data(), &rc), "ndtgpu_pgo3_poses");
    ndtgpu_pgo3_destroy(h);

    int equal = 0;
    double worst = 0, tilt = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) same = same && graph.nodes[i].T.data()[e] == out[16 * i + e];
        CHECK(same, "node %zu: the mirror differs from the C-ABI", i);
        equal += same ? 1 : 0;
        const Eigen::Vector3d d = graph.nodes[i].T.translation() - truth[i].translation();
        worst = std::max(worst, d.norm());
        tilt = std::max(tilt, std::fabs(graph.nodes[i].T(2, 0)));
    }
    CHECK(rm.exit_code == NDTGPU_PGO_CONVERGED && rc.exit_code == NDTGPU_PGO_CONVERGED, "exit codes %d / %d", rm.exit_code, rc.exit_code);
    CHECK(rm.iterations == rc.iterations && rm.linear_iterations == rc.linear_iterations && rm.cost_final == rc.cost_final &&
              rm.cost_initial == rc.cost_initial && rm.max_step == rc.max_step,
          "the reports differ");
    CHECK(rm.n_nodes == (int)n && rm.n_edges == (int)m, "%d nodes, %d factors", rm.n_nodes, rm.n_edges);
    CHECK(rm.cost_final < rm.cost_initial, "cost %.6g -> %.6g", rm.cost_initial, rm.cost_final);
    // (a sanity bound: 12 links of 0.005 rad noise at a lever of up to 10 m put the far side of the loop some 0.17 m off at 1 sigma)
    CHECK(worst < 0.5, "a node ends %.3f m from the truth", worst);
    CHECK(tilt > 0.01, "the poses were flattened (largest |R(2, 0)| %.3g)", tilt);
    std::printf("pgo3_demo: %zu nodes, %d factors, %d equal to the C-ABI bit for bit, cost %.6g -> %.6g in %d updates, worst |dt| %.4f m, "
                "%d failures\n", n, rm.n_edges, equal, rm.cost_initial, rm.cost_final, rm.iterations, worst, g_fails);
    return g_fails ? 1 : 0;
}
