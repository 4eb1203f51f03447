// pgo_wide_demo.cpp -- the host mirror's optimizeGraphUsingISAM(graph, wide) (host/ndt_feature_graph_gpu.h) on a loop of 40 nodes:
// wide = true must give the node poses of ndtgpu_pgo_optimize_wide given the same factors by hand, bit for bit, the default
// (and wide = false) those of ndtgpu_pgo_optimize.  Exit code 0 = every check passed; without a GPU the library fails loudly
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
    const size_t n = 40;
    std::mt19937 rng(40);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::vector<Eigen::Affine3d> truth(n);
    DemoGraph start;
    start.nodes.resize(n);
    for (size_t i = 0; i < n; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)n;
        truth[i] = ndtgpu_host::affine_from_pose(6.0 * std::cos(a), 5.0 * std::sin(a), 0, 0, 0, a + 1.1);
        start.nodes[i].T = i == 0 ? truth[0]
                                  : truth[i] * ndtgpu_host::affine_from_pose(0.005 * (double)i * nd(rng), 0.005 * (double)i * nd(rng), 0, 0, 0, 0.002 * (double)i * nd(rng));
    }
    auto add = [&](size_t ref, size_t mov, double score) {
        NDTFeatureLink l(ref, mov);
        l.T = truth[ref].inverse() * truth[mov] * ndtgpu_host::affine_from_pose(0.01 * nd(rng), 0.01 * nd(rng), 0, 0, 0, 0.005 * nd(rng));
        l.score = score;
        start.links.push_back(l);
    };
    for (size_t i = 0; i + 1 < n; i++) add(i, i + 1, -1.);        // getIncrementalLinks: score -1
    add(n - 1, 0, 0.3);                                           // registered links (getValidLinks)
    for (size_t i = 0; i + 9 < n; i += 4) add(i, i + 9, 0.2);

    // the same factors by hand, the links with score < 0 twice (ndt_offline_mapper.h:74-93)
    std::vector<double> pose(3 * n), meas;
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < n; i++) {
        pose[3 * i] = start.nodes[i].T.translation()(0);
        pose[3 * i + 1] = start.nodes[i].T.translation()(1);
        pose[3 * i + 2] = getRobustYawFromAffine3d(start.nodes[i].T);
    }
    for (int pass = 0; pass < 2; pass++)
        for (const NDTFeatureLink &l : start.links) {
            if (pass == 0 && l.score >= 0.) continue;
            ref.push_back((uint32_t)l.ref_idx);
            mov.push_back((uint32_t)l.mov_idx);
            meas.push_back(l.T.translation()(0));
            meas.push_back(l.T.translation()(1));
            meas.push_back(getRobustYawFromAffine3d(l.T));
        }

    DemoGraph by_default = start, one = start, wide = start;
    ndtgpu_pgo_result rw;
    try {
        optimizeGraphUsingISAM(by_default);
        optimizeGraphUsingISAM(one, false);
        optimizeGraphUsingISAM(wide, nullptr, &rw, true);
        DemoGraph again = start;
        optimizeGraphUsingISAM(again, true);
        for (size_t i = 0; i < n; i++)
            for (int e = 0; e < 16; e++) CHECK(again.nodes[i].T.data()[e] == wide.nodes[i].T.data()[e], "node %zu: the two wide overloads differ", i);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo_wide_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(rw.exit_code == NDTGPU_PGO_CONVERGED && rw.iterations >= 1 && rw.n_nodes == (int)n && rw.n_edges == (int)ref.size(), "report: exit %d", rw.exit_code);

    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(2, 64, 200, &h), "ndtgpu_pgo_create");
    for (size_t g = 0; g < 2; g++)
        ndtgpu_host::check(ndtgpu_pgo_set_graph(h, g, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr), "ndtgpu_pgo_set_graph");
    ndtgpu_host::check(ndtgpu_pgo_optimize(h, 0, 1, nullptr, nullptr), "ndtgpu_pgo_optimize");
    ndtgpu_host::check(ndtgpu_pgo_optimize_wide(h, 1, nullptr, nullptr, nullptr), "ndtgpu_pgo_optimize_wide");
    std::vector<double> out(3 * n), T1(16 * n), Tw(16 * n);
    ndtgpu_pgo_result r1, r2;
    ndtgpu_host::check(ndtgpu_pgo_poses(h, 0, out.data(), T1.data(), &r1), "ndtgpu_pgo_poses");
    ndtgpu_host::check(ndtgpu_pgo_poses(h, 1, out.data(), Tw.data(), &r2), "ndtgpu_pgo_poses");
    ndtgpu_pgo_destroy(h);
    CHECK(r2.linear_iterations == rw.linear_iterations && r2.cost_final == rw.cost_final, "the wide report differs from the C-ABI's");

    int equal = 0;
    for (size_t i = 0; i < n; i++) {
        bool same1 = true, samew = true;
        for (int e = 0; e < 16; e++) {
            same1 = same1 && by_default.nodes[i].T.data()[e] == T1[16 * i + e] && one.nodes[i].T.data()[e] == T1[16 * i + e];
            samew = samew && wide.nodes[i].T.data()[e] == Tw[16 * i + e];
        }
        CHECK(same1, "node %zu: the default form differs from ndtgpu_pgo_optimize", i);
        CHECK(samew, "node %zu: the wide form differs from ndtgpu_pgo_optimize_wide", i);
        equal += (same1 && samew) ? 1 : 0;
    }
    std::printf("pgo_wide_demo: %zu nodes, %zu factors, %d equal to the C-ABI bit for bit in both forms, %d failures\n", n, ref.size(), equal, g_fails);
    return g_fails ? 1 : 0;
}
