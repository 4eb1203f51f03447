// pgo_marginals_demo.cpp -- the host mirror's optimizeGraphUsingISAMWithCov and optimizeGraph3DWithCov
// (host/ndt_feature_graph_gpu.h) on the 12-node graph of pgo_demo.cpp: the node poses must be those of optimizeGraphUsingISAM /
// optimizeGraph3D bit for bit, every node's getCov() the block the C-ABI (ndtgpu_pgo_optimize, then ndtgpu_pgo_marginals) returns
// for the same factors -- the links with score < 0 twice -- bit for bit, and node 0's the inverse of the prior.  Exit code 0 = every
// check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <algorithm>
#include <cmath>
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

// a node's 3x3 covariance against v * I: the largest |entry difference|
static double off_identity(const Eigen::Matrix3d &C, double v)
{
    double d = 0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) d = std::max(d, std::fabs(C(a, b) - (a == b ? v : 0.0)));
    return d;
}

static bool same_pose(const Eigen::Affine3d &a, const Eigen::Affine3d &b)
{
    bool same = true;
    for (int e = 0; e < 16; e++) same = same && a.data()[e] == b.data()[e];
    return same;
}

int main()
{
    const size_t n = 12;
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
        graph.nodes[i].cov.setIdentity();                            // what "the fuser left there": 7 * I
        for (int a = 0; a < 3; a++) graph.nodes[i].cov(a, a) = 7.0;
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
    DemoGraph plain = graph, plain3 = graph, with3 = graph;

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

    ndtgpu_pgo_result rm, rp;
    std::vector<ndtgpu_pgo_marginal_result> records;
    try {
        optimizeGraphUsingISAMWithCov(graph, nullptr, &rm, &records);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo_marginals_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    optimizeGraphUsingISAM(plain, nullptr, &rp);

    // a bank of another shape, the graph in its last slot, every node queried in reversed order
    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(3, 40, 100, &h), "ndtgpu_pgo_create");
    ndtgpu_host::check(ndtgpu_pgo_set_graph(h, 2, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr), "ndtgpu_pgo_set_graph");
    ndtgpu_host::check(ndtgpu_pgo_optimize(h, 2, 1, nullptr, nullptr), "ndtgpu_pgo_optimize");
    std::vector<uint32_t> gi(n, 2), qi(n);
    for (size_t i = 0; i < n; i++) qi[i] = (uint32_t)(n - 1 - i);
    std::vector<double> cov9(9 * n);
    std::vector<ndtgpu_pgo_marginal_result> rc(n);
    ndtgpu_host::check(ndtgpu_pgo_marginals(h, n, gi.data(), qi.data(), nullptr, nullptr, nullptr, cov9.data(), nullptr, rc.data()), "ndtgpu_pgo_marginals");
    ndtgpu_pgo_destroy(h);

    int poses_equal = 0, covs_equal = 0;
    double trace = 0;
    for (size_t i = 0; i < n; i++) {
        const bool same = same_pose(graph.nodes[i].T, plain.nodes[i].T);
        CHECK(same, "node %zu: the pose differs from optimizeGraphUsingISAM's", i);
        poses_equal += same ? 1 : 0;
        const Eigen::Matrix3d &C = graph.getNodeInterface(i).getCov();
        const double *want = &cov9[9 * (n - 1 - i)];
        bool cs = true;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) cs = cs && C(a, b) == want[3 * a + b];
        CHECK(cs, "node %zu: getCov() differs from the C-ABI's block", i);
        covs_equal += cs ? 1 : 0;
        CHECK(C(0, 0) > 0 && C(1, 1) > 0 && C(2, 2) > 0 && C(0, 0) < 7.0, "node %zu: covariance diagonal %.3g %.3g %.3g", i, C(0, 0), C(1, 1), C(2, 2));
        CHECK(records[i].exit_code == NDTGPU_PGO_CONVERGED && records[i].capped_columns == 0 && records[i].linear_iterations >= 3,
              "node %zu: record %d / %d / %d", i, records[i].exit_code, records[i].capped_columns, records[i].linear_iterations);
        CHECK(records[i].linear_iterations == rc[n - 1 - i].linear_iterations && records[i].asymmetry == rc[n - 1 - i].asymmetry, "node %zu: the records differ", i);
        trace += C(0, 0) + C(1, 1) + C(2, 2);
        CHECK(off_identity(plain.nodes[i].cov, 7.0) == 0.0, "node %zu: optimizeGraphUsingISAM touched cov", i);
    }
    CHECK(rm.iterations == rp.iterations && rm.cost_final == rp.cost_final && rm.linear_iterations == rp.linear_iterations, "the reports differ");
    // (H^-1)[0, 0] is the prior's inverse, 0.01 I.  A column stops at |r| <= eps_linear |b| = 1e-8, so it is within |H^-1| 1e-8 of the
    // exact one, and the trace of H^-1 -- the sum of the nodes' traces -- bounds |H^-1|
    const double tol = 1e-8 * trace;
    const double off0 = off_identity(graph.nodes[0].cov, 0.01);
    CHECK(off0 <= tol, "node 0's covariance is %.3g off the prior's inverse (allowed %.3g)", off0, tol);

    // SE(3): the same nodes and links (no cov_3d: 100 * I6 per link, every link once)
    std::vector<double> cov36;
    std::vector<ndtgpu_pgo_marginal_result> records3;
    ndtgpu_pgo_result r3, r3p;
    optimizeGraph3DWithCov(with3, with3.links, cov36, nullptr, &r3, &records3);
    optimizeGraph3D(plain3, plain3.links, nullptr, &r3p);
    CHECK(cov36.size() == 36 * n && records3.size() == n, "%zu doubles, %zu records", cov36.size(), records3.size());
    int poses3_equal = 0;
    double trace3 = 0, off3 = 0;
    for (size_t i = 0; i < n; i++) {
        const bool same = same_pose(with3.nodes[i].T, plain3.nodes[i].T);
        CHECK(same, "node %zu: the pose differs from optimizeGraph3D's", i);
        poses3_equal += same ? 1 : 0;
        CHECK(records3[i].exit_code == NDTGPU_PGO_CONVERGED, "node %zu: exit code %d", i, records3[i].exit_code);
        for (int a = 0; a < 6; a++) trace3 += cov36[36 * i + 7 * a];
        CHECK(off_identity(with3.nodes[i].cov, 7.0) == 0.0, "node %zu: optimizeGraph3DWithCov touched the 3x3 cov", i);
    }
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) off3 = std::max(off3, std::fabs(cov36[6 * a + b] - (a == b ? 0.01 : 0.0)));
    CHECK(off3 <= 1e-8 * trace3, "node 0's 6x6 covariance is %.3g off the prior's inverse (allowed %.3g)", off3, 1e-8 * trace3);
    CHECK(r3.cost_final == r3p.cost_final && r3.iterations == r3p.iterations, "the SE(3) reports differ");

    std::printf("pgo_marginals_demo: %zu nodes, %d factors, %d poses and %d covariances equal bit for bit, node 0 %.3g off 0.01 I (allowed %.3g); "
                "SE(3): %d poses equal, node 0 %.3g off (allowed %.3g), %d failures\n",
                n, rm.n_edges, poses_equal, covs_equal, off0, tol, poses3_equal, off3, 1e-8 * trace3, g_fails);
    return g_fails ? 1 : 0;
}
