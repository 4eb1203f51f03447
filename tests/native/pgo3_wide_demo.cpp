// pgo3_wide_demo.cpp -- the host mirror's optimizeGraph3D(graph, links, params, result, wide) (host/ndt_feature_graph_gpu.h) on
// a graph read from a file (tests/test_host_pgo3_wide.py writes the hub graph of tests/pgo3_wide_graphs.py: 588 nodes in three
// node tiles, 1817 links in eight link tiles): wide = true must give the node poses of ndtgpu_pgo3_optimize_wide given the same
// factors by hand, bit for bit, and agree with wide = false within the pose and cost tolerances given on the command line (the
// test passes twice the graph's tolerance).  Exit code 0 = every check passed; without a GPU the library fails loudly (exit
// code 3).
// usage: pgo3_wide_demo GRAPH POSE_TOLERANCE COST_RTOL
//   GRAPH: text; "n m", then n lines of a node's pose (16 numbers, column-major), then m lines "ref mov" and the link's T (16
//   numbers, column-major).  Every link is taken without a covariance: 100 * I6.
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <cstdlib>

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

static bool read16(FILE *f, double *T)
{
    for (int e = 0; e < 16; e++)
        if (std::fscanf(f, "%lf", &T[e]) != 1) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::printf("usage: pgo3_wide_demo GRAPH POSE_TOLERANCE COST_RTOL\n");
        return 2;
    }
    const double tol = std::atof(argv[2]), cost_rtol = std::atof(argv[3]);
    FILE *f = std::fopen(argv[1], "r");
    size_t n = 0, m = 0;
    if (!f || std::fscanf(f, "%zu %zu", &n, &m) != 2 || n == 0) {
        std::printf("pgo3_wide_demo: cannot read %s\n", argv[1]);
        return 2;
    }
    DemoGraph start;
    start.nodes.resize(n);
    std::vector<double> T16(16 * n), Z16(16 * m), W36(36 * m);
    std::vector<uint32_t> ref(m), mov(m);
    bool ok = true;
    for (size_t i = 0; ok && i < n; i++) {
        ok = read16(f, &T16[16 * i]);
        std::copy_n(&T16[16 * i], 16, start.nodes[i].T.data());
    }
    for (size_t k = 0; ok && k < m; k++) {
        unsigned a = 0, b = 0;
        double T[16];
        ok = std::fscanf(f, "%u %u", &a, &b) == 2 && read16(f, T);
        NDTFeatureLink l(a, b);
        std::copy_n(T, 16, l.T.data());
        l.cov_3d.resize(0, 0);                                    // (no covariance: 100 * I6)
        start.links.push_back(l);
        // the same factor by hand, for the C-ABI
        ref[k] = a;
        mov[k] = b;
        if (ok) ndtgpu_host::check(ndtgpu_pgo3_link_from_registration(T, nullptr, 0, &Z16[16 * k], &W36[36 * k]), "link_from_registration");
    }
    std::fclose(f);
    if (!ok) {
        std::printf("pgo3_wide_demo: %s ends early\n", argv[1]);
        return 2;
    }
    uint32_t tile = 0;
    size_t node_tiles = 0, link_tiles = 0;
    ndtgpu_host::check(ndtgpu_pgo3_wide_plan(n, m, &tile, &node_tiles, &link_tiles, nullptr), "ndtgpu_pgo3_wide_plan");
    CHECK(tile == 256 && node_tiles > 1 && link_tiles > 1, "the graph spans %zu node tiles and %zu link tiles", node_tiles, link_tiles);

    DemoGraph one = start, wide = start;
    ndtgpu_pgo_result r1, rw;
    try {
        optimizeGraph3D(one, one.links, nullptr, &r1);
        optimizeGraph3D(wide, wide.links, nullptr, &rw, true);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("pgo3_wide_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(r1.exit_code == NDTGPU_PGO_CONVERGED && rw.exit_code == NDTGPU_PGO_CONVERGED, "exit codes %d / %d", r1.exit_code, rw.exit_code);
    CHECK(rw.iterations >= 1 && rw.n_nodes == (int)n && rw.n_edges == (int)m, "report: %d nodes, %d factors", rw.n_nodes, rw.n_edges);
    CHECK(rw.cost_final < rw.cost_initial, "cost %.6g -> %.6g", rw.cost_initial, rw.cost_final);

    // a bank of another shape, the graph in its last slot
    ndtgpu_pgo3 *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo3_create(2, n + 7, m + 11, &h), "ndtgpu_pgo3_create");
    ndtgpu_host::check(ndtgpu_pgo3_set_graph(h, 1, n, T16.data(), m, ref.data(), mov.data(), Z16.data(), W36.data()), "ndtgpu_pgo3_set_graph");
    ndtgpu_host::check(ndtgpu_pgo3_optimize_wide(h, 1, nullptr, nullptr, nullptr), "ndtgpu_pgo3_optimize_wide");
    std::vector<double> out(16 * n);
    ndtgpu_pgo_result rc;
    ndtgpu_host::check(ndtgpu_pgo3_poses(h, 1, out.data(), &rc), "ndtgpu_pgo3_poses");
    ndtgpu_pgo3_destroy(h);
    CHECK(rc.iterations == rw.iterations && rc.linear_iterations == rw.linear_iterations && rc.cost_final == rw.cost_final &&
              rc.cost_initial == rw.cost_initial && rc.max_step == rw.max_step,
          "the wide report differs from the C-ABI's");

    int equal = 0;
    double worst = 0;
    for (size_t i = 0; i < n; i++) {
        bool same = true;
        for (int e = 0; e < 16; e++) {
            same = same && wide.nodes[i].T.data()[e] == out[16 * i + e];
            worst = std::max(worst, std::fabs(wide.nodes[i].T.data()[e] - one.nodes[i].T.data()[e]));
        }
        CHECK(same, "node %zu: the wide form differs from ndtgpu_pgo3_optimize_wide", i);
        equal += same ? 1 : 0;
    }
    const double dc = std::fabs(rw.cost_final - r1.cost_final) / r1.cost_final;
    CHECK(worst <= tol, "wide and one workgroup differ by %.3g (allowed %.3g)", worst, tol);
    CHECK(dc <= cost_rtol, "cost_final differs by %.3g relative (allowed %.3g)", dc, cost_rtol);
    std::printf("pgo3_wide_demo: %zu nodes (%zu tiles), %zu factors (%zu tiles), %d equal to the C-ABI bit for bit, wide %d updates / %d inner "
                "iterations, one workgroup %d / %d, largest pose difference %.3g (allowed %.3g), cost %.3g relative (allowed %.3g), %d failures\n",
                n, node_tiles, m, link_tiles, equal, rw.iterations, rw.linear_iterations, r1.iterations, r1.linear_iterations, worst, tol, dc,
                cost_rtol, g_fails);
    return g_fails ? 1 : 0;
}
