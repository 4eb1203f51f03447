// world_demo.cpp -- the host mirror's assembleWorldMap (host/ndt_feature_graph_gpu.h): a graph is driven along a corridor the way
// ndt_feature2d_fuser.cpp drives it, then every node's map is put under the node's pose into ONE world map with one call, and the
// world is checked against the node maps: every node cell's moved mean lies in a world cell that holds a Gaussian, the point
// counts add up, a single node under the identity on the nodes' own grid reproduces itself, and the world serves as the map of a
// matcher call.  Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <map>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// a closed corridor (two wavy walls + two end walls) seen from `sensor_pose_world`; points in the sensor frame
static pcl::PointCloud<pcl::PointXYZ> corridor_scan(const Eigen::Affine3d &sensor_pose_world, unsigned seed, int n_beams = 6000)
{
    std::mt19937 rng(seed);
    std::normal_distribution<double> nd(0.0, 0.03);
    std::uniform_real_distribution<double> uz(0.0, 0.02);
    pcl::PointCloud<pcl::PointXYZ> pc;
    const double ox = sensor_pose_world(0, 3), oy = sensor_pose_world(1, 3);
    const double yaw = std::atan2(sensor_pose_world(1, 0), sensor_pose_world(0, 0));
    for (int j = 0; j < n_beams; j++) {
        const double phi = -M_PI + 2.0 * M_PI * (j + 0.5) / n_beams, a = phi + yaw;
        const double dx = std::cos(a), dy = std::sin(a);
        double r = 0.0;
        for (; r < 40.0; r += 0.02) {
            const double x = ox + r * dx, y = oy + r * dy;
            if (x < -9.0 || x > 13.0 || y > 2.0 + 0.3 * std::sin(0.9 * x) || y < -2.0 - 0.2 * std::cos(0.7 * x)) break;
        }
        r += nd(rng);
        if (r < 0.3 || r > 30.0) continue;
        pc.push_back(pcl::PointXYZ((float)(r * std::cos(phi)), (float)(r * std::sin(phi)), (float)uz(rng)));
    }
    return pc;
}

// LazyGrid::getIndexForPoint along one axis
static int cell_index(double p, double centre, double res, int size) { return (int)(std::floor((p - centre) / res + 0.5) + size / 2.0); }

int main()
{
    NDTFeatureFuserHMT::Params fp;
    fp.resolution = 0.5; fp.map_size_x = 30; fp.map_size_y = 30; fp.map_size_z = 1.0; fp.sensor_range = 30;
    fp.useNDT = true; fp.useFeat = false; fp.useOdom = false;
    fp.neighbours = 2; fp.stepcontrol = true; fp.ITR_MAX = 30; fp.DELTA_SCORE = 1e-6;
    NDTFeatureGraph::Params gp;
    gp.newNodeTranslDist = 1.0;
    gp.maxNodes = 8;
    InterestPointVec no_pts;
    NDTFeatureGraph graph(gp, fp);
    const int K = 14;
    std::vector<Eigen::Affine3d> gt;
    for (int k = 0; k < K; k++) gt.push_back(ndtgpu_host::affine_from_pose(-6.0 + 0.3 * k, 0.05 * std::sin(0.7 * k), 0, 0, 0, 0.015 * k));
    try {
        pcl::PointCloud<pcl::PointXYZ> pc = corridor_scan(gt[0], 100);
        graph.initialize(gt[0], pc, no_pts);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("world_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    for (int k = 1; k < K; k++) {
        const Eigen::Affine3d inc = gt[k - 1].inverse() * gt[k];
        pcl::PointCloud<pcl::PointXYZ> pc = corridor_scan(gt[k], 100 + k);
        graph.update(inc, pc, no_pts);
    }
    const size_t n_nodes = graph.getNbNodes();
    CHECK(n_nodes >= 3, "%zu nodes", n_nodes);

    // the world: 48 x 48 x 1 m around the origin at the nodes' resolution
    const double res = fp.resolution, wsize[3] = {48., 48., 1.};
    lslgeneric::NDTMap world(new lslgeneric::LazyGrid(res));
    world.guessSize(0., 0., 0., wsize[0], wsize[1], wsize[2]);
    const ndtgpu_world_result r = assembleWorldMap(graph, world);
    int32_t cpa[3];
    ndtgpu_host::check(ndtgpu_mapset_info(world.handle(), nullptr, cpa, nullptr), "mapset_info");
    CHECK(r.n_nodes == (int)n_nodes && r.overflow == 0 && r.n_rejected == 0, "report: %d nodes, overflow %d, %lld rejected", r.n_nodes, r.overflow,
          (long long)r.n_rejected);
    CHECK(r.n_cells == world.numberOfActiveCells() && r.n_cells > 30, "%d world cells", r.n_cells);

    // the world's cells by index, and what the nodes' cells say they should hold
    std::map<long long, long long> world_n, want_n;
    long long world_points = 0;
    {
        std::vector<lslgeneric::NDTCell *> cells = world.getAllCells();
        for (lslgeneric::NDTCell *c : cells) {
            const Eigen::Vector3d m = c->getMean();
            const long long key = ((long long)cell_index(m(0), 0., res, cpa[0]) * cpa[1] + cell_index(m(1), 0., res, cpa[1])) * cpa[2] + cell_index(m(2), 0., res, cpa[2]);
            world_n[key] = c->getN();
            world_points += c->getN();
            delete c;
        }
    }
    long long contributions = 0, dropped = 0, node_points = 0;
    for (size_t i = 0; i < n_nodes; i++) {
        std::vector<lslgeneric::NDTCell *> cells = graph.getMap((int)i)->pseudoTransformNDT(graph.getNode(i).T);
        for (lslgeneric::NDTCell *c : cells) {
            const Eigen::Vector3d m = c->getMean();
            const int ix = cell_index(m(0), 0., res, cpa[0]), iy = cell_index(m(1), 0., res, cpa[1]), iz = cell_index(m(2), 0., res, cpa[2]);
            contributions++;
            if (ix < 0 || ix >= cpa[0] || iy < 0 || iy >= cpa[1] || iz < 0 || iz >= cpa[2]) dropped++;
            else {
                const long long n = std::max<long long>(c->getN(), 2);
                want_n[((long long)ix * cpa[1] + iy) * cpa[2] + iz] += n;
                node_points += n;
            }
            delete c;
        }
    }
    CHECK(r.n_contributions == contributions && r.n_dropped == dropped && r.n_points == node_points,
          "report: %lld / %lld contributions, %lld / %lld dropped, %lld / %lld points", (long long)r.n_contributions, contributions,
          (long long)r.n_dropped, dropped, (long long)r.n_points, node_points);
    size_t same = 0;
    for (const auto &kv : world_n) {
        auto it = want_n.find(kv.first);
        if (it != want_n.end() && it->second == kv.second) same++;
    }
    // (a merged cell may come out rank deficient and get no Gaussian: the world may hold fewer cells than the nodes touch, never others)
    CHECK(same == world_n.size() && world_n.size() <= want_n.size() && 10 * world_n.size() >= 9 * want_n.size(),
          "%zu world cells, %zu with the nodes' point count, %zu touched by the nodes", world_n.size(), same, want_n.size());
    CHECK(world_points <= node_points, "%lld points in the world, %lld in the nodes", world_points, node_points);

    // one node under the identity on the nodes' own grid reproduces itself
    lslgeneric::NDTMap copy(new lslgeneric::LazyGrid(res));
    {
        double cx, cy, cz;
        graph.getMap(0)->getCentroid(cx, cy, cz);
        copy.guessSize(cx, cy, cz, fp.map_size_x, fp.map_size_y, fp.map_size_z);
    }
    const ndtgpu_world_result r1 = assembleWorldMap({graph.getMap(0)}, {Eigen::Affine3d::Identity()}, copy);
    {
        std::vector<lslgeneric::NDTCell *> a = graph.getMap(0)->getAllCells(), b = copy.getAllCells();
        CHECK(a.size() == b.size() && r1.n_cells == (int)a.size() && r1.n_dropped == 0, "identity copy: %zu / %zu cells", b.size(), a.size());
        double worst_m = 0, worst_c = 0;
        for (size_t k = 0; k < a.size() && k < b.size(); k++) {
            CHECK(a[k]->getN() == b[k]->getN(), "cell %zu: n %d / %d", k, (int)b[k]->getN(), (int)a[k]->getN());
            const Eigen::Vector3d ma = a[k]->getMean(), mb = b[k]->getMean();
            const Eigen::Matrix3d ca = a[k]->getCov(), cb = b[k]->getCov();
            for (int r = 0; r < 3; r++) {
                worst_m = std::max(worst_m, std::fabs(ma(r) - mb(r)));
                for (int c = 0; c < 3; c++) worst_c = std::max(worst_c, std::fabs(ca(r, c) - cb(r, c)));
            }
        }
        CHECK(worst_m < 1e-13 && worst_c < 1e-13, "identity copy: mean off by %.3g, covariance by %.3g", worst_m, worst_c);
        for (auto *c : a) delete c;
        for (auto *c : b) delete c;
    }

    // the world as the map of a consumer: the last node's map registers against it at the node's pose
    lslgeneric::NDTMatcherD2D matcher;
    Eigen::Affine3d T = graph.getNode(n_nodes - 1).T * ndtgpu_host::affine_from_pose(0.05, -0.04, 0, 0, 0, 0.01);
    const bool ok = matcher.match(world, *graph.getMap((int)n_nodes - 1), T, true);
    const Eigen::Affine3d rel = graph.getNode(n_nodes - 1).T.inverse() * T;
    CHECK(ok && rel.translation().norm() < 0.05, "registration against the world: converged %d, %.4f m from the node's pose", (int)ok, rel.translation().norm());

    std::printf("world_demo: %zu nodes, %lld contributions (%lld dropped) -> %d world cells, %lld points; identity copy of %d cells; "
                "registration against the world ends %.4f m from the node's pose; %d failures\n",
                n_nodes, contributions, dropped, r.n_cells, (long long)r.n_points, r1.n_cells, rel.translation().norm(), g_fails);
    return g_fails ? 1 : 0;
}
