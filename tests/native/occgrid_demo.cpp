// occgrid_demo.cpp -- the host mirror's toOccupancyGrid / moveOccupancyMap (host/ndt_occupancy_grid_gpu.h): a graph is driven along
// a short corridor the way ndt_feature2d_fuser.cpp drives it, its node maps are assembled into one world map, and the world and
// one node map are rasterised the way the fuser's publish timer does it (ndt_feature2d_fuser.cpp:428-433, 450-454).  Both grids
// are checked pixel by pixel against the cells (and occupancies) the maps export: the class of every pixel (unknown / free /
// occupied) and, where the cell holds a Gaussian, the value recomputed on the host.  Exit code 0 = every check passed; without
// a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"
#include "ndt_occupancy_grid_gpu.h"

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

// LazyGrid::getIndexForPoint along one axis (-1: outside)
static int cell_index(double p, double centre, double res, int size)
{
    const int k = (int)(std::floor((p - centre) / res + 0.5) + size / 2.0);
    return k >= 0 && k < size ? k : -1;
}

struct GridCheck { long long unknown = 0, free_ = 0, occupied = 0, gaussian = 0, on_face = 0, wrong_class = 0, wrong_value = 0; };

// distance of p to the nearest cell face along one axis
static double face_distance(double p, double centre, double res)
{
    const double t = (p - centre) / res + 0.5;
    return std::fabs(t - std::round(t)) * res;
}

// every pixel of `g` against the map's exported cells and (with_occ) occupancies
static GridCheck check_grid(lslgeneric::NDTMap &map, const OccupancyGridGPU &g, double r, bool with_occ)
{
    GridCheck c;
    int32_t cpa[3];
    ndtgpu_host::check(ndtgpu_mapset_info(map.handle(), nullptr, cpa, nullptr), "mapset_info");
    const double res = map.resolution();
    const double ox = g.info.origin.position.x, oy = g.info.origin.position.y;
    double cx, cy, cz;
    map.getCentroid(cx, cy, cz);
    if (ox != cx - cpa[0] * res / 2 || oy != cy - cpa[1] * res / 2) c.wrong_class++;      // the origin is the map's lower corner
    std::map<long long, lslgeneric::NDTCell *> by_slot;
    std::vector<lslgeneric::NDTCell *> cells = map.getAllCells();
    for (lslgeneric::NDTCell *k : cells) by_slot[((long long)k->idx[0] * cpa[1] + k->idx[1]) * cpa[2] + k->idx[2]] = k;
    std::vector<float> occ;
    if (with_occ) occ = map.getOccupancy();
    const int iz = cell_index(0.0, cz, res, cpa[2]);
    for (uint32_t j = 0; j < g.info.height; j++)
        for (uint32_t i = 0; i < g.info.width; i++) {
            const double px = ox + (i + 0.5) * r, py = oy + (j + 0.5) * r;
            const int v = g.data[(size_t)j * g.info.width + i];
            const int ix = cell_index(px, cx, res, cpa[0]), iy = cell_index(py, cy, res, cpa[1]);
            int want_lo = -1, want_hi = -1;
            if (ix >= 0 && iy >= 0 && iz >= 0) {
                const long long slot = ((long long)ix * cpa[1] + iy) * cpa[2] + iz;
                auto it = by_slot.find(slot);
                const double o = with_occ ? occ[(size_t)slot] : (it != by_slot.end() ? 1.0 : 0.0);
                if (o < 0) want_lo = want_hi = 0;
                else if (o > 0 && it == by_slot.end()) want_lo = want_hi = 100;
                else if (o > 0) {
                    const Eigen::Vector3d m = it->second->getMean();
                    const Eigen::Matrix3d S = it->second->getCov();
                    const double a = S(0, 0), b = S(0, 1), cc = S(0, 2), d = S(1, 1), e = S(1, 2), f = S(2, 2);
                    const double c00 = d * f - e * e, c01 = e * cc - b * f, c02 = b * e - d * cc;
                    const double det = a * c00 + b * c01 + cc * c02;
                    const double dx = px - m(0), dy = py - m(1), dz = 0.0 - m(2);
                    const double i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i11 = (a * f - cc * cc) / det, i12 = (b * cc - a * e) / det,
                                 i22 = (a * d - b * b) / det;
                    const double l = dx * (i00 * dx + i01 * dy + i02 * dz) + dy * (i01 * dx + i11 * dy + i12 * dz) + dz * (i02 * dx + i12 * dy + i22 * dz);
                    const double vv = 0.5 + 0.5 * (std::exp(-l / 2) + 0.1);
                    const int val = vv > 1 ? 100 : (int)(vv * 100);
                    // (one count of slack: 100 v next to an integer may truncate either way between two exp implementations)
                    want_lo = std::max(55, val - 1);
                    want_hi = std::min(100, val + 1);
                    c.gaussian++;
                }
            }
            if (v < 0) c.unknown++;
            else if (v == 0) c.free_++;
            else c.occupied++;
            // (a pixel centre within 1e-9 m of a cell face may fall either way between this arithmetic and the device's: counted only)
            if (face_distance(px, cx, res) < 1e-9 || face_distance(py, cy, res) < 1e-9) { c.on_face++; continue; }
            const bool same_class = (v < 0) == (want_lo < 0) && (v == 0) == (want_lo == 0);
            if (!same_class) c.wrong_class++;
            else if (v < want_lo || v > want_hi) c.wrong_value++;
        }
    for (auto *k : cells) delete k;
    return c;
}

int main()
{
    NDTFeatureFuserHMT::Params fp;
    fp.resolution = 0.5; fp.map_size_x = 30; fp.map_size_y = 30; fp.map_size_z = 1.0; fp.sensor_range = 30;
    fp.useNDT = true; fp.useFeat = false; fp.useOdom = false;
    fp.neighbours = 2; fp.stepcontrol = true; fp.ITR_MAX = 30; fp.DELTA_SCORE = 1e-6;
    NDTFeatureGraph::Params gp;
    gp.newNodeTranslDist = 1.0;
    gp.maxNodes = 6;
    InterestPointVec no_pts;
    NDTFeatureGraph graph(gp, fp);
    const int K = 9;
    std::vector<Eigen::Affine3d> gt;
    for (int k = 0; k < K; k++) gt.push_back(ndtgpu_host::affine_from_pose(-3.0 + 0.3 * k, 0.05 * std::sin(0.7 * k), 0, 0, 0, 0.015 * k));
    try {
        pcl::PointCloud<pcl::PointXYZ> pc = corridor_scan(gt[0], 100);
        graph.initialize(gt[0], pc, no_pts);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("occgrid_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    for (int k = 1; k < K; k++) {
        const Eigen::Affine3d inc = gt[k - 1].inverse() * gt[k];
        pcl::PointCloud<pcl::PointXYZ> pc = corridor_scan(gt[k], 100 + k);
        graph.update(inc, pc, no_pts);
    }
    const size_t n_nodes = graph.getNbNodes();
    CHECK(n_nodes >= 2, "%zu nodes", n_nodes);

    // the world: 48 x 48 x 1 m around the origin at the nodes' resolution (graph->getMap() upstream)
    const double res = fp.resolution, r = 0.1;
    lslgeneric::NDTMap world(new lslgeneric::LazyGrid(res));
    world.guessSize(0., 0., 0., 48., 48., 1.);
    const ndtgpu_world_result wr = assembleWorldMap(graph, world);
    CHECK(wr.n_cells > 30 && wr.overflow == 0, "%d world cells, overflow %d", wr.n_cells, wr.overflow);

    // ndt_feature2d_fuser.cpp:428-431: the world, then moved by the graph's pose
    OccupancyGridGPU omap;
    ndtgpu_occgrid_info wi;
    uint64_t live0[4], live1[4];
    ndtgpu_host::check(ndtgpu_live_resources(live0), "live_resources");
    lslgeneric::toOccupancyGrid(&world, omap, r, "world", nullptr, &wi);
    ndtgpu_host::check(ndtgpu_live_resources(live1), "live_resources");
    CHECK(live0[0] == live1[0] && live0[1] == live1[1] && live0[2] == live1[2] && live0[3] == live1[3], "the call left resources behind");
    CHECK(omap.info.width == 480 && omap.info.height == 480 && omap.data.size() == 480u * 480u, "world grid %u x %u", omap.info.width, omap.info.height);
    CHECK(omap.info.origin.position.x == -24.0 && omap.info.origin.position.y == -24.0 && omap.header.frame_id == "world", "world origin %g %g",
          omap.info.origin.position.x, omap.info.origin.position.y);
    const GridCheck wc = check_grid(world, omap, r, false);
    CHECK(wc.wrong_class == 0 && wc.wrong_value == 0, "world grid: %lld pixels of the wrong class, %lld of the wrong value", wc.wrong_class, wc.wrong_value);
    CHECK(wc.gaussian > 25 * 30 && wc.free_ == 0 && wc.occupied >= wc.gaussian && wc.on_face < wc.unknown, "world grid: %lld Gaussian pixels, %lld free, %lld occupied", wc.gaussian,
          wc.free_, wc.occupied);
    CHECK(wi.n_unknown == wc.unknown && wi.n_free == wc.free_ && wi.n_occupied == wc.occupied, "world grid: the counts of the call");

    const Eigen::Affine3d T = ndtgpu_host::affine_from_pose(1.5, -0.5, 0, 0, 0, 0.3);
    const std::vector<int8_t> before = omap.data;
    moveOccupancyMap(omap, T);
    const Eigen::Vector3d moved = T * Eigen::Vector3d(-24., -24., 0.);
    CHECK(std::fabs(omap.info.origin.position.x - moved(0)) < 1e-12 && std::fabs(omap.info.origin.position.y - moved(1)) < 1e-12 &&
              std::fabs(omap.info.origin.orientation.z - std::sin(0.15)) < 1e-12 && std::fabs(omap.info.origin.orientation.w - std::cos(0.15)) < 1e-12,
          "moved origin %g %g, orientation z %g w %g", omap.info.origin.position.x, omap.info.origin.position.y, omap.info.origin.orientation.z,
          omap.info.origin.orientation.w);
    CHECK(omap.data == before, "moveOccupancyMap resampled the data");
    moveOccupancyMap(omap, T.inverse());
    CHECK(std::fabs(omap.info.origin.position.x + 24.0) < 1e-12 && std::fabs(omap.info.origin.orientation.z) < 1e-12, "moved back: %g", omap.info.origin.position.x);

    // ndt_feature2d_fuser.cpp:450-452: one node's fused map (it carries occupancies: free space shows)
    OccupancyGridGPU nmap;
    lslgeneric::NDTMap *node_map = graph.getMap(0);
    lslgeneric::toOccupancyGrid(node_map, nmap, r, "world");
    CHECK(nmap.info.width == 300 && nmap.info.height == 300, "node grid %u x %u", nmap.info.width, nmap.info.height);
    const GridCheck nc = check_grid(*node_map, nmap, r, true);
    CHECK(nc.wrong_class == 0 && nc.wrong_value == 0, "node grid: %lld pixels of the wrong class, %lld of the wrong value", nc.wrong_class, nc.wrong_value);
    CHECK(nc.free_ > 1000 && nc.gaussian > 500 && nc.unknown > 1000, "node grid: %lld free, %lld Gaussian, %lld unknown pixels", nc.free_, nc.gaussian, nc.unknown);

    std::printf("occgrid_demo: %zu nodes -> %d world cells; world grid %u x %u: %lld occupied / %lld unknown pixels; node grid %u x %u: %lld free / "
                "%lld occupied / %lld unknown pixels; %d failures\n",
                n_nodes, wr.n_cells, omap.info.width, omap.info.height, wc.occupied, wc.unknown, nmap.info.width, nmap.info.height, nc.free_,
                nc.occupied, nc.unknown, g_fails);
    return g_fails ? 1 : 0;
}
