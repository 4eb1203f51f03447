// fuser_feat_demo.cpp -- the host mirror's feature path (host/ndt_feature_graph_gpu.h) called the way the reference's fuser node
// calls it (ndt_feature2d_fuser.cpp:766-790: detect + describe, then graph->update(Tmotion, cloud, pts)):
//   A. NDTFeatureFuserHMT::initialize / update with interest points (ndt_feature_fuser_hmt.cpp:65-102, 108-512 with useFeat):
//      an initialize and three updates through the overloads against the same sequence through the C-ABI
//      (ndtgpu_fuser_bank_attach_features, ndtgpu_fuser_*_batch_feat_host) -- poses and feature records bit for bit -- and
//      getFeatureMap() against the slot's map set;
//   B. NDTFeatureGraph::initialize / update with interest points until a second node opens, then matchNodesUsingFeatureMap
//      (ndt_feature_node.h:254-256) against ndtgpu_featbank_match on the two nodes' map sets.
// Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_graph_gpu.h"

#include <cstdio>
#include <cstring>
#include <random>

using namespace ndt_feature;

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

// a closed corridor seen from `sensor_pose_world` (tests/native/host_demo.cpp's scene, fewer beams); points in the sensor frame
static pcl::PointCloud<pcl::PointXYZ> corridor_scan(const Eigen::Affine3d &sensor_pose_world, unsigned seed, int n_beams = 2000)
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
        double r = 0.0, step = 0.02;
        for (; r < 40.0; r += step) {
            const double x = ox + r * dx, y = oy + r * dy;
            if (x < -9.0 || x > 13.0 || y > 2.0 + 0.3 * std::sin(0.9 * x) || y < -2.0 - 0.2 * std::cos(0.7 * x)) break;
        }
        r += nd(rng);
        if (r < 0.3 || r > 30.0) continue;
        pc.push_back(pcl::PointXYZ((float)(r * std::cos(phi)), (float)(r * std::sin(phi)), (float)uz(rng)));
    }
    return pc;
}

// K interest points fixed in the world (a jittered grid, 0.8 m spacing) with random histograms, seen from `sensor_pose_world`
// with 1e-3 m of noise
struct World {
    std::vector<InterestPointGPU> pts;
    explicit World(size_t K)
    {
        std::mt19937 rng(5);
        std::uniform_real_distribution<double> U(0.0, 1.0);
        pts.resize(K);
        for (size_t i = 0; i < K; i++) {
            pts[i].x = -5.0 + 0.8 * (double)(i % 5) + 0.2 * U(rng) - 0.1;
            pts[i].y = -1.6 + 0.8 * (double)(i / 5) + 0.2 * U(rng) - 0.1;
            pts[i].theta = 2.0 * U(rng) - 1.0;
            pts[i].descriptor.resize(48);
            for (double &d : pts[i].descriptor) d = 0.1 + 0.9 * U(rng);
        }
    }
    InterestPointGPUVec seen(const Eigen::Affine3d &sensor_pose_world, unsigned seed) const
    {
        std::mt19937 rng(seed);
        std::uniform_real_distribution<double> U(-1e-3, 1e-3);
        const double ox = sensor_pose_world(0, 3), oy = sensor_pose_world(1, 3);
        const double yaw = std::atan2(sensor_pose_world(1, 0), sensor_pose_world(0, 0)), c = std::cos(yaw), s = std::sin(yaw);
        InterestPointGPUVec out(pts);
        for (size_t i = 0; i < pts.size(); i++) {
            const double dx = pts[i].x - ox, dy = pts[i].y - oy;
            out[i].x = c * dx + s * dy + U(rng);
            out[i].y = -s * dx + c * dy + U(rng);
            out[i].theta = std::atan2(std::sin(pts[i].theta - yaw), std::cos(pts[i].theta - yaw));
        }
        return out;
    }
};

static bool same_points(const InterestPointGPUVec &a, const std::vector<double> &pos, const std::vector<double> &desc, size_t n, size_t D)
{
    if (a.size() != n) return false;
    for (size_t i = 0; i < n; i++) {
        if (a[i].x != pos[3 * i] || a[i].y != pos[3 * i + 1] || a[i].theta != pos[3 * i + 2] || a[i].descriptor.size() != D) return false;
        for (size_t k = 0; k < D; k++)
            if (a[i].descriptor[k] != desc[i * D + k]) return false;
    }
    return true;
}

int main()
{
    const size_t K = 24, D = 48, MP = 256;
    NDTFeatureFuserHMT::Params fp;
    fp.resolution = 0.5; fp.map_size_x = 60; fp.map_size_y = 60; fp.map_size_z = 1.0; fp.sensor_range = 30;
    fp.useNDT = true; fp.useFeat = true; fp.useOdom = true;
    fp.neighbours = 2; fp.stepcontrol = true; fp.ITR_MAX = 30; fp.DELTA_SCORE = 1e-6;
    const MotionModel2d::Params mp;
    const Eigen::Affine3d sensor = ndtgpu_host::affine_from_pose(0.2, -0.03, 0, 0, 0, 0.01);
    const World world(K);
    std::vector<Eigen::Affine3d> gt;
    for (int k = 0; k < 8; k++) gt.push_back(ndtgpu_host::affine_from_pose(-6.0 + 0.3 * k, 0.05 * std::sin(0.7 * k), 0, 0, 0, 0.015 * k));
    std::vector<pcl::PointCloud<pcl::PointXYZ>> scans;
    std::vector<InterestPointGPUVec> pts;
    std::vector<Eigen::Affine3d> Tmotion(1, Eigen::Affine3d::Identity());
    for (size_t k = 0; k < gt.size(); k++) {
        scans.push_back(corridor_scan(gt[k] * sensor, 600 + (unsigned)k));
        pts.push_back(world.seen(gt[k] * sensor, 900 + (unsigned)k));
        if (k) {
            const Eigen::Affine3d inc = gt[k - 1].inverse() * gt[k];
            Tmotion.push_back(ndtgpu_host::affine_from_pose(inc(0, 3) + 0.004 * (double)k, inc(1, 3) - 0.003 * (double)k, 0, 0, 0,
                                                            std::atan2(inc(1, 0), inc(0, 0)) + 0.002));
        }
    }

    // ---- A. one fuser through the overloads, and the same sequence through the C-ABI
    NDTFeatureFuserHMT one(fp);
    one.setMotionParams(mp);
    one.setSensorPose(sensor);
    try {
        one.initialize(gt[0], scans[0], pts[0]);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("fuser_feat_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    const ndtgpu_fuser_params q = NDTFeatureFuserHMT::bankParams(fp, mp, sensor);
    const double c0[3] = {0, 0, 0}, sz[3] = {fp.map_size_x, fp.map_size_y, fp.map_size_z};
    ndtgpu_host::MapPool pool(fp.resolution, c0, sz, 1);
    ndtgpu_fuser_bank *bank = nullptr;
    ndtgpu_featbank *fb = nullptr;
    ndtgpu_host::check(ndtgpu_fuser_bank_create(&q, 1, pool.handle(), &bank), "ndtgpu_fuser_bank_create");
    ndtgpu_host::check(ndtgpu_featbank_create(3, MP, D, &fb), "ndtgpu_featbank_create");
    ndtgpu_host::check(ndtgpu_fuser_bank_attach_features(bank, fb, 1, 2, nullptr), "ndtgpu_fuser_bank_attach_features");
    const uint32_t cur = 0;
    auto stage = [&](const InterestPointGPUVec &v) {
        std::vector<double> pos, desc;
        for (const InterestPointGPU &p : v) {
            pos.push_back(p.x); pos.push_back(p.y); pos.push_back(p.theta);
            desc.insert(desc.end(), p.descriptor.begin(), p.descriptor.end());
        }
        ndtgpu_host::check(ndtgpu_featbank_set(fb, cur, v.size(), pos.data(), desc.data()), "ndtgpu_featbank_set");
    };
    int equal = 0, ok_records = 0;
    for (int k = 0; k <= 3; k++) {
        stage(pts[k]);
        if (k == 0) {
            double c[3] = {gt[0](0, 3), gt[0](1, 3), 0.0};
            ndtgpu_host::check(ndtgpu_mapset_set_centre(pool.handle(), 0, c), "ndtgpu_mapset_set_centre");
            ndtgpu_host::check(ndtgpu_fuser_initialize_batch_feat_host(bank, 0, 1, gt[0].data(), scans[0].points.data(), scans[0].size(), 16,
                                                                       scans[0].size() * 16, &cur),
                               "ndtgpu_fuser_initialize_batch_feat_host");
        } else {
            one.update(Tmotion[k], scans[k], pts[k]);
            ndtgpu_host::check(ndtgpu_fuser_update_batch_feat_host(bank, 0, 1, Tmotion[k].data(), scans[k].points.data(), scans[k].size(), 16,
                                                                   scans[k].size() * 16, &cur, 1, 1),
                               "ndtgpu_fuser_update_batch_feat_host");
        }
        double Tn[16];
        ndtgpu_fuser_feat_result rec;
        ndtgpu_host::check(ndtgpu_fuser_poses(bank, 0, 1, Tn, nullptr), "ndtgpu_fuser_poses");
        ndtgpu_host::check(ndtgpu_fuser_feat_results(bank, 0, 1, &rec), "ndtgpu_fuser_feat_results");
        const bool same = std::memcmp(Tn, one.Tnow.data(), sizeof Tn) == 0 && std::memcmp(&rec, &one.last_feat, sizeof rec) == 0;
        CHECK(same, "call %d: the overloads differ from the C-ABI", k);
        equal += same ? 1 : 0;
        if (k) {
            CHECK(rec.ransac_run == 1 && rec.n_odom_cells == 40, "call %d: ransac_run %d, odometry cells %d", k, rec.ransac_run, rec.n_odom_cells);
            ok_records += rec.ransac.status == NDTGPU_FEATMATCH_OK && rec.ransac.n_inliers == (int)K && rec.n_feat_cells == 24;
        }
        CHECK(rec.n_prev == (int)K && rec.n_map == (int)K, "call %d: n_prev %d, n_map %d", k, rec.n_prev, rec.n_map);
    }
    CHECK(ok_records == 3, "%d of 3 RANSAC records OK with %zu inliers", ok_records, K);
    {
        std::vector<double> pos(3 * MP), desc(MP * D);
        size_t n = 0;
        ndtgpu_host::check(ndtgpu_featbank_get(fb, 2, &n, pos.data(), desc.data()), "ndtgpu_featbank_get");
        const NDTFeatureMapGPU fm = one.getFeatureMap();
        CHECK(n == K && same_points(fm.map, pos, desc, n, D), "getFeatureMap() differs from the map set (%zu points against %zu)", fm.map.size(), n);
    }
    ndtgpu_fuser_bank_destroy(bank);
    ndtgpu_featbank_destroy(fb);

    // ---- B. the graph: a second node opens, and the two nodes' feature maps are matched where they are
    NDTFeatureGraph::Params gp;
    gp.newNodeTranslDist = 0.5;
    gp.maxNodes = 4;
    NDTFeatureGraph graph(gp, fp);
    graph.setMotionParams(mp);
    graph.setSensorPose(sensor);
    graph.initialize(gt[0], scans[0], pts[0]);
    for (size_t k = 1; k < gt.size() && graph.getNbNodes() < 2; k++) graph.update(Tmotion[k], scans[k], pts[k]);
    CHECK(graph.getNbNodes() == 2, "%zu nodes", graph.getNbNodes());
    int matched = 0;
    if (graph.getNbNodes() == 2) {
        CorrespondencesGPU matches;
        Eigen::Affine3d T = Eigen::Affine3d::Identity();
        const double score = graph.matchNodesUsingFeatureMap(0, 1, matches, T);
        const std::shared_ptr<ndtgpu_host::FuserBank> &gb = graph.getNode(0).getFuser().bank();
        const uint32_t ref = (uint32_t)gb->mapSet(graph.getNode(0).getFuser().slot()), mov = (uint32_t)gb->mapSet(graph.getNode(1).getFuser().slot());
        ndtgpu_host::check(ndtgpu_featbank_match(gb->features(), &ref, &mov, 1, nullptr, nullptr), "ndtgpu_featbank_match");
        ndtgpu_featmatch_result res;
        double T16[16];
        std::vector<uint32_t> corr(2 * gb->featMaxPoints());
        ndtgpu_host::check(ndtgpu_featbank_results(gb->features(), 0, 1, &res, T16, corr.data()), "ndtgpu_featbank_results");
        bool same = score == res.score && matches.size() == (size_t)res.n_inliers && std::memcmp(T16, T.data(), sizeof T16) == 0;
        for (size_t i = 0; same && i < matches.size(); i++) same = matches[i].first == corr[2 * i] && matches[i].second == corr[2 * i + 1];
        CHECK(same, "matchNodesUsingFeatureMap differs from ndtgpu_featbank_match on the map sets");
        CHECK(res.status == NDTGPU_FEATMATCH_OK && res.n_inliers == (int)K, "the nodes' feature maps: status %d, %d inliers", res.status, res.n_inliers);
        matched = same ? 1 : 0;
        // the pose maps node 1's map into node 0's: node0.T^-1 * node1.T
        const Eigen::Affine3d rel = graph.getNode(0).T.inverse() * graph.getNode(1).T;
        CHECK(std::hypot(T(0, 3) - rel(0, 3), T(1, 3) - rel(1, 3)) < 0.05, "the feature link ends %.3f m from the nodes' relative pose",
              std::hypot(T(0, 3) - rel(0, 3), T(1, 3) - rel(1, 3)));
        CHECK(graph.getNode(1).getFuser().getFeatureMap().map.size() == K, "node 1's feature map");
    }
    std::printf("fuser_feat_demo: %d of 4 calls equal to the C-ABI bit for bit, %d RANSAC records OK, %d node match equal, %d failures\n", equal,
                ok_records, matched, g_fails);
    return g_fails ? 1 : 0;
}
