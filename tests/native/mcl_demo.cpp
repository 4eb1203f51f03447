// mcl_demo.cpp -- the host mirror's NDTMCL3D (host/ndt_mcl_gpu.h) walked the way ndt_feature_mcl_node.cpp drives it (:174-184
// construct and set the parameters, :335 initializeFilter, :361 updateAndPredictEff per odometry step, :377-396 pf.pcloud /
// pf.size() / pf.getMean()), against the C-ABI calls it wraps on the same map and clouds: after every step the particles,
// weights, likelihoods and the mean must be those of ndtgpu_mcl_* bit for bit.  Exit code 0 = every check passed; without a
// GPU the library fails loudly (exit code 3).
#include "ndt_mcl_gpu.h"

#include <cstdio>
#include <cstring>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

// a rectangular room with a pillar, seen from `pose` (x, y, yaw in the room): one return per beam, in the sensor frame
static pcl::PointCloud<pcl::PointXYZ> room_scan(double px, double py, double yaw, unsigned seed, int n_beams = 8000)
{
    struct Seg { double x0, y0, x1, y1; };
    const Seg segs[] = {{-10, -7, 12, -7}, {12, -7, 12, 8}, {12, 8, -10, 8}, {-10, 8, -10, -7},      // walls
                        {3, 1, 4.5, 1}, {4.5, 1, 4.5, 2.5}, {4.5, 2.5, 3, 2.5}, {3, 2.5, 3, 1},       // pillar
                        {-6, -3, -4, -5}};                                                           // a slanted cabinet
    std::mt19937 rng(seed);
    std::normal_distribution<double> nd(0.0, 0.02);
    pcl::PointCloud<pcl::PointXYZ> pc;
    for (int j = 0; j < n_beams; j++) {
        const double a = -M_PI + 2.0 * M_PI * (j + 0.5) / n_beams + yaw, dx = std::cos(a), dy = std::sin(a);
        double best = 1e30;
        for (const Seg &s : segs) {
            const double ex = s.x1 - s.x0, ey = s.y1 - s.y0, den = dx * ey - dy * ex;
            if (std::fabs(den) < 1e-12) continue;
            const double t = ((s.x0 - px) * ey - (s.y0 - py) * ex) / den, u = ((s.x0 - px) * dy - (s.y0 - py) * dx) / den;
            if (t > 0 && u >= 0 && u <= 1) best = std::min(best, t);
        }
        if (best > 25.0) continue;
        const double r = best + nd(rng), b = a - yaw;
        pc.push_back(pcl::PointXYZ((float)(r * std::cos(b)), (float)(r * std::sin(b)), (float)(0.01 * nd(rng))));
    }
    return pc;
}

int main()
{
    const double res = 0.5;
    lslgeneric::NDTMap map(new lslgeneric::LazyGrid(res));
    try {
        map.guessSize(0, 0, 0, 40, 40, 4);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("mcl_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    map.loadPointCloud(room_scan(0, 0, 0, 1, 20000));
    map.computeNDTCells();

    // :174-184
    NDTMCL3D mcl(res, map, -5);
    mcl.forceSIR = false;
    mcl.SIR_varP_threshold = 0.006;
    mcl.SIR_max_iters_wo_resampling = 25;
    mcl.scan_size[0] = 40; mcl.scan_size[1] = 40; mcl.scan_size[2] = 4;
    mcl.max_scan_cells = 4096;
    const int numParticles = 100;
    // :335, the node's spreads
    const double d2r = M_PI / 180.0;
    mcl.initializeFilter(0.2, -0.1, 0, 0, 0, 0.05, 0.5, 0.5, 0.1, 2 * d2r, 2 * d2r, 2 * d2r, numParticles);

    // the same filter through the C-ABI
    const ndtgpu_mcl_params prm = mcl.params();
    const uint32_t idx = (uint32_t)map.slot();
    ndtgpu_mcl *h = nullptr;
    ndtgpu_host::check(ndtgpu_mcl_create(map.handle(), &idx, &prm, 1, numParticles, &h), "ndtgpu_mcl_create");
    const double pose6[6] = {0.2, -0.1, 0, 0, 0, 0.05}, sigma6[6] = {0.5, 0.5, 0.1, 2 * d2r, 2 * d2r, 2 * d2r};
    ndtgpu_host::check(ndtgpu_mcl_initialize(h, 0, 1, pose6, sigma6), "ndtgpu_mcl_initialize");

    std::mt19937 rng(5);
    std::normal_distribution<double> nd(0.0, 1.0);
    const int steps = 12;
    int equal = 0;
    double x = 0, y = 0, yaw = 0, dt = 0;
    for (int s = 1; s <= steps; s++) {
        const double nx = 0.08 * s, ny = 0.03 * s, nyaw = 0.01 * s;
        const Eigen::Affine3d T0 = ndtgpu_host::affine_from_pose(x, y, 0, 0, 0, yaw), T1 = ndtgpu_host::affine_from_pose(nx, ny, 0, 0, 0, nyaw);
        // the odometry increment Tm = Todo_old^-1 * Todo (:341), with a little noise
        const Eigen::Affine3d Tm = T0.inverse() * T1 * ndtgpu_host::affine_from_pose(0.005 * nd(rng), 0.005 * nd(rng), 0, 0, 0, 0.002 * nd(rng));
        x = nx; y = ny; yaw = nyaw;
        const pcl::PointCloud<pcl::PointXYZ> cloud = room_scan(x, y, yaw, 100 + s);
        mcl.updateAndPredictEff(Tm, cloud, 1.0);                                       // :361
        ndtgpu_host::check(ndtgpu_mcl_update_host(h, 0, 1, Tm.data(), 1.0, &cloud.points[0], cloud.size(), sizeof(pcl::PointXYZ),
                                                  cloud.size() * sizeof(pcl::PointXYZ)), "ndtgpu_mcl_update_host");
        std::vector<double> T(16 * numParticles), w(numParticles), lik(numParticles), M(16);
        ndtgpu_host::check(ndtgpu_mcl_particles(h, 0, 1, T.data(), w.data(), lik.data()), "ndtgpu_mcl_particles");
        ndtgpu_host::check(ndtgpu_mcl_mean(h, 0, 1, M.data(), nullptr), "ndtgpu_mcl_mean");
        bool same = mcl.pf.size() == (size_t)numParticles;
        for (size_t i = 0; same && i < mcl.pf.size(); i++) {                          // :377-396
            double px, py, pz;
            mcl.pf.pcloud[i].getXYZ(px, py, pz);
            same = std::memcmp(mcl.pf.pcloud[i].T.data(), &T[16 * i], 16 * sizeof(double)) == 0 && mcl.pf.pcloud[i].p == w[i] &&
                   mcl.pf.pcloud[i].lik == lik[i] && px == T[16 * i + 12] && py == T[16 * i + 13] && pz == T[16 * i + 14];
        }
        const Eigen::Affine3d mean = mcl.pf.getMean();
        same = same && std::memcmp(mean.data(), M.data(), 16 * sizeof(double)) == 0;
        CHECK(same, "step %d: the mirror differs from the C-ABI", s);
        equal += same ? 1 : 0;
        dt = std::hypot(mean(0, 3) - x, mean(1, 3) - y);
    }
    ndtgpu_mcl_destroy(h);
    const ndtgpu_mcl_result r = mcl.pf.lastResult();
    CHECK(r.n_scan_cells > 0 && r.overflow == 0 && r.terms > 0, "last update: %d scan cells, overflow %d", r.n_scan_cells, r.overflow);
    CHECK(dt < 0.15, "the mean ends %.3f m from the true pose", dt);
    std::printf("mcl_demo: %d steps, %d equal to the C-ABI bit for bit, final |dt| %.4f m, %d failures\n", steps, equal, dt, g_fails);
    return g_fails ? 1 : 0;
}
