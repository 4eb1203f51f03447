// calib_demo.cpp -- the host mirror's extrinsic calibration (host/ndt_calibration_gpu.h) called the way the reference's program
// calls its own functions (laser2d_extrinsic_calibration.cpp): scans of a rectangular room from a base that turns on the spot, the
// laser at a planted offset on it, go through CalibrationPairCollector::add; bruteForceOptimization searches the lattice in one
// device call; errorFunction and scoreICP at the winner must give the volume's entry bit for bit.  Exit code 0 = every check
// passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_calibration_gpu.h"

#include <cstdio>
#include <cstring>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

int main()
{
    const double hx = 2.5, hy = 2.0;                          // a room of 5 m x 4 m around the origin
    const double planted[3] = {0.23, 0.02, 0.01};
    const size_t n_beams = 360;
    std::mt19937 rng(7);
    std::normal_distribution<double> nd(0.0, 0.003);
    std::uniform_real_distribution<double> ud(0.0, 0.01);
    const Eigen::Affine3d Ts = calibGetAsAffine(planted[0], planted[1], planted[2]);
    // the base: steps of 30 degrees within a few centimetres, one step of 2 m (the anchor is reset), one of 10 degrees (dropped)
    const double base[][3] = {{0, 0, 0}, {0.05, 0.02, 0.55}, {0.1, 0.0, 1.1}, {0.12, 0.01, 1.27}, {0.1, -0.05, 1.7}, {0.3, 1.1, 1.8},
                              {0.3, 1.0, 2.4}, {0.25, 1.05, 1.8}};
    CalibrationPairCollector collector;
    size_t completed = 0;
    for (const auto &b : base) {
        const Eigen::Affine3d Tgt = calibGetAsAffine(b[0], b[1], b[2]), S = Tgt * Ts;
        const double ox = S(0, 3), oy = S(1, 3), yaw = std::atan2(S(1, 0), S(0, 0));
        pcl::PointCloud<pcl::PointXYZ> cloud;
        for (size_t i = 0; i < n_beams; i++) {
            const double a = -M_PI + (i + 0.5) * 2.0 * M_PI / n_beams, c = std::cos(a + yaw), s = std::sin(a + yaw);
            const double tx = ((c > 0 ? hx : -hx) - ox) / c, ty = ((s > 0 ? hy : -hy) - oy) / s, r = std::min(tx, ty) + nd(rng);
            if (!(r > 0.3 && r < 20.0)) continue;
            pcl::PointXYZ pt;
            pt.x = (float)(r * std::cos(a)); pt.y = (float)(r * std::sin(a)); pt.z = (float)(0.1 + ud(rng));
            cloud.push_back(pt);
        }
        bool pair = false;
        try {
            pair = collector.add(cloud, Tgt);
        } catch (const ndtgpu_host::Error &e) {
            std::printf("calib_demo: %s\n", e.what());
            return 1;
        }
        completed += pair ? 1 : 0;
    }
    // pairs (0,1) (1,2) (2,4) -- 3 is dropped: 10 degrees --, 5 resets the anchor, (5,6) (6,7)
    CHECK(completed == 5 && collector.pairs.size() == 5, "%zu pairs collected", collector.pairs.size());

    CalibrationResultGPU best;
    try {
        best = bruteForceOptimization(collector.pairs, 0.19, 0.0, 0.01, 0.1, 0.1, 0.1, 0.02, 0.05, nullptr, true);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("calib_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(best.found && best.n_candidates == 11 * 10 * 4 && best.volume.size() == best.n_candidates, "%zu candidates", best.n_candidates);
    CHECK(std::fabs(best.x - planted[0]) < 1e-9 && std::fabs(best.y - planted[1]) < 1e-9 && std::fabs(best.yaw - planted[2]) < 1e-9,
          "the winner (%g, %g, %g) is not the planted offset", best.x, best.y, best.yaw);
    CHECK(best.index < best.volume.size() && std::memcmp(&best.volume[best.index], &best.score, sizeof(double)) == 0, "score and volume disagree");
    size_t below = 0;
    for (double v : best.volume) below += v < best.score ? 1 : 0;
    CHECK(below == 0, "%zu candidates score below the winner", below);

    // errorFunction at the winner: the lattice's own node, with the table's cosine and sine -> the volume's entry bit for bit;
    // scoreICP per pair adds up to it in pair order
    const double e = errorFunction(collector.pairs, best.T);
    CHECK(std::memcmp(&e, &best.score, sizeof e) == 0, "errorFunction %.17g, search %.17g", e, best.score);
    double sum = 0.0;
    for (const ScanPairGPU &p : collector.pairs) sum += p.scoreICP(best.T);
    CHECK(std::memcmp(&sum, &best.score, sizeof sum) == 0, "sum of scoreICP %.17g, search %.17g", sum, best.score);
    const double off = errorFunction(collector.pairs, calibGetAsAffine(0.0, 0.0, 0.0));
    CHECK(off > best.score, "the zero offset scores %.6g, the winner %.6g", off, best.score);

    // no pairs: refused
    bool refused = false;
    try {
        errorFunction({}, best.T);
    } catch (const ndtgpu_host::Error &err) {
        refused = err.status == NDTGPU_ERR_INVALID;
    }
    CHECK(refused, "a search without pairs must be refused");

    std::printf("calib_demo: %zu pairs, %zu candidates, winner (%.2f, %.2f, %.2f) score %.6f, zero offset %.6f, %d failures\n",
                collector.pairs.size(), best.n_candidates, best.x, best.y, best.yaw, best.score, off, g_fails);
    return g_fails ? 1 : 0;
}
