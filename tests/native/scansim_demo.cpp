// scansim_demo.cpp -- the host mirror's scan simulation (host/ndt_scan_simulator_gpu.h) called the way the reference calls
// occupancy_grid_utils (flirtlib_ros place_rec_test.cpp:203-260, simulate_scans.cpp:131): a walled room with a pillar and an unknown
// patch; simulateRangeScanGPU returns the exact ranges along the axes, unknown cells stop a ray only when asked to, and
// generateRefScansGPU returns the poses of three literal loops with a scan each.  Exit code 0 = every check passed; without a GPU the
// library fails loudly (exit code 3).
#include "ndt_scan_simulator_gpu.h"

#include <cstdio>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace flirtlib_ros;

int main()
{
    // 81 x 61 pixels of 0.05 m: walls all round, a pillar right of the centre, an unknown patch above it
    const int W = 81, H = 61;
    OccupancyGridGPU g;
    g.info.resolution = 0.05f;
    g.info.width = W;
    g.info.height = H;
    g.info.origin.position.x = -2.0;
    g.info.origin.position.y = -1.5;
    g.data.assign(W * H, 0);
    for (int i = 0; i < W; i++) g.data[i] = g.data[(H - 1) * W + i] = 100;
    for (int j = 0; j < H; j++) g.data[j * W] = g.data[j * W + W - 1] = 100;
    for (int j = 28; j < 33; j++)
        for (int i = 60; i < 64; i++) g.data[j * W + i] = 100;
    for (int j = 45; j < 50; j++)
        for (int i = 38; i < 43; i++) g.data[j * W + i] = -1;
    const double res = g.info.resolution;
    ScannerInfoGPU info;                       // three beams: right, ahead, left
    info.angle_min = -M_PI / 2;
    info.angle_max = M_PI / 2;
    info.angle_increment = M_PI / 2;
    info.range_max = 10.0;
    const int i0 = 40, j0 = 30;
    const PoseGPU centre = locmonMakePose(-2.0 + (i0 + 0.5) * res, -1.5 + (j0 + 0.5) * res, 1.0, 0.0);

    try {
        CHECK(info.beams() == 3, "beams %zu", info.beams());
        const LaserScanGPU s = simulateRangeScanGPU(g, centre, info, true);
        // right: the bottom wall, 30 cells; ahead: the pillar, 20 cells; left: the unknown patch, 15 cells
        CHECK(s.ranges.size() == 3 && s.ranges[0] == res * std::sqrt(900.0) && s.ranges[1] == res * std::sqrt(400.0) &&
                  s.ranges[2] == res * std::sqrt(225.0),
              "ranges %g %g %g", s.ranges[0], s.ranges[1], s.ranges[2]);
        const LaserScanGPU t = simulateRangeScanGPU(g, centre, info, false);
        CHECK(t.ranges[2] == res * std::sqrt(900.0) && t.ranges[1] == s.ranges[1], "unknown cells are free: left %g", t.ranges[2]);
        ScannerInfoGPU near = info;
        near.range_max = 0.9;                  // R = 17: the patch is in reach, the pillar is not
        const LaserScanGPU u = simulateRangeScanGPU(g, centre, near, true);
        CHECK(u.ranges[0] == 1.9 && u.ranges[1] == 1.9 && u.ranges[2] == s.ranges[2], "a miss reads range_max + 1: %g %g %g", u.ranges[0], u.ranges[1],
              u.ranges[2]);
        ScanSimulatorGPU sim(g, info);
        ndtgpu_scansim_result rep;
        sim.simulate(locmonMakePose(50.0, 50.0, 1.0, 0.0), &rep);
        CHECK(rep.flags == NDTGPU_SCANSIM_OFFMAP && rep.n_hits == 0, "a pose off the map: flags %u", rep.flags);

        // generateRefScans against three literal loops
        const double pos_res = 0.5, ang_res = 1.6, x0 = -1.2, x1 = 1.6, y0 = -1e9, y1 = 0.9;
        const std::vector<SimulatedRefScanGPU> refs = generateRefScansGPU(g, info, pos_res, ang_res, x0, x1, y0, y1);
        const unsigned skip = (unsigned)(pos_res / g.info.resolution);
        size_t k = 0, mismatches = 0, hits = 0;
        for (unsigned x = 0; x < g.info.width; x += skip)
            for (unsigned y = 0; y < g.info.height; y += skip)
                for (double theta = 0; theta < 6.28; theta += ang_res) {
                    const double cx = -2.0 + (x + 0.5) * res, cy = -1.5 + (y + 0.5) * res;
                    if (cx > x1 || cx < x0 || cy > y1 || cy < y0) continue;
                    if (g.data[y * W + x] != 0) continue;
                    if (k < refs.size()) {
                        double p4[4];
                        locmonPose4(refs[k].pose, p4);
                        if (!(refs[k].pose.position.x == cx && refs[k].pose.position.y == cy && std::fabs(p4[2] - std::cos(theta)) < 1e-12 &&
                              std::fabs(p4[3] - std::sin(theta)) < 1e-12 && refs[k].scan.ranges.size() == 3 && refs[k].report.flags == 0))
                            mismatches++;
                        hits += refs[k].report.n_hits;
                    }
                    k++;
                }
        CHECK(skip == 9 || skip == 10, "skip %u", skip);
        CHECK(k == refs.size() && k > 20 && mismatches == 0, "%zu reference scans, the loops give %zu, %zu mismatches", refs.size(), k, mismatches);
        CHECK(hits == 3 * refs.size(), "every beam of a walled room hits: %zu of %zu", hits, 3 * refs.size());
        std::printf("scansim_demo: ranges %.3f %.3f %.3f, unknown free %.3f, %zu reference scans (skip %u), %d failures\n", s.ranges[0], s.ranges[1],
                    s.ranges[2], t.ranges[2], refs.size(), skip, g_fails);
    } catch (const ndtgpu_host::Error &e) {
        if (e.status == NDTGPU_ERR_NO_DEVICE) {
            std::printf("scansim_demo: no HIP device: %s (no CPU fallback)\n", e.what());
            return 3;
        }
        std::printf("scansim_demo: %s\n", e.what());
        return 1;
    }
    return g_fails ? 1 : 0;
}
