// locmon_demo.cpp -- the host mirror's localisation monitor (host/ndt_localization_monitor_gpu.h) called the way the reference's node
// calls its own classes (flirtlib_ros localization_monitor_node.cpp): an occupancy grid of a room with ten pillars, scans of it
// from a known pose; ScanPoseEvaluatorGPU says the true pose is good and a pose 3 m away is not, adjustPose walks back from a
// nudged pose, and LocalizationMonitorGPU::update gives the verdicts of scanCB.  Exit code 0 = every check passed; without a GPU
// the library fails loudly (exit code 3).
#include "ndt_localization_monitor_gpu.h"

#include <cstdio>
#include <cstring>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace flirtlib_ros;

// rectangles (cx, cy, hx, hy): the room's walls (seen from inside) and ten pillars, enough corners for the feature detector
static const double kRects[][4] = {{0.0, 0.0, 4.0, 3.0},   {2.0, 1.2, 0.3, 0.3},    {-1.5, -1.4, 0.4, 0.25}, {-2.5, 1.5, 0.25, 0.4},
                                   {0.0, 2.0, 0.5, 0.2},   {2.8, -1.8, 0.3, 0.35},  {-3.0, -0.2, 0.2, 0.5},  {1.0, -2.2, 0.45, 0.2},
                                   {-0.8, 0.9, 0.2, 0.2},  {3.2, 0.8, 0.2, 0.3},    {-2.0, -2.4, 0.3, 0.2}};

static double cast(double ox, double oy, double a)
{
    const double dx = std::cos(a), dy = std::sin(a);
    double best = 1e9;
    for (const auto &r : kRects)
        for (int side = 0; side < 4; side++) {
            const bool vertical = side < 2;
            const double wall = vertical ? r[0] + (side == 0 ? -r[2] : r[2]) : r[1] + (side == 2 ? -r[3] : r[3]);
            const double t = vertical ? (wall - ox) / dx : (wall - oy) / dy;
            if (!(t > 1e-9)) continue;
            const double hit = vertical ? oy + t * dy : ox + t * dx, c = vertical ? r[1] : r[0], h = vertical ? r[3] : r[2];
            if (hit >= c - h && hit <= c + h && t < best) best = t;
        }
    return best;
}

int main()
{
    // the grid: 10 m x 8 m at 0.05 m around the origin; unknown outside the room, free inside, every rectangle's outline 3 pixels thick
    OccupancyGridGPU g;
    g.info.resolution = 0.05f;
    g.info.width = 200;
    g.info.height = 160;
    g.info.origin.position.x = -5.0;
    g.info.origin.position.y = -4.0;
    g.data.assign(200 * 160, -1);
    const double res = g.info.resolution;
    for (int j = 0; j < 160; j++)
        for (int i = 0; i < 200; i++) {
            const double x = -5.0 + (i + 0.5) * res, y = -4.0 + (j + 0.5) * res;
            if (std::fabs(x) < 4.0 && std::fabs(y) < 3.0) g.data[j * 200 + i] = 0;
            for (const auto &r : kRects) {
                const double ex = std::fabs(std::fabs(x - r[0]) - r[2]), ey = std::fabs(std::fabs(y - r[1]) - r[3]);
                const bool on_x = ex < 1.5 * res && std::fabs(y - r[1]) < r[3] + 1.5 * res, on_y = ey < 1.5 * res && std::fabs(x - r[0]) < r[2] + 1.5 * res;
                if (on_x || on_y) g.data[j * 200 + i] = 100;
            }
        }
    const double truth[3] = {0.5, -0.3, 0.4};
    ndt_feature::LaserScanGPU scan;
    scan.angle_increment = 2.0 * M_PI / 720;
    scan.angle_min = -M_PI + 0.5 * scan.angle_increment;
    for (int i = 0; i < 720; i++) scan.ranges.push_back(cast(truth[0], truth[1], truth[2] + scan.angle_min + i * scan.angle_increment));
    const PoseGPU here = locmonMakePose(truth[0], truth[1], std::cos(truth[2]), std::sin(truth[2]));
    const PoseGPU away = locmonMakePose(truth[0] + 3.0, truth[1], std::cos(truth[2]), std::sin(truth[2]));

    try {
        LocalizationMonitorGPU mon(g, 0.25, 8, 0.0, 0.0);
        ScanPoseEvaluatorGPU &ev = mon.evaluator();
        const ndtgpu_locmon_result good = ev.evaluate(scan, here), bad = ev.evaluate(scan, away);
        CHECK(good.flags == 0 && good.n_kept == 720 && good.key == 0 && good.badness == 0.0, "the true pose: key %u, badness %g", good.key, good.badness);
        CHECK(ev(scan, here) < 0.25f && !(ev(scan, away) < 0.25f), "operator(): %g here, %g 3 m away", ev(scan, here), ev(scan, away));
        CHECK(bad.key >= 0x10000u && bad.badness >= 0.375, "3 m away: key %u", bad.key);

        // adjustPose from a nudged pose: the winner is the first smallest key of the volume, and no worse than the start
        const PoseGPU nudged = locmonMakePose(truth[0] + 0.12, truth[1] - 0.08, std::cos(truth[2] + 0.05), std::sin(truth[2] + 0.05));
        ndtgpu_locmon_adjust_result ar;
        std::vector<uint32_t> vol;
        const PoseGPU fixed = ev.adjustPose(scan, nudged, 0.2, 0.05, 0.1, &ar, &vol);
        size_t first = 0;
        for (size_t k = 1; k < vol.size(); k++)
            if (vol[k] < vol[first]) first = k;
        CHECK(!vol.empty() && ar.index == first && ar.key == vol[first] && ar.flags == 0, "winner %u (key %u), first minimum %zu", ar.index, ar.key, first);
        const ndtgpu_locmon_result at_fixed = ev.evaluate(scan, fixed);
        CHECK(ar.badness < 0.25 && at_fixed.badness < 0.25, "the adjusted pose is good: %g in the search, %g evaluated", ar.badness, at_fixed.badness);
        ndtgpu_locmon_adjust_result off;
        ev.adjustPose(scan, locmonMakePose(500.0, 500.0, 1.0, 0.0), 0.1, 0.05, 1.0, &off);
        CHECK((off.flags & NDTGPU_LOCMON_NO_RESULT) && off.index == 0 && off.badness == 1e9, "a lattice off the map reports NO_RESULT");

        // scanCB: localised -> the first scan becomes a reference set, a second one nearby does not; a wrong pose -> relocalisation
        const LocalizationVerdictGPU v1 = mon.update(scan, here), v2 = mon.update(scan, here);
        CHECK(v1.localised && v1.added_reference && v2.localised && !v2.added_reference && mon.ref_scans.size() == 1, "reference sets: %zu",
              mon.ref_scans.size());
        const LocalizationVerdictGPU v3 = mon.update(scan, away);
        CHECK(!v3.localised && !v3.added_reference, "3 m away is not localised");
        CHECK(v3.relocalised == (v3.ref_scan >= 0 && v3.match_badness < 0.25), "the verdict follows the badness of the picked pose");
        CHECK(v3.ref_scan < 0 || v3.n_matches > 8, "a picked reference scan has more than min_num_matches matches");
        // the scan against its own reference set: the match is the identity, the picked pose the reference's (post is zero here)
        CHECK(v3.relocalised && v3.ref_scan == 0 && std::fabs(v3.pose.position.x - truth[0]) < 0.05 && std::fabs(v3.pose.position.y - truth[1]) < 0.05,
              "relocalised at (%g, %g) from reference %d with %d matches, badness %g", v3.pose.position.x, v3.pose.position.y, v3.ref_scan, v3.n_matches,
              v3.match_badness);
        std::printf("locmon_demo: here %.3f (key %u), away key %u, adjust %zu candidates -> key %u, %zu features, relocalise: ref %d, %d matches, "
                    "badness %.3f, %d failures\n", good.badness, good.key, bad.key, vol.size(), ar.key, mon.ref_scans.empty() ? (size_t)0 : mon.ref_scans[0].raw_pts.size(), v3.ref_scan,
                    v3.n_matches, v3.match_badness, g_fails);
    } catch (const ndtgpu_host::Error &e) {
        if (e.status == NDTGPU_ERR_NO_DEVICE) {
            std::printf("locmon_demo: no HIP device: %s (no CPU fallback)\n", e.what());
            return 3;
        }
        std::printf("locmon_demo: %s\n", e.what());
        return 1;
    }
    return g_fails ? 1 : 0;
}
