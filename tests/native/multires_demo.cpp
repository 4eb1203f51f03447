// multires_demo.cpp -- the raw-cloud overload of the host mirror, NDTMatcherD2D(irregular, useDefault, resolutions)
// .match(target_pc, source_pc, T, useInitialGuess) (ndt_odom_debug.cpp:159-165, ndt_feature_pcl_eval.cpp:620-642), against the
// C-ABI call it wraps: for scan pairs of a synthetic room, the pose and every level's result must be those of
// ndtgpu_register_multires_host on the same clouds, bit for bit.  Also: the constructor's level lists and its refusal of an
// irregular grid.  Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
#include "lslgeneric_gpu.h"

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
    bool threw = false;
    try {
        lslgeneric::NDTMatcherD2D irregular(true, false, std::vector<double>{0.5});
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw, "an irregular grid must be refused");
    lslgeneric::NDTMatcherD2D dflt(false, true, std::vector<double>{7.0});
    CHECK((dflt.resolutions == std::vector<double>{0.2, 0.5, 1.0, 2.0}), "default list");
    lslgeneric::NDTMatcherD2D own(false, false, std::vector<double>{0.5, 1.0, 2.0, 4.0});
    CHECK((own.resolutions == std::vector<double>{0.5, 1.0, 2.0, 4.0}), "caller's list");

    if (ndtgpu_device_count() < 1) {
        pcl::PointCloud<pcl::PointXYZ> t = room_scan(0, 0, 0, 1), s = room_scan(0.3, 0.1, 0.05, 2);
        Eigen::Affine3d T = Eigen::Affine3d::Identity();
        try {
            own.match(t, s, T, true);
            std::printf("multires_demo: match returned without a device\n");
            return 1;
        } catch (const ndtgpu_host::Error &e) {
            std::printf("multires_demo: no HIP device: %s (no CPU fallback)\n", e.what());
            return e.status == NDTGPU_ERR_NO_DEVICE && g_fails == 0 ? 3 : 1;
        }
    }

    int pairs = 0, equal = 0;
    double worst = 0.0;
    for (lslgeneric::NDTMatcherD2D *m : {&dflt, &own}) {
        m->multires_grid.size[2] = 2.0;
        for (int k = 0; k < 3; k++) {
            const double ax = 0.5 * k, ay = -0.3 * k, ayaw = 0.1 * k;
            const double ox = 0.4, oy = 0.15, oyaw = 4.0 * M_PI / 180;    // the source scan's pose in the target scan's frame
            const double bx = ax + std::cos(ayaw) * ox - std::sin(ayaw) * oy, by = ay + std::sin(ayaw) * ox + std::cos(ayaw) * oy;
            pcl::PointCloud<pcl::PointXYZ> target = room_scan(ax, ay, ayaw, 10 + k), source = room_scan(bx, by, ayaw + oyaw, 20 + k);
            const Eigen::Affine3d T_gt = ndtgpu_host::affine_from_pose(ox, oy, 0, 0, 0, oyaw);
            Eigen::Affine3d T = T_gt * ndtgpu_host::affine_from_pose(0.3, -0.2, 0, 0, 0, 3.0 * M_PI / 180);
            Eigen::Affine3d T_abi = T;
            const bool ok = m->match(target, source, T, true);
            // the same call through the C-ABI
            const size_t np = std::max(target.size(), source.size()), L = m->resolutions.size();
            std::vector<float> pts(2 * np * 4, std::nanf(""));
            for (size_t i = 0; i < target.size(); i++) std::memcpy(&pts[4 * i], &target.points[i], 12);
            for (size_t i = 0; i < source.size(); i++) std::memcpy(&pts[4 * (np + i)], &source.points[i], 12);
            ndtgpu_grid_params g;
            g.res = 0.0;
            for (int a = 0; a < 3; a++) { g.centre[a] = m->multires_grid.centre[a]; g.size[a] = m->multires_grid.size[a]; }
            g.max_cells = m->multires_grid.max_cells;
            ndtgpu_multires *mr = nullptr;
            ndtgpu_host::check(ndtgpu_multires_create(&g, m->resolutions.data(), (int)L, 1, &mr), "ndtgpu_multires_create");
            std::vector<ndtgpu_match_result> res(L);
            ndtgpu_match_params p = m->params(0x3f, true);
            ndtgpu_host::check(ndtgpu_register_multires_host(mr, pts.data(), pts.data() + np * 4, np, 16, np * 16, -1.0, nullptr,
                                                             T_abi.data(), 1, &p, 1, res.data()), "ndtgpu_register_multires_host");
            ndtgpu_multires_destroy(mr);
            bool same = std::memcmp(T.data(), T_abi.data(), 16 * sizeof(double)) == 0 && m->multires_results.size() == L;
            for (size_t j = 0; same && j < L; j++) {
                const ndtgpu_match_result &a = m->multires_results[j], &b = res[j];
                same = a.converged == b.converged && a.iterations == b.iterations && a.fevals == b.fevals && a.exit_code == b.exit_code &&
                       a.score == b.score && a.n_source == b.n_source && a.n_target == b.n_target;
            }
            same = same && std::memcmp(&m->last_result.score, &res[0].score, sizeof(double)) == 0 && ok == (res[0].converged != 0);
            const double dt = std::hypot(T(0, 3) - T_gt(0, 3), T(1, 3) - T_gt(1, 3));
            worst = std::max(worst, dt);
            CHECK(same, "list %zu pair %d: the overload differs from ndtgpu_register_multires_host", L, k);
            CHECK(dt < 0.05, "list %zu pair %d: %.4f m from the true pose", L, k, dt);
            pairs++;
            equal += same ? 1 : 0;
        }
    }
    std::printf("multires_demo: %d pairs, %d equal to the C-ABI bit for bit, worst |dt| %.4f m, %d failures\n", pairs, equal, worst,
                g_fails);
    return g_fails ? 1 : 0;
}
