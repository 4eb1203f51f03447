// featextract_demo.cpp -- the host mirror's scan front end (host/ndt_feature_map_gpu.h: LaserScanGPU, detectAndDescribe) called the
// way the fuser calls flirtlib for every scan it fuses (ndt_feature2d_fuser.cpp:772-776): 4 scans of one room from 4 poses in one
// device call, against the ndtgpu_featbank_extract / _get calls it wraps given the same ranges by hand -- positions, headings and
// descriptors must be those of the C-ABI bit for bit.  Exit code 0 = every check passed; without a GPU the library fails loudly
// (exit code 3).
#include "ndt_feature_map_gpu.h"

#include <cstdio>
#include <random>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

using namespace ndt_feature;

// the range along (dx, dy) from (ox, oy) to the nearest side of the axis-aligned rectangles (cx, cy, hx, hy)
static double cast(const std::vector<std::array<double, 4>> &rects, double ox, double oy, double dx, double dy)
{
    double best = 1e9;
    for (const std::array<double, 4> &r : rects)
        for (int side = 0; side < 2; side++) {
            const double sgn = side ? 1.0 : -1.0;
            const double tx = (r[0] + sgn * r[2] - ox) / dx, y = oy + tx * dy;
            if (tx > 1e-9 && y >= r[1] - r[3] && y <= r[1] + r[3]) best = std::min(best, tx);
            const double ty = (r[1] + sgn * r[3] - oy) / dy, x = ox + ty * dx;
            if (ty > 1e-9 && x >= r[0] - r[2] && x <= r[0] + r[2]) best = std::min(best, ty);
        }
    return best;
}

int main()
{
    const size_t n_scans = 4, n_beams = 541;
    const std::vector<std::array<double, 4>> room = {{0, 0, 9, 7}, {4, 3, 1, 1.5}, {-5, -3, 1.5, 0.5}, {-3, 4, 0.7, 0.7}};
    std::mt19937 rng(11);
    std::normal_distribution<double> nd(0.0, 0.005);
    std::vector<LaserScanGPU> scans(n_scans);
    for (size_t b = 0; b < n_scans; b++) {
        const double ox = 0.3 * (double)b, oy = -0.2 * (double)b, yaw = 0.1 * (double)b;
        scans[b].angle_increment = 2.0 * M_PI / (double)n_beams;
        scans[b].angle_min = -M_PI + 0.5 * scans[b].angle_increment;
        for (size_t i = 0; i < n_beams; i++) {
            const double a = scans[b].angle_min + (double)i * scans[b].angle_increment + yaw;
            scans[b].ranges.push_back(cast(room, ox, oy, std::cos(a), std::sin(a)) + nd(rng));
        }
        scans[b].ranges[17 + b] = std::numeric_limits<double>::quiet_NaN();      // a dropped beam
    }

    std::vector<InterestPointGPUVec> pts;
    std::vector<ndtgpu_featextract_result> records;
    try {
        pts = detectAndDescribe(scans, nullptr, 64, &records);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("featextract_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(pts.size() == n_scans && records.size() == n_scans, "%zu scans, %zu records", pts.size(), records.size());

    // the same by hand: a bank of another shape, the scans in its last slots and in reverse order
    ndtgpu_featbank *h = nullptr;
    ndtgpu_host::check(ndtgpu_featbank_create(n_scans + 1, 50, 48, &h), "ndtgpu_featbank_create");
    std::vector<double> ranges;
    std::vector<uint32_t> idx;
    for (size_t b = 0; b < n_scans; b++) {
        const LaserScanGPU &s = scans[n_scans - 1 - b];
        ranges.insert(ranges.end(), s.ranges.begin(), s.ranges.end());
        idx.push_back((uint32_t)(n_scans - b));
    }
    ndtgpu_host::check(ndtgpu_featbank_extract(h, idx.data(), ranges.data(), n_scans, n_beams, scans[0].angle_min, scans[0].angle_increment,
                                               nullptr, nullptr), "ndtgpu_featbank_extract");
    std::vector<ndtgpu_featextract_result> res(n_scans);
    ndtgpu_host::check(ndtgpu_featbank_extract_results(h, 0, n_scans, res.data(), nullptr, nullptr, nullptr), "ndtgpu_featbank_extract_results");
    int equal = 0;
    size_t total = 0;
    for (size_t b = 0; b < n_scans && b < pts.size(); b++) {
        std::vector<double> pos(50 * 3), desc(50 * 48);
        size_t m = 0;
        ndtgpu_host::check(ndtgpu_featbank_get(h, b + 1, &m, pos.data(), desc.data()), "ndtgpu_featbank_get");
        const ndtgpu_featextract_result &r = res[n_scans - 1 - b];
        bool same = m == pts[b].size() && r.status == NDTGPU_FEATEXTRACT_OK && records[b].status == r.status &&
                    records[b].n_found == r.n_found && records[b].n_valid == r.n_valid && (size_t)r.n_stored == m &&
                    r.n_valid == (int)n_beams - 1;
        for (size_t i = 0; same && i < m; i++) {
            const InterestPointGPU &p = pts[b][i];
            same = p.x == pos[3 * i] && p.y == pos[3 * i + 1] && p.theta == pos[3 * i + 2] && p.descriptor.size() == 48;
            for (size_t k = 0; same && k < 48; k++) same = p.descriptor[k] == desc[48 * i + k];
        }
        CHECK(same, "scan %zu: the mirror differs from the C-ABI", b);
        CHECK(m >= 4, "scan %zu: %zu interest points", b, m);
        equal += same ? 1 : 0;
        total += m;
    }
    ndtgpu_featbank_destroy(h);

    // scans of different shapes are refused, no scans give no points
    std::vector<LaserScanGPU> odd = {scans[0], scans[1]};
    odd[1].ranges.pop_back();
    bool refused = false;
    try {
        detectAndDescribe(odd);
    } catch (const ndtgpu_host::Error &e) {
        refused = e.status == NDTGPU_ERR_INVALID;
    }
    CHECK(refused, "scans of different sizes must be refused");
    CHECK(detectAndDescribe({}).empty(), "no scans, no points");

    std::printf("featextract_demo: %zu scans, %zu interest points, %d scans equal to the C-ABI bit for bit, %d failures\n", n_scans, total,
                equal, g_fails);
    return g_fails ? 1 : 0;
}
