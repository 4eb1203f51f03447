// scanproject_demo.cpp -- the host mirror's scan projection (host/ndt_feature_map_gpu.h: projectLaserGPU) called the way every
// consumer of a scan calls projector_.projectLaser, the range gate and the z jitter (ndt_feature2d_fuser.cpp:747-765): 4 scans of
// one room from 4 poses in one device call, against the ndtgpu_scanproj_project call it wraps given the same ranges by hand in
// another order and with other strides -- every point must be that of the C-ABI bit for bit, and a cloud's front() and back() the
// first and the last kept beam.  Exit code 0 = every check passed; without a GPU the library fails loudly (exit code 3).
#include "ndt_feature_map_gpu.h"

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
    const size_t n_scans = 4, n_beams = 1441;                 // two tiles, the second of them short
    const double hx = 9.0, hy = 7.0;                          // a room of 18 m x 14 m around the origin
    std::mt19937 rng(13);
    std::normal_distribution<double> nd(0.0, 0.005);
    std::vector<LaserScanGPU> scans(n_scans);
    std::vector<size_t> want_kept(n_scans, 0), first(n_scans, n_beams), last(n_scans, 0);
    for (size_t b = 0; b < n_scans; b++) {
        const double ox = 0.3 * (double)b, oy = -0.2 * (double)b, yaw = 0.1 * (double)b;
        scans[b].angle_increment = 2.0 * M_PI / (double)n_beams;
        scans[b].angle_min = -M_PI + 0.5 * scans[b].angle_increment;
        for (size_t i = 0; i < n_beams; i++) {
            const double a = scans[b].angle_min + (double)i * scans[b].angle_increment + yaw, c = std::cos(a), s = std::sin(a);
            const double tx = ((c > 0 ? hx : -hx) - ox) / c, ty = ((s > 0 ? hy : -hy) - oy) / s;
            scans[b].ranges.push_back(std::min(tx, ty) + nd(rng));
        }
        scans[b].ranges[0] = 0.2;                                                  // too near
        scans[b].ranges[17 + b] = std::numeric_limits<double>::quiet_NaN();        // dropped beams
        scans[b].ranges[n_beams - 1 - b] = std::numeric_limits<double>::infinity();
        scans[b].ranges[700] = 31.0;                                               // too far
        for (size_t i = 0; i < n_beams; i++) {
            const double r = scans[b].ranges[i];
            if (!(r > 0.5 && r < 30.0)) continue;
            want_kept[b]++;
            first[b] = std::min(first[b], i);
            last[b] = std::max(last[b], i);
        }
    }
    ndtgpu_scanproject_params prm;
    ndtgpu_default_scanproject_params(&prm);
    prm.seed = 5;
    const std::vector<uint64_t> ids = {40, 41, 42, 1ull << 40};

    std::vector<pcl::PointCloud<pcl::PointXYZ>> clouds;
    try {
        clouds = projectLaserGPU(scans, &prm, ids);
    } catch (const ndtgpu_host::Error &e) {
        std::printf("scanproject_demo: no HIP device: %s (no CPU fallback)\n", e.what());
        return e.status == NDTGPU_ERR_NO_DEVICE ? 3 : 1;
    }
    CHECK(clouds.size() == n_scans, "%zu clouds", clouds.size());

    // the same by hand: a larger handle, the scans in reverse order, records of 32 bytes and a gap between the scans
    ndtgpu_scanproj *h = nullptr;
    ndtgpu_host::check(ndtgpu_scanproj_create(n_scans + 3, 2 * n_beams, &h), "ndtgpu_scanproj_create");
    const size_t stride = 32, map_stride = n_beams * stride + 64;
    std::vector<double> ranges;
    std::vector<uint64_t> rids;
    for (size_t b = 0; b < n_scans; b++) {
        const LaserScanGPU &s = scans[n_scans - 1 - b];
        ranges.insert(ranges.end(), s.ranges.begin(), s.ranges.end());
        rids.push_back(ids[n_scans - 1 - b]);
    }
    std::vector<unsigned char> raw(n_scans * map_stride, 0xCD);
    std::vector<uint32_t> n_kept(n_scans);
    ndtgpu_host::check(ndtgpu_scanproj_project(h, ranges.data(), rids.data(), n_scans, n_beams, scans[0].angle_min, scans[0].angle_increment, &prm,
                                               raw.data(), stride, map_stride, n_kept.data()), "ndtgpu_scanproj_project");
    int equal = 0;
    size_t total = 0, untouched_bad = 0;
    for (size_t b = 0; b < n_scans && b < clouds.size(); b++) {
        const unsigned char *blk = raw.data() + (n_scans - 1 - b) * map_stride;
        const size_t m = n_kept[n_scans - 1 - b];
        bool same = m == clouds[b].size() && m == want_kept[b];
        for (size_t k = 0; same && k < m; k++) same = std::memcmp(&clouds[b].points[k], blk + k * stride, sizeof(pcl::PointXYZ)) == 0;
        CHECK(same, "scan %zu: the mirror differs from the C-ABI (%zu points, %zu by hand, %zu expected)", b, clouds[b].size(), m, want_kept[b]);
        equal += same ? 1 : 0;
        total += m;
        // the pads are NaN with the fourth float 1, and bytes 16 .. 31 of every record and the gap stay as they were
        for (size_t k = m; k < n_beams; k++) {
            float f[4];
            std::memcpy(f, blk + k * stride, sizeof f);
            CHECK(f[0] != f[0] && f[1] != f[1] && f[2] != f[2] && f[3] == 1.0f, "scan %zu: row %zu is not a pad", b, k);
        }
        for (size_t k = 0; k < n_beams; k++)
            for (size_t c = 16; c < stride; c++) untouched_bad += blk[k * stride + c] != 0xCD ? 1 : 0;
        for (size_t c = n_beams * stride; c < map_stride; c++) untouched_bad += blk[c] != 0xCD ? 1 : 0;
        if (m == 0) continue;
        // front() and back(): the first and the last kept beam, as the reference's push_back leaves them
        const pcl::PointXYZ &f = clouds[b].front(), &l = clouds[b].back();
        const double af = scans[b].angle_min + (double)first[b] * scans[b].angle_increment, al = scans[b].angle_min + (double)last[b] * scans[b].angle_increment;
        CHECK(std::fabs(f.x - scans[b].ranges[first[b]] * std::cos(af)) < 1e-5 && std::fabs(f.y - scans[b].ranges[first[b]] * std::sin(af)) < 1e-5,
              "scan %zu: front() is not beam %zu", b, first[b]);
        CHECK(std::fabs(l.x - scans[b].ranges[last[b]] * std::cos(al)) < 1e-5 && std::fabs(l.y - scans[b].ranges[last[b]] * std::sin(al)) < 1e-5,
              "scan %zu: back() is not beam %zu", b, last[b]);
        // the host function's flag and z for the first kept beam
        float p[3];
        CHECK(ndtgpu_scanproj_beam(&prm, scans[b].angle_min, scans[b].angle_increment, ids[b], (uint32_t)first[b], scans[b].ranges[first[b]], p) == 1 &&
              p[2] == f.z && f.z >= 0.f && f.z < 0.02f && f.pad == 1.0f, "scan %zu: z of front()", b);
    }
    CHECK(untouched_bad == 0, "%zu bytes outside the records' first 16 were written", untouched_bad);
    ndtgpu_scanproj_destroy(h);

    // scans of different shapes are refused, no scans give no clouds
    std::vector<LaserScanGPU> odd = {scans[0], scans[1]};
    odd[1].ranges.pop_back();
    bool refused = false;
    try {
        projectLaserGPU(odd);
    } catch (const ndtgpu_host::Error &e) {
        refused = e.status == NDTGPU_ERR_INVALID;
    }
    CHECK(refused, "scans of different sizes must be refused");
    CHECK(projectLaserGPU({}).empty(), "no scans, no clouds");

    std::printf("scanproject_demo: %zu scans, %zu points, %d scans equal to the C-ABI bit for bit, %d failures\n", n_scans, total, equal, g_fails);
    return g_fails ? 1 : 0;
}
