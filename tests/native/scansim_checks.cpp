// scansim_checks.cpp -- the scan simulator's shared header (csrc/ndt_scansim.h) on the host, a plain g++ program with its own main,
// built with -fsanitize=address,undefined by tests/test_host_scansim.py: the reach, the cell of a point, the closed form of a step
// against the accumulator of the walk, walks from every cell of small grids in every direction, the lattice's positions, the
// headings and the argument checks.  Every grid, table and output lives in a heap block of exactly the size a call may touch.
#include "../../ndt_feature_graph_amd/csrc/ndt_scansim.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

static uint32_t g_seed = 12345u;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

// the walk by the closed form alone: the specification
static bool walk_spec(const int8_t *grid, int w, int h, int i0, int j0, int di, int dj, int R, int occ, int unk, uint32_t &d2)
{
    const NdtScansimRay r = ndt_scansim_ray_of(di, dj);
    for (int k = 1; k <= r.n; k++) {
        int32_t a, b;
        ndt_scansim_step_cell(r, k, a, b);
        const int i = i0 + a, j = j0 + b;
        if (i < 0 || j < 0 || i >= w || j >= h) return false;
        if (a * a + b * b > R * R) return false;
        const int v = grid[(size_t)j * w + i];
        if (v >= occ || (unk && v < 0)) { d2 = (uint32_t)(a * a + b * b); return true; }
    }
    return false;
}

int main()
{
    // the reach and the skip
    CHECK(ndt_scansim_reach(10.0, 0.05) == 200 && ndt_scansim_reach(0.04, 0.05) == 0 && ndt_scansim_reach(4094.5, 1.0) == 4094 &&
              ndt_scansim_reach(4095.0, 1.0) == 0 && ndt_scansim_reach(NAN, 1.0) == 0, "reach");
    CHECK(ndt_scansim_skip(1.0, 0.05) == 20 && ndt_scansim_skip(0.04, 0.05) == 0 && ndt_scansim_skip(1e9, 0.05) == 0 && ndt_scansim_skip(NAN, 1.0) == 0 &&
              ndt_scansim_skip(32768.5, 1.0) == 32768, "skip");
    // the cell of a point
    {
        int32_t i = -7, j = -7;
        CHECK(ndt_scansim_point_cell(0.49, 0.0, 0.0, 0.0, 0.05, 10, 10, i, j) && i == 9 && j == 0, "cell (%d, %d)", i, j);
        CHECK(!ndt_scansim_point_cell(0.5, 0.0, 0.0, 0.0, 0.05, 10, 10, i, j) && !ndt_scansim_point_cell(-1e-12, 0.0, 0.0, 0.0, 0.05, 10, 10, i, j) &&
                  !ndt_scansim_point_cell(NAN, 0.0, 0.0, 0.0, 0.05, 10, 10, i, j) && !ndt_scansim_point_cell(0.1, INFINITY, 0.0, 0.0, 0.05, 10, 10, i, j),
              "points off the map");
    }
    // the closed form: ends on (di, dj), steps of at most one cell, point symmetry; up to the largest ray without overflow
    size_t rays = 0;
    for (int di = -40; di <= 40; di++)
        for (int dj = -40; dj <= 40; dj++) {
            const NdtScansimRay r = ndt_scansim_ray_of(di, dj), q = ndt_scansim_ray_of(-di, -dj);
            int32_t pa = 0, pb = 0;
            for (int k = 1; k <= r.n; k++) {
                int32_t a, b, a2, b2;
                ndt_scansim_step_cell(r, k, a, b);
                ndt_scansim_step_cell(q, k, a2, b2);
                CHECK(std::abs(a - pa) <= 1 && std::abs(b - pb) <= 1 && a2 == -a && b2 == -b, "ray (%d, %d) step %d", di, dj, k);
                pa = a;
                pb = b;
            }
            CHECK(pa == di && pb == dj, "ray (%d, %d) ends on (%d, %d)", di, dj, pa, pb);
            rays++;
        }
    {
        int32_t a, b;
        ndt_scansim_step_cell(ndt_scansim_ray_of(32768, -32768), 32768, a, b);
        CHECK(a == 32768 && b == -32768, "the longest ray ends on (%d, %d)", a, b);
        ndt_scansim_step_cell(ndt_scansim_ray_of(-32768, 32767), 16384, a, b);
        CHECK(a == -16384 && b == 16384, "the longest ray, half way: (%d, %d)", a, b);
    }
    // walks: the accumulator against the closed form, from every cell of small grids, every direction, in blocks of exactly w * h bytes
    size_t walks = 0, hits = 0;
    const int shapes[][2] = {{1, 1}, {3, 5}, {7, 4}, {13, 11}};
    for (const auto &s : shapes) {
        const int w = s[0], h = s[1];
        for (int fill = 0; fill < 3; fill++) {
            std::unique_ptr<int8_t[]> grid(new int8_t[(size_t)w * h]);
            for (int k = 0; k < w * h; k++) {
                const uint32_t v = rnd() >> 24;
                grid[k] = fill == 0 ? 0 : (v < 20 ? 100 : (v < 40 ? -1 : (v < 50 ? 55 : (v < 60 ? 30 : 0))));
            }
            for (int j0 = 0; j0 < h; j0++)
                for (int i0 = 0; i0 < w; i0++)
                    for (int di = -15; di <= 15; di++)
                        for (int dj = -15; dj <= 15; dj++) {
                            const int R = 1 + (int)(rnd() % 16), occ = (rnd() & 1) ? 55 : 70, unk = (int)(rnd() >> 31);
                            uint32_t d2 = 0, want2 = 0;
                            const bool hit = ndt_scansim_walk(grid.get(), (uint32_t)w, (uint32_t)h, i0, j0, ndt_scansim_ray_of(di, dj), R, occ, unk, d2);
                            const bool want = walk_spec(grid.get(), w, h, i0, j0, di, dj, R, occ, unk, want2);
                            CHECK(hit == want && d2 == want2, "walk from (%d, %d) by (%d, %d) in %d x %d", i0, j0, di, dj, w, h);
                            CHECK(!hit || (d2 >= 1 && d2 <= (uint32_t)(R * R)), "d2 %u beyond the reach %d", d2, R);
                            walks++;
                            hits += hit;
                        }
        }
    }
    CHECK(hits > walks / 50 && hits < walks, "%zu hits of %zu walks", hits, walks);
    // the ray of a beam: unit directions give at most R + 2 steps; a direction that is no unit vector, or a NaN, is a miss without a walk
    for (int t = 0; t < 2000; t++) {
        const double a = (rnd() % 62832) * 1e-4, b = (rnd() % 62832) * 1e-4, res = 0.05, rm = res * (1 + rnd() % 4094) + 0.01;
        const double x = (rnd() % 1000) * 0.013, y = (rnd() % 1000) * 0.017;
        int32_t i0, j0;
        if (!ndt_scansim_point_cell(x, y, -1.0, -2.0, res, 400, 400, i0, j0)) continue;
        NdtScansimRay r;
        const bool ok = ndt_scansim_beam_ray(x, y, cos(a), sin(a), cos(b), sin(b), rm, -1.0, -2.0, res, i0, j0, r);
        CHECK(ok && r.n <= ndt_scansim_reach(rm, res) + 2 && r.dmin <= r.n, "a unit ray of %d steps, R %d", r.n, ndt_scansim_reach(rm, res));
    }
    {
        NdtScansimRay r;
        CHECK(!ndt_scansim_beam_ray(0.0, 0.0, 1e9, 0.0, 1.0, 0.0, 10.0, 0.0, 0.0, 0.05, 0, 0, r) &&
                  !ndt_scansim_beam_ray(0.0, 0.0, NAN, 0.0, 1.0, 0.0, 10.0, 0.0, 0.0, 0.05, 0, 0, r) &&
                  !ndt_scansim_beam_ray(0.0, 0.0, 1.0, 0.0, 1.0, INFINITY, 10.0, 0.0, 0.0, 0.05, 0, 0, r),
              "rays that are refused");
    }
    CHECK(ndt_scansim_metres(400, 0.05) == 0.05 * sqrt(400.0) && ndt_scansim_metres(0, 0.05) == 0.0, "metres");
    // the lattice: every position of the last row and column reads inside the block
    const int lat[][3] = {{5, 9, 7}, {9, 7, 1}, {9, 7, 2}, {1, 1, 3}, {64, 3, 5}};
    for (const auto &l : lat) {
        const uint32_t w = (uint32_t)l[0], h = (uint32_t)l[1], skip = (uint32_t)l[2];
        std::unique_ptr<int8_t[]> grid(new int8_t[(size_t)w * h]);
        for (uint32_t k = 0; k < w * h; k++) grid[k] = (rnd() >> 30) ? 0 : 100;
        const uint32_t npx = ndt_scansim_axis_nodes(w, skip), npy = ndt_scansim_axis_nodes(h, skip);
        const double box[4] = {-0.1, 0.41, 0.12, 1e9};
        uint32_t kept = 0, want = 0;
        for (uint32_t px = 0; px < npx; px++)
            for (uint32_t py = 0; py < npy; py++) {
                double cx, cy;
                kept += ndt_scansim_position(grid.get(), w, px, py, skip, -0.2, 0.4, 0.05, box, cx, cy);
                CHECK(cx == -0.2 + (px * skip + 0.5) * 0.05 && cy == 0.4 + (py * skip + 0.5) * 0.05, "centre of (%u, %u)", px, py);
            }
        for (uint32_t ix = 0; ix < w; ix += skip)
            for (uint32_t iy = 0; iy < h; iy += skip) {
                const double cx = -0.2 + (ix + 0.5) * 0.05, cy = 0.4 + (iy + 0.5) * 0.05;
                want += grid[(size_t)iy * w + ix] == 0 && cx >= box[0] && cx <= box[2] && cy >= box[1] && cy <= box[3];
            }
        CHECK(kept == want && (npx - 1) * skip < w && (npy - 1) * skip < h, "lattice %u x %u skip %u: %u kept, %u by the loops", w, h, skip, kept, want);
    }
    CHECK(ndt_scansim_tiles(0) == 0 && ndt_scansim_tiles(256) == 1 && ndt_scansim_tiles(257) == 2, "tiles");
    // the headings, into tables of exactly their size
    {
        const size_t n = ndt_scansim_headings(M_PI / 4, nullptr, nullptr, 0);
        std::unique_ptr<double[]> cs(new double[n]), sn(new double[n]);
        CHECK(n == 8 && ndt_scansim_headings(M_PI / 4, cs.get(), sn.get(), n) == 8 && cs[0] == 1.0 && sn[0] == 0.0 && fabs(cs[4] + 1.0) < 1e-15, "headings");
        double one_c = 7.0, one_s = 7.0;
        CHECK(ndt_scansim_headings(1.0, &one_c, &one_s, 1) == 7 && one_c == 1.0 && one_s == 0.0, "headings beyond the room are counted, not written");
        CHECK(ndt_scansim_headings(6.28, nullptr, nullptr, 0) == 1 && ndt_scansim_headings(7.0, nullptr, nullptr, 0) == 1, "one heading");
        double theta = 0.0;
        size_t want = 0;
        for (; theta < 6.28; theta += 0.1) want++;
        CHECK(ndt_scansim_headings(0.1, nullptr, nullptr, 0) == want, "repeated addition");
    }
    // the checks: every bad argument is refused with a message that names it
    int refused = 0, asked = 0;
    ndtgpu_scansim_params p{10.0, 11.0, 55, 1};
    auto bad = [&](const char *msg, const char *word) {
        asked++;
        if (msg && std::strstr(msg, word)) refused++;
        else std::printf("FAIL: expected a message with '%s', got '%s'\n", word, msg ? msg : "(accepted)");
    };
    CHECK(!ndt_scansim_check_params(p) && !ndt_scansim_check_grids(1024, 1 << 15, 1 << 15, 0.05) && !ndt_scansim_check_reach(0.05, p) &&
              !ndt_scansim_check_beams(8192, -3.0, 0.1) && !ndt_scansim_check_poses(1 << 24) && !ndt_scansim_check_capacity(1024, 8192, 1 << 24) &&
              !ndt_scansim_check_lattice(1 << 15, 1 << 15, 1, 3, nullptr, 1 << 24),
          "good arguments are accepted");
    ndtgpu_scansim_params q = p;
    q.range_max = 0.0; bad(ndt_scansim_check_params(q), "range_max");
    q.range_max = NAN; bad(ndt_scansim_check_params(q), "range_max");
    q.range_max = INFINITY; bad(ndt_scansim_check_params(q), "range_max");
    q = p; q.miss = NAN; bad(ndt_scansim_check_params(q), "miss");
    q = p; q.occupied_min = 128; bad(ndt_scansim_check_params(q), "occupied_min");
    q = p; q.occupied_min = -129; bad(ndt_scansim_check_params(q), "occupied_min");
    q = p; q.unknown_is_obstacle = 2; bad(ndt_scansim_check_params(q), "unknown_is_obstacle");
    q = p; q.range_max = 0.04; bad(ndt_scansim_check_reach(0.05, q), "reach");
    q = p; q.range_max = 204.8; bad(ndt_scansim_check_reach(0.05, q), "reach");
    bad(ndt_scansim_check_grids(0, 4, 4, 0.05), "n_grids");
    bad(ndt_scansim_check_grids(1025, 4, 4, 0.05), "n_grids");
    bad(ndt_scansim_check_grids(1, 0, 4, 0.05), "width");
    bad(ndt_scansim_check_grids(1, (1 << 15) + 1, 4, 0.05), "width");
    bad(ndt_scansim_check_grids(1, 4, 0, 0.05), "height");
    bad(ndt_scansim_check_grids(1, 4, (1 << 15) + 1, 0.05), "height");
    bad(ndt_scansim_check_grids(1, 4, 4, 0.0), "resolution");
    bad(ndt_scansim_check_grids(1, 4, 4, NAN), "resolution");
    bad(ndt_scansim_check_beams(0, 0.0, 0.1), "n_beams");
    bad(ndt_scansim_check_beams(8193, 0.0, 0.1), "n_beams");
    bad(ndt_scansim_check_beams(4, NAN, 0.1), "angle_min");
    bad(ndt_scansim_check_beams(4, 0.0, INFINITY), "angle_increment");
    bad(ndt_scansim_check_poses(0), "n_poses");
    bad(ndt_scansim_check_poses((1 << 24) + 1), "n_poses");
    bad(ndt_scansim_check_capacity(0, 8, 8), "max_grids");
    bad(ndt_scansim_check_capacity(1, 8193, 8), "max_beams");
    bad(ndt_scansim_check_capacity(1, 8, 0), "max_poses");
    bad(ndt_scansim_check_lattice(8, 8, 0, 3, nullptr, 8), "skip");
    bad(ndt_scansim_check_lattice(8, 8, (1 << 15) + 1, 3, nullptr, 8), "skip");
    bad(ndt_scansim_check_lattice(8, 8, 1, 0, nullptr, 8), "nyaw");
    bad(ndt_scansim_check_lattice(8, 8, 1, 3, nullptr, 0), "capacity");
    bad(ndt_scansim_check_lattice(8, 8, 1, 3, nullptr, (1 << 24) + 1), "capacity");
    const double nan_box[4] = {0.0, 0.0, NAN, 1.0};
    bad(ndt_scansim_check_lattice(8, 8, 1, 3, nan_box, 8), "box4");
    bad(ndt_scansim_check_lattice(1 << 15, 1 << 15, 1, 8, nullptr, 8), "nodes");
    CHECK(refused == asked, "%d of %d refused", refused, asked);
    std::printf("scansim_checks: %zu rays, %zu walks (%zu hits), %d of %d bad arguments refused, %d failures\n", rays, walks, hits, refused, asked, g_fails);
    return g_fails ? 1 : 0;
}
