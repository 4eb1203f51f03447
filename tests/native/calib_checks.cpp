// calib_checks.cpp -- a stand-alone host program (no HIP, no device) over what csrc/ndt_calib.h shares with host code: the lattice
// walk, the motion of a pair, the pair selection, the checks of a search's arguments, parameters and tables, and the chunk
// arithmetic of the launches.  The outputs go into heap blocks of exactly the size a call may touch, so the address sanitizer sees
// any step past an end (build it with -fsanitize=address,undefined to check that).  Exit code 0 = every check passed.
#include "../../ndt_feature_graph_amd/csrc/ndt_calib.h"
#include "../../ndt_feature_graph_amd/csrc/ndt_lattice.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

static void pose(double x, double y, double yaw, double *p) { p[0] = x; p[1] = y; p[2] = std::cos(yaw); p[3] = std::sin(yaw); }

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const size_t cap = NDT_CALIB_MAX_CANDIDATES;

    // ---- the lattice: the loop itself, into blocks of exactly the count
    {
        const size_t n = ndt_calib_axis(0.19, 0.1, 0.02, nullptr, 0, cap);
        CHECK(n == 11, "0.19 +- 0.1 by 0.02: %zu nodes (rounding gives an eleventh)", n);
        std::vector<double> v(n);
        CHECK(ndt_calib_axis(0.19, 0.1, 0.02, v.data(), n, cap) == n, "second walk");
        double w = 0.19 - 0.1;
        for (size_t k = 0; k < n; k++, w += 0.02) CHECK(v[k] == w, "node %zu", k);
        CHECK(v[n - 1] < 0.19 + 0.1 && !(w < 0.19 + 0.1), "the end of the walk");
        std::vector<double> few(3);
        CHECK(ndt_calib_axis(0.19, 0.1, 0.02, few.data(), 3, cap) == n && few[2] == v[2], "a short block gets the first nodes only");
        CHECK(ndt_calib_axis(0.2, 0.05, 0.01, nullptr, 0, cap) == 10, "0.2 +- 0.05 by 0.01");
        CHECK(ndt_calib_axis(0.0, 1.0, 4.0, nullptr, 0, cap) == 1, "a step beyond the span: one node");
        CHECK(ndt_calib_axis(0.0, 1.0, 1e-12, nullptr, 0, 1000) == 1001, "more nodes than the cap: cap + 1, and the walk stops");
        CHECK(ndt_calib_axis(1e17, 1.0, 1e-3, nullptr, 0, 1000) <= 1001, "a step below the spacing of the doubles ends at the cap");
    }
    int refused = 0, tried = 0;
#define REFUSED(expr, word)                                                                              \
    do {                                                                                                 \
        const char *m_ = (expr);                                                                         \
        tried++;                                                                                         \
        if (m_ && std::strstr(m_, word)) refused++; else CHECK(false, "%s: %s", #expr, m_ ? m_ : "accepted"); \
    } while (0)
    CHECK(!ndt_calib_check_lattice(0.2, 0, 0, 0.05, 0.05, 0.02, 0.01, 0.001), "the defaults' kind of lattice");
    REFUSED(ndt_calib_check_lattice(nan, 0, 0, 0.05, 0.05, 0.02, 0.01, 0.001), "ix");
    REFUSED(ndt_calib_check_lattice(0, inf, 0, 0.05, 0.05, 0.02, 0.01, 0.001), "iy");
    REFUSED(ndt_calib_check_lattice(0, 0, 0, 0.0, 0.05, 0.02, 0.01, 0.001), "x_s");
    REFUSED(ndt_calib_check_lattice(0, 0, 0, 0.05, -1.0, 0.02, 0.01, 0.001), "y_s");
    REFUSED(ndt_calib_check_lattice(0, 0, 0, 0.05, 0.05, nan, 0.01, 0.001), "yaw_s");
    REFUSED(ndt_calib_check_lattice(0, 0, 0, 0.05, 0.05, 0.02, 0.0, 0.001), "t_r");
    REFUSED(ndt_calib_check_lattice(0, 0, 0, 0.05, 0.05, 0.02, 0.01, inf), "yaw_r");

    // ---- the motion of a pair
    {
        double p1[4], p2[4], D[4];
        pose(1.0, 2.0, 0.3, p1);
        pose(1.5, 1.0, 1.1, p2);
        ndt_calib_pair_motion(p1, p2, D);
        CHECK(std::fabs(D[2] - std::cos(0.8)) < 1e-15 && std::fabs(D[3] - std::sin(0.8)) < 1e-15, "the rotation of D");
        // pose1 o D = pose2
        const double x = p1[0] + p1[2] * D[0] - p1[3] * D[1], y = p1[1] + p1[3] * D[0] + p1[2] * D[1];
        CHECK(std::fabs(x - p2[0]) < 1e-15 && std::fabs(y - p2[1]) < 1e-15, "pose1 o D is pose2");
        pose(1.0, 2.0, 0.0, p1);
        ndt_calib_pair_motion(p1, p1, D);
        CHECK(D[0] == 0.0 && D[1] == 0.0 && D[2] == 1.0 && D[3] == 0.0, "the same pose twice at yaw 0: exactly the identity");
        double tx, ty;
        ndt_calib_translation(D, 0.3, -0.2, std::cos(0.4), std::sin(0.4), tx, ty);
        CHECK(tx == 0.0 && ty == 0.0, "D = I: every candidate's translation is exactly 0");
        CHECK(ndt_calib_term(0.015625, 0.015625) == 0.015625 && ndt_calib_term(0.02, 0.015625) == 0.015625 && ndt_calib_term(0.01, 0.015625) == 0.01,
              "the threshold is strict");
        CHECK(ndt_calib_d2(1, 2, 3, 1, 2, 3) == 0.0 && ndt_calib_d2(1, 0, 0, 0, 2, 0.5) == 5.25, "d2");
        CHECK(ndt_calib_better(1.0, 7, 2.0, 3) && !ndt_calib_better(2.0, 3, 1.0, 7) && ndt_calib_better(1.0, 3, 1.0, 7) && !ndt_calib_better(1.0, 7, 1.0, 3) &&
              !ndt_calib_better(1.0, 3, 1.0, 3), "smallest score, then lowest index");
        CHECK(ndt_calib_usable(1.f, -2.f, 0.f) && !ndt_calib_usable((float)nan, 0.f, 0.f) && !ndt_calib_usable(0.f, (float)inf, 0.f) &&
              !ndt_calib_usable(0.f, 0.f, -(float)inf) && ndt_calib_usable(3.4028234663852886e38f, 0.f, 0.f), "usable rows are the finite ones");
    }

    // ---- the pair selection
    {
        const double deg = M_PI / 180.0;
        const double xy[][3] = {{0, 0, 0}, {0.1, 0, 10 * deg}, {0.2, 0, 24.9 * deg}, {0.3, 0, 25.1 * deg}, {0.35, 0, 30 * deg}, {2.0, 0, 80 * deg},
                                {2.1, 0, 100 * deg}, {2.2, 0.1, 50 * deg}, {2.2, 0.1, 50 * deg}, {2.0, 0.3, 76 * deg}};
        const size_t n = sizeof xy / sizeof xy[0];
        std::vector<double> p4(4 * n);
        for (size_t k = 0; k < n; k++) pose(xy[k][0], xy[k][1], xy[k][2], &p4[4 * k]);
        const size_t m = ndt_calib_select_pairs(p4.data(), n, 1.0, 25 * deg, nullptr, 0);
        CHECK(m == 3, "%zu pairs", m);
        std::vector<uint32_t> pr(2 * m);
        CHECK(ndt_calib_select_pairs(p4.data(), n, 1.0, 25 * deg, pr.data(), m) == m, "second walk");
        const uint32_t want[] = {0, 3, 5, 7, 7, 9};
        CHECK(std::memcmp(pr.data(), want, sizeof want) == 0, "the pairs are (0,3) (5,7) (7,9)");
        std::vector<uint32_t> one(2);
        CHECK(ndt_calib_select_pairs(p4.data(), n, 1.0, 25 * deg, one.data(), 1) == m && one[0] == 0 && one[1] == 3, "room for one pair");
        CHECK(ndt_calib_select_pairs(p4.data(), 1, 1.0, 25 * deg, nullptr, 0) == 0 && ndt_calib_select_pairs(nullptr, 0, 1.0, 25 * deg, nullptr, 0) == 0,
              "one pose or none: no pair");
        CHECK(ndt_calib_select_pairs(p4.data(), n, 1.0, 0.0, nullptr, 0) == 8, "without the yaw gate every step within a metre is a pair");
        CHECK(ndt_calib_abs_yaw(1.0000000000000002) == 0.0 && std::fabs(ndt_calib_abs_yaw(-1.0000000000000002) - M_PI) < 1e-15, "the cosine is clamped");
    }

    // ---- the checks of a search
    ndtgpu_calib_params prm;
    prm.max_dist = 0.1;
    CHECK(!ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 100, 100, 20) && !ndt_calib_check_params(prm), "the launch files' shape");
    CHECK(!ndt_calib_check_args(1u << 20, 1u << 16, 12, (size_t)12 << 16, 1024, 1u << 24, 1, 1), "the limits themselves");
    REFUSED(ndt_calib_check_args(0, 720, 16, 720 * 16, 16, 10, 10, 10), "n_scans");
    REFUSED(ndt_calib_check_args((1u << 20) + 1, 720, 16, 720 * 16, 16, 10, 10, 10), "n_scans");
    REFUSED(ndt_calib_check_args(32, 0, 16, 16, 16, 10, 10, 10), "n_points");
    REFUSED(ndt_calib_check_args(32, (1u << 16) + 1, 16, ((size_t)16 << 16) + 16, 16, 10, 10, 10), "n_points");
    REFUSED(ndt_calib_check_args(32, 720, 8, 720 * 16, 16, 10, 10, 10), "stride_bytes");
    REFUSED(ndt_calib_check_args(32, 720, 14, 720 * 16, 16, 10, 10, 10), "stride_bytes");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16 - 4, 16, 10, 10, 10), "map_stride_bytes");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16 + 2, 16, 10, 10, 10), "map_stride_bytes");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 0, 10, 10, 10), "n_pairs");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 1025, 10, 10, 10), "n_pairs");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 0, 10, 10), "nx");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 10, 0, 10), "ny");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 10, 10, 0), "nyaw");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 4096, 4096, 2), "candidates");
    REFUSED(ndt_calib_check_args(32, 720, 16, 720 * 16, 16, 1u << 24, 1u << 24, 1u << 24), "candidates");
    prm.max_dist = 0.0;
    REFUSED(ndt_calib_check_params(prm), "max_dist");
    prm.max_dist = nan;
    REFUSED(ndt_calib_check_params(prm), "max_dist");
    prm.max_dist = inf;
    REFUSED(ndt_calib_check_params(prm), "max_dist");
    REFUSED(ndt_calib_check_capacity(0, 720, 1000), "max_pairs");
    REFUSED(ndt_calib_check_capacity(1025, 720, 1000), "max_pairs");
    REFUSED(ndt_calib_check_capacity(16, 0, 1000), "max_points");
    REFUSED(ndt_calib_check_capacity(16, 720, (1u << 24) + 1), "max_candidates");
    {
        const std::vector<double> xs = {0.1, 0.2}, ys = {0.0}, cs = {1.0, std::cos(0.3)}, sn = {0.0, std::sin(0.3)};
        CHECK(!ndt_lattice_check_tables(xs.data(), 2, ys.data(), 1, cs.data(), sn.data(), 2), "tables");
        const std::vector<double> bx = {0.1, nan}, by = {inf}, bc = {1.0, 0.5};
        REFUSED(ndt_lattice_check_tables(bx.data(), 2, ys.data(), 1, cs.data(), sn.data(), 2), "xs");
        REFUSED(ndt_lattice_check_tables(xs.data(), 2, by.data(), 1, cs.data(), sn.data(), 2), "ys");
        REFUSED(ndt_lattice_check_tables(xs.data(), 2, ys.data(), 1, bc.data(), sn.data(), 2), "cs / sn");
    }

    // ---- the chunks: a multiple of the tile, at least one tile, pairs x chunk within the scratch; the walk of a lattice covers
    // every candidate once and every tile index stays below the tile count
    for (size_t pairs : {(size_t)1, (size_t)3, (size_t)16, (size_t)1000, (size_t)1024})
        for (size_t cands : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)200000, (size_t)1 << 24}) {
            const size_t chunk = ndt_calib_handle_chunk(pairs, cands), tiles = ndt_calib_tiles(cands);
            CHECK(chunk >= NDT_CALIB_TILE && chunk % NDT_CALIB_TILE == 0, "chunk %zu", chunk);
            CHECK(pairs * chunk <= NDT_CALIB_PARTIAL_DOUBLES || chunk == NDT_CALIB_TILE, "pairs %zu x chunk %zu", pairs, chunk);
            CHECK(chunk <= tiles * NDT_CALIB_TILE, "a chunk is never longer than the lattice's tiles");
            size_t covered = 0, top_tile = 0;
            for (size_t first = 0; first < cands; first += chunk) {
                const size_t n = cands - first < chunk ? cands - first : chunk;
                CHECK(first % NDT_CALIB_TILE == 0 && ndt_calib_tiles(n) * NDT_CALIB_TILE <= chunk, "a chunk's tiles fit its stride");
                covered += n;
                top_tile = first / NDT_CALIB_TILE + ndt_calib_tiles(n) - 1;
            }
            CHECK(covered == cands && top_tile == tiles - 1, "pairs %zu, %zu candidates: %zu covered, last tile %zu of %zu", pairs, cands, covered, top_tile, tiles);
        }
    CHECK(ndt_calib_handle_chunk(16, 200000) == 200192 && ndt_calib_handle_chunk(1024, 5000) == 4096, "the chunks the header documents");

    std::printf("calib_checks: %d of %d bad arguments refused, %d failures\n", refused, tried, g_fails);
    return g_fails ? 1 : 0;
}
