// locmon_checks.cpp -- a stand-alone host program (no HIP, no device) over what csrc/ndt_locmon.h shares with host code: the radius,
// the two passes of the distance field, the range gate, the pixel of an endpoint, the keys and their badness, the composition of
// a picked pose, the words of the two ordered selections, the chunk arithmetic and the checks of every call's arguments.  The
// grids, the row pass's bytes and the fields live in heap blocks of exactly width x height elements, so the address sanitizer sees
// any step past an end (build it with -fsanitize=address,undefined to check that).  Exit code 0 = every check passed.
#include "../../ndt_feature_graph_amd/csrc/ndt_locmon.h"
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

// the field of one grid by the two passes, every block exactly sized
static std::vector<uint16_t> field_two_pass(const std::vector<int8_t> &g, uint32_t w, uint32_t h, int R, int occ)
{
    std::vector<uint8_t> row((size_t)w * h);
    std::vector<uint16_t> f((size_t)w * h);
    for (uint32_t y = 0; y < h; y++) {
        std::vector<int8_t> line(g.begin() + (size_t)y * w, g.begin() + (size_t)(y + 1) * w);   // (a row of its own: a step past it is seen)
        for (uint32_t x = 0; x < w; x++) row[(size_t)y * w + x] = (uint8_t)ndt_locmon_row_dist(line.data(), x, w, R, occ);
    }
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) f[(size_t)y * w + x] = (uint16_t)ndt_locmon_col_dist(row.data(), x, y, w, h, R);
    return f;
}

// ... and by the definition: the smallest dx^2 + dy^2 <= R^2 over the obstacle pixels
static std::vector<uint16_t> field_brute(const std::vector<int8_t> &g, uint32_t w, uint32_t h, int R, int occ)
{
    std::vector<uint16_t> f((size_t)w * h, (uint16_t)NDT_LOCMON_FIELD_FAR);
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++)
            for (int yy = 0; yy < (int)h; yy++)
                for (int xx = 0; xx < (int)w; xx++) {
                    if ((int)g[(size_t)yy * w + xx] < occ) continue;
                    const int k = (xx - x) * (xx - x) + (yy - y) * (yy - y);
                    if (k <= R * R && k < (int)f[(size_t)y * w + x]) f[(size_t)y * w + x] = (uint16_t)k;
                }
    return f;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the radius
    CHECK(ndt_locmon_radius(0.375, 0.05) == 7 && ndt_locmon_radius(0.375, 0.1) == 3 && ndt_locmon_radius(1.0, 1.0) == 1, "radius");
    CHECK(ndt_locmon_radius(0.04, 0.05) == 0 && ndt_locmon_radius(255.0, 1.0) == 0 && ndt_locmon_radius(254.0, 1.0) == 254, "radius limits");
    CHECK(ndt_locmon_radius(nan, 0.05) == 0 && ndt_locmon_radius(inf, 0.05) == 0, "radius of a non-finite reach");

    // ---- the field: two passes against the definition, on grids with every kind of pixel
    {
        uint64_t s = 88172645463325252ull;
        auto next = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        const uint32_t shapes[][2] = {{1, 1}, {5, 3}, {3, 5}, {17, 9}, {31, 23}};
        const int8_t kinds[] = {-1, 0, 0, 0, 0, 0, 30, 54, 55, 70, 100, 0, 0, 0, 0, 0};
        for (const auto &sh : shapes)
            for (int R : {1, 2, 7, 20, 254})
                for (int occ : {55, 70}) {
                    std::vector<int8_t> g((size_t)sh[0] * sh[1]);
                    for (int8_t &v : g) v = kinds[next() % 16];
                    const std::vector<uint16_t> a = field_two_pass(g, sh[0], sh[1], R, occ), b = field_brute(g, sh[0], sh[1], R, occ);
                    CHECK(a == b, "field %u x %u, R %d, occupied_min %d", sh[0], sh[1], R, occ);
                }
        std::vector<int8_t> empty(35, 0), full(35, 100), corner(35, 0);
        corner[0] = 55;
        CHECK(field_two_pass(empty, 7, 5, 3, 55) == std::vector<uint16_t>(35, (uint16_t)NDT_LOCMON_FIELD_FAR), "an empty grid is far everywhere");
        CHECK(field_two_pass(full, 7, 5, 3, 55) == std::vector<uint16_t>(35, (uint16_t)0), "all obstacle");
        const std::vector<uint16_t> c = field_two_pass(corner, 7, 5, 3, 55);
        CHECK(c[0] == 0 && c[3] == 9 && c[4] == NDT_LOCMON_FIELD_FAR && c[2 * 7 + 2] == 8 && c[3 * 7 + 1] == NDT_LOCMON_FIELD_FAR, "a corner obstacle");
        CHECK(field_two_pass(corner, 7, 5, 3, 56) == std::vector<uint16_t>(35, (uint16_t)NDT_LOCMON_FIELD_FAR), "55 is no obstacle at 56");
    }

    // ---- the range gate
    CHECK(ndt_locmon_kept(1.0, 0.0, inf) && ndt_locmon_kept(1e300, 0.0, inf) && ndt_locmon_kept(0.5, 0.4, 0.6), "kept");
    CHECK(!ndt_locmon_kept(nan, 0.0, inf) && !ndt_locmon_kept(inf, 0.0, inf) && !ndt_locmon_kept(-inf, 0.0, inf), "non-finite ranges are dropped");
    CHECK(!ndt_locmon_kept(0.0, 0.0, inf) && !ndt_locmon_kept(-1.0, 0.0, inf) && !ndt_locmon_kept(0.4, 0.4, 0.6) && !ndt_locmon_kept(0.6, 0.4, 0.6),
          "at or below r_min, at or above r_max");

    // ---- the pixel of an endpoint
    {
        uint32_t fi = 77, fj = 77;
        CHECK(ndt_locmon_pixel(0, 0, 1, 0, 1, 0, 0.49, 0, 0, 0.05, 10, 10, fi, fj) && fi == 9 && fj == 0, "the last pixel of the row");
        CHECK(!ndt_locmon_pixel(0, 0, 1, 0, 1, 0, 0.5, 0, 0, 0.05, 10, 10, fi, fj), "fi = width is off the map");
        CHECK(!ndt_locmon_pixel(-1e-12, 0, 1, 0, 1, 0, 0.0, 0, 0, 0.05, 10, 10, fi, fj), "fi = -1 is off the map");
        CHECK(!ndt_locmon_pixel(0, 0, 1, 0, 1, 0, nan, 0, 0, 0.05, 10, 10, fi, fj) && !ndt_locmon_pixel(nan, 0, 1, 0, 1, 0, 1.0, 0, 0, 0.05, 10, 10, fi, fj),
              "a NaN is off the map");
        CHECK(!ndt_locmon_pixel(0, 0, 1, 0, 1, 0, 1e300, 0, 0, 0.05, 10, 10, fi, fj) && !ndt_locmon_pixel(0, 0, 1, 0, 0, 1, 1e300, 0, 0, 1e-300, 10, 10, fi, fj),
              "an overflowing quotient is off the map");
        CHECK(ndt_locmon_pixel(1.0, 2.0, 0, 1, 1, 0, 0.26, 1.0, 2.0, 0.05, 10, 10, fi, fj) && fi == 0 && fj == 5, "a quarter turn: the beam looks along y");
        CHECK(fi == 0 && fj == 5, "outputs are written only in bounds");
    }

    // ---- keys and badness
    CHECK(ndt_locmon_key_of_field(0) == 0 && ndt_locmon_key_of_field(49) == 49 && ndt_locmon_key_of_field(NDT_LOCMON_FIELD_FAR) == NDT_LOCMON_KEY_FAR, "keys");
    CHECK(ndt_locmon_metres(0, 0.05, 0.375) == 0.0 && ndt_locmon_metres(49, 0.05, 0.375) == 0.05 * 7.0 && ndt_locmon_metres(2, 0.1, 0.375) == 0.1 * std::sqrt(2.0),
          "metres");
    CHECK(ndt_locmon_metres(NDT_LOCMON_KEY_FAR, 0.05, 0.375) == 0.375 && ndt_locmon_metres(NDT_LOCMON_KEY_OFFMAP, 0.05, 0.375) == 1e9 &&
          ndt_locmon_metres(0xFFFFFFFFu, 0.05, 0.375) == 1e9, "far and off the map");
    CHECK(NDT_LOCMON_KEY_OFFMAP < (1u << NDT_LOCMON_KEY_BITS) && NDT_LOCMON_MAX_RADIUS * NDT_LOCMON_MAX_RADIUS < (int)NDT_LOCMON_FIELD_FAR, "key ranges");

    // ---- the picked pose
    {
        std::vector<double> out(4);
        const double ref[4] = {1.0, 2.0, std::cos(0.5), std::sin(0.5)}, m[4] = {0.4, -0.1, std::cos(0.3), std::sin(0.3)};
        ndt_locmon_compose(ref, m, -0.275, 0.0, out.data());
        const double c = std::cos(0.5), s = std::sin(0.5), wx = 1.0 + c * 0.4 + s * 0.1, wy = 2.0 + s * 0.4 - c * 0.1;
        CHECK(std::fabs(out[0] - (wx - 0.275 * std::cos(0.8))) < 1e-12 && std::fabs(out[1] - (wy - 0.275 * std::sin(0.8))) < 1e-12, "compose: position");
        CHECK(std::fabs(out[2] - std::cos(0.8)) < 1e-12 && std::fabs(out[3] - std::sin(0.8)) < 1e-12, "compose: heading");
        const double id[4] = {0, 0, 1, 0};
        ndt_locmon_compose(ref, id, 0.0, 0.0, out.data());
        CHECK(out[0] == ref[0] && out[1] == ref[1] && out[2] == ref[2] && out[3] == ref[3], "compose with the identity");
    }

    // ---- the ordered selections
    CHECK(ndt_locmon_min_word(3, 9) < ndt_locmon_min_word(4, 0) && ndt_locmon_min_word(3, 9) < ndt_locmon_min_word(3, 10), "smaller key, then lower index");
    CHECK(ndt_locmon_min_word(NDT_LOCMON_KEY_OFFMAP, 0xFFFFFFu) < ~0ull, "every candidate beats the filler");
    CHECK(ndt_locmon_pick_word(0, 8, 8, 0) == 0 && ndt_locmon_pick_word(1, 50, 8, 0) == 0 && ndt_locmon_pick_word(0, 0, 0, 0) == 0 &&
          ndt_locmon_pick_word(0, -3, -5, 0) == 0, "a pair that does not qualify");
    CHECK(ndt_locmon_pick_word(0, 9, 8, 5) > 0 && ndt_locmon_pick_word(0, 10, 8, 7) > ndt_locmon_pick_word(0, 9, 8, 5) &&
          ndt_locmon_pick_word(0, 9, 8, 5) > ndt_locmon_pick_word(0, 9, 8, 6), "more inliers, then the lower pair");
    CHECK((uint32_t)(ndt_locmon_pick_word(0, 9, 8, 5) >> 32) == 9 && 0xFFFFFFFFu - (uint32_t)ndt_locmon_pick_word(0, 9, 8, 5) == 5, "the word gives both back");

    // ---- chunks
    CHECK(ndt_locmon_tiles(1) == 1 && ndt_locmon_tiles(256) == 1 && ndt_locmon_tiles(257) == 2, "tiles");
    CHECK(ndt_locmon_handle_chunk(8192, 1 << 24) == 1024 && ndt_locmon_handle_chunk(8192, 1127) == 1024 && ndt_locmon_handle_chunk(8192, 300) == 512,
          "8192 beams: 1024 candidates a chunk, or the lattice rounded up to the tile");
    CHECK(ndt_locmon_handle_chunk(1440, 126000) == 5632 && ndt_locmon_handle_chunk(1, 1 << 24) == (size_t)1 << 23 && ndt_locmon_handle_chunk(64, 1) == 256, "chunks");
    for (size_t mb : {(size_t)1, (size_t)33, (size_t)1440, (size_t)8192})
        CHECK(ndt_locmon_handle_chunk(mb, 1 << 24) % NDT_LOCMON_TILE == 0 && ndt_locmon_handle_chunk(mb, 1 << 24) >= NDT_LOCMON_TILE, "a multiple of the tile");

    // ---- the checks
    int refused = 0, tried = 0;
#define REFUSED(expr, word)                                                                              \
    do {                                                                                                 \
        const char *m_ = (expr);                                                                         \
        tried++;                                                                                         \
        if (m_ && std::strstr(m_, word)) refused++; else CHECK(false, "%s: %s", #expr, m_ ? m_ : "accepted"); \
    } while (0)
    ndtgpu_locmon_params p{};
    p.max_dist = 0.375; p.r_min = 0.0; p.r_max = inf; p.post_x = -0.275; p.post_y = 0.0; p.occupied_min = 55; p.min_num_matches = 8;
    CHECK(!ndt_locmon_check_params(p) && !ndt_locmon_check_grids(3, 67, 65, 0.05, p) && !ndt_locmon_check_grids(1024, 1 << 15, 64, 0.05, p), "fine");
    CHECK(!ndt_locmon_check_beams(1, 0.0, 0.0) && !ndt_locmon_check_beams(8192, -3.14, 1e-3) && !ndt_locmon_check_counts(1, 0) &&
          !ndt_locmon_check_counts(1 << 24, 1 << 24) && !ndt_locmon_check_lattice(20, 20, 315) && !ndt_locmon_check_capacity(1, 1, 1, 1), "fine");
    auto with = [&p](auto set) { ndtgpu_locmon_params q = p; set(q); return q; };
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.max_dist = 0.0; })), "max_dist");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.max_dist = nan; })), "max_dist");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.max_dist = inf; })), "max_dist");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.r_min = -0.1; })), "r_min");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.r_min = nan; })), "r_min");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.r_min = 1.0; q.r_max = 1.0; })), "r_max");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.r_max = nan; })), "r_max");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.post_x = nan; })), "post_x");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.post_y = inf; })), "post_y");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.occupied_min = 128; })), "occupied_min");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.occupied_min = -129; })), "occupied_min");
    REFUSED(ndt_locmon_check_params(with([&](ndtgpu_locmon_params &q) { q.min_num_matches = -1; })), "min_num_matches");
    REFUSED(ndt_locmon_check_grids(0, 8, 8, 0.05, p), "n_grids");
    REFUSED(ndt_locmon_check_grids(1025, 8, 8, 0.05, p), "n_grids");
    REFUSED(ndt_locmon_check_grids(1, 0, 8, 0.05, p), "width");
    REFUSED(ndt_locmon_check_grids(1, (1 << 15) + 1, 8, 0.05, p), "width");
    REFUSED(ndt_locmon_check_grids(1, 8, 0, 0.05, p), "height");
    REFUSED(ndt_locmon_check_grids(1, 8, (1 << 15) + 1, 0.05, p), "height");
    REFUSED(ndt_locmon_check_grids(4, 1 << 15, 1 << 15, 0.05, p), "pixels");
    REFUSED(ndt_locmon_check_grids(1, 8, 8, 0.0, p), "resolution");
    REFUSED(ndt_locmon_check_grids(1, 8, 8, nan, p), "resolution");
    REFUSED(ndt_locmon_check_grids(1, 8, 8, inf, p), "resolution");
    REFUSED(ndt_locmon_check_grids(1, 8, 8, 0.5, p), "radius");
    REFUSED(ndt_locmon_check_grids(1, 8, 8, 0.001, p), "radius");
    REFUSED(ndt_locmon_check_beams(0, 0.0, 0.1), "n_beams");
    REFUSED(ndt_locmon_check_beams(8193, 0.0, 0.1), "n_beams");
    REFUSED(ndt_locmon_check_beams(8, nan, 0.1), "angle_min");
    REFUSED(ndt_locmon_check_beams(8, 0.0, inf), "angle_increment");
    REFUSED(ndt_locmon_check_counts(0, 1), "n_scans");
    REFUSED(ndt_locmon_check_counts((1 << 24) + 1, 1), "n_scans");
    REFUSED(ndt_locmon_check_counts(1, (1 << 24) + 1), "n_queries");
    REFUSED(ndt_locmon_check_lattice(0, 1, 1), "nx");
    REFUSED(ndt_locmon_check_lattice(1, 0, 1), "ny");
    REFUSED(ndt_locmon_check_lattice(1, 1, 0), "nyaw");
    REFUSED(ndt_locmon_check_lattice((1 << 24) + 1, 1, 1), "nx");
    REFUSED(ndt_locmon_check_lattice(1 << 13, 1 << 13, 1), "candidates");
    REFUSED(ndt_locmon_check_lattice(1 << 23, 2, 2), "candidates");
    {
        std::vector<double> xs = {0.1, 0.2, 0.3}, ys = {0.0, 0.1}, cs = {1.0, std::cos(0.1)}, sn = {0.0, std::sin(0.1)};
        CHECK(!ndt_lattice_check_tables(xs.data(), 3, ys.data(), 2, cs.data(), sn.data(), 2), "tables");
        xs[2] = nan;
        REFUSED(ndt_lattice_check_tables(xs.data(), 3, ys.data(), 2, cs.data(), sn.data(), 2), "xs");
        xs[2] = 0.3; ys[0] = inf;
        REFUSED(ndt_lattice_check_tables(xs.data(), 3, ys.data(), 2, cs.data(), sn.data(), 2), "ys");
        ys[0] = 0.0; cs[1] = 0.5;
        REFUSED(ndt_lattice_check_tables(xs.data(), 3, ys.data(), 2, cs.data(), sn.data(), 2), "cs / sn");
        cs[1] = std::cos(0.1); sn[0] = nan;
        REFUSED(ndt_lattice_check_tables(xs.data(), 3, ys.data(), 2, cs.data(), sn.data(), 2), "cs / sn");
    }
    REFUSED(ndt_locmon_check_capacity(0, 1, 1, 1), "max_grids");
    REFUSED(ndt_locmon_check_capacity(1025, 1, 1, 1), "max_grids");
    REFUSED(ndt_locmon_check_capacity(1, 0, 1, 1), "max_pixels");
    REFUSED(ndt_locmon_check_capacity(1, ((size_t)1 << 31) + 1, 1, 1), "max_pixels");
    REFUSED(ndt_locmon_check_capacity(1, 1, 0, 1), "max_beams");
    REFUSED(ndt_locmon_check_capacity(1, 1, 8193, 1), "max_beams");
    REFUSED(ndt_locmon_check_capacity(1, 1, 1, 0), "max_candidates");
    REFUSED(ndt_locmon_check_capacity(1, 1, 1, (1 << 24) + 1), "max_candidates");

    std::printf("locmon_checks: %d of %d bad arguments refused, %d failures\n", refused, tried, g_fails);
    return g_fails || refused != tried ? 1 : 0;
}
