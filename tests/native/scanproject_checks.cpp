// scanproject_checks.cpp -- a stand-alone host program (no HIP, no device) over what csrc/ndt_scanproject.h shares with host code:
// the checks of a projection's arguments and parameters, the tile arithmetic of the launches, the gate and the point of a beam.
// The kernels' walk over a scan is replayed on the host with that arithmetic -- count per tile, first row from the counts in
// front, rows, pads -- into heap blocks of exactly the size a call may touch, so the address sanitizer sees any step past an end
// (build it with -fsanitize=address,undefined to check that).  Exit code 0 = every check passed.
#include "../../ndt_feature_graph_amd/csrc/ndt_scanproject.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

static ndtgpu_scanproject_params defaults()
{
    ndtgpu_scanproject_params p;
    std::memset(&p, 0, sizeof p);
    p.r_min = 0.5; p.r_max = 30.0; p.varz = 0.02; p.seed = 0;
    return p;
}

// the two launches of csrc/ndt_scanproject.hip for one scan, tile by tile, on the host: rows of `words` 4-byte words
static uint32_t replay(const std::vector<double> &r, const ndtgpu_scanproject_params &p, size_t words, std::vector<uint32_t> &out,
                       std::vector<uint32_t> &written)
{
    const size_t n_beams = r.size();
    const uint32_t n_tiles = ndt_scanproject_tiles(n_beams);
    std::vector<uint32_t> tile(n_tiles);                      // exactly the scratch of one scan
    for (uint32_t t = 0; t < n_tiles; t++) {
        uint32_t b, e, c = 0;
        ndt_scanproject_tile_range(t, n_beams, b, e);
        for (uint32_t i = b; i < e; i++) c += ndt_scanproject_kept(r[i], p.r_min, p.r_max) ? 1u : 0u;
        tile[t] = c;
    }
    uint32_t n_kept = 0;
    for (uint32_t t = 0; t < n_tiles; t++) n_kept += tile[t];
    for (uint32_t t = 0; t < n_tiles; t++) {
        uint32_t at = 0, b, e;
        for (uint32_t k = 0; k < t; k++) at += tile[k];
        ndt_scanproject_tile_range(t, n_beams, b, e);
        for (uint32_t i = b; i < e; i++) {
            if (!ndt_scanproject_kept(r[i], p.r_min, p.r_max)) continue;
            float xyz[3];
            ndt_scanproject_point(-1.0, 0.001, i, r[i], p.varz, 0.25, xyz);
            std::memcpy(&out[(size_t)at * words], xyz, sizeof xyz);
            written[at]++;
            at++;
        }
        uint32_t pb, pe;
        ndt_scanproject_pad_range(t, n_beams, n_kept, pb, pe);
        for (uint32_t k = pb; k < pe; k++) {
            for (size_t c = 0; c < 3; c++) out[(size_t)k * words + c] = 0x7FC00000u;
            written[k]++;
        }
    }
    return n_kept;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const size_t T = NDT_SCANPROJECT_TILE;
    // arguments
    CHECK(!ndt_scanproject_check_args(0, 1, 0.0, 0.1, 12, 12) && !ndt_scanproject_check_args(1u << 24, 1u << 20, -3.0, 1e-3, 16, (size_t)16 << 20) &&
          !ndt_scanproject_check_args(3, 7, 0.0, 0.0, 32, 7 * 32 + 4), "good arguments");
    CHECK(ndt_scanproject_check_args(1, 0, 0.0, 0.1, 12, 12) && ndt_scanproject_check_args(1, (1u << 20) + 1, 0.0, 0.1, 12, (size_t)13 << 20), "n_beams");
    CHECK(ndt_scanproject_check_args((1u << 24) + 1, 16, 0.0, 0.1, 12, 192), "n_scans");
    CHECK(ndt_scanproject_check_args(1, 16, nan, 0.1, 12, 192) && ndt_scanproject_check_args(1, 16, 0.0, inf, 12, 192) &&
          ndt_scanproject_check_args(1, 16, -inf, 0.1, 12, 192), "angles");
    CHECK(ndt_scanproject_check_args(1, 16, 0.0, 0.1, 8, 192) && ndt_scanproject_check_args(1, 16, 0.0, 0.1, 14, 16 * 14) &&
          ndt_scanproject_check_args(1, 16, 0.0, 0.1, 0, 192) && ndt_scanproject_check_args(1, 16, 0.0, 0.1, ~(size_t)3, ~(size_t)3), "stride_bytes");
    CHECK(ndt_scanproject_check_args(1, 16, 0.0, 0.1, 12, 188) && ndt_scanproject_check_args(1, 16, 0.0, 0.1, 12, 194) &&
          ndt_scanproject_check_args(1, 16, 0.0, 0.1, 16, 192), "map_stride_bytes");
    // parameters
    CHECK(!ndt_scanproject_check_params(defaults()), "the defaults");
    int refused = 0, cases = 0;
#define BAD(field, value)                                  \
    do {                                                   \
        ndtgpu_scanproject_params p = defaults();          \
        p.field = (value);                                 \
        cases++;                                           \
        refused += ndt_scanproject_check_params(p) ? 1 : 0; \
        CHECK(ndt_scanproject_check_params(p), #field " = " #value " must be refused"); \
    } while (0)
    BAD(r_min, -0.1); BAD(r_min, nan); BAD(r_min, inf); BAD(r_min, 30.0); BAD(r_min, 31.0);
    BAD(r_max, 0.5); BAD(r_max, 0.0); BAD(r_max, nan); BAD(r_max, -inf);
    BAD(varz, -1e-9); BAD(varz, nan); BAD(varz, inf);
    {
        ndtgpu_scanproject_params p = defaults();
        p.r_min = 0.0; p.r_max = inf; p.varz = 0.0; p.seed = ~0ull;
        CHECK(!ndt_scanproject_check_params(p), "the limits themselves pass");
        const NdtScanProjectParamsDev d = ndt_scanproject_params_dev(p);
        CHECK(d.r_min == 0.0 && d.r_max == inf && d.varz == 0.0 && d.seed == ~0ull, "device form");
    }
    CHECK(!ndt_scanproject_check_capacity(1, 1) && !ndt_scanproject_check_capacity(1u << 24, 1u << 20) && ndt_scanproject_check_capacity(0, 1) &&
          ndt_scanproject_check_capacity(1, 0) && ndt_scanproject_check_capacity((1u << 24) + 1, 1) && ndt_scanproject_check_capacity(1, (1u << 20) + 1),
          "capacity");

    // the gate
    const ndtgpu_scanproject_params dp = defaults();
    CHECK(!ndt_scanproject_kept(0.5, dp.r_min, dp.r_max) && ndt_scanproject_kept(std::nextafter(0.5, 1.0), dp.r_min, dp.r_max) &&
          !ndt_scanproject_kept(30.0, dp.r_min, dp.r_max) && ndt_scanproject_kept(std::nextafter(30.0, 0.0), dp.r_min, dp.r_max) &&
          !ndt_scanproject_kept(nan, dp.r_min, dp.r_max) && !ndt_scanproject_kept(inf, dp.r_min, dp.r_max) &&
          !ndt_scanproject_kept(-inf, dp.r_min, dp.r_max) && !ndt_scanproject_kept(0.0, dp.r_min, dp.r_max) &&
          !ndt_scanproject_kept(-3.0, dp.r_min, dp.r_max), "the gate is strict and drops what is not finite");
    CHECK(ndt_scanproject_kept(1e300, 0.5, inf) && !ndt_scanproject_kept(inf, 0.5, inf) && !ndt_scanproject_kept(nan, 0.5, inf), "no upper gate");
    {
        float xyz[3];
        ndt_scanproject_point(0.25, 0.5, 3, 2.0, 0.02, 0.5, xyz);
        CHECK(xyz[0] == (float)(2.0 * std::cos(1.75)) && xyz[1] == (float)(2.0 * std::sin(1.75)) && xyz[2] == (float)0.01, "the point");
    }

    // the tile arithmetic: tiles, their ranges, the pads' shares
    size_t shapes = 0;
    for (size_t n_beams : {(size_t)1, T - 1, T, T + 1, 2 * T + 1, (size_t)1 << 20}) {
        const uint32_t n_tiles = ndt_scanproject_tiles(n_beams);
        CHECK(n_tiles == (n_beams + T - 1) / T && n_tiles >= 1, "%zu beams: %u tiles", n_beams, n_tiles);
        CHECK(ndt_scanproject_scans_per_launch(n_beams) * n_tiles <= NDT_SCANPROJECT_MAX_GRID && ndt_scanproject_scans_per_launch(n_beams) >= 1,
              "%zu beams: scans of a launch", n_beams);
        uint32_t next = 0;
        for (uint32_t t = 0; t < n_tiles; t++) {
            uint32_t b, e;
            ndt_scanproject_tile_range(t, n_beams, b, e);
            CHECK(b == next && e > b && e - b <= T && e <= n_beams, "%zu beams: tile %u is [%u, %u)", n_beams, t, b, e);
            next = e;
        }
        CHECK(next == n_beams, "%zu beams: the tiles cover %u beams", n_beams, next);
        for (uint32_t n_kept : {0u, 1u, (uint32_t)(n_beams / 2), (uint32_t)(n_beams - 1), (uint32_t)n_beams}) {
            uint32_t at = n_kept;
            for (uint32_t t = 0; t < n_tiles; t++) {
                uint32_t b, e;
                ndt_scanproject_pad_range(t, n_beams, n_kept, b, e);
                CHECK(b <= e && e <= n_beams, "%zu beams, %u kept: pads of tile %u are [%u, %u)", n_beams, n_kept, t, b, e);
                if (b < e) {
                    CHECK(b == at, "%zu beams, %u kept: pads of tile %u start at %u, not %u", n_beams, n_kept, t, b, at);
                    at = e;
                }
            }
            CHECK(at == n_beams, "%zu beams, %u kept: the pads end at %u", n_beams, n_kept, at);
        }
        // the walk of the two launches, for three kinds of scan and rows of 3, 4 and 8 words: every row written exactly once
        for (int kind = 0; kind < 3; kind++) {
            for (size_t words : {(size_t)3, (size_t)4, (size_t)8}) {
                if (n_beams == ((size_t)1 << 20) && words != 3) continue;
                std::vector<double> r(n_beams);
                for (size_t i = 0; i < n_beams; i++)
                    r[i] = kind == 0 ? 2.0 : kind == 1 ? (i % 3 == 0 ? nan : i % 5 == 0 ? 31.0 : 1.0 + 1e-3 * (double)(i % 1000))
                                                        : (i + 1 == n_beams ? 4.0 : 0.1);
                std::vector<uint32_t> out(n_beams * words, 0xABABABABu), written(n_beams, 0);
                const uint32_t n_kept = replay(r, dp, words, out, written);
                size_t want = 0, once = 0, pads = 0;
                for (size_t i = 0; i < n_beams; i++) {
                    want += ndt_scanproject_kept(r[i], dp.r_min, dp.r_max) ? 1 : 0;
                    once += written[i] == 1 ? 1 : 0;
                    pads += out[i * words] == 0x7FC00000u ? 1 : 0;
                }
                CHECK(n_kept == want && once == n_beams && pads == n_beams - want, "%zu beams, kind %d, %zu words: %u kept, %zu rows written once, %zu pads",
                      n_beams, kind, words, n_kept, once, pads);
                shapes++;
            }
        }
    }
    std::printf("scanproject_checks: %d of %d bad parameters refused, %zu scans walked, %d failures\n", refused, cases, shapes, g_fails);
    return g_fails ? 1 : 0;
}
