// featextract_checks.cpp -- a stand-alone host program (no HIP, no device) over what csrc/ndt_featextract.h shares with host code:
// the checks of ndtgpu_featbank_extract's arguments and parameters, the device form of the parameters, the LDS size of a
// workgroup and the unpacking of a bank's transposed descriptors that ndtgpu_featbank_get uses.  Every array is a heap block of
// exactly the size the functions may touch, so the address sanitizer sees any step past an end (build it with
// -fsanitize=address,undefined to check that).  Exit code 0 = every check passed.
#include "../../ndt_feature_graph_amd/csrc/ndt_featextract.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_fails = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL (%s:%d): ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); g_fails++; } \
    } while (0)

static ndtgpu_featextract_params defaults()
{
    ndtgpu_featextract_params p;
    std::memset(&p, 0, sizeof p);
    p.scales = 5; p.base_sigma = 0.2; p.sigma_step = 1.4; p.dmst = 2.0; p.min_value = 0.34; p.min_diff = 0.001;
    p.min_rho = 0.02; p.max_rho = 1.0; p.bin_rho = 4; p.bin_phi = 12; p.min_separation = 0.2; p.r_min = 0.5; p.r_max = 30.0;
    return p;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // arguments
    CHECK(!ndt_featextract_check_args(0, 1, 0.0, 0.1) && !ndt_featextract_check_args(1u << 24, 2048, -3.0, 1e-3), "good arguments");
    CHECK(ndt_featextract_check_args(1, 0, 0.0, 0.1) && ndt_featextract_check_args(1, 2049, 0.0, 0.1), "n_beams");
    CHECK(ndt_featextract_check_args((1u << 24) + 1, 16, 0.0, 0.1), "n_scans");
    CHECK(ndt_featextract_check_args(1, 16, nan, 0.1) && ndt_featextract_check_args(1, 16, 0.0, inf) &&
          ndt_featextract_check_args(1, 16, -inf, 0.1), "angles");
    // parameters: the defaults pass, every field out of its range fails
    CHECK(!ndt_featextract_check_params(defaults()), "the defaults");
    int refused = 0, cases = 0;
#define BAD(field, value)                                  \
    do {                                                   \
        ndtgpu_featextract_params p = defaults();          \
        p.field = (value);                                 \
        cases++;                                           \
        refused += ndt_featextract_check_params(p) ? 1 : 0; \
        CHECK(ndt_featextract_check_params(p), #field " = " #value " must be refused"); \
    } while (0)
    BAD(scales, 0); BAD(scales, 9); BAD(scales, -1);
    BAD(base_sigma, 0.0); BAD(base_sigma, nan); BAD(base_sigma, inf);
    BAD(sigma_step, 1.0); BAD(sigma_step, nan); BAD(sigma_step, inf);
    BAD(dmst, 0.0); BAD(dmst, -1.0); BAD(dmst, nan);
    BAD(min_rho, -0.1); BAD(min_rho, 1.0); BAD(min_rho, nan); BAD(max_rho, inf); BAD(max_rho, nan); BAD(max_rho, 0.01);
    BAD(bin_rho, 0); BAD(bin_phi, 0); BAD(bin_rho, 6); BAD(bin_phi, 17); BAD(bin_rho, 65536); BAD(bin_phi, -3);
    BAD(r_min, -1.0); BAD(r_min, 30.0); BAD(r_min, nan); BAD(r_max, inf); BAD(r_max, nan);
    BAD(min_value, nan); BAD(min_value, inf); BAD(min_diff, nan); BAD(min_diff, -inf);
    BAD(min_separation, nan); BAD(min_separation, -0.1); BAD(min_separation, inf);
    {
        ndtgpu_featextract_params p = defaults();
        p.bin_rho = 8; p.bin_phi = 8; p.scales = 8; p.min_rho = 0.0; p.r_min = 0.0; p.min_separation = 0.0; p.min_value = -1.0;
        CHECK(!ndt_featextract_check_params(p), "the limits themselves pass");
        const NdtFeatExtractParamsDev d = ndt_featextract_params_dev(p);
        CHECK(d.scales == 8 && d.sigma[0] == 0.2 && d.sigma[7] > d.sigma[6] && d.drho == 0.125 && d.delta == 0.0625, "device form");
    }
    const NdtFeatExtractParamsDev d = ndt_featextract_params_dev(defaults());
    CHECK(d.sigma[1] == 0.2 * 1.4 && d.sigma[2] == (0.2 * 1.4) * 1.4 && d.sigma[5] == 0.0 && d.drho == (1.0 - 0.02) / 4.0 &&
          d.delta == d.drho / 2.0 && d.bin_rho * d.bin_phi == 48, "device form of the defaults");
    CHECK(ndt_featextract_lds_bytes(2048) == 2560 + 2048 * 48 && ndt_featextract_lds_bytes(1) == 2560 + 8 * 48 &&
          ndt_featextract_lds_bytes(721) == 2560 + 728 * 48, "LDS bytes");

    // the unpacking: sets of every fill of banks of several shapes, packed as ndtgpu_featbank_set packs them
    size_t sets = 0;
    const size_t shapes[][2] = {{1, 1}, {4, 48}, {7, 5}, {33, 48}, {64, 64}, {1024, 3}};
    for (const auto &shape : shapes) {
        const size_t MP = shape[0], D = shape[1];
        for (size_t n : {(size_t)0, (size_t)1, MP / 2, MP}) {
            if (n > MP) continue;
            std::vector<double> desc(n * D), packed(D * MP, -1.0), out(n * D, -2.0);
            for (size_t i = 0; i < n; i++)
                for (size_t k = 0; k < D; k++) desc[i * D + k] = (double)(i * 1000 + k) + 0.5;
            for (size_t k = 0; k < D; k++)
                for (size_t i = 0; i < n; i++) packed[k * MP + i] = desc[i * D + k];
            ndt_featextract_unpack_desc(packed.data(), n, D, MP, out.data());
            CHECK(out == desc, "unpack of %zu points of a %zu x %zu bank", n, MP, D);
            sets++;
        }
    }
    std::printf("featextract_checks: %d of %d bad parameters refused, %zu sets unpacked, %d failures\n", refused, cases, sets, g_fails);
    return g_fails ? 1 : 0;
}
