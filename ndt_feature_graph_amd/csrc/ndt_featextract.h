// ndt_featextract.h -- what the laser-scan feature extraction's kernel (csrc/ndt_featextract.hip) and its C-ABI
// (csrc/ndtgpu_featextract.hip) share: the device form of the parameters, the checks of a call's arguments and the unpacking of a
// bank's transposed descriptors.  The checks and the unpacking need include/ndtgpu.h alone, so a host program can call them
// (tests/native/featextract_checks.cpp does, under the address and undefined-behaviour sanitizers); the launcher is declared for
// HIP translation units only.  tests/flirt_model.py restates the algorithm (include/ndtgpu.h "laser-scan feature extraction",
// steps 1-8) in NumPy.
#pragma once
#include "../../include/ndtgpu.h"

#include <cmath>
#include <cstddef>

#define NDT_FEATEXTRACT_THREADS 256               // one workgroup per scan
#define NDT_FEATEXTRACT_WAVES (NDT_FEATEXTRACT_THREADS / 64)
#define NDT_FEATEXTRACT_MAX_BEAMS 2048            // beams per thread <= 8; the per-point LDS arrays: 48 B a beam
#define NDT_FEATEXTRACT_MAX_SCALES 8
#define NDT_FEATEXTRACT_MAX_BINS 64               // the bins a beam's samples visit are one 64-bit mask
#define NDT_FEATEXTRACT_POINT_BYTES 48            // LDS per beam (FxLayout in csrc/ndt_featextract.hip)
#define NDT_FEATEXTRACT_FIXED_BYTES 2560          // ... and per workgroup (FxFixed), rounded up

struct NdtFeatExtractParamsDev {
    double sigma[NDT_FEATEXTRACT_MAX_SCALES];     // sigma_s, by repeated multiplication
    double dmst, min_value, min_diff, min_rho, max_rho, drho, dphi, delta, min_separation, r_min, r_max;
    int scales, bin_rho, bin_phi;
};

// what ndtgpu_featbank_extract / _extract_device check before the handle is read and the device is looked for; NULL: fine, else
// the message
inline const char *ndt_featextract_check_args(size_t n_scans, size_t n_beams, double angle_min, double angle_increment)
{
    if (n_scans > (1u << 24)) return "more than 2^24 scans";
    if (n_beams == 0 || n_beams > NDT_FEATEXTRACT_MAX_BEAMS) return "n_beams must be 1 .. 2048";
    if (!(std::fabs(angle_min) < 1e300) || !(std::fabs(angle_increment) < 1e300)) return "angle_min and angle_increment must be finite";
    return nullptr;
}
inline const char *ndt_featextract_check_params(const ndtgpu_featextract_params &p)
{
    if (p.scales < 1 || p.scales > NDT_FEATEXTRACT_MAX_SCALES) return "scales must be 1 .. 8";
    if (!(p.base_sigma > 0.0 && p.base_sigma < 1e300)) return "base_sigma must be finite and > 0";
    if (!(p.sigma_step > 1.0 && p.sigma_step < 1e300)) return "sigma_step must be finite and > 1";
    if (!(p.dmst > 0.0 && p.dmst < 1e300)) return "dmst must be finite and > 0";
    if (!(p.min_rho >= 0.0 && p.min_rho < p.max_rho && p.max_rho < 1e300)) return "0 <= min_rho < max_rho (finite) is required";
    if (p.bin_rho < 1 || p.bin_phi < 1 || p.bin_rho > NDT_FEATEXTRACT_MAX_BINS || p.bin_phi > NDT_FEATEXTRACT_MAX_BINS ||
        p.bin_rho * p.bin_phi > NDT_FEATEXTRACT_MAX_BINS)
        return "bin_rho * bin_phi must be 1 .. 64";
    if (!(p.r_min >= 0.0 && p.r_min < p.r_max && p.r_max < 1e300)) return "0 <= r_min < r_max (finite) is required";
    if (!(std::fabs(p.min_value) < 1e300) || !(std::fabs(p.min_diff) < 1e300) || !(p.min_separation >= 0.0 && p.min_separation < 1e300))
        return "min_value, min_diff and min_separation (>= 0) must be finite";                             // (NaN fails)
    return nullptr;
}

// the device form of checked parameters
inline NdtFeatExtractParamsDev ndt_featextract_params_dev(const ndtgpu_featextract_params &p)
{
    NdtFeatExtractParamsDev d{};
    double s = p.base_sigma;
    for (int k = 0; k < p.scales; k++) {
        d.sigma[k] = s;
        s = s * p.sigma_step;
    }
    d.dmst = p.dmst;
    d.min_value = p.min_value;
    d.min_diff = p.min_diff;
    d.min_rho = p.min_rho;
    d.max_rho = p.max_rho;
    d.drho = (p.max_rho - p.min_rho) / (double)p.bin_rho;
    d.dphi = 2.0 * 3.14159265358979323846 / (double)p.bin_phi;
    d.delta = d.drho / 2.0;
    d.min_separation = p.min_separation;
    d.r_min = p.r_min;
    d.r_max = p.r_max;
    d.scales = p.scales;
    d.bin_rho = p.bin_rho;
    d.bin_phi = p.bin_phi;
    return d;
}

// dynamic LDS of a workgroup for scans of n_beams beams
inline size_t ndt_featextract_lds_bytes(size_t n_beams)
{
    return NDT_FEATEXTRACT_FIXED_BYTES + ((n_beams + 7) & ~(size_t)7) * NDT_FEATEXTRACT_POINT_BYTES;
}

// host-side unpacking of one set from the bank's layout: packed ([desc_len][max_points], bin k of point i at k * max_points + i)
// -> out (n x desc_len row-major); the inverse of ndt_featmatch_pack_desc
inline void ndt_featextract_unpack_desc(const double *packed, size_t n, size_t desc_len, size_t max_points, double *out)
{
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < desc_len; k++) out[i * desc_len + k] = packed[k * max_points + i];
}

#if defined(__HIPCC__)
#include "ndt_featmatch.h"   // NdtFeatBankView
// host launcher (csrc/ndt_featextract.hip): n_scans workgroups of one launch.  Scan b (ranges_dev + b * n_beams) fills set
// set_idx_dev[b] of the bank, whose arrays are written through `count`, `pos` and `desc`.  beam / level / response
// ([n_scans][max_points]) may be NULL.
hipError_t ndt_featextract_launch(const NdtFeatBankView &v, uint32_t *count, double *pos, double *desc, const uint32_t *set_idx_dev,
                                  const double *ranges_dev, size_t n_scans, size_t n_beams, double angle_min, double angle_increment,
                                  const NdtFeatExtractParamsDev &prm, ndtgpu_featextract_result *results_dev, uint32_t *beam_dev,
                                  int32_t *level_dev, double *response_dev, hipStream_t st);
#endif
