// ndt_lattice.h -- the lattice tables of a brute-force search, as the extrinsic calibration (csrc/ndt_calib.h) and the localisation
// monitor's adjustPose (csrc/ndt_locmon.h) take them: xs [nx], ys [ny] and the cosine and sine cs, sn [nyaw] of the yaws; candidate
// (ix * ny + iy) * nyaw + iyaw is (xs[ix], ys[iy], cs[iyaw], sn[iyaw]) -- the kernels decode the index.  Host only, plain C++:
// tests/native/calib_checks.cpp and locmon_checks.cpp compile this file with g++ alone (under the address and undefined-behaviour
// sanitizers).  The upload of the tables is LatticeTables in csrc/ndtgpu_host.h.
#pragma once
#include <cmath>
#include <cstddef>

// NULL: fine, else the message (it names the argument): finite, and c * c + s * s within 1e-6 of 1
inline const char *ndt_lattice_check_tables(const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn, size_t nyaw)
{
    for (size_t k = 0; k < nx; k++)
        if (!(std::fabs(xs[k]) < 1e150)) return "xs must be finite";
    for (size_t k = 0; k < ny; k++)
        if (!(std::fabs(ys[k]) < 1e150)) return "ys must be finite";
    for (size_t k = 0; k < nyaw; k++)
        if (!(std::fabs(cs[k] * cs[k] + sn[k] * sn[k] - 1.0) < 1e-6)) return "cs / sn must be the cosine and sine of an angle";
    return nullptr;
}
