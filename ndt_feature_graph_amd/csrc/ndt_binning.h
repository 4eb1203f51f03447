// ndt_binning.h -- point -> LazyGrid cell for the build kernels, and the cell finaliser (product code; host and device, so that
// tests/native/build_checks.hip can run every function here on both; scalarize() is device only).
//
// LazyGrid::getIndexForPoint (perception_oru; call sites ndt_feature_fuser_hmt.cpp:195-226) evaluates, per axis,
// floor((p - c) / res + 0.5) + size / 2.0 in fp64 and truncates to int; NDTMap::loadPointCloud drops NaN points and, with
// a range limit, points with |p - origin| > range.  fast() evaluates both in fp32 with derived error bounds and reports the
// points whose fp32 result could differ from the reference's; exact() decides those with the reference's own formulas.
// Binning is therefore bit-identical to the reference's for every point (tests/test_build_direct.py).  Domain: any grid centre and
// range origin in fp64 (init() measures what their rounding to fp32 costs and widens the guards by it; where a guard would reach a
// quarter cell, or the range band the range itself, every point takes the fp64 path), grids of up to 2^23 cells per axis, and a
// range whose square is finite in fp32.
#pragma once
#include "ndt_math.h"

struct NdtBinner {
    double cx, cy, cz, res, ox, oy, oz, range_limit;
    double hx, hy, hz;          // size / 2.0 (NdtGrid::half: scalar registers)
    int sx, sy, sz;
    float inv32, kx32, ky32, kz32, ox32, oy32, oz32, r2, r2eff, r2band, frac_lim, z_max32;

    // centre: the map's grid centre, origin: the range test's origin (the sensor; 0 without one)
    NDT_HD void init(const NdtGrid &g, double cx_, double cy_, double cz_, double ox_, double oy_, double oz_,
                    double range_limit_, float z_max32_)
    {
        cx = cx_; cy = cy_; cz = cz_; res = g.res; ox = ox_; oy = oy_; oz = oz_; range_limit = range_limit_;
        sx = g.size[0]; sy = g.size[1]; sz = g.size[2];
        z_max32 = z_max32_;
        const double inv_res = 1.0 / g.res;
        hx = g.half[0]; hy = g.half[1]; hz = g.half[2];
        inv32 = (float)inv_res;
        // fast-path constants: idx = floor(p*inv + k), k = 0.5 + size/2 - c*inv.  Only for EVEN sizes (size/2
        // integral); with an odd size the reference's double->int truncation makes the index formula
        // non-monotone, so every point takes the exact path then (force_exact).
        const bool force_exact = ((g.size[0] | g.size[1] | g.size[2]) & 1) != 0;
        const double kxd = 0.5 + hx - cx * inv_res, kyd = 0.5 + hy - cy * inv_res, kzd = 0.5 + hz - cz * inv_res;
        kx32 = (float)kxd; ky32 = (float)kyd; kz32 = (float)kzd;
        ox32 = (float)ox; oy32 = (float)oy; oz32 = (float)oz;
        r2 = (float)(range_limit * range_limit);
        r2eff = range_limit > 0 ? r2 : __builtin_inff();
        // fp32 error of dd = |p - o32|^2 against |p - o|^2 at distance r: the three differences, squares and the two sums round
        // once each, as does r2 (below 8 2^-24 r^2 together, and 1e-3 r^2 is the margin over that), and the origin moved by
        // e = |o - (float)o| (summed over the axes) on its way to fp32: 2 r e + e^2, taken twice.  For an origin of fp32 numbers
        // e is 0 and the band is 1e-3 r^2.  The sign of dd - r2 outside the band is the reference's as long as e < r / 4, which a
        // band below r^2 implies; where there is none (an origin far from an fp32 number, relative to the range), the band is
        // infinite and the fp64 test of exact() decides for every point.
        r2band = -1.0f;
        if (range_limit > 0) {
            const double e = fabs(ox - (double)ox32) + fabs(oy - (double)oy32) + fabs(oz - (double)oz32);
            r2band = 1e-3f * r2 + (float)(2.0 * (2.0 * range_limit * e + e * e));
            if (!(r2band < r2)) r2band = __builtin_inff();
        }
        // fp32 error of v = fma(p, inv32, k32) against V = (p - c)/res + 0.5 + size/2 for a point in or next to the grid
        // (|v| <= size + 1, |p/res| <= |v| + |k|):  |p/res| |inv32 res - 1| + |k32 - k| + 2^-24 |v| for the fma's rounding.  The
        // first two are measured here in fp64, not bounded by 2^-24 each (a cell size with an fp32 reciprocal and a centre on
        // the cell lattice cost nothing); 2^-50 covers the fp64 roundings of this measurement, of k and of the reference's own
        // evaluation of V.  Points whose fraction is within twice that bound of a cell face take the exact path; a
        // point further outside the grid is out of bounds on either path (error < 1 cell up to 2^23 cells, above
        // that the float -> int conversion saturates).
        const float kmax = fmaxf(fmaxf(fabsf(kx32), fabsf(ky32)), fabsf(kz32));
        const float smax = (float)max(max(g.size[0], g.size[1]), g.size[2]) + 1.0f;
        const double e_inv = fabs((double)inv32 * g.res - 1.0) + 0x1p-50;
        const double e_k = fmax(fmax(fabs((double)kx32 - kxd), fabs((double)ky32 - kyd)), fabs((double)kz32 - kzd));
        const float face_guard = (float)(2.0001 * (((double)smax + (double)kmax) * e_inv + e_k + 0x1.000002p-24 * (double)smax));
        // fast path: |frac - 0.5| <= frac_lim on every axis; odd sizes / absurd centres: exact path for every point.  (Absurd is
        // |k| of a million cells, where the bound without the measurement reaches a quarter cell: fp32 coordinates are then
        // a sixteenth of a cell apart and more, and a good share of the points lies ON faces whatever the guard.)
        frac_lim = (force_exact || !(2.4e-7f * (smax + kmax) < 0.25f)) ? -1.0f : 0.5f - face_guard;
    }

    // The fp32 constants come out of the vector ALU and would each occupy a vector register although they are the same
    // in every lane; a readfirstlane moves them to scalar registers (for kernels whose vector registers are scarce).
    NDT_D void scalarize()
    {
        float *f[] = {&inv32, &kx32, &ky32, &kz32, &ox32, &oy32, &oz32, &r2, &r2eff, &r2band, &frac_lim, &z_max32};
#pragma unroll
        for (int k = 0; k < 12; k++) *f[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(*f[k])));
    }

    // fp32 fast path of one point -> cell index.  Every test is false for a NaN (NaN points are skipped, like padding);
    // an Inf passes the range test when no range is set and is then out of the grid.  Returns true when the
    // reference's fp64 formulas must decide (exact()): the point is within the fp32 error bound of a cell face or
    // of the range sphere (frac_lim < 0 sends every point there: odd grid sizes, absurd centres).
    // (the cell index leaves as the three floats floor() made: the offset arithmetic wants them as floats again)
    NDT_HD bool fast(float fx, float fy, float fz, float &gx, float &gy, float &gz, int &slot) const
    {
        const float dx = fx - ox32, dy = fy - oy32, dz = fz - oz32;
        const float dd = dx * dx + dy * dy + dz * dz;
        const bool okz = fz <= z_max32;                                 // addPointCloud's maxz (+inf otherwise)
        const bool okr = (dd <= r2eff) & okz;                           // r2eff = +inf without a range limit
        const bool near_r = fabsf(dd - r2) < r2band;                    // r2band < 0 without a range limit
        // v = (p - c)/res + 0.5 + size/2 in one fma per axis; the integer part is the cell index
        const float vx = fmaf(fx, inv32, kx32), vy = fmaf(fy, inv32, ky32), vz = fmaf(fz, inv32, kz32);
        const float flx = floorf(vx), fly = floorf(vy), flz = floorf(vz);
        const float tx = fabsf((vx - flx) - 0.5f), ty = fabsf((vy - fly) - 0.5f), tz = fabsf((vz - flz) - 0.5f);
        const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
        gx = flx; gy = fly; gz = flz;
        const bool inb = ((unsigned)ix < (unsigned)sx) & ((unsigned)iy < (unsigned)sy) & ((unsigned)iz < (unsigned)sz);
        const int sl = (int)(((unsigned)ix * (unsigned)sy + (unsigned)iy) * (unsigned)sz + (unsigned)iz);
        slot = (okr & inb) ? sl : -1;
        return (okr | (near_r & okz)) & (near_r | !(fmaxf(fmaxf(tx, ty), tz) <= frac_lim));
    }

    // ... and the reference's own formulas for those few points
    NDT_HD void exact(float fx, float fy, float fz, float &gx, float &gy, float &gz, int &slot) const
    {
        int ix = (int)gx, iy = (int)gy, iz = (int)gz;
        const float dx = fx - ox32, dy = fy - oy32, dz = fz - oz32;
        const float dd = dx * dx + dy * dy + dz * dz;
        const bool okz = fz <= z_max32;
        bool ok = (dd <= r2eff) & okz;
        if (fabsf(dd - r2) < r2band) {
#pragma clang fp contract(off)
            double ex = (double)fx - ox, ey = (double)fy - oy, ez = (double)fz - oz;
            ok = !(sqrt(ex * ex + ey * ey + ez * ez) > range_limit) && okz;
        }
        const float vx = fmaf(fx, inv32, kx32), vy = fmaf(fy, inv32, ky32), vz = fmaf(fz, inv32, kz32);
        if (!(fabsf((vx - floorf(vx)) - 0.5f) <= frac_lim)) ix = lazygrid_index_half((double)fx, cx, res, hx);
        if (!(fabsf((vy - floorf(vy)) - 0.5f) <= frac_lim)) iy = lazygrid_index_half((double)fy, cy, res, hy);
        if (!(fabsf((vz - floorf(vz)) - 0.5f) <= frac_lim)) iz = lazygrid_index_half((double)fz, cz, res, hz);
        slot = (ok && (unsigned)ix < (unsigned)sx && (unsigned)iy < (unsigned)sy && (unsigned)iz < (unsigned)sz)
                   ? (int)(((unsigned)ix * (unsigned)sy + (unsigned)iy) * (unsigned)sz + (unsigned)iz) : -1;
        gx = (float)ix; gy = (float)iy; gz = (float)iz;           // (only cells of the grid matter: exact below 2^24)
    }
};

// rint(t) of a double |t| < 2^62 as a 64-bit integer (there is no fp64 -> int64 conversion instruction): the upper word
// by floor(t 2^-32), the lower one from the exact remainder in [0, 2^32)
NDT_HD long long ndt_fixed_from_double(double t)
{
    double hi = floor(t * (1.0 / 4294967296.0));
    double lo = rint(fma(-hi, 4294967296.0, t));            // exact remainder, rounded to an integer in [0, 2^32]
    const bool carry = lo >= 4294967296.0;
    lo = carry ? 0.0 : lo;
    const long long h = (long long)(int)hi + (carry ? 1 : 0);
    return (long long)((unsigned long long)h << 32) + (long long)(unsigned long long)(unsigned)lo;
}

// What the eigenvalues of a FIRST Gaussian [m^2] can be off by, given what the moments carry.  The covariance is
// (S2 - S1 S1^T / n) res^2 / (n - 1) with S1, S2 the sums of u and u u^T in cell units, |u| < 2 (1/2 on even grids):
//   * each of the up to n runs that were added to an accumulator rounded once to 2^-shift, so an entry of S2 is off by at most
//     n 2^-s2 / 2 and one of S1 by n 2^-s1 / 2; S1's error enters an entry through m_a dS1_b + m_b dS1_a with |m| < 2: 2 n 2^-s1;
//   * the finaliser's fp64 roundings (two int64 -> fp64 conversions, the division by n, the two products and the difference of
//     S - n m m^T) are each 2^-53 of an entry of S2 or of n m m^T, at most 4 n, and Jacobi's rotations stay below ten more
//     of them: 16 * 2^-53 * 4 n = 2^-47 n;
//   * a symmetric 3 x 3 matrix of entries <= e moves the eigenvalues by at most 3 e; res^2 / (n - 1) converts to m^2, and
//     n / (n - 1) <= 2.
// With shifts of 45 this is 4.7e-13 cell^2: a spread of about 7e-7 cell.  The same for every cell of a launch: the host computes it
// and the kernels take it as an argument (a scalar register pair; computed in the finaliser, per cell or hoisted, it is one more
// fp64 value across the Jacobi rotations, which the flat build kernel pays with spills).
static inline __host__ __device__ double ndt_first_gaussian_floor(double res, int s1_shift, int s2_shift)
{
    return 6.0 * res * res * (2.0 * ldexp(1.0, -s1_shift) + 0.5 * ldexp(1.0, -s2_shift) + 0x1p-47);
}

// "This first Gaussian is rank deficient" (NDTCell::rescaleCovariance: an eigenvalue <= 0), for eigenvalues mx >= mn that carry
// the noise above: nothing above the floor, lambda_min <= NDT_DEGENERATE_REL lambda_max, or lambda_min not above the floor (in
// exact arithmetic a cell of identical, collinear or coplanar points has lambda_min = 0; without the floor the noise of
// S - n m m^T decided for tight clusters).  True for a NaN.  The ONE place of this decision (the finaliser below and the
// first-Gaussian branch of csrc/ndt_fuse.hip).  (mn <= mx, so "nothing above the floor" needs no comparison of its own.)
NDT_HD bool ndt_first_gaussian_rank_deficient(double mx, double mn, double floor_m2)
{
    return !(mn > NDT_DEGENERATE_REL * mx && mn > floor_m2);
}

// NDTCell::computeGaussian (first Gaussian of a cell) + rescaleCovariance on the exact moments of a cell: n points,
// s1 = sum u * 2^s1_shift, s2 = sum u u^T * 2^s2_shift with u = (p - cell centre) / res.  `centre` = the cell's centre
// (c + (k - size/2) res per axis).  Returns a record with n == 0 when the cell gets no Gaussian (fewer than n_min
// points, or a rank-deficient covariance: ndt_first_gaussian_rank_deficient).  `floor_m2` = ndt_first_gaussian_floor of the launch, which the
// kernels take as an argument.
NDT_HD NdtCell ndt_gaussian_from_moments(const NdtAcc &a, unsigned slot, const double centre[3], double res, int n_min,
                                        double eval_factor, double IS1, double IS2, double floor_m2)
{
    NdtCell c;
    c.n = 0;
    c.slot = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) c.mean[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) c.cov[k] = 0;
    const unsigned long long n = (unsigned long long)a.n;
    if (n >= 2 && n >= (unsigned long long)n_min) {
        double dn = (double)n;
        double m[3];   // mean offset in cell units
#pragma unroll
        for (int k = 0; k < 3; k++) m[k] = ((double)a.s1[k] / dn) * IS1;
        double S[6];
#pragma unroll
        for (int k = 0; k < 6; k++) S[k] = (double)a.s2[k] * IS2;
        double sc = res * res / (dn - 1.0);
        double C[3][3], V[3][3];
        C[0][0] = (S[0] - dn * m[0] * m[0]) * sc;
        C[0][1] = (S[1] - dn * m[0] * m[1]) * sc;
        C[0][2] = (S[2] - dn * m[0] * m[2]) * sc;
        C[1][1] = (S[3] - dn * m[1] * m[1]) * sc;
        C[1][2] = (S[4] - dn * m[1] * m[2]) * sc;
        C[2][2] = (S[5] - dn * m[2] * m[2]) * sc;
        C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
        double E[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q2 = 0; q2 < 3; q2++) E[r][q2] = C[r][q2];
        jacobi_static<3, true>(E, V);
        double ev[3] = {E[0][0], E[1][1], E[2][2]};
        double mx = dmax3(ev[0], ev[1], ev[2]), mn = dmin3(ev[0], ev[1], ev[2]);
        // NDTCell::rescaleCovariance
        if (!ndt_first_gaussian_rank_deficient(mx, mn, floor_m2)) {
            bool recalc = false;
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (mx > ev[k] * eval_factor) { ev[k] = mx / eval_factor; recalc = true; }
            if (recalc) {
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int q2 = r; q2 < 3; q2++) {
                        double s = 0;
#pragma unroll
                        for (int k = 0; k < 3; k++) s += V[r][k] * ev[k] * V[q2][k];
                        C[r][q2] = s;
                    }
            }
            c.mean[0] = centre[0] + m[0] * res;
            c.mean[1] = centre[1] + m[1] * res;
            c.mean[2] = centre[2] + m[2] * res;
            c.cov[0] = C[0][0]; c.cov[1] = C[0][1]; c.cov[2] = C[0][2];
            c.cov[3] = C[1][1]; c.cov[4] = C[1][2]; c.cov[5] = C[2][2];
            c.n = (uint32_t)n;
            c.slot = slot;
        }
    }
    return c;
}
