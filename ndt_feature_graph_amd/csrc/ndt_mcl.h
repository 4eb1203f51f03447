// ndt_mcl.h -- what the NDT Monte Carlo localisation kernels (csrc/ndt_mcl.hip) and its C-ABI (csrc/ndtgpu_mcl.hip) share:
// the per-filter records, the counter-based random numbers and the Euler-angle helpers, one definition each for host and
// device.  tests/mcl_model.py restates every function of this file in NumPy.
#pragma once
#include "ndt_math.h"
#include "ndt_pose.h"   // ndt_euler012: Eigen's eulerAngles(0, 1, 2), one definition for the fuser and the filters

#define NDT_MCL_THREADS 256         // likelihood / predict workgroups: one particle per lane
#define NDT_MCL_NORM_THREADS 1024   // normalise / SIR / mean: one workgroup per filter
#define NDT_MCL_STAGE 256           // scan cells staged in LDS at a time
#define NDT_MCL_MAX_CHUNKS 16       // a filter's scan cells are scored in at most this many chunks (fixed per handle)
#define NDT_MCL_FX_SHIFT 52         // cumulative weights in units of 2^-52: exact integer sums (sum of weights ~ 1 < 2^11)

// the draws of one filter update (ndtgpu_mcl_* draw index d, see ndt_mcl_stream)
enum { NDT_MCL_DRAW_POSE = 0, NDT_MCL_DRAW_SUBSAMPLE = 6, NDT_MCL_DRAW_SIR = 7 };

// what the host derives from Tmotion for one filter (updateAndPredictEff, step 3)
struct NdtMclMotion {
    double tr[3];         // Tmotion.translation()
    double rot[3];        // Tmotion.rotation().eulerAngles(0, 1, 2)
    double sigma[6];      // motion_model * (|tr|, |rot|) + motion_model_offset
};

// per filter, device resident
struct NdtMclState {
    unsigned long long draws;   // initialize + update calls so far: the counter of the random-number keys
    unsigned long long terms;   // (particle, scan cell) terms scored by the last update (atomic integer sum)
    double var_p, lik_sum;
    int since_sir, resampled;
    int n_scan_cells, overflow;
};

struct NdtMclParamsDev {
    double zfilt_min, subsample_level, sir_varp_threshold;
    int force_sir, sir_max_iters_wo_resampling;
    unsigned long long seed;
};

// ---- counter-based random numbers: synth.hash_uniform / hash_normal (SplitMix64 + Box-Muller) ----------------------------
NDT_HD unsigned long long ndt_splitmix(unsigned long long x)
{
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// U[0,1) from (seed, stream, idx): synth.hash_uniform
NDT_HD double ndt_hash_uniform(unsigned long long seed, unsigned long long stream, unsigned long long idx)
{
    const unsigned long long key = ndt_splitmix(seed * 1000003ull + stream);
    const unsigned long long z = ndt_splitmix(key ^ (idx * 0x9E3779B97F4A7C15ull));
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
// N(0,1): synth.hash_normal (streams `stream` and `stream + 1`)
NDT_HD double ndt_hash_normal(unsigned long long seed, unsigned long long stream, unsigned long long idx)
{
#pragma clang fp contract(off)
    double u1 = ndt_hash_uniform(seed, stream, idx);
    if (u1 < 1e-300) u1 = 1e-300;
    const double u2 = ndt_hash_uniform(seed, stream + 1, idx);
    return sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793 * u2);
}
// the stream of draw d of filter slot f at its draw counter c: a filter's numbers depend on (seed, f, c, d, idx) alone
NDT_HD unsigned long long ndt_mcl_stream(unsigned long long f, unsigned long long c, int d)
{
    return (((f << 32) | (c & 0xFFFFFFFFull)) << 4) | (unsigned long long)(2 * d);
}

// ---- rotations -------------------------------------------------------------------------------------------------------------
// Translation(t) * AngleAxis(a, X) * AngleAxis(b, Y) * AngleAxis(c, Z), closed form
NDT_HD void ndt_mcl_xyz_rigid(double tx, double ty, double tz, double a, double b, double c, rigid &T)
{
#pragma clang fp contract(off)
    const double sa = sin(a), ca = cos(a), sb = sin(b), cb = cos(b), sc = sin(c), cc = cos(c);
    T.r[0] = cb * cc;                   T.r[1] = -(cb * sc);                T.r[2] = sb;
    T.r[3] = ca * sc + sa * sb * cc;    T.r[4] = ca * cc - sa * sb * sc;    T.r[5] = -(sa * cb);
    T.r[6] = sa * sc - ca * sb * cc;    T.r[7] = sa * cc + ca * sb * sc;    T.r[8] = ca * cb;
    T.t[0] = tx; T.t[1] = ty; T.t[2] = tz;
}

// updateAndPredictEff step 3: tr, rot = eulerAngles(0,1,2), sigma = motion_model (row-major 6x6) * |(tr, rot)| + offset
NDT_HD void ndt_mcl_motion(const double *T16, const double *mm36, const double *off6, NdtMclMotion &o)
{
#pragma clang fp contract(off)
    o.tr[0] = T16[12]; o.tr[1] = T16[13]; o.tr[2] = T16[14];
    ndt_euler012(T16, o.rot);
    const double incr[6] = {fabs(o.tr[0]), fabs(o.tr[1]), fabs(o.tr[2]), fabs(o.rot[0]), fabs(o.rot[1]), fabs(o.rot[2])};
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
        for (int j = 0; j < 6; j++) s = s + mm36[i * 6 + j] * incr[j];
        o.sigma[i] = s + off6[i];
    }
}

// column-major 4x4 <-> rigid
NDT_HD void ndt_rigid_from16(const double *T16, rigid &T)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T.r[i * 3 + j] = T16[j * 4 + i];
        T.t[i] = T16[12 + i];
    }
}
NDT_HD void ndt_rigid_to16(const rigid &T, double *T16)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T16[j * 4 + i] = T.r[i * 3 + j];
        T16[12 + i] = T.t[i];
        T16[i * 4 + 3] = 0.0;
    }
    T16[15] = 1.0;
}

// host launchers (csrc/ndt_mcl.hip).  pose12_dev: per filter of the range {pose6, sigma6}; motion_dev, state, T, w, lik,
// partial, cum: indexed by filter slot
hipError_t ndt_mcl_launch_init(size_t first, size_t count, unsigned n_particles, const double *pose12_dev, unsigned long long seed,
                               NdtMclState *state, rigid *T, double *w, hipStream_t st);
hipError_t ndt_mcl_launch_predict(size_t first, size_t count, unsigned n_particles, const NdtMclMotion *motion_dev,
                                  unsigned long long seed, NdtMclState *state, rigid *T, hipStream_t st);
hipError_t ndt_mcl_launch_likelihood(const NdtSetView &map, const uint32_t *map_idx_dev, const NdtSetView &scan, size_t first,
                                     size_t count, unsigned n_particles, unsigned chunk, unsigned n_chunks, const NdtMclParamsDev &prm,
                                     NdtMclState *state, const rigid *T, double *partial, hipStream_t st);
hipError_t ndt_mcl_launch_normalise(size_t first, size_t count, unsigned n_particles, unsigned chunk, unsigned n_chunks,
                                    const NdtMclParamsDev &prm, const NdtSetView &scan, NdtMclState *state, rigid *T, rigid *T_tmp,
                                    double *w, double *lik, const double *partial, long long *cum, hipStream_t st);
hipError_t ndt_mcl_launch_mean(size_t first, size_t count, unsigned n_particles, const rigid *T, const double *w, double *mean16_dev,
                               hipStream_t st);
