// ndt_multires.hip -- the device side of ndtgpu_register_multires_device (csrc/ndtgpu_multires.hip): what sits between the
// levels of a coarse-to-fine registration, NDTMatcherD2D(irregular, useDefaultGridResolutions, resolutions)
// .match(target_pc, source_pc, T, useInitialGuess) (perception_oru's ndt_matcher_d2d.cpp; call sites
// ndt_feature/src/ndt_odom_debug.cpp:159-165, ndt_feature_pcl_eval.cpp:620-642).  The builds and the matcher are the
// library's own kernels; the source build of a level moves the cloud on load (ndt_build_flat_kernel<SD, true>, or
// ndt_cloud_transform_kernel followed by the general build).
//
// One thread per registration, 4x4 products in the order of csrc/ndt_pose.h (no fused multiply-adds): a pose that went
// through the device is the pose the host composition computes.
#include "ndt_pose.h"
#include "ndt_common.h"

// the raw source scans, range-filtered around their own origin (NDTMap::loadPointCloud's test in fp64: what the build
// kernels decide for a range limit, csrc/ndt_binning.h), packed: a point beyond the range becomes NaN, which every build drops
__global__ __launch_bounds__(256) void ndt_multires_range_kernel(const char *__restrict__ in, size_t n_points, size_t stride,
                                                                  size_t map_stride, double range_limit, float *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t k = blockIdx.y;
    const char *src = in + k * map_stride;
    float *dst = out + k * n_points * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_points; i += (size_t)gridDim.x * blockDim.x) {
        const float *p = reinterpret_cast<const float *>(src + i * stride);
        float x = p[0], y = p[1], z = p[2];
        const double ex = (double)x, ey = (double)y, ez = (double)z;
        if (sqrt(ex * ex + ey * ey + ez * ez) > range_limit) x = y = z = __builtin_nanf("");
        dst[i * 3 + 0] = x;
        dst[i * 3 + 1] = y;
        dst[i * 3 + 2] = z;
    }
}

// Per registration k, with the matcher's result of the level at list position `level` in res_lvl[k]:
//   step < 0 (before the first level): Tinit = use_initial_guess ? T16[k] : I, the first source build moves by Tinit, T = I.
//   else: a registration that ran adds its increment (Tacc = Temp * Tacc); one that did not (a map over max_cells: -3; a grid
//   barrier that gave up: -4) stops: its finer levels are not run (their source index is out of range for the matcher) and
//   report the code of the level that stopped it.  The next build moves by Temp, Temp goes back to I.  After the last level
//   T16[k] = Tacc * Tinit.
// st: per registration {Tacc[16], Tinit[16]}; stopped: per registration 0, or the exit code that stopped it.
__global__ __launch_bounds__(64) void ndt_multires_step_kernel(unsigned count, int step, int level, int n_levels, int last,
                                                                int use_initial_guess, double *__restrict__ T16,
                                                                double *__restrict__ Temp16, double *__restrict__ X16,
                                                                double *__restrict__ st, int *__restrict__ stopped,
                                                                uint32_t *__restrict__ sidx,
                                                                const NdtMatchResultDev *__restrict__ res_lvl,
                                                                NdtMatchResultDev *__restrict__ results)
{
#pragma clang fp contract(off)
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    double *Tacc = st + 32 * (size_t)k, *Tinit = Tacc + 16, *Temp = Temp16 + 16 * (size_t)k, *X = X16 + 16 * (size_t)k;
    if (step < 0) {
        for (int q = 0; q < 16; q++) {
            const double id = (q % 5 == 0) ? 1.0 : 0.0;
            Tinit[q] = use_initial_guess ? T16[16 * (size_t)k + q] : id;
            X[q] = Tinit[q];
            Tacc[q] = id;
            Temp[q] = id;
        }
        stopped[k] = 0;
        sidx[k] = k;
        return;
    }
    NdtMatchResultDev r = res_lvl[k];
    if (stopped[k]) {
        r.converged = 0; r.iterations = 0; r.fevals = 0; r.exit_code = stopped[k];
        r.score = 0.0; r.n_source = 0; r.n_target = 0;
        r.cycles_eval = 0; r.cycles_solver = 0; r.pair_terms_g = 0; r.pair_terms_h = 0;
    } else if (r.exit_code < 0) {
        stopped[k] = r.exit_code;                        // (the matcher left Temp at I)
    } else {
        double C[16];
        ndt_pose_mul(Temp, Tacc, C);
        for (int q = 0; q < 16; q++) Tacc[q] = C[q];
    }
    results[(size_t)k * n_levels + level] = r;
    for (int q = 0; q < 16; q++) {
        X[q] = Temp[q];
        Temp[q] = (q % 5 == 0) ? 1.0 : 0.0;
    }
    sidx[k] = stopped[k] ? 0xFFFFFFFFu : k;
    if (last) ndt_pose_mul(Tacc, Tinit, T16 + 16 * (size_t)k);
}

hipError_t ndt_launch_multires_range(const void *xyz_dev, size_t count, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                     double range_limit, float *out_dev, hipStream_t stream)
{
    if (!count || !n_points) return hipSuccess;
    const unsigned bx = (unsigned)std::min<size_t>((n_points + 1023) / 1024, 64);
    hipLaunchKernelGGL(ndt_multires_range_kernel, dim3(bx, (unsigned)count), dim3(256), 0, stream, (const char *)xyz_dev, n_points,
                       stride_bytes, map_stride_bytes, range_limit, out_dev);
    return hipGetLastError();
}

hipError_t ndt_launch_multires_step(size_t count, int step, int level, int n_levels, int last, int use_initial_guess, double *T16_dev,
                                    double *Temp16_dev, double *X16_dev, double *state_dev, int *stopped_dev, uint32_t *sidx_dev,
                                    const NdtMatchResultDev *res_lvl_dev, NdtMatchResultDev *results_dev, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(ndt_multires_step_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, stream, (unsigned)count, step, level,
                       n_levels, last, use_initial_guess, T16_dev, Temp16_dev, X16_dev, state_dev, stopped_dev, sidx_dev, res_lvl_dev,
                       results_dev);
    return hipGetLastError();
}
