// Direct checks of csrc/ndt_pairterm.h: the matcher's pair term, its exponential and its reciprocal, one case per thread, with
// nothing of the matcher around them.
//   pairterm_checks <mode>      stdin: uint32 n, then n rows of IN[mode] doubles;  stdout: n rows of OUT[mode] doubles
// The functions are device-only, so there is no host target: tests/test_gpu_pairterm.py builds this program and runs it on
// the device.  Includes the header alone and links only the HIP runtime.  Checks every HIP call and exits 2 with the error
// string on the first failure.
//
// Row layouts (symmetric matrices as xx xy xz yy yz zz):
//   term  in  m (3) C (6) mu (3) Cj (6) lfd1 lfd2
//         out the 28 accumulators (score, gradient, upper triangle of the Hessian), started from +0, of
//             pair_term<false, false>, pair_term<true, false>, pair_term<false, true>, pair_term<true, true>  -- 4 x 28;
//             every instance is a kernel of its own, so that none shares subexpressions with another
//   exp   in  x     out exp_nonpos(x)
//   rcp   in  x     out rcp_nr(x)
#include "../../ndt_feature_graph_amd/csrc/ndt_pairterm.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            fprintf(stderr, "pairterm_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                             \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

enum { MODE_TERM = 0, MODE_EXP = 1, MODE_RCP = 2, N_MODES = 3 };
static const char *const MODE_NAME[N_MODES] = {"term", "exp", "rcp"};
static const int MODE_IN[N_MODES] = {20, 1, 1};
static const int MODE_OUT[N_MODES] = {4 * 28, 1, 1};

template <bool WITH_H, bool PLANAR>
__global__ __launch_bounds__(64) void term_kernel(const double *in, double *out, unsigned n, int slot)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    const double *c = in + (size_t)k * 20;
    double acc[28];
    for (int a = 0; a < 28; a++) acc[a] = 0.0;
    pair_term<WITH_H, PLANAR>(d3{c[0], c[1], c[2]}, sym3{c[3], c[4], c[5], c[6], c[7], c[8]}, d3{c[9], c[10], c[11]},
                              sym3{c[12], c[13], c[14], c[15], c[16], c[17]}, c[18], c[19], acc);
    double *o = out + (size_t)k * (4 * 28) + slot * 28;
    for (int a = 0; a < 28; a++) o[a] = acc[a];
}

template <int MODE>
__global__ __launch_bounds__(64) void scalar_kernel(const double *in, double *out, unsigned n)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    out[k] = MODE == MODE_EXP ? exp_nonpos(in[k]) : rcp_nr(in[k]);
}

int main(int argc, char **argv)
{
    int mode = -1;
    for (int m = 0; m < N_MODES; m++)
        if (argc > 1 && strcmp(argv[1], MODE_NAME[m]) == 0) mode = m;
    if (mode < 0 || argc != 2) {
        fprintf(stderr, "usage: pairterm_checks term|exp|rcp < cases > results\n");
        return 64;
    }
    unsigned n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > (1u << 20)) {
        fprintf(stderr, "pairterm_checks: no case count on stdin (1 .. 2^20)\n");
        return 65;
    }
    std::vector<double> in((size_t)n * MODE_IN[mode]), out((size_t)n * MODE_OUT[mode]);
    if (fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) {
        fprintf(stderr, "pairterm_checks: %s takes %d doubles per case, the table is short\n", MODE_NAME[mode], MODE_IN[mode]);
        return 65;
    }
    int n_dev = 0;
    CHECK_HIP(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) {
        fprintf(stderr, "pairterm_checks: no HIP device\n");
        return 3;
    }
    double *din = nullptr, *dout = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, in.size() * sizeof(double)));
    CHECK_HIP(hipMalloc((void **)&dout, out.size() * sizeof(double)));
    CHECK_HIP(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out.size() * sizeof(double)));          // (NaN wherever a case writes nothing)
    const dim3 grid((n + 63u) / 64u), block(64);
    if (mode == MODE_TERM) {
        hipLaunchKernelGGL((term_kernel<false, false>), grid, block, 0, 0, din, dout, n, 0);
        CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL((term_kernel<true, false>), grid, block, 0, 0, din, dout, n, 1);
        CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL((term_kernel<false, true>), grid, block, 0, 0, din, dout, n, 2);
        CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL((term_kernel<true, true>), grid, block, 0, 0, din, dout, n, 3);
    } else if (mode == MODE_EXP) {
        hipLaunchKernelGGL((scalar_kernel<MODE_EXP>), grid, block, 0, 0, din, dout, n);
    } else {
        hipLaunchKernelGGL((scalar_kernel<MODE_RCP>), grid, block, 0, 0, din, dout, n);
    }
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}
