// Direct checks of csrc/ndt_binning.h and csrc/ndt_wave.h: the point -> cell binner, the fixed-point conversion, the cell
// finaliser and the cross-lane primitives of the build kernels, one function per case, with nothing of a build kernel around them.
//   build_checks <mode> host|gpu|gpu256     stdin: uint32 n, then n rows of IN[mode] 64-bit words;  stdout: n rows of OUT[mode] words
// A word is a double, an int64 or packed 32-bit values, as the layouts below say.  The per-case work of bin, fixed, gauss and
// lanemap is ONE host/device function: `host` calls it in a loop, `gpu` / `gpu256` call it from a kernel, one thread per row in
// workgroups of 64 / 256 threads -- both targets run the same source, and tests/test_build_direct.py (which builds and drives
// this program) holds both to the same references.  scan, xor, swapadd and moments exist on the device only: a row is a LANE,
// consecutive rows fill the waves of a workgroup, and n must be a multiple of the workgroup size (every lane active).
// Includes the two headers alone and links only the HIP runtime.  The GPU path makes one launch per run, checks every HIP call,
// and exits 2 with the error string on the first failure.
//
// Row layouts:
//   bin       in  rows 0..5: twelve doubles {res, sx, sy, sz, cx, cy, cz, ox, oy, oz, range (0: none), z_max}; rows 6..: one
//                 point {bits(x) | bits(y) << 32, bits(z)}
//             out row 0: {bits(frac_lim) | bits(r2band) << 32, 0, 0, 0}, rows 1..5 zero; a point's row: int32 x 8
//                 {slot after fast(), fast()'s return, slot after exact() where fast() asked for it (else the slot of fast()),
//                  1 when the three floats fast() / exact() leave name that slot's cell (or the slot is -1)}, then the same four
//                 with the constants moved to scalar registers by scalarize() first (host: a copy)
//   fixed     in  t (double)                                    out ndt_fixed_from_double(t) (int64)
//   gauss     in  n, s1[3], s2[6] (int64), slot (int64), centre[3], res, n_min, eval_factor, s1_shift, s2_shift (doubles)
//             out the 80 bytes of the NdtCell record
//   lanemap   in  lane (int64)                                  out ndt_moment_of_lane(lane) (int64)
//   scan      in  v (low 32 bits)                               out ndt_wave_incl_scan(v) (low 32 bits)
//   xor       in  x (any 64 bits)                               out xor_lane<1>, <2>, <4>, <8>(x)
//   swapadd   in  a, b (doubles)                                out pl_swap_add(a, b, false), pl_swap_add(a, b, true)
//   moments   in  sd[3], se[6] (doubles)                        out wave_sum_moments(sd, se, lane)
#include "../../ndt_feature_graph_amd/csrc/ndt_binning.h"
#include "../../ndt_feature_graph_amd/csrc/ndt_wave.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            fprintf(stderr, "build_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                                \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

typedef unsigned long long u64;

enum { MODE_BIN = 0, MODE_FIXED, MODE_GAUSS, MODE_LANEMAP, MODE_SCAN, MODE_XOR, MODE_SWAPADD, MODE_MOMENTS, N_MODES };
static const char *const MODE_NAME[N_MODES] = {"bin", "fixed", "gauss", "lanemap", "scan", "xor", "swapadd", "moments"};
static const int MODE_IN[N_MODES] = {2, 1, 19, 1, 1, 1, 2, 9};
static const int MODE_OUT[N_MODES] = {4, 1, 10, 1, 1, 4, 2, 1};
static const unsigned BIN_HEAD = 6;     // rows of the geometry in front of the points

NDT_HD double word_f64(u64 w) { double d; memcpy(&d, &w, 8); return d; }
NDT_HD u64 f64_word(double d) { u64 w; memcpy(&w, &d, 8); return w; }
NDT_HD float half_f32(unsigned h) { float f; memcpy(&f, &h, 4); return f; }
NDT_HD unsigned f32_half(float f) { unsigned h; memcpy(&h, &f, 4); return h; }
NDT_HD u64 pack2(int lo, int hi) { return (u64)(unsigned)lo | ((u64)(unsigned)hi << 32); }

// fast(), then exact() where it asked: what every build kernel does with a point
NDT_HD void bin_point(const NdtBinner &b, float fx, float fy, float fz, int res4[4])
{
    float gx, gy, gz;
    int slot;
    const bool need = b.fast(fx, fy, fz, gx, gy, gz, slot);
    res4[0] = slot;
    res4[1] = need ? 1 : 0;
    if (need) b.exact(fx, fy, fz, gx, gy, gz, slot);
    res4[2] = slot;
    int named = -1;
    if (gx >= 0.0f && gy >= 0.0f && gz >= 0.0f && gx < (float)b.sx && gy < (float)b.sy && gz < (float)b.sz)
        named = ((int)gx * b.sy + (int)gy) * b.sz + (int)gz;
    res4[3] = (slot < 0 || named == slot) ? 1 : 0;
}

NDT_HD void case_bin(const u64 *in, u64 *out, unsigned k)
{
    u64 *o = out + (size_t)k * 4;
    NdtGrid g;
    g.res = word_f64(in[0]);
    for (int a = 0; a < 3; a++) {
        g.size[a] = (int)word_f64(in[1 + a]);
        g.half[a] = g.size[a] / 2.0;
    }
    g.slots = g.size[0] * g.size[1] * g.size[2];
    g.max_cells = 0;
    NdtBinner b;
    b.init(g, word_f64(in[4]), word_f64(in[5]), word_f64(in[6]), word_f64(in[7]), word_f64(in[8]), word_f64(in[9]), word_f64(in[10]),
           (float)word_f64(in[11]));
    if (k < BIN_HEAD) {
        o[0] = k == 0 ? pack2((int)f32_half(b.frac_lim), (int)f32_half(b.r2band)) : 0;
        o[1] = o[2] = o[3] = 0;
        return;
    }
    const u64 w0 = in[(size_t)k * 2], w1 = in[(size_t)k * 2 + 1];
    const float fx = half_f32((unsigned)w0), fy = half_f32((unsigned)(w0 >> 32)), fz = half_f32((unsigned)w1);
    int r[4], s[4];
    bin_point(b, fx, fy, fz, r);
#if defined(__HIP_DEVICE_COMPILE__)
    NdtBinner sb = b;
    sb.scalarize();
    bin_point(sb, fx, fy, fz, s);
#else
    for (int a = 0; a < 4; a++) s[a] = r[a];
#endif
    o[0] = pack2(r[0], r[1]); o[1] = pack2(r[2], r[3]);
    o[2] = pack2(s[0], s[1]); o[3] = pack2(s[2], s[3]);
}

NDT_HD void case_fixed(const u64 *in, u64 *out, unsigned k) { out[k] = (u64)ndt_fixed_from_double(word_f64(in[k])); }

NDT_HD void case_gauss(const u64 *in, u64 *out, unsigned k)
{
    const u64 *w = in + (size_t)k * 19;
    NdtAcc a;
    a.n = (long long)w[0];
    for (int i = 0; i < 3; i++) a.s1[i] = (long long)w[1 + i];
    for (int i = 0; i < 6; i++) a.s2[i] = (long long)w[4 + i];
    const double centre[3] = {word_f64(w[11]), word_f64(w[12]), word_f64(w[13])};
    const int s1_shift = (int)word_f64(w[17]), s2_shift = (int)word_f64(w[18]);
    // (the floor as the launchers hand it to the kernels: from the cell size and the shifts)
    const NdtCell c = ndt_gaussian_from_moments(a, (unsigned)w[10], centre, word_f64(w[14]), (int)word_f64(w[15]), word_f64(w[16]),
                                                ldexp(1.0, -s1_shift), ldexp(1.0, -s2_shift),
                                                ndt_first_gaussian_floor(word_f64(w[14]), s1_shift, s2_shift));
    u64 *o = out + (size_t)k * 10;
    for (int i = 0; i < 3; i++) o[i] = f64_word(c.mean[i]);
    for (int i = 0; i < 6; i++) o[3 + i] = f64_word(c.cov[i]);
    o[9] = (u64)c.n | ((u64)c.slot << 32);
}

NDT_HD void case_lanemap(const u64 *in, u64 *out, unsigned k) { out[k] = (u64)(long long)ndt_moment_of_lane((unsigned)in[k]); }

template <int MODE>
NDT_HD void run_case(const u64 *in, u64 *out, unsigned k)
{
    if constexpr (MODE == MODE_BIN) case_bin(in, out, k);
    else if constexpr (MODE == MODE_FIXED) case_fixed(in, out, k);
    else if constexpr (MODE == MODE_GAUSS) case_gauss(in, out, k);
    else case_lanemap(in, out, k);
}

// the wave modes: every lane of the wave is active (n is a multiple of the workgroup size)
template <int MODE>
__device__ void run_lane(const u64 *in, u64 *out, unsigned k)
{
    if constexpr (MODE == MODE_SCAN) {
        out[k] = (u64)ndt_wave_incl_scan((unsigned)in[k]);
    } else if constexpr (MODE == MODE_XOR) {
        const double x = word_f64(in[k]);
        u64 *o = out + (size_t)k * 4;
        o[0] = f64_word(xor_lane<1>(x)); o[1] = f64_word(xor_lane<2>(x)); o[2] = f64_word(xor_lane<4>(x)); o[3] = f64_word(xor_lane<8>(x));
    } else if constexpr (MODE == MODE_SWAPADD) {
        const double a = word_f64(in[(size_t)k * 2]), b = word_f64(in[(size_t)k * 2 + 1]);
        out[(size_t)k * 2] = f64_word(pl_swap_add(a, b, false));
        out[(size_t)k * 2 + 1] = f64_word(pl_swap_add(a, b, true));
    } else {
        const u64 *w = in + (size_t)k * 9;
        const double sd[3] = {word_f64(w[0]), word_f64(w[1]), word_f64(w[2])};
        const double se[6] = {word_f64(w[3]), word_f64(w[4]), word_f64(w[5]), word_f64(w[6]), word_f64(w[7]), word_f64(w[8])};
        out[k] = f64_word(wave_sum_moments(sd, se, threadIdx.x & 63u));
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void cases_kernel(const u64 *in, u64 *out, unsigned n)
{
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if constexpr (MODE >= MODE_SCAN) run_lane<MODE>(in, out, k);
    else run_case<MODE>(in, out, k);
}

template <int MODE>
static void run_host(const std::vector<u64> &in, std::vector<u64> &out, unsigned n)
{
    if constexpr (MODE >= MODE_SCAN) {
        fprintf(stderr, "build_checks: %s exists on the device only\n", MODE_NAME[MODE]);
        exit(64);
    } else {
        for (unsigned k = 0; k < n; k++) run_case<MODE>(in.data(), out.data(), k);
    }
}

template <int MODE>
static void run_gpu(const std::vector<u64> &in, std::vector<u64> &out, unsigned n, unsigned wg)
{
    int n_dev = 0;
    CHECK_HIP(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) {
        fprintf(stderr, "build_checks: no HIP device\n");
        exit(3);
    }
    if (MODE >= MODE_SCAN && n % wg != 0) {
        fprintf(stderr, "build_checks: %s takes a multiple of %u rows (every lane active)\n", MODE_NAME[MODE], wg);
        exit(65);
    }
    u64 *din = nullptr, *dout = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, in.size() * sizeof(u64)));
    CHECK_HIP(hipMalloc((void **)&dout, out.size() * sizeof(u64)));
    CHECK_HIP(hipMemcpy(din, in.data(), in.size() * sizeof(u64), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out.size() * sizeof(u64)));              // (NaN / -1 wherever a case writes nothing)
    hipLaunchKernelGGL((cases_kernel<MODE>), dim3((n + wg - 1u) / wg), dim3(wg), 0, 0, din, dout, n);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(u64), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
}

template <int MODE>
static void run_mode(unsigned wg, const std::vector<u64> &in, std::vector<u64> &out, unsigned n)
{
    if (wg) run_gpu<MODE>(in, out, n, wg);
    else run_host<MODE>(in, out, n);
}

int main(int argc, char **argv)
{
    int mode = -1;
    for (int m = 0; m < N_MODES; m++)
        if (argc > 1 && strcmp(argv[1], MODE_NAME[m]) == 0) mode = m;
    unsigned wg = 0;
    bool target_ok = false;
    if (argc == 3) {
        target_ok = true;
        if (strcmp(argv[2], "gpu") == 0) wg = 64;
        else if (strcmp(argv[2], "gpu256") == 0) wg = 256;
        else target_ok = strcmp(argv[2], "host") == 0;
    }
    if (mode < 0 || !target_ok) {
        fprintf(stderr, "usage: build_checks bin|fixed|gauss|lanemap|scan|xor|swapadd|moments host|gpu|gpu256 < rows > results\n");
        return 64;
    }
    unsigned n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > (1u << 22) || (mode == MODE_BIN && n <= BIN_HEAD)) {
        fprintf(stderr, "build_checks: no row count on stdin (1 .. 2^22; bin: the geometry and at least one point)\n");
        return 65;
    }
    std::vector<u64> in((size_t)n * MODE_IN[mode]), out((size_t)n * MODE_OUT[mode]);
    if (fread(in.data(), sizeof(u64), in.size(), stdin) != in.size()) {
        fprintf(stderr, "build_checks: %s takes %d words per row, the table is short\n", MODE_NAME[mode], MODE_IN[mode]);
        return 65;
    }
    switch (mode) {
    case MODE_BIN: run_mode<MODE_BIN>(wg, in, out, n); break;
    case MODE_FIXED: run_mode<MODE_FIXED>(wg, in, out, n); break;
    case MODE_GAUSS: run_mode<MODE_GAUSS>(wg, in, out, n); break;
    case MODE_LANEMAP: run_mode<MODE_LANEMAP>(wg, in, out, n); break;
    case MODE_SCAN: run_mode<MODE_SCAN>(wg, in, out, n); break;
    case MODE_XOR: run_mode<MODE_XOR>(wg, in, out, n); break;
    case MODE_SWAPADD: run_mode<MODE_SWAPADD>(wg, in, out, n); break;
    default: run_mode<MODE_MOMENTS>(wg, in, out, n); break;
    }
    if (fwrite(out.data(), sizeof(u64), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}
