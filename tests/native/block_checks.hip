// Direct checks of csrc/ndt_block.h on the device: every operation in workgroups of 256 and 1024 threads, one workgroup per
// launch, against expected values that this program computes on the host in plain C++ by restating the header's order (per
// wave v += lane ^ 32, 16, 8, 4, 2, 1, then the waves ascending from 0.0).  Comparison is by bits, never by tolerance.
// Built and run by tests/test_block.py; includes the header alone and links only the HIP runtime.  There is no CPU fallback:
// without a device it says so and exits 3.
#include "../../ndt_feature_graph_amd/csrc/ndt_block.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            printf("block_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                                         \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

static const int SUM_CALLS = 4, MAX_CALLS = 3, COUNT_CALLS = 2, RANK_CALLS = 6;

// ---- kernels: the calls of a kernel follow each other with no barrier but their own ---------------------------------------------
template <int WAVES, int N>
__global__ __launch_bounds__(WAVES * 64) void sum_kernel(const double *in, double *out)
{
    __shared__ NdtBlockSums<WAVES, N> red;
    int par = 0;
    for (int c = 0; c < SUM_CALLS; c++) {
        const size_t at = ((size_t)c * WAVES * 64 + threadIdx.x) * N;
        double v[N];
        for (int k = 0; k < N; k++) v[k] = in[at + k];
        if constexpr (N == 1) v[0] = ndt_block_sum(v[0], red, par);
        else ndt_block_sum(v, red, par);
        for (int k = 0; k < N; k++) out[at + k] = v[k];
    }
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void max_kernel(const double *in, double *out)
{
    __shared__ NdtBlockSums<WAVES, 1> red;
    int par = 0;
    for (int c = 0; c < MAX_CALLS; c++) {
        const size_t at = (size_t)c * WAVES * 64 + threadIdx.x;
        out[at] = ndt_block_max(in[at], red, par);
    }
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void count_kernel(const unsigned *in, unsigned *out)
{
    __shared__ NdtBlockCounts<WAVES> cnt;
    int par = 0;
    for (int c = 0; c < COUNT_CALLS; c++) {
        const size_t at = (size_t)c * WAVES * 64 + threadIdx.x;
        out[at] = ndt_block_count(in[at], cnt, par);
    }
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void rank_kernel(const unsigned *keep, unsigned *rank, unsigned *total)
{
    __shared__ NdtBlockCounts<WAVES> cnt;
    int par = 0;
    for (int c = 0; c < RANK_CALLS; c++) {
        const size_t at = (size_t)c * WAVES * 64 + threadIdx.x;
        rank[at] = ndt_block_rank(keep[at] != 0, cnt, par, total[at]);
    }
}

// ---- the host's restatement -----------------------------------------------------------------------------------------------------
static unsigned hash3(unsigned a, unsigned b, unsigned c)
{
    unsigned h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (c + 0x165667B1u) * 0xC2B2AE35u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

// mixed magnitude and sign: +-2^60, +-1, +-2^-40, each times a factor in [1, 2) with a full mantissa, so that sums round
static double mixed(unsigned h)
{
    const double mag[3] = {ldexp(1.0, 60), 1.0, ldexp(1.0, -40)};
    const double f = 1.0 + ldexp((double)hash3(h, 1u, 2u), -32) + ldexp((double)(hash3(h, 3u, 4u) >> 11), -53);
    const double v = mag[(h >> 9) % 3] * f;
    return (h & 256u) ? -v : v;
}

template <typename OP>
static double wave_tree(const double *x, OP op)
{
    double t[64], n[64];
    memcpy(t, x, sizeof t);
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; l++) n[l] = op(t[l], t[l ^ o]);
        memcpy(t, n, sizeof t);
    }
    return t[0];
}

static double block_sum(const double *x, int waves)       // x: one value per thread
{
    double s = 0.0;
    for (int w = 0; w < waves; w++) s += wave_tree(x + 64 * w, [](double a, double b) { return a + b; });
    return s;
}

static double block_max(const double *x, int waves)
{
    double m = 0.0;
    for (int w = 0; w < waves; w++) m = fmax(m, wave_tree(x + 64 * w, [](double a, double b) { return fmax(a, b); }));
    return m;
}

static int failures = 0;
static bool any_order_dependent = false;

static void report(const char *what, int threads, int n, int bad)
{
    printf("%-5s threads %4d N %d: %s\n", what, threads, n, bad ? "WRONG" : "ok");
    if (bad) {
        printf("  %d values differ from the host's\n", bad);
        failures++;
    }
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n;
    explicit DevBuf(size_t n_) : n(n_) { CHECK_HIP(hipMalloc((void **)&p, n * sizeof(T))); CHECK_HIP(hipMemset(p, 0xFF, n * sizeof(T))); }
    ~DevBuf() { (void)hipFree(p); }
    void put(const std::vector<T> &h) { CHECK_HIP(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> get()
    {
        std::vector<T> h(n);
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

template <int WAVES, int N>
static void check_sum()
{
    const int T = WAVES * 64;
    std::vector<double> in((size_t)SUM_CALLS * T * N);
    for (int c = 0; c < SUM_CALLS; c++)
        for (int t = 0; t < T; t++)
            for (int k = 0; k < N; k++) in[((size_t)c * T + t) * N + k] = mixed(hash3((unsigned)t, (unsigned)k, (unsigned)(c * 64 + WAVES)));
    DevBuf<double> din(in.size()), dout(in.size());
    din.put(in);
    hipLaunchKernelGGL((sum_kernel<WAVES, N>), dim3(1), dim3(T), 0, 0, din.p, dout.p);
    CHECK_HIP(hipGetLastError());
    const std::vector<double> out = dout.get();
    int bad = 0;
    std::vector<double> col(T);
    for (int c = 0; c < SUM_CALLS; c++)
        for (int k = 0; k < N; k++) {
            double plain = 0.0;
            for (int t = 0; t < T; t++) {
                col[t] = in[((size_t)c * T + t) * N + k];
                plain += col[t];
            }
            const double want = block_sum(col.data(), WAVES);
            if (memcmp(&plain, &want, sizeof want) != 0) any_order_dependent = true;
            for (int t = 0; t < T; t++)
                if (memcmp(&out[((size_t)c * T + t) * N + k], &want, sizeof want) != 0) bad++;
        }
    report("sum", T, N, bad);
}

template <int WAVES>
static void check_max()
{
    const int T = WAVES * 64;
    std::vector<double> in((size_t)MAX_CALLS * T);
    for (int t = 0; t < T; t++) {
        in[t] = (double)(hash3((unsigned)t, 1u, (unsigned)WAVES) % 100000u) / 100.0;      // the largest: the last thread's
        in[T + t] = (double)(hash3((unsigned)t, 2u, (unsigned)WAVES) % 100000u) / 100.0;  // one NaN among finite values
        in[2 * T + t] = NAN;                                                               // all NaN
    }
    in[T - 1] = 1.0e6;
    in[T + 70] = NAN;
    DevBuf<double> din(in.size()), dout(in.size());
    din.put(in);
    hipLaunchKernelGGL((max_kernel<WAVES>), dim3(1), dim3(T), 0, 0, din.p, dout.p);
    CHECK_HIP(hipGetLastError());
    const std::vector<double> out = dout.get();
    int bad = 0;
    for (int c = 0; c < MAX_CALLS; c++) {
        double want = block_max(&in[(size_t)c * T], WAVES);
        const double fixed = c == 0 ? 1.0e6 : 0.0;                       // what the restatement itself must give
        if (c != 1 && memcmp(&want, &fixed, sizeof want) != 0) bad++;
        if (c == 1 && !(want > 0.0 && want < 1000.0)) bad++;
        for (int t = 0; t < T; t++)
            if (memcmp(&out[(size_t)c * T + t], &want, sizeof want) != 0) bad++;
    }
    report("max", T, 1, bad);
}

template <int WAVES>
static void check_count()
{
    const int T = WAVES * 64;
    std::vector<unsigned> in((size_t)COUNT_CALLS * T);
    for (int c = 0; c < COUNT_CALLS; c++)
        for (int t = 0; t < T; t++) in[(size_t)c * T + t] = 300u + hash3((unsigned)t, (unsigned)c, (unsigned)WAVES) % 1000u;
    DevBuf<unsigned> din(in.size()), dout(in.size());
    din.put(in);
    hipLaunchKernelGGL((count_kernel<WAVES>), dim3(1), dim3(T), 0, 0, din.p, dout.p);
    CHECK_HIP(hipGetLastError());
    const std::vector<unsigned> out = dout.get();
    int bad = 0;
    for (int c = 0; c < COUNT_CALLS; c++) {
        unsigned want = 0;
        for (int t = 0; t < T; t++) want += in[(size_t)c * T + t];
        if (want <= 65536u) bad++;                                       // (the total is to exceed 2^16)
        for (int t = 0; t < T; t++)
            if (out[(size_t)c * T + t] != want) bad++;
    }
    report("count", T, 1, bad);
}

template <int WAVES>
static void check_rank()
{
    const int T = WAVES * 64;
    std::vector<unsigned> keep((size_t)RANK_CALLS * T);
    for (int t = 0; t < T; t++) {
        keep[t] = 0;                                                         // none
        keep[T + t] = 1;                                                     // all
        keep[2 * T + t] = t & 1;                                             // alternating
        keep[3 * T + t] = hash3((unsigned)t, 3u, (unsigned)WAVES) % 3u == 0; // a fixed pseudo-random mask
        keep[4 * T + t] = t == T - 1;                                        // only the last thread of the last wave
        keep[5 * T + t] = hash3((unsigned)t, 5u, (unsigned)WAVES) % 5u != 0; // another mask, on the half the first call used
    }
    DevBuf<unsigned> dkeep(keep.size()), drank(keep.size()), dtotal(keep.size());
    dkeep.put(keep);
    hipLaunchKernelGGL((rank_kernel<WAVES>), dim3(1), dim3(T), 0, 0, dkeep.p, drank.p, dtotal.p);
    CHECK_HIP(hipGetLastError());
    const std::vector<unsigned> rank = drank.get(), total = dtotal.get();
    int bad = 0;
    for (int c = 0; c < RANK_CALLS; c++) {
        unsigned want_total = 0;
        for (int t = 0; t < T; t++) want_total += keep[(size_t)c * T + t];
        unsigned below = 0;
        for (int t = 0; t < T; t++) {
            const size_t at = (size_t)c * T + t;
            if (total[at] != want_total) bad++;
            if (keep[at] && rank[at] != below) bad++;                    // the kept threads: 0 .. total - 1 in thread order
            below += keep[at];
        }
    }
    report("rank", T, 1, bad);
}

template <int WAVES>
static void check_all()
{
    check_sum<WAVES, 1>();
    check_sum<WAVES, 2>();
    check_sum<WAVES, 4>();
    check_sum<WAVES, 9>();
    check_max<WAVES>();
    check_count<WAVES>();
    check_rank<WAVES>();
}

int main()
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
        printf("block_checks: no HIP device, and there is no CPU fallback\n");
        return 3;
    }
    check_all<4>();
    check_all<16>();
    // unless rounding depends on the order somewhere, equal bits prove nothing about the order
    printf("order: the plain left-to-right sum %s the tree's in at least one case\n", any_order_dependent ? "differs from" : "NEVER differs from");
    if (!any_order_dependent) failures++;
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
