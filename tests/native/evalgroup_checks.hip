// Direct checks of csrc/ndt_evalgroup.h: the matcher's cell index, wave scan, wave sums and eval_group itself (transform, PROBE,
// hit list, list reuse, pair terms, segment rows) with nothing of the matcher around them.
//   evalgroup_checks <mode>     stdin: uint32 n, then a table of doubles;  stdout: rows of doubles
// The functions are device-only, so there is no host target: tests/test_gpu_evalgroup.py builds this program and runs it on
// the device.  Includes the header alone and links only the HIP runtime.  One launch per run.  Checks every HIP call and exits 2
// with the error string on the first failure.
//
// -DEG_NN=n (0..3) chooses the n_neighbours whose instances of eval_group the program holds (one program per n keeps every
// compile short).  Instance number = FORM * 4 + WITH_H * 2 + (0: QL = 64, 1: the library's QL of that form):
//   FORM 0  <NN, H, QL, false, false>          persistent / stream matcher      library QL 1024
//   FORM 1  <NN, H, QL, false, false, true>    the same, planar pair term       library QL 640
//   FORM 2  <NN, H, QL, false, true>           eval_derivs                      library QL 2048
//   FORM 3  <NN, H, QL, true, true>            eval_chunks (segment rows)       library QL 2048
// eg_compiled() below says which of them a program holds.
//
// Modes index, scan, totals, terms, terms_g: n rows.
//   index   in  p centre res half                out lazygrid_index_h, lazygrid_index_p2 with pow2_reciprocal(res), pow2_reciprocal(res)
//   scan    in  v (a row is a lane, n % 64 == 0)  out wave_incl_scan_u32(v)
//   totals  in  32 values (a row is a lane)       out wave_sum_all<8> of the first 8, wave_sum_all<32> of all, as the lane holds them
//   terms   in  m (3) C (6) mu (3) Cj (6) lfd1 lfd2   out the 28 sums of pair_term<true, false>, started from +0
//   terms_g the same                                  out the 28 sums of pair_term<false, false> (the Hessian's stay +0)
// Mode group: n doubles follow.  [0] = number of cases, then per case
//   sx sy sz cx cy cz res n_occ n_src n_calls seg_lanes
//   n_occ x { slot, mean (3), cov (6) }   strictly increasing slots: the target map's cells in rank order
//   n_src x { mean (3), cov (6) }         the source cells
//   n_calls (<= 4) x { R (9, row-major) t (3) cache_key base stride end lfd1 lfd2 instance marker }
// A case is one workgroup of one wave whose LDS (tile, windows, list, cells, HitCache) lives through its calls.  marker >= 0:
// before the call, list[0] = marker and HitCache::count = 1.  The accumulators, w.terms and the segment rows are zeroed before
// every call.  Per call one row of EG_OUTW doubles (NaN where nothing was written):
//   [0, 576) tile, 9 columns of 64      [576, 768) mycell, 3 rows of 64      [768, 772) HitCache key base count pad
//   [772] w.terms      [773, 801) wave_totals      [801, 1057) 8 segment rows of 32      [1057, 1057 + min(count, QL)) the list
// The rank bitmap is built as ndt_common.h lays it out; its padding word, and the .y of every word whose .x is 0, hold poison:
// all bits set in .x, and in .y a rank beyond the map that points into 64 guard records of NaNs behind the cells.
#include "../../ndt_feature_graph_amd/csrc/ndt_evalgroup.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef EG_NN
#define EG_NN 2
#endif

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            fprintf(stderr, "evalgroup_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                            \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

enum { MODE_INDEX = 0, MODE_SCAN, MODE_TOTALS, MODE_TERMS, MODE_TERMS_G, MODE_GROUP, N_MODES };
static const char *const MODE_NAME[N_MODES] = {"index", "scan", "totals", "terms", "terms_g", "group"};
static const int MODE_IN[N_MODES] = {4, 1, 32, 20, 20, 0};
static const int MODE_OUT[N_MODES] = {3, 1, 2, 28, 28, 0};

enum { EG_TILE = 0, EG_CELL = 576, EG_CACHE = 768, EG_TERMS = 772, EG_TOT = 773, EG_ROWS = 801, EG_LIST = 1057, EG_QMAX = 2048,
       EG_OUTW = EG_LIST + EG_QMAX, EG_GUARD = 64, EG_MAX_CALLS = 4 };

static constexpr int eg_lib_ql(int form) { return form == 0 ? 1024 : form == 1 ? 640 : 2048; }
static constexpr bool eg_compiled(int nn, int form, bool h)
{
    (void)h;
    return nn >= 0 && nn <= 3 && form >= 0 && form <= 3;      // all of them: the library dispatches every form for n = 0..3
}

struct CaseDev {
    unsigned long long rank_off, cell_off, src_off, call_off;
    int n_cells, sx, sy, sz, n_calls;
    unsigned seg_lanes;
    double cx, cy, cz, res;
};
struct CallDev {
    rigid T;
    double lfd1, lfd2;
    unsigned key;
    int base, stride, end, inst;
    long long marker;
};

struct GroupLds {
    double tile[9 * 64];
    double rows[8 * 32];
    uint2 win[7 * 64];
    uint32_t list[EG_QMAX];
    int cell[3 * 64];
    HitCache cache;
};

template <int FORM, bool WITH_H, int QL>
NDT_D void run_instance(GroupLds &L, const MapView &tg, gcell_ptr src, const CallDev &c, unsigned seg_lanes, double *o)
{
    if constexpr (eg_compiled(EG_NN, FORM, WITH_H)) {
        constexpr int NACC = WaveEval<WITH_H>::NACC, SH = WITH_H ? 1 : 3;
        const unsigned lane = threadIdx.x & 63u;
        WaveEval<WITH_H> w;
        w.mysrc = L.tile; w.mywin = L.win; w.myq = L.list; w.mycell = L.cell; w.cache = &L.cache;
        w.terms = 0;
#pragma unroll
        for (int k = 0; k < NACC; k++) w.acc[k] = 0.0;
        if constexpr (FORM == 3) eval_group<EG_NN, WITH_H, QL, true, true>(w, tg, src, c.base, c.stride, c.end, c.T, c.lfd1, c.lfd2, c.key, seg_lanes, L.rows, 32u);
        else if constexpr (FORM == 2) eval_group<EG_NN, WITH_H, QL, false, true>(w, tg, src, c.base, c.stride, c.end, c.T, c.lfd1, c.lfd2, c.key);
        else if constexpr (FORM == 1) eval_group<EG_NN, WITH_H, QL, false, false, true>(w, tg, src, c.base, c.stride, c.end, c.T, c.lfd1, c.lfd2, c.key);
        else eval_group<EG_NN, WITH_H, QL, false, false>(w, tg, src, c.base, c.stride, c.end, c.T, c.lfd1, c.lfd2, c.key);
        const double tot = wave_totals<WITH_H>(w);
        if ((lane & ((1u << SH) - 1u)) == 0u && (lane >> SH) < (unsigned)NACC) o[EG_TOT + (lane >> SH)] = tot;
        if (lane == 0) o[EG_TERMS] = (double)w.terms;
        ndt_wave_sync();
        const unsigned n = min(L.cache.count, (unsigned)QL);
        for (unsigned k = lane; k < n; k += 64u) o[EG_LIST + k] = (double)L.list[k];
    }
}

template <int FORM>
NDT_D void run_form(GroupLds &L, const MapView &tg, gcell_ptr src, const CallDev &c, unsigned seg_lanes, double *o)
{
    switch (c.inst & 3) {
    case 0: run_instance<FORM, false, 64>(L, tg, src, c, seg_lanes, o); break;
    case 1: run_instance<FORM, false, eg_lib_ql(FORM)>(L, tg, src, c, seg_lanes, o); break;
    case 2: run_instance<FORM, true, 64>(L, tg, src, c, seg_lanes, o); break;
    default: run_instance<FORM, true, eg_lib_ql(FORM)>(L, tg, src, c, seg_lanes, o); break;
    }
}

__global__ __launch_bounds__(64) void group_kernel(const CaseDev *cases, const unsigned long long *ranks, const NdtCell *cells,
                                                   const NdtCell *srcs, const CallDev *calls, double *out)
{
    __shared__ GroupLds L;
    const unsigned lane = threadIdx.x & 63u;
    const CaseDev cs = cases[blockIdx.x];
    for (int k = 0; k < 9; k++) L.tile[k * 64 + lane] = __builtin_nan("");
    for (int k = 0; k < 7; k++) L.win[k * 64 + lane] = make_uint2(0u, 0u);
    for (int k = 0; k < EG_QMAX / 64; k++) L.list[k * 64 + lane] = 0u;
    for (int k = 0; k < 3; k++) L.cell[k * 64 + lane] = (int)0x80000000u;
    if (lane == 0) { L.cache.key = 0u; L.cache.base = 0; L.cache.count = 0u; L.cache.pad = 0u; }
    MapView tg;
    tg.rankmap = (grank_ptr)(ranks + cs.rank_off);
    tg.cells = (gcell_ptr)(cells + cs.cell_off);
    tg.n_cells = cs.n_cells;
    tg.sx = cs.sx; tg.sy = cs.sy; tg.sz = cs.sz;
    tg.cx = cs.cx; tg.cy = cs.cy; tg.cz = cs.cz; tg.res = cs.res;
    tg.hx = cs.sx / 2.0; tg.hy = cs.sy / 2.0; tg.hz = cs.sz / 2.0;
    tg.inv_res = pow2_reciprocal(cs.res);
    const gcell_ptr src = (gcell_ptr)(srcs + cs.src_off);
    ndt_wave_sync();
    for (int k = 0; k < cs.n_calls; k++) {
        const CallDev c = calls[cs.call_off + k];
        double *o = out + (cs.call_off + k) * (size_t)EG_OUTW;
        for (int r = 0; r < 4; r++) L.rows[r * 64 + lane] = 0.0;
        if (c.marker >= 0 && lane == 0) { L.list[0] = (uint32_t)c.marker; L.cache.count = 1u; }
        ndt_wave_sync();
        switch (c.inst >> 2) {
        case 0: run_form<0>(L, tg, src, c, cs.seg_lanes, o); break;
        case 1: run_form<1>(L, tg, src, c, cs.seg_lanes, o); break;
        case 2: run_form<2>(L, tg, src, c, cs.seg_lanes, o); break;
        default: run_form<3>(L, tg, src, c, cs.seg_lanes, o); break;
        }
        ndt_wave_sync();
        for (int q = 0; q < 9; q++) o[EG_TILE + q * 64 + lane] = L.tile[q * 64 + lane];
        for (int q = 0; q < 3; q++) o[EG_CELL + q * 64 + lane] = (double)L.cell[q * 64 + lane];
        for (int r = 0; r < 4; r++) o[EG_ROWS + r * 64 + lane] = L.rows[r * 64 + lane];
        if (lane == 0) {
            o[EG_CACHE + 0] = (double)L.cache.key; o[EG_CACHE + 1] = (double)L.cache.base;
            o[EG_CACHE + 2] = (double)L.cache.count; o[EG_CACHE + 3] = (double)L.cache.pad;
        }
        ndt_wave_sync();
    }
}

__global__ __launch_bounds__(64) void index_kernel(const double *in, double *out, unsigned n)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    const double *c = in + (size_t)k * 4;
    const double inv = pow2_reciprocal(c[2]);
    out[k * 3 + 0] = (double)lazygrid_index_h(c[0], c[1], c[2], c[3]);
    out[k * 3 + 1] = (double)lazygrid_index_p2(c[0], c[1], inv, c[3]);
    out[k * 3 + 2] = inv;
}

__global__ __launch_bounds__(64) void scan_kernel(const double *in, double *out)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    out[k] = (double)wave_incl_scan_u32((unsigned)in[k]);
}

__global__ __launch_bounds__(64) void totals_kernel(const double *in, double *out)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    double a[8], b[32];
    for (int q = 0; q < 8; q++) a[q] = in[(size_t)k * 32 + q];
    for (int q = 0; q < 32; q++) b[q] = in[(size_t)k * 32 + q];
    out[k * 2 + 0] = wave_sum_all<8>(a);
    out[k * 2 + 1] = wave_sum_all<32>(b);
}

template <bool WITH_H>
__global__ __launch_bounds__(64) void terms_kernel(const double *in, double *out, unsigned n)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    const double *c = in + (size_t)k * 20;
    double acc[28];
    for (int a = 0; a < 28; a++) acc[a] = 0.0;
    pair_term<WITH_H, false>(d3{c[0], c[1], c[2]}, sym3{c[3], c[4], c[5], c[6], c[7], c[8]}, d3{c[9], c[10], c[11]},
                             sym3{c[12], c[13], c[14], c[15], c[16], c[17]}, c[18], c[19], acc);
    double *o = out + (size_t)k * 28;
    for (int a = 0; a < 28; a++) o[a] = acc[a];
}

static void bad_input(const char *what)
{
    fprintf(stderr, "evalgroup_checks: group table: %s\n", what);
    exit(65);
}

static int run_group(const std::vector<double> &in)
{
    size_t p = 0;
    auto next = [&]() -> double { if (p >= in.size()) bad_input("the table is short"); return in[p++]; };
    auto next_int = [&](double lo, double hi, const char *what) -> long long {
        const double v = next();
        if (!(v >= lo && v <= hi) || v != std::floor(v)) bad_input(what);
        return (long long)v;
    };
    const int n_cases = (int)next_int(1, 4096, "number of cases (1 .. 4096)");
    std::vector<CaseDev> cases;
    std::vector<unsigned long long> ranks;
    std::vector<NdtCell> cells, srcs;
    std::vector<CallDev> calls;
    NdtCell guard;
    memset(&guard, 0, sizeof guard);
    for (int k = 0; k < 3; k++) guard.mean[k] = NAN;
    for (int k = 0; k < 6; k++) guard.cov[k] = NAN;
    for (int ci = 0; ci < n_cases; ci++) {
        CaseDev cs;
        memset(&cs, 0, sizeof cs);
        cs.sx = (int)next_int(1, 4096, "sx"); cs.sy = (int)next_int(1, 4096, "sy"); cs.sz = (int)next_int(1, 4096, "sz");
        cs.cx = next(); cs.cy = next(); cs.cz = next(); cs.res = next();
        const long long slots = (long long)cs.sx * cs.sy * cs.sz;
        if (slots > (1 << 16)) bad_input("more than 2^16 slots");
        const int n_occ = (int)next_int(0, (double)slots, "n_occ"), n_src = (int)next_int(1, 4096, "n_src");
        cs.n_calls = (int)next_int(1, EG_MAX_CALLS, "n_calls (1 .. 4)");
        cs.seg_lanes = (unsigned)next_int(8, 64, "seg_lanes");
        if (cs.seg_lanes & (cs.seg_lanes - 1u)) bad_input("seg_lanes is 8, 16, 32 or 64");
        cs.n_cells = n_occ;
        cs.rank_off = ranks.size(); cs.cell_off = cells.size(); cs.src_off = srcs.size(); cs.call_off = calls.size();
        const size_t words = (size_t)((slots + 31) / 32) + 1;         // ndt_rm_stride
        const unsigned poison = (unsigned)n_occ + 1u;
        std::vector<unsigned> bits(words, 0u), first(words, poison);
        long long last = -1;
        for (int k = 0; k < n_occ; k++) {
            const long long slot = next_int(0, (double)(slots - 1), "slot");
            if (slot <= last) bad_input("slots must increase");
            last = slot;
            if (bits[slot >> 5] == 0u) first[slot >> 5] = (unsigned)k;
            bits[slot >> 5] |= 1u << (slot & 31);
            NdtCell c;
            memset(&c, 0, sizeof c);
            for (int q = 0; q < 3; q++) c.mean[q] = next();
            for (int q = 0; q < 6; q++) c.cov[q] = next();
            c.n = 3; c.slot = (uint32_t)slot;
            cells.push_back(c);
        }
        bits[words - 1] = 0xFFFFFFFFu;                               // the padding word: its content never matters
        for (size_t wd = 0; wd < words; wd++) ranks.push_back((unsigned long long)first[wd] << 32 | bits[wd]);
        for (int k = 0; k < EG_GUARD; k++) cells.push_back(guard);
        for (int k = 0; k < n_src; k++) {
            NdtCell c;
            memset(&c, 0, sizeof c);
            for (int q = 0; q < 3; q++) c.mean[q] = next();
            for (int q = 0; q < 6; q++) c.cov[q] = next();
            c.n = 3;
            srcs.push_back(c);
        }
        for (int k = 0; k < cs.n_calls; k++) {
            CallDev c;
            memset(&c, 0, sizeof c);
            for (int q = 0; q < 9; q++) c.T.r[q] = next();
            for (int q = 0; q < 3; q++) c.T.t[q] = next();
            c.key = (unsigned)next_int(0, 4294967295.0, "cache_key");
            c.base = (int)next_int(0, n_src, "base");
            c.stride = (int)next_int(1, 64, "stride");
            c.end = (int)next_int(0, n_src, "end (<= n_src)");
            c.lfd1 = next(); c.lfd2 = next();
            c.inst = (int)next_int(0, 15, "instance");
            if (!eg_compiled(EG_NN, c.inst >> 2, (c.inst & 2) != 0)) bad_input("this program does not hold that instance");
            c.marker = next_int(-1, 4294967295.0, "marker");
            if (c.marker >= 0 && ((c.marker & 0xFFFFFF) >= n_occ + EG_GUARD || (c.marker >> 24) >= 64)) bad_input("marker names no cell");
            calls.push_back(c);
        }
        cases.push_back(cs);
    }
    if (p != in.size()) bad_input("doubles left over");
    CaseDev *dcases = nullptr;
    unsigned long long *dranks = nullptr;
    NdtCell *dcells = nullptr, *dsrcs = nullptr;
    CallDev *dcalls = nullptr;
    double *dout = nullptr;
    const size_t out_n = calls.size() * (size_t)EG_OUTW;
    CHECK_HIP(hipMalloc((void **)&dcases, cases.size() * sizeof(CaseDev)));
    CHECK_HIP(hipMalloc((void **)&dranks, ranks.size() * sizeof(unsigned long long)));
    CHECK_HIP(hipMalloc((void **)&dcells, cells.size() * sizeof(NdtCell)));
    CHECK_HIP(hipMalloc((void **)&dsrcs, srcs.size() * sizeof(NdtCell)));
    CHECK_HIP(hipMalloc((void **)&dcalls, calls.size() * sizeof(CallDev)));
    CHECK_HIP(hipMalloc((void **)&dout, out_n * sizeof(double)));
    CHECK_HIP(hipMemcpy(dcases, cases.data(), cases.size() * sizeof(CaseDev), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dranks, ranks.data(), ranks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dcells, cells.data(), cells.size() * sizeof(NdtCell), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dsrcs, srcs.data(), srcs.size() * sizeof(NdtCell), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dcalls, calls.data(), calls.size() * sizeof(CallDev), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out_n * sizeof(double)));
    hipLaunchKernelGGL(group_kernel, dim3((unsigned)cases.size()), dim3(64), 0, 0, dcases, dranks, dcells, dsrcs, dcalls, dout);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> out(out_n);
    CHECK_HIP(hipMemcpy(out.data(), dout, out_n * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(dcases)); CHECK_HIP(hipFree(dranks)); CHECK_HIP(hipFree(dcells)); CHECK_HIP(hipFree(dsrcs));
    CHECK_HIP(hipFree(dcalls)); CHECK_HIP(hipFree(dout));
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}

int main(int argc, char **argv)
{
    int mode = -1;
    for (int m = 0; m < N_MODES; m++)
        if (argc > 1 && strcmp(argv[1], MODE_NAME[m]) == 0) mode = m;
    if (mode < 0 || argc != 2) {
        fprintf(stderr, "usage: evalgroup_checks index|scan|totals|terms|terms_g|group < cases > results\n");
        return 64;
    }
    unsigned n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > (1u << 26)) {
        fprintf(stderr, "evalgroup_checks: no count on stdin (1 .. 2^26)\n");
        return 65;
    }
    if ((mode == MODE_SCAN || mode == MODE_TOTALS) && n % 64u != 0u) {
        fprintf(stderr, "evalgroup_checks: %s takes whole waves of 64 rows\n", MODE_NAME[mode]);
        return 65;
    }
    std::vector<double> in(mode == MODE_GROUP ? (size_t)n : (size_t)n * MODE_IN[mode]);
    if (fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) {
        fprintf(stderr, "evalgroup_checks: the table is short\n");
        return 65;
    }
    int n_dev = 0;
    CHECK_HIP(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) {
        fprintf(stderr, "evalgroup_checks: no HIP device\n");
        return 3;
    }
    if (mode == MODE_GROUP) return run_group(in);
    std::vector<double> out((size_t)n * MODE_OUT[mode]);
    double *din = nullptr, *dout = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, in.size() * sizeof(double)));
    CHECK_HIP(hipMalloc((void **)&dout, out.size() * sizeof(double)));
    CHECK_HIP(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out.size() * sizeof(double)));          // (NaN wherever a case writes nothing)
    const dim3 grid((n + 63u) / 64u), block(64);
    if (mode == MODE_INDEX) {
        hipLaunchKernelGGL(index_kernel, grid, block, 0, 0, din, dout, n);
    } else if (mode == MODE_SCAN) {
        hipLaunchKernelGGL(scan_kernel, grid, block, 0, 0, din, dout);
    } else if (mode == MODE_TOTALS) {
        hipLaunchKernelGGL(totals_kernel, grid, block, 0, 0, din, dout);
    } else if (mode == MODE_TERMS) {
        hipLaunchKernelGGL((terms_kernel<true>), grid, block, 0, 0, din, dout, n);
    } else {
        hipLaunchKernelGGL((terms_kernel<false>), grid, block, 0, 0, din, dout, n);
    }
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}
