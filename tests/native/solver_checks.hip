// Direct checks of csrc/ndt_solver.h (and through it the solves of csrc/ndt_math.h): the stages of the Newton iteration, the
// More-Thuente line search and the covariance tail, one case per call, with nothing of the matcher around them.
//   solver_checks <mode> host|gpu      stdin: uint32 n, then n rows of IN[mode] doubles;  stdout: n rows of OUT[mode] doubles
// The per-case work of a mode is ONE host/device function: `host` calls it in a loop, `gpu` calls it from a kernel, one thread
// per case in workgroups of 64 -- both targets run the same source, and tests/test_solver_direct.py (which builds and drives
// this program) holds both to the same references.  Includes the header alone and links only the HIP runtime.  The GPU path
// makes one launch per run, checks every HIP call, and exits 2 with the error string on the first failure.
//
// Row layouts (integers travel as doubles):
//   cstep       in  stx fx dx sty fy dy stp fp dp brackt stmin stmax
//               out info stx fx dx sty fy dy stp brackt
//   linesearch  in  finit dginit K (f_k dg_k) x 41: the search runs along dof 0 with a unit increment and is fed the recorded pairs
//               out the 41 requested steps, step_size, nfev, final_from_trial, spec_ok, reuse_sums, pairs consumed,
//                   cut (0: the search ended; 1: cut off after 41 trials; 2: the recording ran out), first stage's return,
//                   trial_has_h of the last trial
//   trialpose   in  T (rigid, 12) incr (6) stp: one trial at step stp that meets the More-Thuente conditions
//               out Teval of the trial (12), st.T after apply_step (12), final_from_trial, step_size
//   solve       in  H (36, row-major) g (6) JJ (21, upper triangle)
//               out is_pd, x by newton_factor (6; zeros unless is_pd), x by newton_ldlt (6), cov_from_sums' return and 36 outputs
//   newton      in  sums (28) dof_mask delta_score step_control fusion_flags Q (36) pose_local (6) T (rigid, 12) Tinit (rigid, 12)
//               out return, exit_code, done, score_here, is_pd, gnorm, st.incr (6), ws.H diagonal (6), st.x0 (6), step_size, ws.dx (6)
#include "../../ndt_feature_graph_amd/csrc/ndt_solver.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK_HIP(x)                                                                                                    \
    do {                                                                                                                \
        hipError_t e_ = (x);                                                                                            \
        if (e_ != hipSuccess) {                                                                                         \
            fprintf(stderr, "solver_checks: %s failed: %s\n", #x, hipGetErrorString(e_));                               \
            exit(2);                                                                                                    \
        }                                                                                                               \
    } while (0)

enum { MODE_CSTEP = 0, MODE_LINESEARCH = 1, MODE_TRIALPOSE = 2, MODE_SOLVE = 3, MODE_NEWTON = 4, N_MODES = 5 };
static const int MAX_TRIALS = 41;
static const char *const MODE_NAME[N_MODES] = {"cstep", "linesearch", "trialpose", "solve", "newton"};
static const int MODE_IN[N_MODES] = {12, 3 + 2 * MAX_TRIALS, 19, 63, 98};
static const int MODE_OUT[N_MODES] = {9, MAX_TRIALS + 9, 26, 50, 31};

// the state of one case: in memory (a global buffer indexed by case), as the solver's state is in the kernels that run it
struct Work {
    MatchState st;
    NewtonWs ws;
    double w[72], t[36];
};

NDT_HD NdtMatchParamsDev default_params()
{
    NdtMatchParamsDev prm;
    prm.n_neighbours = 2; prm.itr_max = 30; prm.step_control = 1; prm.dof_mask = 0x3f; prm.use_initial_guess = 0;
    prm.fusion_flags = 0;
    prm.delta_score = 1e-6; prm.lfd1 = 1.0; prm.lfd2 = 0.05;
    return prm;
}

NDT_HD void case_cstep(const double *in, double *out, Work &)
{
    double stx = in[0], fx = in[1], dx = in[2], sty = in[3], fy = in[4], dy = in[5], stp = in[6];
    int brackt = in[9] != 0.0;
    const int info = mt_cstep(stx, fx, dx, sty, fy, dy, stp, in[7], in[8], brackt, in[10], in[11]);
    out[0] = info;
    out[1] = stx; out[2] = fx; out[3] = dx; out[4] = sty; out[5] = fy; out[6] = dy; out[7] = stp;
    out[8] = brackt;
}

// a search along dof 0 from the identity: value finit and slope dginit at step 0
NDT_HD int start_search(MatchState &st, const NdtMatchParamsDev &prm, double finit, double dginit)
{
    match_state_init(st, nullptr, prm);
    double incr[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double g6[6] = {dginit, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int next = mt_start_local(st, finit, g6, incr);
    for (int a = 0; a < 6; a++) st.incr[a] = incr[a];
    return next;
}

NDT_HD void case_linesearch(const double *in, double *out, Work &wk)
{
    MatchState &st = wk.st;
    const NdtMatchParamsDev prm = default_params();
    int K = (int)in[2];
    if (K > MAX_TRIALS) K = MAX_TRIALS;
    for (int k = 0; k < MAX_TRIALS + 9; k++) out[k] = 0.0;
    int next = start_search(st, prm, in[0], in[1]);
    const int first = next;
    int used = 0, cut = 0;
    if (next == NEXT_REQUEST_TRIAL) {
        cut = 1;
        for (int k = 0; k < MAX_TRIALS; k++) {
            mt_request_trial(st);
            out[k] = st.mt.stp;
            if (k >= K) { cut = 2; break; }
            double sums[28];
            for (int a = 0; a < 28; a++) sums[a] = 0.0;
            sums[0] = in[3 + 2 * k];
            sums[1] = in[4 + 2 * k];
            next = linesearch_step(st, sums, prm);
            used++;
            if (next != NEXT_REQUEST_TRIAL) { cut = 0; break; }
        }
    }
    double *o = out + MAX_TRIALS;
    o[0] = st.step_size; o[1] = (first == NEXT_REQUEST_TRIAL) ? st.mt.nfev : 0; o[2] = st.final_from_trial; o[3] = st.spec_ok;
    o[4] = st.reuse_sums; o[5] = used; o[6] = cut; o[7] = first;
    o[8] = (first == NEXT_REQUEST_TRIAL) ? st.trial_has_h : 0;
}

NDT_HD void case_trialpose(const double *in, double *out, Work &wk)
{
    MatchState &st = wk.st;
    const NdtMatchParamsDev prm = default_params();
    match_state_init(st, nullptr, prm);
    for (int k = 0; k < 9; k++) st.T.r[k] = in[k];
    for (int k = 0; k < 3; k++) st.T.t[k] = in[9 + k];
    // value 0 and gradient -incr at the current pose: dginit = -|incr|^2 < 0, the increment is a descent direction as it stands
    double incr[6], g6[6];
    double dginit = 0.0;
    for (int a = 0; a < 6; a++) { incr[a] = in[12 + a]; g6[a] = -incr[a]; dginit += incr[a] * g6[a]; }
    const int first = mt_start_local(st, 0.0, g6, incr);
    for (int a = 0; a < 6; a++) st.incr[a] = incr[a];
    for (int k = 0; k < 26; k++) out[k] = 0.0;
    if (first != NEXT_REQUEST_TRIAL) return;
    st.mt.stp = in[18];                         // (the step a cstep would have left there)
    mt_request_trial(st);
    const double stp = st.mt.stp;
    for (int k = 0; k < 9; k++) out[k] = st.Teval.r[k];
    for (int k = 0; k < 3; k++) out[9 + k] = st.Teval.t[k];
    // half the decrease the initial slope promises and a flat slope there: sufficient decrease and curvature both hold
    double sums[28];
    for (int a = 0; a < 28; a++) sums[a] = 0.0;
    sums[0] = 0.5 * stp * dginit;
    const int next = linesearch_step(st, sums, prm);
    if (next != NEXT_APPLY_STEP) return;
    apply_step(st, prm);
    for (int k = 0; k < 9; k++) out[12 + k] = st.T.r[k];
    for (int k = 0; k < 3; k++) out[21 + k] = st.T.t[k];
    out[24] = st.final_from_trial;
    out[25] = st.step_size;
}

NDT_HD void case_solve(const double *in, double *out, Work &wk)
{
    NewtonWs &ws = wk.ws;
    for (int k = 0; k < 36; k++) ws.H[k] = in[k];
    for (int k = 0; k < 6; k++) { ws.g[k] = in[36 + k]; ws.dx[k] = 0.0; }
    newton_factor(ws);
    out[0] = ws.is_pd;
    for (int k = 0; k < 6; k++) out[1 + k] = ws.is_pd ? ws.dx[k] : 0.0;
    newton_ldlt(ws);
    for (int k = 0; k < 6; k++) out[7 + k] = ws.dx[k];
    double h21[21];
    int o = 0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) h21[o++] = in[a * 6 + b];
    out[13] = cov_from_sums(h21, in + 42, wk.w, wk.t, out + 14);
}

NDT_HD void case_newton(const double *in, double *out, Work &wk)
{
    MatchState &st = wk.st;
    NewtonWs &ws = wk.ws;
    NdtMatchParamsDev prm = default_params();
    prm.dof_mask = (int)in[28];
    prm.delta_score = in[29];
    prm.step_control = (int)in[30];
    prm.fusion_flags = (int)in[31];
    prm.use_initial_guess = 1;
    const double *Ti = in + 86;
    double T16[16];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T16[c * 4 + r] = Ti[r * 3 + c];
        T16[12 + r] = Ti[9 + r];
        T16[r * 4 + 3] = 0.0;
    }
    T16[15] = 1.0;
    match_state_init(st, T16, prm, in + 32);
    for (int k = 0; k < 9; k++) st.T.r[k] = in[74 + k];
    for (int k = 0; k < 3; k++) st.T.t[k] = in[83 + k];
    st.Teval = st.T;
    for (int k = 0; k < 6; k++) st.pose_local[k] = in[68 + k];
    for (int k = 0; k < 6; k++) { st.incr[k] = 0.0; ws.dx[k] = 0.0; }
    st.step_size = 0.0;
    ws.is_pd = -1;
    const int next = newton_solve(st, in, nullptr, prm, ws);
    out[0] = next; out[1] = st.exit_code; out[2] = st.done; out[3] = st.score_here; out[4] = ws.is_pd; out[5] = ws.gnorm;
    for (int k = 0; k < 6; k++) {
        out[6 + k] = st.incr[k];
        out[12 + k] = ws.H[k * 7];
        out[18 + k] = st.x0[k];
        out[25 + k] = ws.dx[k];
    }
    out[24] = st.step_size;
}

template <int MODE>
NDT_HD void run_case(const double *in, double *out, Work &wk)
{
    if constexpr (MODE == MODE_CSTEP) case_cstep(in, out, wk);
    else if constexpr (MODE == MODE_LINESEARCH) case_linesearch(in, out, wk);
    else if constexpr (MODE == MODE_TRIALPOSE) case_trialpose(in, out, wk);
    else if constexpr (MODE == MODE_SOLVE) case_solve(in, out, wk);
    else case_newton(in, out, wk);
}

template <int MODE>
__global__ __launch_bounds__(64) void cases_kernel(const double *in, double *out, Work *work, unsigned n, int n_in, int n_out)
{
    const unsigned k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    run_case<MODE>(in + (size_t)k * n_in, out + (size_t)k * n_out, work[k]);
}

template <int MODE>
static void run_host(const std::vector<double> &in, std::vector<double> &out, unsigned n)
{
    std::vector<Work> work(n);              // (value-initialised: all zero, like the device's buffer)
    for (unsigned k = 0; k < n; k++) run_case<MODE>(in.data() + (size_t)k * MODE_IN[MODE], out.data() + (size_t)k * MODE_OUT[MODE], work[k]);
}

template <int MODE>
static void run_gpu(const std::vector<double> &in, std::vector<double> &out, unsigned n)
{
    int n_dev = 0;
    CHECK_HIP(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) {
        fprintf(stderr, "solver_checks: no HIP device\n");
        exit(3);
    }
    double *din = nullptr, *dout = nullptr;
    Work *dwork = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, in.size() * sizeof(double)));
    CHECK_HIP(hipMalloc((void **)&dout, out.size() * sizeof(double)));
    CHECK_HIP(hipMalloc((void **)&dwork, (size_t)n * sizeof(Work)));
    CHECK_HIP(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemset(dout, 0xFF, out.size() * sizeof(double)));          // (NaN wherever a case writes nothing)
    CHECK_HIP(hipMemset(dwork, 0, (size_t)n * sizeof(Work)));
    hipLaunchKernelGGL((cases_kernel<MODE>), dim3((n + 63u) / 64u), dim3(64), 0, 0, din, dout, dwork, n, MODE_IN[MODE], MODE_OUT[MODE]);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
    CHECK_HIP(hipFree(dwork));
}

template <int MODE>
static void run_mode(bool gpu, const std::vector<double> &in, std::vector<double> &out, unsigned n)
{
    if (gpu) run_gpu<MODE>(in, out, n);
    else run_host<MODE>(in, out, n);
}

int main(int argc, char **argv)
{
    int mode = -1;
    for (int m = 0; m < N_MODES; m++)
        if (argc > 1 && strcmp(argv[1], MODE_NAME[m]) == 0) mode = m;
    const bool gpu = argc > 2 && strcmp(argv[2], "gpu") == 0;
    if (mode < 0 || argc != 3 || (!gpu && strcmp(argv[2], "host") != 0)) {
        fprintf(stderr, "usage: solver_checks cstep|linesearch|trialpose|solve|newton host|gpu < cases > results\n");
        return 64;
    }
    unsigned n = 0;
    if (fread(&n, sizeof n, 1, stdin) != 1 || n < 1 || n > (1u << 20)) {
        fprintf(stderr, "solver_checks: no case count on stdin (1 .. 2^20)\n");
        return 65;
    }
    std::vector<double> in((size_t)n * MODE_IN[mode]), out((size_t)n * MODE_OUT[mode]);
    if (fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) {
        fprintf(stderr, "solver_checks: %s takes %d doubles per case, the table is short\n", MODE_NAME[mode], MODE_IN[mode]);
        return 65;
    }
    switch (mode) {
    case MODE_CSTEP: run_mode<MODE_CSTEP>(gpu, in, out, n); break;
    case MODE_LINESEARCH: run_mode<MODE_LINESEARCH>(gpu, in, out, n); break;
    case MODE_TRIALPOSE: run_mode<MODE_TRIALPOSE>(gpu, in, out, n); break;
    case MODE_SOLVE: run_mode<MODE_SOLVE>(gpu, in, out, n); break;
    default: run_mode<MODE_NEWTON>(gpu, in, out, n); break;
    }
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size() || fflush(stdout) != 0) return 66;
    return 0;
}
