// ndt_pgo_wide_core.h -- what the chip-wide forms of the two pose-graph optimisers (csrc/ndt_pgo_wide.hip for SE(2),
// csrc/ndt_pgo3_wide.hip for SE(3): ONE graph spread over the device, one plain launch per pass) have in common, once: the tile,
// the control block that carries the run's scalars from launch to launch, the passes, the combiners of the per-tile sums, the
// head of an inner iteration, and the host's steering loop.  Nothing here knows the size of a block or the layout of a graph:
// the launch arguments (NdtPgoWide, NdtPgo3Wide) name their fields alike and the templates below take either.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "ndt_block.h"

#define NDT_PGO_WIDE_TILE 256                     // items (links or nodes) per tile = threads per workgroup: part of the summation order
#define NDT_PGO_WIDE_WAVES (NDT_PGO_WIDE_TILE / 64)

// The run's scalars, counters and flags.  There are TWO in device memory: a launch reads one (src) and, where it is a node
// pass, one lane of its workgroup 0 writes the other (dst) IN FULL -- a launch whose phase is over copies src to dst -- and the
// host swaps the two after every node pass.  So no word is written by a launch in which any workgroup reads it.  The link
// passes write no control word: they read the src of the node pass behind them and come to the same decisions from the same
// partial sums.
struct NdtPgoWideCtl {
    int32_t run_done;                             // the Gauss-Newton loop has ended: exit_code holds, the result record is written
    int32_t solve_done;                           // the inner solve of this update has stopped: x is the step
    int32_t exit_code, iterations, linear;        // as ndtgpu_pgo_result; linear: inner iterations TAKEN, all updates together
    int32_t any_capped;                           // an inner solve of the run stopped at max_linear_iterations
    int32_t k;                                    // inner iterations of this solve
    int32_t pad_;
    double rz, tol2;                              // r.z of the iterate, eps_linear^2 * r.r of the solve's start
    double cost, cost_initial, max_step;
    double prior_cost;                            // SE(2): the prior's term at the updated poses (written by the pose update)
};

inline size_t ndt_pgo_wide_tiles(size_t n) { return (n + NDT_PGO_WIDE_TILE - 1) / NDT_PGO_WIDE_TILE; }

// the passes, one plain launch each; src / dst of the launch argument as the steering loop set them
enum NdtPgoWidePass {
    NDT_PGO_WIDE_LINEARISE,       // link pass: jac, te, per-tile cost
    NDT_PGO_WIDE_ASSESS_FIRST,    // node pass: the cost at the poses as set; ends the run where it must
    NDT_PGO_WIDE_ASSESS,          // node pass: the cost after an update, the roll-back, the stop rule, the result record
    NDT_PGO_WIDE_START,           // node pass: gather b and the diagonal blocks, x = 0, r = b, z = p = M^-1 r
    NDT_PGO_WIDE_LINK,            // link pass: t_e = W (J_ref p_ref + J_mov p_mov), p = z + beta p formed on the fly
    NDT_PGO_WIDE_NODE,            // node pass: the solve's break rules, p = z + beta p stored, A p, per-tile p.Ap
    NDT_PGO_WIDE_STEP,            // node pass: alpha, x, r, z, per-tile r.z and r.r
    NDT_PGO_WIDE_UPDATE           // node pass: prev = pose, the pose update, per-tile largest |x|
};
inline bool ndt_pgo_wide_is_link_pass(NdtPgoWidePass p) { return p == NDT_PGO_WIDE_LINEARISE || p == NDT_PGO_WIDE_LINK; }

// The host steers the phases: it enqueues the passes on `st` one launch each -- launch(pass, src, dst) -- and after every chunk
// of check_every inner iterations, and after every cost assessment, copies the control block to pinned memory and waits for it.
// A link pass reads the control block the node pass behind it reads; a node pass writes the other one.  Launches enqueued past
// a stop do nothing, so the result does not depend on check_every.  ctl: the two control blocks (device); mirror: pinned.
template <class Launch>
inline hipError_t ndt_pgo_wide_steer(Launch &&launch, NdtPgoWideCtl *ctl, NdtPgoWideCtl *mirror, int check_every, hipStream_t st)
{
    int cur = 0;                           // which of the two control blocks holds the state
    auto pass = [&](NdtPgoWidePass what) -> hipError_t {
        const hipError_t e = launch(what, (const NdtPgoWideCtl *)(ctl + cur), ctl + (cur ^ 1));
        if (!ndt_pgo_wide_is_link_pass(what)) cur ^= 1;
        return e;
    };
    auto look = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(mirror, ctl + cur, sizeof *mirror, hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    };
#define NDT_PGO_WIDE_TRY(expr)              \
    do {                                    \
        const hipError_t _e = (expr);       \
        if (_e != hipSuccess) return _e;    \
    } while (0)
    NDT_PGO_WIDE_TRY(hipMemsetAsync(ctl, 0, 2 * sizeof *ctl, st));
    NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_LINEARISE));
    NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_ASSESS_FIRST));
    NDT_PGO_WIDE_TRY(look());
    while (!mirror->run_done) {
        NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_START));
        do {
            for (int k = 0; k < check_every; k++) {
                NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_LINK));
                NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_NODE));
                NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_STEP));
            }
            NDT_PGO_WIDE_TRY(look());
        } while (!mirror->solve_done && !mirror->run_done);
        NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_UPDATE));
        NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_LINEARISE));
        NDT_PGO_WIDE_TRY(pass(NDT_PGO_WIDE_ASSESS));
        NDT_PGO_WIDE_TRY(look());
    }
#undef NDT_PGO_WIDE_TRY
    return hipSuccess;
}

#if defined(__HIPCC__)
// ---- device side: what every pass of either form begins or ends with ----
typedef NdtBlockSums<NDT_PGO_WIDE_WAVES, 2> WideRed;

// the graph's sums of N interleaved-by-stride partial arrays, in every thread
template <int N>
__device__ __forceinline__ void wide_combine(const double *part, unsigned tiles, double (&v)[N], WideRed &red, int &par)
{
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = 0.0;
    for (unsigned t = threadIdx.x; t < tiles; t += NDT_PGO_WIDE_TILE) {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += part[(size_t)k * tiles + t];
    }
    ndt_block_sum(v, red, par);
}

__device__ __forceinline__ double wide_combine_max(const double *part, unsigned tiles, WideRed &red, int &par)
{
    double m = 0.0;
    for (unsigned t = threadIdx.x; t < tiles; t += NDT_PGO_WIDE_TILE) m = fmax(m, part[t]);
    return ndt_block_max(m, red, par);
}

// one lane of the launch writes the next control block, every word of it (ordinary stores)
template <class Wide>
__device__ __forceinline__ void wide_store(const Wide &W, const NdtPgoWideCtl &n)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    NdtPgoWideCtl *d = W.dst;
    d->run_done = n.run_done;
    d->solve_done = n.solve_done;
    d->exit_code = n.exit_code;
    d->iterations = n.iterations;
    d->linear = n.linear;
    d->any_capped = n.any_capped;
    d->k = n.k;
    d->pad_ = 0;
    d->rz = n.rz;
    d->tol2 = n.tol2;
    d->cost = n.cost;
    d->cost_initial = n.cost_initial;
    d->max_step = n.max_step;
    d->prior_cost = n.prior_cost;
}

// the new search direction of a node: z + beta p, the same bits in the link pass that uses it and the node pass that stores it
__device__ __forceinline__ double wide_direction(double z, double beta, double p) { return fma(beta, p, z); }

// The head of an inner iteration, from the per-tile r.z / r.r of the solve's start (k == 0) or of the step before: the break
// rules of pgo_solve / pgo3_solve -- `rr > tol2`, then the cap -- and beta.
struct WideHead {
    bool stop, capped;
    double beta, rz, tol2;
};
template <class Wide>
__device__ __forceinline__ WideHead wide_head(const Wide &W, const NdtPgoWideCtl &c, WideRed &red, int &par)
{
    double dot[2];
    wide_combine(W.part_dot, W.node_tiles, dot, red, par);
    WideHead h;
    h.rz = dot[0];
    h.beta = 0.0;
    h.tol2 = c.tol2;
    if (c.k == 0) h.tol2 = W.prm.eps_linear * W.prm.eps_linear * dot[1];
    else h.beta = dot[0] / c.rz;
    h.capped = false;
    h.stop = !(dot[1] > h.tol2);
    if (!h.stop && c.k >= W.prm.max_linear_iterations) h.stop = h.capped = true;
    return h;
}
#endif
