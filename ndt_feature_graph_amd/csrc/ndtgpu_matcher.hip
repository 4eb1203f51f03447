// ndtgpu_matcher.hip -- the matcher entries of the C-ABI (include/ndtgpu.h): host- and device-pointer batches, fusion,
// covariance, derivatives, and the choice between the persistent, grid-barrier, task-pool and host-driven forms.
#include "ndtgpu_host.h"

#include <chrono>
#include <mutex>

static_assert(sizeof(NdtMatchResultDev) == sizeof(ndtgpu_match_result), "result layouts must agree");

#define NDTGPU_HOST_LOOP_MAX 8             // up to this many registrations per call: the latency shapes (grid barrier / host loop)
#define NDTGPU_COOP_MIN_SET_CELLS 16384u   // source sets with room for fewer cells per map hold small (2D) maps

// ---- switches ------------------------------------------------------------------------------------------------------------
// The matcher's environment switches: A/B and debugging aids, read per call by match_knobs (tests switch them
// between calls).  Switch [default]: meaning (who sets it besides tests/test_gpu_parity.py)
struct MatchKnobs {
    bool host_loop;          // NDTGPU_HOST_LOOP=1 [0]: <= 8 pairs of a host-pointer entry run the host-driven loop (tools/spec_stats.py)
    int coop;                // NDTGPU_COOP [unset]: 9 .. n_cu/2 pairs of a host-pointer entry: 0 always the persistent kernel, 1 always
                             //   a grid-barrier / pool launch; unset (or another value): such a launch on sets of large maps only
    bool device_coop;        // NDTGPU_DEVICE_COOP=0 [1]: the device-pointer entry keeps small batches on the persistent kernel (bench.py)
    int pool;                // NDTGPU_POOL=0 / 1 [unset: -1]: a multi-workgroup batch always takes the grid-barrier kernel / the task
                             //   pool; unset: the pool above 8 pairs (bench.py)
    int coop_cells;          // NDTGPU_COOP_CELLS [96; 256 on sets of large maps]: source cells per chunk of those two kernels
    bool coop_api;           // NDTGPU_COOP_API=1 [0]: grid-barrier launches through hipLaunchCooperativeKernel (residency checked)
    int slots;               // NDTGPU_SLOTS [2]: registrations in flight per persistent workgroup, 1 .. 3 (tools/*.sh)
    int park_iters;          // NDTGPU_PARK_ITERS [6]: iterations after which a long registration yields (0: never; tools/sweep_bench.sh)
    bool double_thresh_set;  // NDTGPU_DOUBLE_THRESH [the workgroups]: a persistent workgroup resumes a second parked registration
    unsigned double_thresh;  //   only when more than this many are waiting (tools/*.sh)
    int match_groups;        // NDTGPU_MATCH_GROUPS [one per CU]: workgroups of a persistent launch (bench.py --cu-split)
    bool trace;              // NDTGPU_TRACE [unset]: set, the host-driven loop prints one line per evaluation (tools/spec_stats.py)
};

static MatchKnobs match_knobs()
{
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    MatchKnobs knobs;
    knobs.host_loop = num("NDTGPU_HOST_LOOP", 0) != 0;
    knobs.coop = num("NDTGPU_COOP", -1);
    knobs.device_coop = num("NDTGPU_DEVICE_COOP", 1) != 0;
    knobs.pool = getenv("NDTGPU_POOL") ? (num("NDTGPU_POOL", 0) != 0) : -1;
    knobs.coop_cells = num("NDTGPU_COOP_CELLS", 0);
    knobs.coop_api = num("NDTGPU_COOP_API", 0) != 0;
    knobs.slots = num("NDTGPU_SLOTS", 2);
    if (knobs.slots < 1 || knobs.slots > 3) knobs.slots = 2;
    knobs.park_iters = num("NDTGPU_PARK_ITERS", 6);
    knobs.double_thresh_set = getenv("NDTGPU_DOUBLE_THRESH") != nullptr;
    knobs.double_thresh = (unsigned)num("NDTGPU_DOUBLE_THRESH", 0);
    knobs.match_groups = num("NDTGPU_MATCH_GROUPS", 0);
    knobs.trace = getenv("NDTGPU_TRACE") != nullptr;
    return knobs;
}

ndtgpu_status match_params_dev(const ndtgpu_match_params *prm, int fusion_flags, NdtMatchParamsDev &p)
{
    p = to_dev(prm);
    p.fusion_flags = fusion_flags;
    if (p.n_neighbours < 0 || p.n_neighbours > 3 || (p.dof_mask & 0x3f) == 0)
        return fail(NDTGPU_ERR_INVALID, "match: n_neighbours must be 0..3 and dof_mask non-empty");
    return NDTGPU_OK;
}

// ---- the grid-barrier matcher (csrc/ndt_match.hip ndt_match_coop_kernel): several workgroups per registration ---------
// One such launch at a time on the device: two of them could each hold part of the chip and wait for the rest.  Every
// launch waits (on its stream, not on the host) for the event of the one before it.
static std::mutex g_coop_mutex;
// (per device: an event belongs to the device it was created on, and launches on one device need not wait for another's)
// Static storage, so a raw event handle and no Fence: these live until the process ends, when the HIP runtime may already be
// gone -- nothing here is destroyed, and ndtgpu_live_resources does not count it.
struct CoopOrder {
    hipEvent_t ev = nullptr;       // recorded behind the device's last asynchronous grid-barrier launch
    bool valid = false;
};
#define NDTGPU_MAX_DEVICES 64
static CoopOrder g_coop_order[NDTGPU_MAX_DEVICES];
static CoopOrder &coop_order()     // (the current device's; read and written under g_coop_mutex)
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
    return g_coop_order[d % NDTGPU_MAX_DEVICES];
}

ndtgpu_status ndtgpu_mapset::ensure_coop(size_t bytes, const CoopOrder &last)
{
    if (bytes <= coop_work.capacity()) return NDTGPU_OK;
    if (last.valid) HIP_TRY(hipEventSynchronize(last.ev));      // an asynchronous launch may still use the area
    coop_clean_upto = 0;
    HIP_TRY(coop_work.reserve(bytes));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_mapset::ensure_pin(size_t bytes, const CoopOrder &last)
{
    if (bytes <= pin.capacity()) return NDTGPU_OK;
    if (last.valid) HIP_TRY(hipEventSynchronize(last.ev));      // a grid-barrier kernel may still write into the block
    HIP_TRY(pin.reserve(bytes));
    return NDTGPU_OK;
}

struct CoopPlan {
    unsigned groups, per_group;   // workgroups per registration in the grid (task pool: of the launch); source cells per chunk
    size_t stride;                // bytes of work area per registration
    int checked;                  // launch through hipLaunchCooperativeKernel
    bool pool;                    // the task-pool kernel (default) instead of the grid-barrier kernel (NDTGPU_POOL=0)
};

// The grid of a batch: every registration gets the same number of workgroups, as many as fit on the chip together
// (occupancy query), at most one per chunk of the largest map the source set can hold.  No look at the maps: the kernel
// cuts a registration into chunks by its own cell count and surplus workgroups leave at once.  False: the batch does not
// fit (more registrations than resident workgroups).
static bool coop_plan(const ndtgpu_mapset *ss, size_t n_pairs, const NdtMatchParamsDev &p, const MatchKnobs &knobs, CoopPlan &pl)
{
    const unsigned capacity = ndt_match_coop_capacity(p.n_neighbours);
    if (capacity == 0 || n_pairs == 0 || n_pairs > capacity) return false;
    // Source cells per chunk -- a property of the source SET (its cell capacity), so that a registration's rows, and with
    // them its bits, do not depend on the batch it is in.  Sets of small maps (planar scans): 96 (12 per wave; with ONE grid
    // barrier per evaluation, round 6: 64 / 96 / 128 / 192 cells 0.295 / 0.282 / 0.297 / 0.288 ms for the 2D pair of 100 k
    // points, build included).  Sets that hold large maps (3D sweeps, >= 16 k cells): 256 -- every chunk
    // costs its own pass over the pair terms (batches of 64 that end half empty) and its own wave sum, and every row a
    // hand-over: 12 k-cell maps, 4 / 8 / 16 / 32 pairs 1.41 / 2.33 / 3.57 / 4.75 ms with 128 against 1.34 / 2.20 / 3.29 /
    // 4.34 ms with 256 (384: 32 pairs 4.63, 512: 4.56); one pair alone 1.11 against 1.33 ms -- half as many workgroups.
    // (Round 6, one barrier per evaluation: one pair alone 1.04 / 1.17 / 1.26 ms with 96 / 192 / 256, but the pool's 32 pairs
    //  5.07 / 4.83 / 4.63 ms: the batch decides, 256 stays.)
    pl.per_group = knobs.coop_cells > 0 ? (unsigned)knobs.coop_cells : (ss->v.grid.max_cells >= 16384u ? 256u : 96u);
    const unsigned n_chunks = std::max(1u, (ss->v.grid.max_cells + pl.per_group - 1u) / pl.per_group);
    // Up to 8 registrations: the grid-barrier kernel (static teams, the solver state stays in one workgroup's LDS: 12 k-cell
    // 3D maps, 1 / 4 / 8 pairs 1.63 / 2.30 / 3.01 ms against 1.94 / 2.57 / 3.14 ms).  More: the task pool (any workgroup
    // takes any task of any registration, the long registrations get the workgroups the others leave: 16 / 32 pairs
    // 5.6 / 6.9 ms against 7.2 / 10.7 ms).  Same chunks, same order of sums: the same bits.  NDTGPU_POOL=0 / 1 forces one.
    pl.pool = knobs.pool >= 0 ? knobs.pool != 0 : n_pairs > NDTGPU_HOST_LOOP_MAX;
    if (pl.pool) {
        // any workgroup takes any task of any registration: as many workgroups as the chip holds, or as there can be tasks
        pl.groups = (unsigned)std::max<size_t>(1, std::min<size_t>(capacity, n_pairs * (size_t)n_chunks));
        pl.stride = ndt_match_pool_pair_bytes(n_chunks);
    } else {
        pl.groups = std::max<unsigned>(1u, std::min<size_t>(n_chunks, capacity / n_pairs));
        pl.stride = ndt_match_coop_work_bytes(n_chunks);
    }
    pl.checked = knobs.coop_api ? 1 : 0;
    return true;
}

// ---- which form runs a batch ---------------------------------------------------------------------------------------------
enum class MatchEntry { host, device };     // host-pointer entries (synchronous) / ndtgpu_match_batch_device (asynchronous)
enum class MatchForm { persistent, grid_barrier, pool, host_loop };

// The one place that decides.  "Large maps": the source set has room for >= 16 k cells per map; n_cu: the device's CUs.
//
//   entry    pairs           form
//   host     1 .. 8          the host loop with NDTGPU_HOST_LOOP; else the grid barrier on any set (the pool with NDTGPU_POOL=1)
//   host     9 .. n_cu/2     the pool (the grid barrier with NDTGPU_POOL=0) on large maps or with NDTGPU_COOP=1; the
//                            persistent kernel on small maps or with NDTGPU_COOP=0
//   device   1 .. n_cu/2     on large maps: the grid barrier up to 8 pairs, the pool above (NDTGPU_POOL forces one) -- unless
//                            NDTGPU_DEVICE_COOP=0, the stream is being captured (the ordering event is not part of a capture),
//                            or a covariance is asked for without room to save the initial guesses (cov_unsaved)
//   any      above n_cu/2    the persistent kernel
//   and the persistent kernel whenever coop_plan declines (more registrations than resident workgroups).
static MatchForm choose_form(MatchEntry entry, size_t n_pairs, const ndtgpu_mapset *ss, const NdtMatchParamsDev &p,
                             const MatchKnobs &knobs, hipStream_t st, bool cov_unsaved, CoopPlan &pl)
{
    const bool large = ss->v.grid.max_cells >= NDTGPU_COOP_MIN_SET_CELLS;
    if (entry == MatchEntry::host) {
        if (n_pairs <= NDTGPU_HOST_LOOP_MAX && knobs.host_loop) return MatchForm::host_loop;
        if (n_pairs > (size_t)device_cus() / 2) return MatchForm::persistent;
        // More than a handful of registrations on a set of small maps (fewer than 16 k cells per map, i.e. 2D scans: four
        // chunks each): one CU per registration is as fast or faster (2D, 100 k points: 16 / 64 / 128 pairs 1.47 / 1.59 / 2.39 ms
        // here against 1.46 / 1.47 / 1.48 ms on the persistent kernel; 12 k-cell 3D maps: 4.9 / 12.8 ms against 46 ms).
        if (n_pairs > NDTGPU_HOST_LOOP_MAX && (knobs.coop == 0 || (!large && knobs.coop != 1))) return MatchForm::persistent;
    } else {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (n_pairs == 0 || n_pairs > (size_t)device_cus() / 2 || !large || !knobs.device_coop ||
            hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
            return MatchForm::persistent;
    }
    if (!coop_plan(ss, n_pairs, p, knobs, pl) || (entry == MatchEntry::device && cov_unsaved)) return MatchForm::persistent;
    return pl.pool ? MatchForm::pool : MatchForm::grid_barrier;
}

// ---- the forms -----------------------------------------------------------------------------------------------------------

// Enqueues ONE launch for the whole batch on `st` behind the previous grid-barrier launch of the device (g_coop_mutex held).
static ndtgpu_status coop_enqueue(ndtgpu_mapset *ts, ndtgpu_mapset *ss, const uint32_t *tidx_dev, const uint32_t *sidx_dev,
                                  double *T16_dev, NdtMatchResultDev *res_dev, const double *Q36_dev, size_t n_pairs,
                                  const NdtMatchParamsDev &p, const CoopPlan &pl, bool clear, bool record, CoopOrder &order,
                                  hipStream_t st, unsigned *done_host = nullptr)
{
    if (order.valid) HIP_TRY(hipStreamWaitEvent(st, order.ev, 0));
    // the control blocks must be zero (barrier counters only grow while a registration runs); the kernels leave them so
    hipError_t e;
    if (pl.pool) {
        if (clear) {
            HIP_TRY(hipMemsetAsync(ts->coop_work.get(), 0, ndt_match_pool_ctrl_bytes(), st));
            HIP_TRY(hipMemset2DAsync((char *)ts->coop_work.get() + ndt_match_pool_ctrl_bytes(), pl.stride, 0, ndt_match_pool_head_bytes(), n_pairs, st));
        }
        e = ndt_launch_match_pool(ts->v, tidx_dev, ss->v, sidx_dev, T16_dev, n_pairs, p, res_dev, Q36_dev, pl.groups, pl.per_group,
                                  ts->coop_work.get(), pl.stride, st);
    } else {
        if (clear) HIP_TRY(hipMemset2DAsync(ts->coop_work.get(), pl.stride, 0, ndt_match_coop_ctrl_bytes(), n_pairs, st));
        e = ndt_launch_match_coop(ts->v, tidx_dev, ss->v, sidx_dev, T16_dev, 0, n_pairs, p, res_dev, Q36_dev, pl.groups,
                                  pl.per_group, ts->coop_work.get(), pl.stride, pl.checked, st, done_host);
    }
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "match: grid-barrier launch", e);
    if (record) {     // (a caller that waits for its launch under the mutex leaves nothing for later launches to wait for)
        if (!order.ev) HIP_TRY(hipEventCreateWithFlags(&order.ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(order.ev, st));
        order.valid = true;
    }
    { ndtgpu_status trc = ts->touch(st); if (trc != NDTGPU_OK) return trc; }
    if (ss != ts) { ndtgpu_status trc = ss->touch(st); if (trc != NDTGPU_OK) return trc; }
    return NDTGPU_OK;
}

// (knobs_in: the calling entry's switches; nullptr: read them now)
ndtgpu_status match_device_core(ndtgpu_mapset *ts, const uint32_t *tidx_dev, ndtgpu_mapset *ss, const uint32_t *sidx_dev,
                                double *T16_dev, size_t n_pairs, const NdtMatchParamsDev &p, ndtgpu_match_result *results_dev,
                                const double *Q36_dev, hipStream_t st, const unsigned *feat_off_dev, const double *feat_cells_dev,
                                int cov_mode, double *cov36_dev, int32_t *cov_flags_dev, const MatchKnobs *knobs_in)
{
    if (n_pairs == 0) return NDTGPU_OK;
    const MatchKnobs knobs = knobs_in ? *knobs_in : match_knobs();
    // persistent workgroups, one per CU (8 waves x 256 VGPRs), each with `slots` registrations in flight whose evaluation
    // shares its waves take in turn (csrc/ndt_match.hip); pairs are pulled from a ticket counter.
    unsigned n_groups = (unsigned)std::min<size_t>(n_pairs, (size_t)device_cus());
    // (a stream that owns only part of the chip -- a CU-masked stream, bench.py --cu-split -- wants one workgroup
    //  per CU it has, not per CU of the device)
    if (ts->match_groups) n_groups = (unsigned)std::min<size_t>(n_pairs, (size_t)ts->match_groups);
    // (more workgroups than CUs: narrow-workgroup builds of the kernel, -DNDT_MATCH_THREADS=256, of which two share a CU)
    if (knobs.match_groups > 0) n_groups = (unsigned)std::min<size_t>(n_pairs, (size_t)knobs.match_groups);
    const unsigned double_thresh = knobs.double_thresh_set ? knobs.double_thresh : n_groups;
    // The work area (ticket counters, parked solver states) belongs to the target set: a launch on another stream
    // waits for the previous one, and growing the area waits for everything that may still use the old one.
    if (ts->work_stream != st) HIP_TRY(ts->work_used.order(st));
    HIP_TRY(ts->work.reserve(ndt_match_work_bytes(n_pairs, (size_t)n_groups * knobs.slots), ts->work_used));
    if (ts->profiling) HIP_TRY(ts->ev[2].record(st));
    hipError_t e = ndt_launch_match(ts->v, tidx_dev, ss->v, sidx_dev, T16_dev, n_pairs, p,
                                    reinterpret_cast<NdtMatchResultDev *>(results_dev), Q36_dev, feat_off_dev, feat_cells_dev,
                                    n_groups, knobs.park_iters, knobs.slots, double_thresh, ts->work.get(), st, cov_mode, cov36_dev, cov_flags_dev);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "match: launch", e);
    if (ts->profiling) HIP_TRY(ts->ev[3].record(st));
    HIP_TRY(ts->work_used.record(st));
    ts->work_stream = st;
    // the launch reads both sets' maps: host-synchronous rebuilds of either wait for it
    { ndtgpu_status trc = ts->touch(st); if (trc != NDTGPU_OK) return trc; }
    if (ss != ts) { ndtgpu_status trc = ss->touch(st); if (trc != NDTGPU_OK) return trc; }
    return NDTGPU_OK;
}

ndtgpu_status match_batch_device_ex(ndtgpu_mapset *ts, const uint32_t *tidx_dev, ndtgpu_mapset *ss, const uint32_t *sidx_dev,
                                    double *T16_dev, size_t n_pairs, const ndtgpu_match_params *prm,
                                    ndtgpu_match_result *results_dev, ndtgpu_stream stream, int cov_mode, double *cov36_dev,
                                    int32_t *cov_flags_dev, double *T16_save_dev)
{
    if (!ts || !ss || (n_pairs && (!tidx_dev || !sidx_dev || !T16_dev || !results_dev)))
        return fail(NDTGPU_ERR_INVALID, "match_batch_device: bad argument");
    NdtMatchParamsDev p;
    ndtgpu_status rc = match_params_dev(prm, 0, p);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MatchKnobs knobs = match_knobs();
    CoopPlan pl;
    if (choose_form(MatchEntry::device, n_pairs, ss, p, knobs, st, cov_mode >= 0 && !T16_save_dev, pl) == MatchForm::persistent)
        return match_device_core(ts, tidx_dev, ss, sidx_dev, T16_dev, n_pairs, p, results_dev, nullptr, st, nullptr, nullptr,
                                 cov_mode, cov36_dev, cov_flags_dev, &knobs);
    std::lock_guard<std::mutex> coop_lock(g_coop_mutex);
    CoopOrder &order = coop_order();
    rc = ts->ensure_coop(n_pairs * pl.stride + (pl.pool ? ndt_match_pool_ctrl_bytes() : 0), order);
    if (rc != NDTGPU_OK) return rc;
    ts->coop_clean_stride = pl.stride;
    ts->coop_clean_upto = 0;                            // (nobody will look how this launch ended: the next call clears)
    ts->ev[3].clear();
    if (cov_mode >= 0) HIP_TRY(hipMemcpyAsync(T16_save_dev, T16_dev, n_pairs * 16 * sizeof(double), hipMemcpyDeviceToDevice, st));
    rc = coop_enqueue(ts, ss, tidx_dev, sidx_dev, T16_dev, reinterpret_cast<NdtMatchResultDev *>(results_dev), nullptr,
                      n_pairs, p, pl, true, true, order, st);
    if (rc != NDTGPU_OK || cov_mode < 0) return rc;
    // (these registrations run on many workgroups each: the covariance is a follow-on launch, as in the fuser bank)
    hipError_t e = ndt_launch_covariance(ts->v, tidx_dev, ss->v, sidx_dev, T16_dev, n_pairs, p.n_neighbours, p.lfd1, p.lfd2,
                                         cov_mode, cov36_dev, cov_flags_dev, st);
    if (e == hipSuccess)
        e = ndt_launch_cov_flags(T16_save_dev, T16_dev, reinterpret_cast<const NdtMatchResultDev *>(results_dev), cov36_dev,
                                 cov_flags_dev, n_pairs, st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "match: covariance launch", e);
    { ndtgpu_status trc = ts->touch(st); if (trc != NDTGPU_OK) return trc; }
    if (ss != ts) { ndtgpu_status trc = ss->touch(st); if (trc != NDTGPU_OK) return trc; }
    return NDTGPU_OK;
}

// host arrays -> staging -> persistent matcher -> host arrays; synchronous
static ndtgpu_status match_persistent_host(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                           double *T16, size_t n_pairs, const NdtMatchParamsDev &p, const double *Q36,
                                           ndtgpu_match_result *results, hipStream_t st, const MatchKnobs &knobs,
                                           const uint32_t *feat_off = nullptr, const double *feat_cells = nullptr)
{
    const size_t bT = n_pairs * 16 * sizeof(double), bR = n_pairs * sizeof(ndtgpu_match_result), bI = n_pairs * sizeof(uint32_t);
    const size_t bQ = Q36 ? n_pairs * 36 * sizeof(double) : 0;
    const size_t bFo = feat_off ? (n_pairs + 1) * sizeof(uint32_t) : 0, bFc = feat_off ? (size_t)feat_off[n_pairs] * 18 * sizeof(double) : 0;
    StageLayout L;
    const size_t off_T = L.take(bT), off_R = L.take(bR), off_ti = L.take(bI), off_si = L.take(bI), off_Q = L.take(bQ),
                 off_Fo = L.take(bFo), off_Fc = L.take(bFc);
    ndtgpu_status rc = ts->ensure_stage(off_Fc + bFc);
    if (rc != NDTGPU_OK) return rc;
    char *base = ts->stage.get();
    HIP_TRY(hipMemcpyAsync(base + off_T, T16, bT, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_ti, tidx, bI, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_si, sidx, bI, hipMemcpyHostToDevice, st));
    if (Q36) HIP_TRY(hipMemcpyAsync(base + off_Q, Q36, bQ, hipMemcpyHostToDevice, st));
    if (feat_off) {
        HIP_TRY(hipMemcpyAsync(base + off_Fo, feat_off, bFo, hipMemcpyHostToDevice, st));
        if (bFc) HIP_TRY(hipMemcpyAsync(base + off_Fc, feat_cells, bFc, hipMemcpyHostToDevice, st));
    }
    rc = match_device_core(ts, (const uint32_t *)(base + off_ti), ss, (const uint32_t *)(base + off_si), (double *)(base + off_T),
                           n_pairs, p, (ndtgpu_match_result *)(base + off_R), Q36 ? (const double *)(base + off_Q) : nullptr, st,
                           feat_off ? (const unsigned *)(base + off_Fo) : nullptr, feat_off ? (const double *)(base + off_Fc) : nullptr,
                           -1, nullptr, nullptr, &knobs);
    if (rc != NDTGPU_OK) return rc;
    unsigned aborted = 0;
    HIP_TRY(hipMemcpyAsync(T16, base + off_T, bT, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(results, base + off_R, bR, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&aborted, ts->work.get() + ndt_match_abort_offset(), sizeof aborted, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (aborted) return fail(NDTGPU_ERR_HIP, "match: the persistent matcher gave up (a wave found no work for ~1 s)");
    return NDTGPU_OK;
}

// Small batches: the host runs the Newton / More-Thuente state machine (the same ndt_solver.h code the
// persistent kernel runs on the device) and every derivative evaluation is one multi-workgroup kernel,
// so a single registration uses the whole chip instead of one CU.  Used below NDTGPU_HOST_LOOP_MAX pairs.
static ndtgpu_status match_host_driven(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                       double *T16, size_t n_pairs, const NdtMatchParamsDev &p, const double *Q36,
                                       ndtgpu_match_result *results, hipStream_t st, const MatchKnobs &knobs)
{
    const unsigned max_groups = 128;
    ndtgpu_status rc = ts->ensure_stage(max_groups * 32 * sizeof(double));
    if (rc != NDTGPU_OK) return rc;
    double *partials_dev = (double *)ts->stage.get();
    std::vector<double> partials(max_groups * 32);
    for (size_t k = 0; k < n_pairs; k++) {
        long long terms_g = 0, terms_h = 0;
        NdtMapCounters cs, ct;
        HIP_TRY(hipMemcpy(&cs, ss->v.counters + sidx[k], sizeof cs, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&ct, ts->v.counters + tidx[k], sizeof ct, hipMemcpyDeviceToHost));
        unsigned groups = (cs.n_cells + 511u) / 512u;
        if (groups < 1) groups = 1;
        if (groups > max_groups) groups = max_groups;
        ts->ev[3].clear();
        MatchState ms;
        NewtonWs ws;
        match_state_init(ms, T16 + 16 * k, p, Q36 ? Q36 + 36 * k : nullptr);
        while (!ms.done) {
            hipError_t e = ndt_launch_eval(ts->v, tidx[k], ss->v, sidx[k], ms.Teval, p.n_neighbours, ms.with_h, p.lfd1,
                                           p.lfd2, groups, partials_dev, st);
            if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "match: eval launch", e);
            HIP_TRY(hipMemcpyAsync(partials.data(), partials_dev, groups * 32 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            double sums[29];
            for (int q = 0; q < 29; q++) {
                double s = 0;
                for (unsigned g = 0; g < groups; g++) s += partials[g * 32 + q];
                sums[q] = s;
            }
            if (ms.with_h) terms_h += (long long)sums[28]; else terms_g += (long long)sums[28];
            if (knobs.trace)      // (debugging aid of the host-driven loop: one line per evaluation)
                fprintf(stderr, "hip eval with_h %d phase %d itr %d nfev %d score %.17g g %.9e %.9e %.9e\n", ms.with_h, ms.phase, ms.itr_ctr, ms.mt.nfev,
                        sums[0], sums[1], sums[2], sums[6]);
            match_state_step(ms, sums, p, ws);
        }
        NdtMatchResultDev o;
        match_state_result(ms, T16 + 16 * k, o);
        o.n_source = (int32_t)cs.n_cells;
        o.n_target = (int32_t)ct.n_cells;
        o.cycles_eval = 0;
        o.cycles_solver = 0;
        o.pair_terms_g = terms_g;
        o.pair_terms_h = terms_h;
        memcpy(&results[k], &o, sizeof o);
    }
    return NDTGPU_OK;
}

// Host-pointer batches that cannot fill the chip with one workgroup per registration (the reference's one-link-at-a-time
// call is the extreme case): ONE grid-barrier or task-pool launch, synchronous.
static ndtgpu_status match_coop_host(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                     double *T16, size_t n_pairs, const NdtMatchParamsDev &p, const double *Q36,
                                     ndtgpu_match_result *results, hipStream_t st, const MatchKnobs &knobs, const CoopPlan &pl)
{
    // One pinned host block mirrors the device staging block [T | results | target idx | source idx | Q], followed by the
    // control words read back at the end: one copy in, the launch, one copy of poses + results and the control words out,
    // ONE wait.  (Round 2: eight pageable copies and four waits -- a third of a single-pair call.)
    const size_t bT = n_pairs * 16 * sizeof(double), bR = n_pairs * sizeof(ndtgpu_match_result), bI = n_pairs * sizeof(uint32_t);
    const size_t bQ = Q36 ? n_pairs * 36 * sizeof(double) : 0, bCtrl = n_pairs * 16 + n_pairs * sizeof(unsigned);
    StageLayout L;
    const size_t off_T = L.take(bT), off_R = L.take(bR), off_ti = L.take(bI), off_si = L.take(bI), off_Q = L.take(bQ);
    const size_t total = off_Q + bQ, off_ctrl = L.take(bCtrl);
    ndtgpu_status rc = ts->ensure_stage(total);
    if (rc != NDTGPU_OK) return rc;
    std::vector<double> Tin(T16, T16 + 16 * n_pairs);          // (the poses as they came in: a registration that has to be re-run)
    char *pin;                        // (the pinned block: grown under the lock, read after it)
    std::vector<size_t> bad;          // registrations the launch gave up on
    {
        std::lock_guard<std::mutex> coop_lock(g_coop_mutex);
        CoopOrder &order = coop_order();
        rc = ts->ensure_coop(n_pairs * pl.stride + (pl.pool ? ndt_match_pool_ctrl_bytes() : 0), order);
        if (rc != NDTGPU_OK) return rc;
        rc = ts->ensure_pin(off_ctrl + bCtrl, order);
        if (rc != NDTGPU_OK) return rc;
        pin = ts->pin.get();
        memcpy(pin + off_T, T16, bT);
        memcpy(pin + off_ti, tidx, bI);
        memcpy(pin + off_si, sidx, bI);
        if (Q36) memcpy(pin + off_Q, Q36, bQ);
        // The grid-barrier kernel (up to eight registrations) reads poses, indices and Tcov from the pinned block where it is and
        // writes poses and results there: 16 doubles per workgroup over the link at the start, 192 bytes back at the end, instead of
        // two copies on the stream (~6 us each) around a 0.2 ms launch.  The host then watches one word per registration in that
        // block, which workgroup 0 sets behind pose and result, instead of waiting for the stream (the runtime's completion signal
        // costs ~8 us more than the store takes to arrive); the next launch of this kind is ordered behind the kernel's end by its
        // event, like any asynchronous one.  The task pool keeps its staging copies and waits for the stream.
        const bool direct = !pl.pool;
        unsigned *ctrl = reinterpret_cast<unsigned *>(pin + off_ctrl), *flags = ctrl + 4 * n_pairs;
        char *base = direct ? pin : ts->stage.get();
        if (direct) for (size_t k = 0; k < n_pairs; k++) __atomic_store_n(&flags[k], 0u, __ATOMIC_RELEASE);
        else HIP_TRY(hipMemcpyAsync(base, pin, total, hipMemcpyHostToDevice, st));
        // only blocks this set has not seen finish cleanly at this stride are cleared
        const bool clear = ts->coop_clean_stride != pl.stride || ts->coop_clean_upto < n_pairs;
        const size_t clean_before = clear ? n_pairs : ts->coop_clean_upto;
        ts->coop_clean_stride = pl.stride;
        ts->coop_clean_upto = 0;                                // (until this call is known to have ended cleanly)
        rc = coop_enqueue(ts, ss, (const uint32_t *)(base + off_ti), (const uint32_t *)(base + off_si), (double *)(base + off_T),
                          reinterpret_cast<NdtMatchResultDev *>(base + off_R), Q36 ? (const double *)(base + off_Q) : nullptr,
                          n_pairs, p, pl, clear, direct, order, st, direct ? flags : nullptr);
        if (rc != NDTGPU_OK) return rc;
        if (!direct) HIP_TRY(hipMemcpyAsync(pin, base, off_R + bR, hipMemcpyDeviceToHost, st));         // poses + results
        bool seen = direct;
        if (direct) {
            const auto t_poll = std::chrono::steady_clock::now();
            for (size_t k = 0; k < n_pairs && seen; k++) {
                unsigned spins = 0;
                while (__atomic_load_n(&flags[k], __ATOMIC_ACQUIRE) == 0u) {
                    __builtin_ia32_pause();
                    if ((++spins & 0xFFFFu) == 0u && std::chrono::steady_clock::now() - t_poll > std::chrono::seconds(2)) { seen = false; break; }
                }
            }
        }
        if (!seen) {
            HIP_TRY(hipStreamSynchronize(st));
            order.valid = false;          // (this stream waited for the last asynchronous launch, and is drained now)
        }
        // a registration the launch gave up on reports exit code -4 (both kernels)
        const ndtgpu_match_result *hr = reinterpret_cast<const ndtgpu_match_result *>(pin + off_R);
        for (size_t k = 0; k < n_pairs; k++) {
            ctrl[4 * k] = 0u;
            ctrl[4 * k + 1] = hr[k].exit_code == -4 ? 1u : 0u;
            if (ctrl[4 * k + 1]) bad.push_back(k);
        }
        ts->coop_clean_upto = bad.empty() ? clean_before : 0;
    }
    ts->ev[3].clear();          // (ndtgpu_last_kernel_ms(1): no persistent launch was timed by this call)
    memcpy(T16, pin + off_T, bT);
    memcpy(results, pin + off_R, bR);
    // A registration whose grid barrier gave up (it cannot with a co-resident grid; the bounded spin stays as a guard
    // against a foreign kernel holding CUs) is run again on the persistent kernel: the call does not fail.
    if (!bad.empty()) {
        std::vector<double> bT16(16 * bad.size()), bQ36(Q36 ? 36 * bad.size() : 0);
        std::vector<uint32_t> bt(bad.size()), bs(bad.size());
        std::vector<ndtgpu_match_result> br(bad.size());
        for (size_t j = 0; j < bad.size(); j++) {
            memcpy(&bT16[16 * j], &Tin[16 * bad[j]], 16 * sizeof(double));
            if (Q36) memcpy(&bQ36[36 * j], Q36 + 36 * bad[j], 36 * sizeof(double));
            bt[j] = tidx[bad[j]];
            bs[j] = sidx[bad[j]];
        }
        rc = match_persistent_host(ts, bt.data(), ss, bs.data(), bT16.data(), bad.size(), p, Q36 ? bQ36.data() : nullptr, br.data(),
                                   st, knobs);
        if (rc != NDTGPU_OK) return rc;
        for (size_t j = 0; j < bad.size(); j++) {
            memcpy(T16 + 16 * bad[j], &bT16[16 * j], 16 * sizeof(double));
            results[bad[j]] = br[j];
        }
    }
    return NDTGPU_OK;
}

// The host-pointer entries: validate, choose, run.
static ndtgpu_status match_batch_common(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                        double *T16, size_t n_pairs, const ndtgpu_match_params *prm, const double *Q36,
                                        int fusion_flags, ndtgpu_match_result *results, ndtgpu_stream stream)
{
    if (!ts || !ss || (n_pairs && (!tidx || !sidx || !T16 || !results)))
        return fail(NDTGPU_ERR_INVALID, "match_batch: bad argument");
    if (n_pairs == 0) return NDTGPU_OK;
    for (size_t k = 0; k < n_pairs; k++)
        if (tidx[k] >= ts->n_maps || sidx[k] >= ss->n_maps) return fail(NDTGPU_ERR_INVALID, "match_batch: map index");
    hipStream_t st = (hipStream_t)stream;
    // builds on other streams must have finished before the maps are read (a build on THIS stream is ordered by the stream: the
    // host stages the call while it runs -- a third of the build of a single pair, tools/latency_probe.py)
    { ndtgpu_status wrc_ = ts->wait_all_on(st); if (wrc_ != NDTGPU_OK) return wrc_; }
    { ndtgpu_status wrc_ = ss->wait_all_on(st); if (wrc_ != NDTGPU_OK) return wrc_; }
    NdtMatchParamsDev p;
    ndtgpu_status rc = match_params_dev(prm, fusion_flags, p);
    if (rc != NDTGPU_OK) return rc;
    const MatchKnobs knobs = match_knobs();
    CoopPlan pl;
    switch (choose_form(MatchEntry::host, n_pairs, ss, p, knobs, st, false, pl)) {
    case MatchForm::host_loop: return match_host_driven(ts, tidx, ss, sidx, T16, n_pairs, p, Q36, results, st, knobs);
    case MatchForm::grid_barrier:
    case MatchForm::pool: return match_coop_host(ts, tidx, ss, sidx, T16, n_pairs, p, Q36, results, st, knobs, pl);
    case MatchForm::persistent: break;
    }
    { ndtgpu_status wrc_ = ts->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    { ndtgpu_status wrc_ = ss->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    return match_persistent_host(ts, tidx, ss, sidx, T16, n_pairs, p, Q36, results, st, knobs);
}

bool invert6(const double *A, double *inv)
{
    double a[6][12];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) { a[i][j] = A[i * 6 + j]; a[i][6 + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < 6; c++) {
        int piv = c;
        for (int r = c + 1; r < 6; r++)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < 12; j++) std::swap(a[c][j], a[piv][j]);
        double d = a[c][c];
        for (int j = 0; j < 12; j++) a[c][j] /= d;
        for (int r = 0; r < 6; r++) {
            if (r == c) continue;
            double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 12; j++) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) inv[i * 6 + j] = a[i][6 + j];
    return true;
}

extern "C" {

ndtgpu_status ndtgpu_derivatives(ndtgpu_mapset *t, size_t tmap, const double *src_mean3, const double *src_cov9,
                                 size_t m, int n_neighbours, int compute_hessian, double lfd1, double lfd2,
                                 double *score, double g[6], double H[36])
{
    if (!t || tmap >= t->n_maps || (m && (!src_mean3 || !src_cov9)) || !score || !g || n_neighbours < 0 ||
        n_neighbours > 3)
        return fail(NDTGPU_ERR_INVALID, "derivatives: bad argument");
    std::vector<NdtCell> cells;
    pack_cells(t->v.grid, nullptr, src_mean3, src_cov9, m, false, cells);
    size_t bytes = cells.size() * sizeof(NdtCell) + 32 * sizeof(double);
    ndtgpu_status rc = t->ensure_stage(bytes);
    if (rc != NDTGPU_OK) return rc;
    double *out_dev = (double *)t->stage.get();
    NdtCell *src_dev = (NdtCell *)(t->stage.get() + 32 * sizeof(double));
    { ndtgpu_status wrc_ = t->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    if (!cells.empty()) HIP_TRY(hipMemcpy(src_dev, cells.data(), cells.size() * sizeof(NdtCell), hipMemcpyHostToDevice));
    hipError_t e = ndt_launch_derivatives(t->v, tmap, src_dev, cells.size(), n_neighbours, compute_hessian, lfd1, lfd2,
                                          out_dev, nullptr);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "derivatives: launch", e);
    double out[28];
    HIP_TRY(hipMemcpy(out, out_dev, sizeof out, hipMemcpyDeviceToHost));
    *score = out[0];
    for (int a = 0; a < 6; a++) g[a] = out[1 + a];
    if (compute_hessian && H) {
        int o = 7;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++) { H[a * 6 + b] = out[o]; H[b * 6 + a] = out[o]; o++; }
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_match_batch_device(ndtgpu_mapset *ts, const uint32_t *tidx_dev, ndtgpu_mapset *ss,
                                        const uint32_t *sidx_dev, double *T16_dev, size_t n_pairs,
                                        const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev,
                                        ndtgpu_stream stream)
{
    return match_batch_device_ex(ts, tidx_dev, ss, sidx_dev, T16_dev, n_pairs, prm, results_dev, stream, -1, nullptr, nullptr, nullptr);
}

ndtgpu_status ndtgpu_match_aborted(ndtgpu_mapset *ts, int *aborted)
{
    if (!ts || !aborted) return fail(NDTGPU_ERR_INVALID, "match_aborted: bad argument");
    *aborted = 0;
    if (!ts->work.get()) return NDTGPU_OK;                     // no persistent launch has used this set as a target
    { ndtgpu_status wrc_ = ts->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    unsigned w = 0;
    HIP_TRY(hipMemcpy(&w, ts->work.get() + ndt_match_abort_offset(), sizeof w, hipMemcpyDeviceToHost));
    *aborted = w != 0u;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_match_batch(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                 double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                 ndtgpu_match_result *results, ndtgpu_stream stream)
{
    return match_batch_common(ts, tidx, ss, sidx, T16, n_pairs, prm, nullptr, 0, results, stream);
}

ndtgpu_status ndtgpu_match_fusion_batch(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                        double *T16, const double *Tcov36, size_t n_pairs,
                                        const ndtgpu_match_params *prm, int use_soft_constraints,
                                        ndtgpu_match_result *results, ndtgpu_stream stream)
{
    if (use_soft_constraints < 0 || use_soft_constraints > 3)
        return fail(NDTGPU_ERR_INVALID, "match_fusion: use_soft_constraints is a 2-bit set (bit 0 useSoftConstraints, bit 1 useTikhonovRegularization)");
    const int flags = use_soft_constraints;       // bit 0 useSoftConstraints, bit 1 useTikhonovRegularization
    if (!flags) return match_batch_common(ts, tidx, ss, sidx, T16, n_pairs, prm, nullptr, 0, results, stream);
    if (!Tcov36) return fail(NDTGPU_ERR_INVALID, "match_fusion: Tcov missing");
    std::vector<double> Q(36 * n_pairs);
    for (size_t k = 0; k < n_pairs; k++)
        if (!invert6(Tcov36 + 36 * k, Q.data() + 36 * k)) return fail(NDTGPU_ERR_INVALID, "match_fusion: singular Tcov");
    return match_batch_common(ts, tidx, ss, sidx, T16, n_pairs, prm, Q.data(), flags, results, stream);
}

ndtgpu_status ndtgpu_match_fusion_feat_batch(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                             double *T16, const double *Tcov36, const ndtgpu_feat_pairs *feat, size_t n_pairs,
                                             const ndtgpu_match_params *prm, int flags, ndtgpu_match_result *results,
                                             ndtgpu_stream stream)
{
    if (flags < 0 || flags > 7) return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: flags is a 3-bit set");
    if (!feat || !feat->offsets)   // no feature maps: bit 2 (the joint line search of the feature maps) has nothing to act on
        return ndtgpu_match_fusion_batch(ts, tidx, ss, sidx, T16, Tcov36, n_pairs, prm, flags & 3, results, stream);
    if (!ts || !ss || (n_pairs && (!tidx || !sidx || !T16 || !results)))
        return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: bad argument");
    if (n_pairs == 0) return NDTGPU_OK;
    for (size_t k = 0; k < n_pairs; k++) {
        if (tidx[k] >= ts->n_maps || sidx[k] >= ss->n_maps) return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: map index");
        if (feat->offsets[k + 1] < feat->offsets[k]) return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: offsets must not decrease");
        if (feat->offsets[k + 1] - feat->offsets[k] > 64u)
            return fail(NDTGPU_ERR_CAPACITY, "match_fusion_feat: at most 64 correspondences per registration");
    }
    const size_t total = feat->offsets[n_pairs];
    if (total && (!feat->src_mean || !feat->src_cov || !feat->tgt_mean || !feat->tgt_cov))
        return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: cell arrays missing");
    std::vector<double> Q;
    if (flags & 3) {
        if (!Tcov36) return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: Tcov missing");
        Q.resize(36 * n_pairs);
        for (size_t k = 0; k < n_pairs; k++)
            if (!invert6(Tcov36 + 36 * k, Q.data() + 36 * k)) return fail(NDTGPU_ERR_INVALID, "match_fusion_feat: singular Tcov");
    }
    std::vector<double> cells(total * 18);
    for (size_t i = 0; i < total; i++) {
        double *c = cells.data() + 18 * i;
        for (int a = 0; a < 3; a++) { c[a] = feat->src_mean[3 * i + a]; c[9 + a] = feat->tgt_mean[3 * i + a]; }
        for (int a = 0; a < 6; a++) { c[3 + a] = feat->src_cov[6 * i + a]; c[12 + a] = feat->tgt_cov[6 * i + a]; }
    }
    hipStream_t st = (hipStream_t)stream;
    { ndtgpu_status wrc_ = ts->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    { ndtgpu_status wrc_ = ss->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    // (bit 2 of the flags, step_control_fusion, selects lineSearchMTFusion when bit 0 is clear: fusion.h:1004)
    NdtMatchParamsDev p;
    ndtgpu_status rc = match_params_dev(prm, flags, p);
    if (rc != NDTGPU_OK) return rc;
    // (always the persistent matcher: the feature sums are evaluated inside its solver step)
    return match_persistent_host(ts, tidx, ss, sidx, T16, n_pairs, p, Q.empty() ? nullptr : Q.data(), results, st, match_knobs(),
                                 feat->offsets, cells.data());
}

ndtgpu_status ndtgpu_covariance_batch(ndtgpu_mapset *ts, const uint32_t *tidx, ndtgpu_mapset *ss, const uint32_t *sidx,
                                      const double *T16, size_t n_links, const ndtgpu_match_params *prm, int mode,
                                      double *cov36, int32_t *singular, ndtgpu_stream stream)
{
    if (!ts || !ss || (n_links && (!tidx || !sidx || !T16 || !cov36)) || mode < 0 || mode > 1)
        return fail(NDTGPU_ERR_INVALID, "covariance: bad argument");
    if (n_links == 0) return NDTGPU_OK;
    for (size_t k = 0; k < n_links; k++)
        if (tidx[k] >= ts->n_maps || sidx[k] >= ss->n_maps) return fail(NDTGPU_ERR_INVALID, "covariance: map index");
    NdtMatchParamsDev p = to_dev(prm);
    if (p.n_neighbours < 0 || p.n_neighbours > 3) return fail(NDTGPU_ERR_INVALID, "covariance: n_neighbours must be 0..3");
    hipStream_t st = (hipStream_t)stream;
    { ndtgpu_status wrc_ = ts->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    { ndtgpu_status wrc_ = ss->wait_all(); if (wrc_ != NDTGPU_OK) return wrc_; }
    const size_t bT = n_links * 16 * sizeof(double), bI = n_links * sizeof(uint32_t), bC = n_links * 36 * sizeof(double);
    StageLayout L;
    const size_t off_T = L.take(bT), off_t = L.take(bI), off_s = L.take(bI), off_c = L.take(bC), off_f = L.take(n_links * sizeof(int));
    ndtgpu_status rc = ts->ensure_stage(off_f + n_links * sizeof(int));
    if (rc != NDTGPU_OK) return rc;
    char *base = ts->stage.get();
    HIP_TRY(hipMemcpyAsync(base + off_T, T16, bT, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_t, tidx, bI, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + off_s, sidx, bI, hipMemcpyHostToDevice, st));
    hipError_t e = ndt_launch_covariance(ts->v, (const uint32_t *)(base + off_t), ss->v, (const uint32_t *)(base + off_s),
                                         (const double *)(base + off_T), n_links, p.n_neighbours, p.lfd1, p.lfd2, mode,
                                         (double *)(base + off_c), (int *)(base + off_f), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "covariance: launch", e);
    HIP_TRY(hipMemcpyAsync(cov36, base + off_c, bC, hipMemcpyDeviceToHost, st));
    if (singular) HIP_TRY(hipMemcpyAsync(singular, base + off_f, n_links * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_match_d2d(ndtgpu_mapset *ts, size_t tmap, ndtgpu_mapset *ss, size_t smap, double T16[16],
                               const ndtgpu_match_params *prm, ndtgpu_match_result *result)
{
    uint32_t ti = (uint32_t)tmap, si = (uint32_t)smap;
    return ndtgpu_match_batch(ts, &ti, ss, &si, T16, 1, prm, result, nullptr);
}

}  // extern "C"
