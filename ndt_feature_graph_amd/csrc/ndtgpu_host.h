// ndtgpu_host.h -- what the C-ABI sources share (ndtgpu_api.hip: map sets; ndtgpu_matcher.hip; ndtgpu_registrar.hip;
// ndtgpu_fuser_bank.hip; every ndtgpu_<subsystem>.hip): error reporting, the skeleton of a handle's create and destroy, the
// staging of a synchronous host form, the upload of a search's lattice tables, the map set handle and the helpers one of them
// defines for the others.  Host side only and internal: not installed, and nothing declared here is exported from libndtgpu.so.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndtgpu_resource.h"
#include "ndt_math.h"
#include "ndt_solver.h"
#include "ndt_pose.h"
#include "ndt_lattice.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;      // (ndtgpu_api.hip: what ndtgpu_last_error returns)

inline ndtgpu_status fail(ndtgpu_status s, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return s;
}

// ... with the message "<who>: <what>": who is the entry's name
inline ndtgpu_status fail_in(ndtgpu_status s, const char *who, const char *what)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s", who, what);
    g_err = buf;
    return s;
}

// the caller's parameters, or the defaults where it passed NULL
template <class P>
inline P params_or_default(const P *prm, void (*defaults)(P *))
{
    P p;
    defaults(&p);
    if (prm) p = *prm;
    return p;
}

#define HIP_TRY(expr)                                                       \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) return fail(NDTGPU_ERR_HIP, #expr, _e);       \
    } while (0)

inline bool have_device()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

inline int device_cus()
{
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
        n_cu = 256;
    return n_cu;
}

// An experiment's environment variable overrides a field the caller LEFT AT ITS DEFAULT (0 / auto); what a caller sets wins.
inline int env_int(const char *name, int fallback)
{
    const char *e = getenv(name);
    return e ? atoi(e) : fallback;
}

struct CoopOrder;     // (ndtgpu_matcher.hip: the last grid-barrier launch of a device)

struct ndtgpu_mapset {
    // what the kernels receive: filled from the owners below (create, enable_occupancy).  Stays the FIRST member: the debug
    // entries of ndt_match.hip read a handle as its view
    NdtSetView v{};
    DeviceBuffer<uint2> rankmap;
    DeviceBuffer<int32_t> wtable;
    DeviceBuffer<uint32_t> bitmap, acc_slot, rank_agg, cell_sel;
    DeviceBuffer<NdtCell> cells, cells_alt;
    DeviceBuffer<NdtAcc> acc;
    DeviceBuffer<NdtMapCounters> counters;
    DeviceBuffer<double> centres;
    DeviceBuffer<float> occ;
    DeviceBuffer<long long> occ_delta;
    DeviceBuffer<unsigned char> occ_touched;
    size_t n_maps = 0;
    std::vector<double> centres_host;
    std::vector<unsigned char> nice_host;   // per map: fp32 cell offsets are exact (ndt_grid_is_nice)
    int nice_range(size_t first, size_t count) const
    {
        for (size_t m = first; m < first + count; m++)
            if (!nice_host[m]) return 0;
        return 1;
    }
    // Streams that may still hold work on this set (writers: builds, unpack, add_cloud; readers: matcher launches): one fence
    // per recently used stream, recorded AFTER the launch.  The host-synchronous entries wait for these fences -- not for
    // stream handles, which the caller may have destroyed since, and not only for the last writer (a matcher that still reads
    // the maps on another stream is waited for as well).
    struct StreamMark { hipStream_t st; Fence ev; };
    std::vector<StreamMark> marks;
    bool null_stream_used = false;       // the null stream needs no event: its handle is always valid (and an event record
                                         // costs the reference's one-pair-at-a-time call shape ~10 us of its 0.37 ms)
    ndtgpu_status touch(hipStream_t st)
    {
        if (st == nullptr) { null_stream_used = true; return NDTGPU_OK; }
        for (StreamMark &m : marks)
            if (m.st == st) { HIP_TRY(m.ev.record(st)); return NDTGPU_OK; }
        if (marks.size() >= 8) {                 // many streams over time: retire the oldest entry once its work is done
            HIP_TRY(marks.front().ev.sync());
            marks.erase(marks.begin());
        }
        StreamMark m{st, {}};
        HIP_TRY(m.ev.record(st));
        marks.push_back(std::move(m));
        return NDTGPU_OK;
    }
    // ... for work that is about to be enqueued on `st`: what was recorded on `st` itself is ordered by the stream
    ndtgpu_status wait_all_on(hipStream_t st)
    {
        if (null_stream_used && st != nullptr) { HIP_TRY(hipStreamSynchronize(nullptr)); null_stream_used = false; }
        for (StreamMark &m : marks)
            if (m.st != st) HIP_TRY(m.ev.sync());
        return NDTGPU_OK;
    }
    ndtgpu_status wait_all()
    {
        if (null_stream_used) { HIP_TRY(hipStreamSynchronize(nullptr)); null_stream_used = false; }
        for (StreamMark &m : marks) HIP_TRY(m.ev.sync());
        return NDTGPU_OK;
    }
    // staging buffers reused across calls
    DeviceBuffer<char> stage;
    Fence stage_free;                    // recorded after the last kernel that reads the staged clouds of a host-cloud call
    ndtgpu_status ensure_stage(size_t bytes)
    {
        if (bytes <= stage.capacity()) return NDTGPU_OK;
        HIP_TRY(stage_free.sync());      // (those kernels may still read the block that is replaced)
        stage_free.clear();
        HIP_TRY(stage.reserve(bytes));
        return NDTGPU_OK;
    }
    DeviceBuffer<double> origins;
    Fence origins_used;                  // recorded after the last launch that reads `origins` (it may be on another stream)
    // room for `n` doubles in `origins`, ordered behind its last reader: `st` waits for that launch before the buffer is
    // overwritten (or the host does, before it is replaced)
    ndtgpu_status origins_reserve(size_t n, hipStream_t st)
    {
        if (origins.capacity() < n) HIP_TRY(origins.reserve(n, origins_used));
        else HIP_TRY(origins_used.order(st));
        return NDTGPU_OK;
    }
    // workgroups the persistent matcher launches with this set as target get at most (0: one per CU).  The registrar keeps its
    // matcher launches on part of the chip: the rest stays free for the next sub-batch's builds while a launch runs
    unsigned match_groups = 0;
    // matcher work area: ticket counters, parked list, parked solver states (match_device_core)
    DeviceBuffer<char> work;
    Fence work_used;                     // recorded after the last launch that uses `work`
    hipStream_t work_stream = nullptr;   // ... the stream it was recorded on
    // profiling hooks: [0,1] bracket the build kernel, [2,3] the match kernel (timed events, made by ndtgpu_profiling_enable;
    // ndtgpu_last_kernel_ms(which) reads a bracket whose end, ev[2 which + 1], is valid)
    bool profiling = false;
    bool profile_span = false;         // a chunked host build is ONE bracket: the chunks' launches do not re-record the events
    Fence ev[4];
    // work area of the grid-barrier matcher (a control block + partial sums per registration); its kernels leave the
    // control blocks zeroed, so a call only clears what it cannot know to be clean
    DeviceBuffer<char> coop_work;
    size_t coop_clean_stride = 0, coop_clean_upto = 0;
    // (both defined in ndtgpu_matcher.hip: a block that grows is freed once the device's last grid-barrier launch, which may
    //  still use it, has ended)
    ndtgpu_status ensure_coop(size_t bytes, const CoopOrder &last);
    // pinned host mirror of small staging blocks (poses, indices, results of a host-pointer matcher call): copies from /
    // to pinned memory are truly asynchronous and skip the runtime's own bounce buffer
    PinnedBuffer<char> pin;
    ndtgpu_status ensure_pin(size_t bytes, const CoopOrder &last);
    // Host clouds (the reference's call sites hand over pcl::PointCloud on the host): a ring of pinned slots that host
    // threads fill from the caller's pageable memory while earlier slots travel to the device and earlier chunks of
    // maps are being built (stage_host_clouds).  The copies run on a stream of their own.
    static constexpr int HOST_SLOTS = 6;
    static constexpr size_t HOST_SLOT_BYTES = 16u << 20;
    PinnedBuffer<char> host_ring[HOST_SLOTS];
    Fence host_ev[HOST_SLOTS];           // recorded behind a slot's copy to the device; valid: the slot may still be in flight
    // (the streams last: ndtgpu_resource.h)
    Stream host_copy_stream;
    Stream host_build_stream;            // the synchronous host-cloud entries build on a stream of their own (no device-wide wait)
    ndtgpu_status ensure_host_build_stream()
    {
        if (!host_build_stream.get()) HIP_TRY(host_build_stream.create(hipStreamNonBlocking));
        return NDTGPU_OK;
    }
    ndtgpu_status ensure_host_ring()
    {
        if (host_copy_stream.get()) return NDTGPU_OK;
        for (int k = 0; k < HOST_SLOTS; k++) {
            HIP_TRY(host_ring[k].alloc(HOST_SLOT_BYTES));
            HIP_TRY(host_ev[k].create());
        }
        HIP_TRY(stage_free.create());
        HIP_TRY(host_copy_stream.create(hipStreamNonBlocking));
        return NDTGPU_OK;
    }
};

// a map set that another handle owns (registrar, fuser bank, multires, MCL)
struct MapsetDestroy { void operator()(ndtgpu_mapset *s) const { (void)ndtgpu_mapset_destroy(s); } };
using MapsetOwner = std::unique_ptr<ndtgpu_mapset, MapsetDestroy>;
inline ndtgpu_status mapset_create_owned(const ndtgpu_grid_params *grid, size_t n_maps, MapsetOwner &out)
{
    ndtgpu_mapset *s = nullptr;
    const ndtgpu_status rc = ndtgpu_mapset_create(grid, n_maps, &s);
    out.reset(s);
    return rc;
}

// In a create function: a HIP call that fails deletes the half-built handle and returns `status` with the message `what`.
#define CREATE_TRY(handle, status, what, expr)                              \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) { delete (handle); return fail((status), (what), _e); } \
    } while (0)

// The tail of every create, behind the entry's own argument checks: a handle of type H, or why there is none.  The caller fills
// it (TRY / CREATE_TRY over its own buffers, then used.create() and hst.create() last) and hands it out.
template <class H>
inline ndtgpu_status handle_new(const char *who, H *&h)
{
    h = nullptr;
    if (!have_device()) return fail_in(NDTGPU_ERR_NO_DEVICE, who, "no HIP device");
    h = new (std::nothrow) H();
    return h ? NDTGPU_OK : fail_in(NDTGPU_ERR_ALLOC, who, "host alloc");
}

// ... and every destroy, of a handle whose calls record `used` behind their last launch
template <class H>
inline ndtgpu_status handle_destroy(H *h, const char *who)
{
    if (!h) return fail_in(NDTGPU_ERR_INVALID, who, "null");
    (void)h->used.sync();                  // (the last call may have run on a stream of the caller's)
    delete h;
    return NDTGPU_OK;
}

// Consecutive regions of one staging block, each on a 256-byte boundary: take(bytes) returns where the region starts; `at` is
// where the next one would.
struct StageLayout {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t o = at;
        at = (at + bytes + 255) & ~(size_t)255;
        return o;
    }
};

// The staging of a synchronous host form: one device block and its pinned mirror, the `in` regions (host -> device in one copy
// before the work) in front of the `outl` regions (device -> host in one copy behind it).  It owns neither the stream nor the
// fence: those are the handle's `hst` and `used`, declared behind this (ndtgpu_resource.h: the stream goes first).  A host form
//   lays out its regions in two StageLayouts, open()s with them, fills in_host(), upload()s, calls its _device form on h->hst
//   with in_dev() / out_dev() pointers, finish()es and reads out_host().
// HIP_TRY reports the text of its expression: the names below are the ones those messages carry.
struct HostStage {
    DeviceBuffer<char> stage;
    PinnedBuffer<char> pin;
    StageLayout in, outl;                  // of the call in progress

    // room for the call's regions, once the previous call's work has ended (the blocks may be replaced, and are overwritten)
    template <class H>
    ndtgpu_status open(H *h, const char *who, const StageLayout &in_regions, const StageLayout &out_regions)
    {
        in = in_regions;
        outl = out_regions;
        HIP_TRY(h->used.sync());
        const size_t bytes = in.at + outl.at;
        if (stage.reserve(bytes) != hipSuccess || pin.reserve(bytes) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "staging buffers");
        return NDTGPU_OK;
    }
    char *in_host(size_t o) const { return pin.get() + o; }
    char *in_dev(size_t o) const { return stage.get() + o; }
    char *out_host(size_t o) const { return pin.get() + in.at + o; }
    char *out_dev(size_t o) const { return stage.get() + in.at + o; }
    ndtgpu_status upload(hipStream_t st)
    {
        char *pin = this->pin.get(), *dev = stage.get();
        HIP_TRY(hipMemcpyAsync(dev, pin, in.at, hipMemcpyHostToDevice, st));
        return NDTGPU_OK;
    }
    // the results back, the fence behind them, and the wait: out_host() is valid on return
    template <class H>
    ndtgpu_status finish(H *h, hipStream_t st)
    {
        char *pin_out = out_host(0), *dev_out = out_dev(0);
        HIP_TRY(hipMemcpyAsync(pin_out, dev_out, outl.at, hipMemcpyDeviceToHost, st));
        HIP_TRY(h->used.record(st));
        HIP_TRY(hipStreamSynchronize(st));
        return NDTGPU_OK;
    }
};

// The lattice tables of a search on the device, xs | ys | cs | sn in one block, and their pinned mirror: made by a handle's first
// search and grown by later ones (csrc/ndt_lattice.h checks what goes in).
struct LatticeTables {
    DeviceBuffer<double> tables;
    PinnedBuffer<double> tables_pin;
    struct Dev { const double *xs, *ys, *cs, *sn; };

    // what every entry that takes the tables checks before it reads its handle
    static ndtgpu_status check(const char *who, const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn,
                               size_t nyaw)
    {
        if (!xs || !ys || !cs || !sn) return fail_in(NDTGPU_ERR_INVALID, who, "null xs, ys, cs or sn");
        const char *bad = ndt_lattice_check_tables(xs, nx, ys, ny, cs, sn, nyaw);
        return bad ? fail_in(NDTGPU_ERR_INVALID, who, bad) : NDTGPU_OK;
    }

    // onto the device on `st`.  The pinned copy is overwritten, so the previous call's upload must have ended (and the blocks may
    // be replaced): the host waits for h->used first
    template <class H>
    ndtgpu_status upload(H *h, const char *who, const double *xs, size_t nx, const double *ys, size_t ny, const double *cs,
                         const double *sn, size_t nyaw, hipStream_t st, Dev &out)
    {
        const size_t n_tab = nx + ny + 2 * nyaw;
        HIP_TRY(h->used.sync());
        if (tables.reserve(n_tab) != hipSuccess || tables_pin.reserve(n_tab) != hipSuccess) return fail_in(NDTGPU_ERR_ALLOC, who, "lattice tables");
        double *tp = tables_pin.get(), *td = tables.get();
        memcpy(tp, xs, nx * sizeof(double));
        memcpy(tp + nx, ys, ny * sizeof(double));
        memcpy(tp + nx + ny, cs, nyaw * sizeof(double));
        memcpy(tp + nx + ny + nyaw, sn, nyaw * sizeof(double));
        HIP_TRY(hipMemcpyAsync(td, tp, n_tab * sizeof(double), hipMemcpyHostToDevice, st));
        out = Dev{td, td + nx, td + nx + ny, td + nx + ny + nyaw};
        return NDTGPU_OK;
    }
};

inline NdtMatchParamsDev to_dev(const ndtgpu_match_params *p)
{
    const ndtgpu_match_params d = params_or_default(p, ndtgpu_default_match_params);
    NdtMatchParamsDev o;
    o.n_neighbours = d.n_neighbours;
    o.itr_max = d.itr_max;
    o.step_control = d.step_control;
    o.dof_mask = d.dof_mask;
    o.use_initial_guess = d.use_initial_guess;
    o.delta_score = d.delta_score;
    o.lfd1 = d.lfd1;
    o.lfd2 = d.lfd2;
    o.fusion_flags = 1;
    return o;
}

// ndtgpu_api.hip
// the build proper; `orig_dev`: per-map range origins already in device memory (or NULL: the grid centres)
ndtgpu_status mapset_build_core(ndtgpu_mapset *s, size_t first, size_t count, const void *xyz_dev, size_t n_points,
                                size_t stride_bytes, size_t map_stride_bytes, double range_limit, const double *orig_dev,
                                const ndtgpu_cell_params *cell, hipStream_t st);
// host-side packing of caller-provided Gaussians into NdtCell records keyed by LazyGrid slot
ndtgpu_status pack_cells(const NdtGrid &g, const double *centre, const double *mean3, const double *cov9, size_t n, bool need_slot,
                         std::vector<NdtCell> &out);

// ndtgpu_matcher.hip
struct MatchKnobs;    // (the matcher's environment switches, read once per call)
// The persistent matcher on device-resident arguments: asynchronous on `stream`.
ndtgpu_status match_device_core(ndtgpu_mapset *ts, const uint32_t *tidx_dev, ndtgpu_mapset *ss, const uint32_t *sidx_dev,
                                double *T16_dev, size_t n_pairs, const NdtMatchParamsDev &p, ndtgpu_match_result *results_dev,
                                const double *Q36_dev, hipStream_t st, const unsigned *feat_off_dev = nullptr,
                                const double *feat_cells_dev = nullptr, int cov_mode = -1, double *cov36_dev = nullptr,
                                int32_t *cov_flags_dev = nullptr, const MatchKnobs *knobs = nullptr);
// ndtgpu_match_batch_device, and with cov_mode >= 0 the registrar's covariance of every pair at its registered pose: the tail of
// the persistent kernel (ndt_match_kernel<.., COV = 1>), or -- grid-barrier / pool batches -- a launch of ndt_covariance_kernel
// behind the match on the same stream and ndt_cov_flags_kernel (T16_save: n_pairs x 16 doubles of device scratch for the initial
// guesses, which the match overwrites).
ndtgpu_status match_batch_device_ex(ndtgpu_mapset *ts, const uint32_t *tidx_dev, ndtgpu_mapset *ss, const uint32_t *sidx_dev,
                                    double *T16_dev, size_t n_pairs, const ndtgpu_match_params *prm,
                                    ndtgpu_match_result *results_dev, ndtgpu_stream stream, int cov_mode, double *cov36_dev,
                                    int32_t *cov_flags_dev, double *T16_save_dev);
// 6x6 inverse by Gauss-Jordan with partial pivoting (Eigen: Tcov.inverse(), fusion.h:845)
bool invert6(const double *A, double *inv);
// the device form of a call's match parameters, checked (every matcher entry, the registrar)
ndtgpu_status match_params_dev(const ndtgpu_match_params *prm, int fusion_flags, NdtMatchParamsDev &p);

// ndtgpu_mcl.hip
// the particle poses (twelve doubles each: rotation row-major, translation) of filters [first, first + count) of a bank, in place,
// with the fence its calls record and the stream of its synchronous entries: what ndtgpu_marker.hip reads of a bank
struct MclParticles {
    const rigid *T;
    size_t n;
    Fence *used;
    hipStream_t hst;
};
ndtgpu_status mcl_particles_view(ndtgpu_mcl *h, size_t first, size_t count, const char *who, MclParticles &out);

#pragma GCC visibility pop
