// ndtgpu_registrar.hip -- the registrar of the C-ABI (include/ndtgpu.h): scans in, poses out.
#include "ndtgpu_host.h"

#include <atomic>
#include <chrono>
#include <thread>

extern "C" {

// ---- the registrar: scans in, poses out (include/ndtgpu.h) ---------------------------------------------------------------
// `depth` map sets with a stream each.  A sub-batch = ONE build launch for its 2 p scans + ONE matcher launch on the next
// stream in turn.  What orders the streams: (i) the inputs (an event recorded on the caller's stream at the call), (ii) the
// builds among themselves -- sub-batch k + 1 builds once sub-batch k's build has finished, i.e. while matcher k runs: the
// matcher's workgroups leave their CUs as soon as no registration is left to start (csrc/ndt_match.hip), so the next builds
// fill the CUs that the few long registrations do not hold --, (iii) a map set against its own previous use (same stream).
// the Gaussian cells of n_maps maps, summed, to two words of pinned host memory: {cells, seq + 1}
__global__ void ndt_reg_stats_kernel(const NdtMapCounters *ctr, unsigned n_maps, unsigned long long seq, unsigned long long *out)
{
    __shared__ unsigned long long part[256];
    unsigned long long c = 0;
    for (unsigned i = threadIdx.x; i < n_maps; i += 256u) c += ctr[i].n_cells;
    part[threadIdx.x] = c;
    __syncthreads();
    for (unsigned o = 128u; o > 0u; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&out[0], part[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&out[1], seq + 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct ndtgpu_registrar {
    size_t per = 0;
    int depth = 0;
    ndtgpu_registrar_params prm{};     // as given to ndtgpu_registrar_create_ex (zeros resolved)
    std::vector<MapsetOwner> sets;
    std::vector<Fence> built;
    // completion fences, one per sub-batch, in a ring of 4 x depth: sub-batch j records done[j % ring] -- an entry always
    // belongs to stream j % depth, so whoever waits on an entry that a later sub-batch has re-recorded waits for a superset
    std::vector<Fence> done;
    Fence in_ev;
    int last_built = -1;
    DeviceBuffer<uint32_t> iota;       // device: 0 .. 2 per - 1 (target indices: iota, source indices: iota + p)
    size_t submitted = 0;              // sub-batches so far
    // stream-fed form (csrc/ndt_match.hip, ndt_match_stream_kernel): build streams, ONE matcher stream on which an instance of
    // the matcher serves batch after batch from a queue in device memory
    DeviceBuffer<char> queue;
    int mst_prio = 0;                  // the matcher stream's priority: a stream of the caller's at this priority may share its hardware queue
    size_t helped = 0;                 // sub-batches submitted when the last helper was launched
    std::vector<Fence> trace_ev;       // NDTGPU_REG_TRACE: start / end of the build of the last 64 sub-batches (timed)
    size_t trace_first = (size_t)-1;   // ... the first sub-batch that has them
    std::vector<Fence> pub_ev;
    unsigned stream_groups = 0;        // workgroups (= CUs) of a matcher instance; 0: to be measured on the next sub-batch
    int stream_slots = 2;              // registrations in flight per workgroup of an instance (2, or 3 with half the hit list each)
    int device = 0;
    Fence probe_ev[2];                 // (timed)
    int stream_nn = -1;
    int stream_cov = 0;                // the running instances' kind: 1 = with the covariance tail (an instance is compiled for one)
    DeviceBuffer<double> cov_save;     // per-batch form, grid-barrier / pool sub-batches with a covariance: the initial guesses of
    size_t cov_save_pairs = 0;         // slot k at [k * per * 16] (the match overwrites them; ndt_cov_flags_kernel compares)
    int n_cu = 256;
    // the split of the chip is measured on a sub-batch and re-measured when the maps change: per slot the map counters of
    // the last build travel to pinned host memory on a side stream; a later call looks at what has arrived (no waiting)
    int calibrations = 0;
    double calib_cells = 0.0;          // mean Gaussian cells per map the split stands for: of the sub-batch it was first measured
                                       // on; after a re-measurement, of the recent sub-batches that asked for it (a registrar
                                       // that is fed two kinds of scenes in turn settles on their mean instead of measuring
                                       // again at every change)
    double recal_ref = 0.0;
    size_t calib_at = 0;               // ... and its number
    PinnedBuffer<unsigned long long> stat_host; // [depth][2]: {Gaussian cells of the slot's maps, sub-batch + 1} written by a
                                             // one-workgroup kernel behind the build (no copy engine, no event: a device-to-host
                                             // copy per sub-batch cost the pipeline a quarter of its rate, measured)
    std::vector<long long> stat_seq;   // sub-batch whose counters slot k was asked for (-1: none / consumed)
    std::vector<unsigned> stat_maps;
    std::vector<double> recent_cells;  // mean cells per map of the last sub-batches seen (at most `depth`)
    // host clouds (ndtgpu_register_batch_host): per slot a device staging area for the scans of a sub-batch, one for the
    // poses / results of a call, a copy stream
    std::vector<DeviceBuffer<char>> hstage;
    DeviceBuffer<char> hio;
    bool profiling = false;
    struct ProfMark { Fence e[4]; long long seq; };   // build start / end, matcher start / end (timed events), or the queue's stamps of `seq`
    std::vector<ProfMark> marks;
    // the streams last (ndtgpu_resource.h): one per map set; stream-fed form: builds (two, in turn), publishes (in order), matcher;
    // the drain helper of ndtgpu_registrar_sync; the host entries' copy stream
    std::vector<Stream> streams;
    Stream bst, bst2, pst, mst, hst, hcopy;
    std::vector<std::pair<unsigned, Stream>> masked;      // streams that own the first F CUs of the mask (the split's build probes)
    ndtgpu_status masked_stream(unsigned n_cus, hipStream_t *out)
    {
        for (auto &m : masked) if (m.first == n_cus) { *out = m.second.get(); return NDTGPU_OK; }
        std::vector<uint32_t> mask(((size_t)n_cu + 31) / 32, 0u);
        for (unsigned i = 0; i < n_cus && i < (unsigned)n_cu; i++) mask[i / 32] |= 1u << (i % 32);
        Stream st;
        HIP_TRY(st.create_cu_mask((uint32_t)mask.size(), mask.data()));
        *out = st.get();
        masked.emplace_back(n_cus, std::move(st));
        return NDTGPU_OK;
    }
};


ndtgpu_status ndtgpu_registrar_destroy(ndtgpu_registrar *r)
{
    if (!r) return NDTGPU_OK;
    // every stream drained before the first one goes (a device-side wait on one of them ends with the matcher's progress on another)
    for (Stream &st : r->streams) (void)hipStreamSynchronize(st.get());
    for (Stream *st : {&r->hcopy, &r->bst, &r->bst2, &r->pst, &r->hst, &r->mst})
        if (st->get()) (void)hipStreamSynchronize(st->get());
    delete r;
    return NDTGPU_OK;
}

void ndtgpu_default_registrar_params(ndtgpu_registrar_params *p)
{
    if (!p) return;
    p->pairs_per_batch = 1024;
    p->depth = 8;
    p->matcher_form = NDTGPU_MATCHER_AUTO;
    p->matcher_groups = 0;
    p->build_streams = 0;
    p->linger_us = 0;
    p->recalibrate_pct = 25;
    p->matcher_slots = 0;
}


ndtgpu_status ndtgpu_registrar_create_ex(const ndtgpu_grid_params *grid, const ndtgpu_registrar_params *params, ndtgpu_registrar **out)
{
    if (!grid || !params || !out) return fail(NDTGPU_ERR_INVALID, "registrar_create: null argument");
    ndtgpu_registrar_params P = *params;
    const size_t pairs_per_batch = P.pairs_per_batch;
    const int depth = P.depth;
    if (pairs_per_batch == 0 || pairs_per_batch > (1u << 30) || depth < 1 || depth > 16)
        return fail(NDTGPU_ERR_INVALID, "registrar_create: bad argument (pairs_per_batch >= 1, 1 <= depth <= 16)");
    if (P.matcher_form < NDTGPU_MATCHER_AUTO || P.matcher_form > NDTGPU_MATCHER_STREAM_FED || P.build_streams < 0 || P.build_streams > 2)
        return fail(NDTGPU_ERR_INVALID, "registrar_create: matcher_form must be 0..2, build_streams 0..2");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "registrar_create: no HIP device");
    // experiments (tools/, A/B runs): only where the caller asked for the default
    if (P.matcher_form == NDTGPU_MATCHER_AUTO && getenv("NDTGPU_REG_STREAM"))
        P.matcher_form = env_int("NDTGPU_REG_STREAM", 1) ? NDTGPU_MATCHER_AUTO : NDTGPU_MATCHER_PER_BATCH;
    if (P.matcher_groups == 0) P.matcher_groups = (unsigned)std::max(0, env_int("NDTGPU_REG_GROUPS", 0));
    if (P.build_streams == 0) P.build_streams = std::min(2, std::max(0, env_int("NDTGPU_REG_BUILD_STREAMS", 0)));
    // An instance that has worked stays for `linger` when it runs dry.  Where the builds are the slower side (a split that gives the
    // matcher more than its share) a batch is complete before the next one is published; an instance that leaves then has to be
    // placed again -- 144 whole CUs among build workgroups that keep arriving -- and the pipeline falls into lockstep: measured on the
    // bench with 144 matcher CUs forced, 259 k registrations/s without linger, 560 k with 1 ms; at the measured split (128) linger
    // changes nothing (0 / 200 / 1000 us: 664 / 666 / 661 k).  Default 1 ms; ndtgpu_registrar_sync switches it off for what is
    // already submitted, so a waiting host does not pay for it.
    if (P.linger_us == 0) P.linger_us = (unsigned)std::max(0, env_int("NDTGPU_REG_LINGER_US", 1000));
    if (P.recalibrate_pct == 0) P.recalibrate_pct = 25;
    if (P.matcher_slots != 0 && P.matcher_slots != 2 && P.matcher_slots != 3)
        return fail(NDTGPU_ERR_INVALID, "registrar_create: matcher_slots must be 0 (auto), 2 or 3");
    if (P.matcher_slots == 0) { const int es = env_int("NDTGPU_REG_SLOTS", 0); if (es == 2 || es == 3) P.matcher_slots = es; }
    ndtgpu_registrar *r = new (std::nothrow) ndtgpu_registrar();
    if (!r) return fail(NDTGPU_ERR_ALLOC, "registrar_create: host alloc");
    r->per = pairs_per_batch;
    r->depth = depth;
    r->n_cu = device_cus();
    (void)hipGetDevice(&r->device);
    r->sets.resize(depth);
    r->streams.resize(depth);
    r->built.resize(depth);
    r->done.resize(4 * (size_t)depth);
#define TRY(expr) CREATE_TRY(r, NDTGPU_ERR_HIP, "registrar_create", expr)
    for (int k = 0; k < depth; k++) {
        const ndtgpu_status rc = mapset_create_owned(grid, 2 * pairs_per_batch, r->sets[k]);
        if (rc != NDTGPU_OK) { delete r; return rc; }
        // Pipelined (depth > 1), a matcher launch keeps to half of the CUs: its persistent workgroups hold a CU each, whole, until
        // their registrations are done, and with all CUs taken the next sub-batch's builds would wait for the launch's first
        // exits (measured, 1024 pairs per sub-batch: 470 k registrations/s with 256 workgroups, 488 k with 128..160)
        if (depth > 1) r->sets[k]->match_groups = P.matcher_groups ? P.matcher_groups : (unsigned)(r->n_cu / 2);
        TRY(r->streams[k].create(hipStreamNonBlocking));
        TRY(r->built[k].create());
    }
    for (Fence &d : r->done) TRY(d.create());
    // The stream-fed matcher: pipelined registrars of small maps.  It needs a hardware queue of its own for the matcher stream:
    // the registrar orders map-set reuse with device-side wait kernels that only end when the running instance makes progress,
    // so an instance launch must never sit in a queue behind such a kernel.  What keeps the streams apart is a priority of
    // their own each -- a device that offers one priority level only (lo == hi) keeps the form with one matcher launch per
    // sub-batch (ordered by events), as does NDTGPU_REG_PRIO=0.
    int lo = 0, hi = 0;
    const bool prio_ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi && env_int("NDTGPU_REG_PRIO", 1) != 0;
    const bool can = depth > 1 && (unsigned)depth <= ndt_stream_ring() && r->sets[0]->v.grid.max_cells < 16384u && prio_ok;
    if (P.matcher_form == NDTGPU_MATCHER_STREAM_FED && !can) {
        delete r;
        return fail(NDTGPU_ERR_INVALID, "registrar_create: the stream-fed matcher needs 2 <= depth <= 8, max_cells < 16384 and a device "
                                        "with more than one stream priority");
    }
    if (P.matcher_form != NDTGPU_MATCHER_PER_BATCH && can) {
        r->stream_groups = P.matcher_groups;            // 0: measured on the first sub-batch
        r->stream_slots = P.matcher_slots ? P.matcher_slots : 2;   // (auto: decided with the split, by the cells per map)
        TRY(r->queue.alloc(ndt_stream_queue_bytes()));
        TRY(hipMemset(r->queue.get(), 0, ndt_stream_queue_bytes()));
        const unsigned ring_linger[2] = {(unsigned)depth, 100u * P.linger_us};   // 100 MHz ticks (measured: no gain from 300 / 1000 us; default 0)
        TRY(hipMemcpy(r->queue.get() + ndt_stream_ring_offset(), ring_linger, sizeof ring_linger, hipMemcpyHostToDevice));
        TRY(r->bst.create(hipStreamNonBlocking));
        // Two build streams that take the sub-batches in turn (build_streams = 1: one): a build launch is one
        // workgroup per map and every map costs about the same, so on F free CUs it takes ceil(maps / 4 F) whole rounds
        // (measured: 1.47 ms beside a matcher instance on 128 CUs, 1.85 ms beside one on 129); with the next launch's
        // workgroups filling the last, nearly empty round the build side runs at its average rate whatever F is.
        // Publishes stay in order on a stream of their own.
        if (P.build_streams == 0) P.build_streams = depth >= 3 ? 2 : 1;
        if (depth < 3) P.build_streams = 1;
        if (P.build_streams == 2) TRY(r->bst2.create(hipStreamNonBlocking));
        TRY(r->pst.create(hipStreamNonBlocking, lo));
        // (a priority of its own: the runtime then never maps the two streams onto one hardware queue, where the build of
        //  batch k + 1 would sit behind the running matcher instance)
        TRY(r->mst.create(hipStreamNonBlocking, hi));
        r->mst_prio = hi;
        (void)hipStreamGetPriority(r->mst.get(), &r->mst_prio);
        r->pub_ev.resize(depth);
        for (Fence &e : r->pub_ev) TRY(e.create());
        // the side channel of the map statistics
        if (P.matcher_groups == 0 && P.recalibrate_pct > 0) {
            TRY(r->stat_host.alloc((size_t)depth * 2));
            memset(r->stat_host.get(), 0, (size_t)depth * 2 * sizeof(unsigned long long));
            r->stat_seq.assign(depth, -1);
            r->stat_maps.assign(depth, 0u);
        }
    } else {
        P.build_streams = 0;
    }
    P.matcher_form = r->queue.get() ? NDTGPU_MATCHER_STREAM_FED : NDTGPU_MATCHER_PER_BATCH;
    r->prm = P;
    TRY(r->in_ev.create());
    TRY(r->iota.alloc(2 * pairs_per_batch + 4));
    std::vector<uint32_t> h(2 * pairs_per_batch);
    for (size_t i = 0; i < h.size(); i++) h[i] = (uint32_t)i;
    TRY(hipMemcpy(r->iota.get(), h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
#undef TRY
    *out = r;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_registrar_create(const ndtgpu_grid_params *grid, size_t pairs_per_batch, int depth, ndtgpu_registrar **out)
{
    ndtgpu_registrar_params p;
    ndtgpu_default_registrar_params(&p);
    p.pairs_per_batch = pairs_per_batch;
    p.depth = depth;
    return ndtgpu_registrar_create_ex(grid, &p, out);
}

ndtgpu_status ndtgpu_registrar_get_info(const ndtgpu_registrar *r, ndtgpu_registrar_info *info)
{
    if (!r || !info) return fail(NDTGPU_ERR_INVALID, "registrar_get_info: null argument");
    info->matcher_form = r->prm.matcher_form;
    info->matcher_groups = r->queue.get() ? r->stream_groups : r->sets[0]->match_groups;
    info->build_streams = r->prm.build_streams;
    info->calibrations = r->calibrations;
    info->submitted = (uint64_t)r->submitted;
    info->cells_per_map = r->calib_cells;
    info->matcher_slots = r->queue.get() ? r->stream_slots : 2;
    info->resident_groups = 0;
    if (r->queue.get()) {                                         // (a 4-byte read on the null stream; the registrar's streams do not block it)
        unsigned live = 0u;
        HIP_TRY(hipMemcpy(&live, r->queue.get() + ndt_stream_live_offset(), sizeof live, hipMemcpyDeviceToHost));
        info->resident_groups = (int32_t)live;
    }
    return NDTGPU_OK;
}

// test aid: raises the stream-fed matcher's abort word, as a workgroup that found no work for ~30 s would
ndtgpu_status ndtgpu_registrar_inject_abort(ndtgpu_registrar *r)
{
    if (!r) return fail(NDTGPU_ERR_INVALID, "registrar_inject_abort: null");
    if (!r->queue.get()) return fail(NDTGPU_ERR_INVALID, "registrar_inject_abort: not the stream-fed form");
    const unsigned one = 1u;
    HIP_TRY(hipMemcpy(r->queue.get() + ndt_stream_abort_offset(), &one, sizeof one, hipMemcpyHostToDevice));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_registrar_mapset(ndtgpu_registrar *r, int slot, ndtgpu_mapset **set)
{
    if (!r || !set || slot < 0 || slot >= r->depth) return fail(NDTGPU_ERR_INVALID, "registrar_mapset: bad argument");
    *set = r->sets[slot].get();
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_registrar_profiling(ndtgpu_registrar *r, int on)
{
    if (!r) return fail(NDTGPU_ERR_INVALID, "registrar_profiling: null");
    r->profiling = on != 0;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_registrar_kernel_ms(ndtgpu_registrar *r, float mean_ms[2], int32_t *launches)
{
    if (!r || !mean_ms || !launches) return fail(NDTGPU_ERR_INVALID, "registrar_kernel_ms: bad argument");
    const size_t n = r->marks.size();
    double sum[2] = {0.0, 0.0};
    size_t cnt[2] = {0, 0};
    if (r->queue.get() && n) {                    // the stamps are complete once the matcher side is
        ndtgpu_status rc = ndtgpu_registrar_sync(r);
        if (rc != NDTGPU_OK) return rc;
    }
    for (size_t k = 0; k < n; k++) {
        ndtgpu_registrar::ProfMark &m = r->marks[k];
        HIP_TRY(m.e[m.seq >= 0 ? 1 : 3].sync());
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, m.e[0].get(), m.e[1].get()));
        sum[0] += ms; cnt[0]++;
        if (m.seq < 0) {
            HIP_TRY(hipEventElapsedTime(&ms, m.e[2].get(), m.e[3].get()));
            sum[1] += ms; cnt[1]++;
        } else if ((size_t)m.seq + ndt_stream_stamps() > r->submitted) {
            // stream-fed form: what the queue saw of the sub-batch -- published (its maps built) until its last registration finished
            unsigned long long st[2] = {0, 0};
            HIP_TRY(ndt_stream_read_stamps(r->queue.get(), (unsigned)m.seq, st));
            if (st[1] > st[0]) { sum[1] += (double)(st[1] - st[0]) * 1e-5; cnt[1]++; }
        }
    }
    r->marks.clear();
    *launches = (int32_t)n;
    mean_ms[0] = cnt[0] ? (float)(sum[0] / (double)cnt[0]) : 0.f;
    mean_ms[1] = cnt[1] ? (float)(sum[1] / (double)cnt[1]) : 0.f;
    return NDTGPU_OK;
}

// ndtgpu_register_batch_device (cov_mode < 0) and ndtgpu_register_batch_cov_device (cov_mode 0 / 1): one code path
static ndtgpu_status register_batch_core(ndtgpu_registrar *r, const void *targets_dev, const void *sources_dev, size_t n_points,
                                         size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                         const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                         const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev, ndtgpu_stream stream,
                                         uint64_t *ticket, int cov_mode, double *cov36_dev, int32_t *cov_flags_dev)
{
    if (ticket) *ticket = r ? (uint64_t)r->submitted : 0;
    if (!r || (n_pairs && (!T16_dev || !results_dev || (n_points && (!targets_dev || !sources_dev)))) || stride_bytes < 12 ||
        (stride_bytes & 3) || n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "register_batch_device: bad argument");
    const bool with_cov = cov_mode >= 0;
    if (with_cov && n_pairs && (!cov36_dev || !cov_flags_dev))
        return fail(NDTGPU_ERR_INVALID, "register_batch_cov_device: bad argument (cov36_dev / cov_flags_dev)");
    if (n_pairs == 0) return NDTGPU_OK;
    NdtMatchParamsDev pdev;
    { ndtgpu_status prc = match_params_dev(prm, 0, pdev); if (prc != NDTGPU_OK) return prc; }
    HIP_TRY(r->in_ev.record((hipStream_t)stream));
    auto new_mark = [&](long long seq, ndtgpu_registrar::ProfMark **out_mark) -> ndtgpu_status {
        ndtgpu_registrar::ProfMark m{};
        m.seq = seq;
        for (int k = 0; k < (seq >= 0 ? 2 : 4); k++) HIP_TRY(m.e[k].create(hipEventDefault));
        r->marks.push_back(std::move(m));
        *out_mark = &r->marks.back();
        return NDTGPU_OK;
    };
    // one build launch when the sources follow the targets in memory, else two
    auto build_pairs = [&](ndtgpu_mapset *set, size_t off, size_t p, hipStream_t st) -> ndtgpu_status {
        const char *tg = (const char *)targets_dev + off * map_stride_bytes, *sc = (const char *)sources_dev + off * map_stride_bytes;
        if (sc == tg + p * map_stride_bytes)
            return ndtgpu_mapset_build(set, 0, 2 * p, tg, n_points, stride_bytes, map_stride_bytes, range_limit, nullptr, cell, st);
        ndtgpu_status rc = ndtgpu_mapset_build(set, 0, p, tg, n_points, stride_bytes, map_stride_bytes, range_limit, nullptr, cell, st);
        if (rc == NDTGPU_OK)
            rc = ndtgpu_mapset_build(set, p, p, sc, n_points, stride_bytes, map_stride_bytes, range_limit, nullptr, cell, st);
        return rc;
    };
    if (r->queue.get()) {
        // ---- stream-fed form: builds on one stream, batches published to the running matcher instance -------------------
        auto drain = [&]() -> ndtgpu_status {
            HIP_TRY(hipStreamSynchronize(r->bst.get()));
            if (r->bst2.get()) HIP_TRY(hipStreamSynchronize(r->bst2.get()));
            HIP_TRY(hipStreamSynchronize(r->pst.get()));
            HIP_TRY(hipStreamSynchronize(r->mst.get()));
            if (r->hst.get()) HIP_TRY(hipStreamSynchronize(r->hst.get()));
            return NDTGPU_OK;
        };
        // (an instance is compiled for one neighbourhood size, and with or without the covariance tail)
        if (r->stream_nn != pdev.n_neighbours || r->stream_cov != (with_cov ? 1 : 0)) {
            if (r->stream_nn >= 0) { ndtgpu_status drc = drain(); if (drc != NDTGPU_OK) return drc; }
            r->stream_nn = pdev.n_neighbours;
            r->stream_cov = with_cov ? 1 : 0;
        }
        for (size_t off = 0; off < n_pairs; off += r->per) {
            const size_t p = std::min(r->per, n_pairs - off);
            const size_t j = r->submitted;
            const int slot = (int)(j % (size_t)r->depth);
            ndtgpu_mapset *set = r->sets[slot].get();
            hipStream_t st = (r->bst2.get() && (j & 1u)) ? r->bst2.get() : r->bst.get();
            // ---- have the maps changed?  The counters of earlier builds that have arrived on the host say how many Gaussian
            // cells a map holds now; when the mean over the last sub-batches has left the figure the split was measured at by
            // more than recalibrate_pct, the pipeline is drained once and this sub-batch measures the split again (a
            // registrar that moves from halls to clutter would otherwise keep 128 matcher CUs where 200 are right).
            if (r->stat_host.get() && r->stream_groups != 0u) {
                // (back-pressure: the host runs at most `depth` sub-batches ahead of the builds -- without it a caller that
                //  never waits would have submitted everything before the first counters arrive)
                if (j >= (size_t)r->depth) HIP_TRY(r->built[slot].sync());
                for (int k = 0; k < r->depth; k++) {
                    volatile unsigned long long *sh = r->stat_host.get() + 2 * k;
                    if (r->stat_seq[k] < 0 || sh[1] != (unsigned long long)r->stat_seq[k] + 1ull) continue;
                    std::atomic_thread_fence(std::memory_order_acquire);
                    if (r->stat_maps[k]) {
                        if (r->recent_cells.size() >= (size_t)r->depth) r->recent_cells.erase(r->recent_cells.begin());
                        r->recent_cells.push_back((double)sh[0] / (double)r->stat_maps[k]);
                    }
                    r->stat_seq[k] = -1;
                }
                if (r->recent_cells.size() >= (size_t)std::min(r->depth, 4) && r->calib_cells > 0 && j >= r->calib_at + 2 * (size_t)r->depth) {
                    double mean = 0;
                    for (double v : r->recent_cells) mean += v;
                    mean /= (double)r->recent_cells.size();
                    if (std::fabs(mean / r->calib_cells - 1.0) * 100.0 > (double)r->prm.recalibrate_pct) {
                        if (getenv("NDTGPU_REG_VERBOSE"))
                            fprintf(stderr, "ndtgpu registrar: %.0f cells per map where the split was measured at %.0f: measuring again\n", mean, r->calib_cells);
                        ndtgpu_status drc = drain();
                        if (drc != NDTGPU_OK) return drc;
                        r->stream_groups = 0u;
                        r->recal_ref = mean;
                    }
                }
            }
            HIP_TRY(r->in_ev.order(st));
            if (r->stream_groups == 0u) {
                // ---- a sub-batch that measures the split of the chip (the first of a registrar's life; later ones after a
                // drain, see above): its maps are built and its pairs registered with nothing else on the device (the whole
                // chip each; the same bits), the host reads the kernels' own clocks -- CU-time of the builds B and of the
                // registrations M -- and a matcher instance gets n_cu M / (M + B) CUs from then on: 128 of 256 on the bench's
                // halls, 200 on a cluttered scene whose maps hold five times the cells.  Costs one synchronisation.
                ndtgpu_registrar::ProfMark *mk0 = nullptr;
                if (r->profiling) { ndtgpu_status mrc = new_mark(-1, &mk0); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk0->e[0].record(st)); }
                ndtgpu_status rc0 = build_pairs(set, off, p, st);
                if (rc0 != NDTGPU_OK) return rc0;
                if (mk0) { HIP_TRY(mk0->e[1].record(st)); HIP_TRY(mk0->e[2].record(st)); }
                const unsigned saved_groups = set->match_groups;
                set->match_groups = 0;                            // (the whole chip)
                rc0 = match_batch_device_ex(set, r->iota.get(), set, r->iota.get() + p, T16_dev + off * 16, p, prm, results_dev + off, st, cov_mode,
                                            with_cov ? cov36_dev + off * 36 : nullptr, with_cov ? cov_flags_dev + off : nullptr, nullptr);
                set->match_groups = saved_groups;
                if (rc0 != NDTGPU_OK) return rc0;
                if (mk0) HIP_TRY(mk0->e[3].record(st));
                hipError_t se = ndt_stream_skip(r->queue.get(), (unsigned)j, st);
                if (se != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: calibration", se);
                HIP_TRY(r->built[slot].record(st));
                HIP_TRY(hipStreamSynchronize(st));
                std::vector<NdtMapCounters> ctr(2 * p);
                std::vector<ndtgpu_match_result> res(p);
                HIP_TRY(hipMemcpy(ctr.data(), set->v.counters, 2 * p * sizeof(NdtMapCounters), hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(res.data(), results_dev + off, p * sizeof(ndtgpu_match_result), hipMemcpyDeviceToHost));
                double B = 0, M = 0, cells = 0;
                for (const NdtMapCounters &c : ctr) {
                    B += (double)c.cyc[0] + (double)c.cyc[1] + (double)c.cyc[2] + (double)c.cyc[3];
                    cells += (double)c.n_cells;
                }
                B /= 4.0;                                         // a build workgroup shares its CU with three others
                // (a clock sum outside any plausible range -- seen once in six runs on the cluttered scene: 2^63 in one result -- is
                //  left out: the split is a heuristic, one registration does not move it; NDTGPU_REG_VERBOSE reports it)
                size_t m_bad = 0;
                for (const ndtgpu_match_result &q : res) {
                    const bool sane = q.cycles_eval >= 0 && q.cycles_eval < (1ll << 44) && q.cycles_solver >= 0 && q.cycles_solver < (1ll << 44);
                    if (sane) M += (double)q.cycles_eval + (double)q.cycles_solver / 8.0;
                    else {
                        if (getenv("NDTGPU_REG_VERBOSE") && m_bad < 4)
                            fprintf(stderr, "ndtgpu registrar: calibration result %zu: cycles_eval %lld cycles_solver %lld iterations %d exit %d\n",
                                    (size_t)(&q - res.data()), (long long)q.cycles_eval, (long long)q.cycles_solver, (int)q.iterations, (int)q.exit_code);
                        m_bad++;
                    }
                }
                if (m_bad < res.size()) M *= (double)res.size() / (double)(res.size() - m_bad);
                const double M_raw = M;                           // CU-clocks of the sub-batch's registrations
                M *= 1.125;                                       // (measured optimum on the bench scene: 144 of 256 CUs where the raw clocks say 138)
                const int n_cu = r->n_cu;
                double share = (M + B) > 0 ? M / (M + B) : 0.5;
                share = std::min(0.9, std::max(0.25, share));
                r->stream_groups = std::max(8u, ((unsigned)(share * n_cu + 4.0) / 8u) * 8u);
                // ... refined by what the build side really does with the CUs it is left: a build launch is one workgroup per
                // map, four to a CU, so on F CUs it takes ceil(maps / 4F) ROUNDS of the mean workgroup time -- 2048 maps take
                // four rounds on 128 CUs and five on 120, 112 or 104.  Of the splits around the proportional one, take the one
                // whose slower side is fastest (the bench halls after the round's matcher savings: 136 by proportion, 573 k
                // registrations/s; 128 by this rule, 624 k; 120: 585 k, 144: 544 k).
                if (B > 0 && M > 0) {
                    const double wg = 4.0 * B / (2.0 * (double)p);            // mean clocks of a build workgroup
                    double best_t = 0;
                    unsigned best_g = r->stream_groups;
                    for (int g8 = (int)r->stream_groups - 32; g8 <= (int)r->stream_groups + 32; g8 += 8) {
                        if (g8 < 16 || g8 > n_cu - 16) continue;
                        const double slots = 4.0 * (n_cu - g8);
                        const double t = std::max(M / g8, std::ceil(2.0 * (double)p / slots) * wg);
                        const bool closer = std::abs(g8 - (int)r->stream_groups) < std::abs((int)best_g - (int)r->stream_groups);
                        if (best_t == 0 || t < 0.99 * best_t || (t <= 1.01 * best_t && closer && t <= best_t)) { best_t = t; best_g = (unsigned)g8; }
                    }
                    r->stream_groups = best_g;
                }
                // ... and, since 0.6.5, MEASURED on the build side (round 6).  The clocks above are those of workgroups that had the
                // whole chip: beside a matcher instance the builds of the bench halls run 20 % faster than that (half as many
                // workgroups pull on the HBM), those of a cluttered scene 30 % slower (four workgroups to a CU where the lone launch
                // had three), and a quarter more or less decides between two splits (halls 120 instead of 128 CUs on one box in
                // three: -5 %; clutter 184 instead of 160: 103 against 127 k registrations/s).  A build launch takes whole rounds,
                // so the only splits worth having are those that leave the builds just enough CUs for k rounds, k = 1, 2, ...:
                // the sub-batch is built again on a stream that owns exactly those CUs (Stream::create_cu_mask: mask bits
                // are dealt to the XCDs in turn, like the CUs a matcher instance leaves), timed with events, and the split whose
                // slower side -- that time, or the registrations' CU-clocks over the matcher's CUs -- is fastest wins.  A few
                // build launches, once per measurement; NDTGPU_REG_PROBE=0 keeps the model above.
                if (B > 0 && M_raw > 0 && env_int("NDTGPU_REG_PROBE", 1) != 0) {
                    int khz = 0;
                    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, r->device) != hipSuccess || khz <= 0) khz = 2400000;
                    const double clk_per_ms = 0.85 * (double)khz;              // (the clock under these kernels: 1.93-2.1 of 2.4 GHz)
                    const size_t maps = 2 * p;
                    struct Cand { unsigned g; double build_ms, t_ms; };
                    std::vector<Cand> cand;
                    auto groups_of = [&](unsigned k) -> unsigned {             // the most matcher CUs that leave the builds k rounds
                        const unsigned F = (unsigned)((maps + 4u * k - 1u) / (4u * k));
                        const unsigned F8 = (F + 7u) / 8u * 8u;
                        return ((unsigned)n_cu > F8 + 15u) ? (unsigned)n_cu - F8 : 0u;
                    };
                    auto probe = [&](unsigned g, double *ms) -> ndtgpu_status {
                        hipStream_t ms_st = nullptr;
                        ndtgpu_status prc = r->masked_stream((unsigned)n_cu - g, &ms_st);
                        if (prc != NDTGPU_OK) return prc;
                        HIP_TRY(r->probe_ev[0].create(hipEventDefault));
                        HIP_TRY(r->probe_ev[1].create(hipEventDefault));
                        float best = 0.f;
                        for (int rep = 0; rep < 2; rep++) {                    // (the first launch on a new stream pays for the stream)
                            HIP_TRY(r->probe_ev[0].record(ms_st));
                            prc = build_pairs(set, off, p, ms_st);
                            if (prc != NDTGPU_OK) return prc;
                            HIP_TRY(r->probe_ev[1].record(ms_st));
                            HIP_TRY(r->probe_ev[1].sync());
                            float e = 0.f;
                            HIP_TRY(hipEventElapsedTime(&e, r->probe_ev[0].get(), r->probe_ev[1].get()));
                            if (rep == 0 || e < best) best = e;
                        }
                        *ms = (double)best;
                        return NDTGPU_OK;
                    };
                    // the round count the model's split stands for, and its neighbours; further out while the edge keeps winning
                    unsigned k0 = 1;
                    for (unsigned k = 1; k <= 16; k++) { k0 = k; if (groups_of(k) >= r->stream_groups) break; }
                    bool ok = true;
                    auto have = [&](unsigned g) { for (const Cand &c : cand) if (c.g == g) return true; return false; };
                    auto add = [&](unsigned k) {
                        const unsigned g = k >= 1 && k <= 16 ? groups_of(k) : 0u;
                        if (!ok || g < 16u || have(g)) return;
                        Cand c{g, 0.0, 0.0};
                        if (probe(g, &c.build_ms) != NDTGPU_OK) { ok = false; return; }
                        c.t_ms = std::max(c.build_ms, M_raw / (double)g / clk_per_ms);
                        cand.push_back(c);
                    };
                    auto best_of = [&]() { size_t b = 0; for (size_t i = 1; i < cand.size(); i++) if (cand[i].t_ms < cand[b].t_ms) b = i; return b; };
                    add(k0); add(k0 > 1 ? k0 - 1 : k0 + 2); add(k0 + 1);
                    for (int more = 0; ok && more < 3 && !cand.empty(); more++) {
                        const Cand &b = cand[best_of()];
                        unsigned kb = 0;
                        for (unsigned k = 1; k <= 16; k++) if (groups_of(k) == b.g) { kb = k; break; }
                        const size_t n_before = cand.size();
                        if (kb > 1 && !have(groups_of(kb - 1))) add(kb - 1);
                        if (kb && kb < 16 && !have(groups_of(kb + 1))) add(kb + 1);
                        if (cand.size() == n_before) break;
                    }
                    if (ok && !cand.empty()) {
                        const Cand &b = cand[best_of()];
                        if (getenv("NDTGPU_REG_VERBOSE"))
                            for (const Cand &c : cand)
                                fprintf(stderr, "ndtgpu registrar: %u matcher CUs: builds %.3f ms on the other %u, registrations %.3f ms -> %.3f ms per sub-batch%s\n",
                                        c.g, c.build_ms, (unsigned)n_cu - c.g, M_raw / (double)c.g / clk_per_ms, c.t_ms, c.g == b.g ? "  <-" : "");
                        r->stream_groups = b.g;
                    } else if (!ok) {
                        (void)hipGetLastError();                               // (no masked streams on this device / runtime: the model's split stands)
                        g_err.clear();
                    }
                    // (the probe streams go at once: each is a hardware queue of its own and of no use until the next measurement;
                    //  creating them is most of what a measurement costs, ~50 ms with three or four candidates)
                    r->masked.clear();
                    HIP_TRY(r->built[slot].record(st));               // (the maps were rebuilt: same contents)
                }
                r->calibrations++;
                // three registrations per workgroup (hit lists of 640 entries per share) where the maps are small -- up to 448 cells: the
                // one-lane solver steps are a third of a registration there --, two with lists of 1024 entries otherwise (measured
                // on the cluttered scene: three are slower)
                if (r->prm.matcher_slots == 0) r->stream_slots = (cells / (double)(2 * p) <= 448.0) ? 3 : 2;
                r->calib_cells = r->recal_ref > 0 ? r->recal_ref : cells / (double)(2 * p);
                r->recal_ref = 0.0;
                r->calib_at = j;
                r->recent_cells.clear();
                for (long long &q : r->stat_seq) q = -1;
                if (getenv("NDTGPU_REG_VERBOSE")) fprintf(stderr, "ndtgpu registrar: build %.3g, registrations %.3g CU-clocks per sub-batch, %.0f cells per map -> matcher instances of %u workgroups\n", B, M, r->calib_cells, r->stream_groups);
                r->submitted++;
                if (ticket) *ticket = (uint64_t)r->submitted;
                continue;
            }
            // This map set was last used by sub-batch j - depth: its registrations must be complete before it is rebuilt.
            // (Depth: a batch is complete 3-5 ms after its publication; with 8 map sets the builds never wait for that, 4 cost
            //  ~5 % on the bench -- include/ndtgpu.h.)
            if (j >= (size_t)r->depth) {
                hipError_t we = ndt_stream_wait(r->queue.get(), (unsigned)r->depth, (unsigned)(j - (size_t)r->depth), st);
                if (we != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: wait launch", we);
            }
            ndtgpu_registrar::ProfMark *mk = nullptr;
            if (r->profiling) { ndtgpu_status mrc = new_mark((long long)j, &mk); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk->e[0].record(st)); }
            const bool tracing = getenv("NDTGPU_REG_TRACE") != nullptr;
            if (tracing) {
                if (r->trace_ev.empty()) {
                    std::vector<Fence> ev(128);
                    for (Fence &e : ev) HIP_TRY(e.create(hipEventDefault));
                    r->trace_ev = std::move(ev);                                      // (all 128 or none)
                }
                HIP_TRY(r->trace_ev[2 * (j % 64)].record(st));
                if (r->trace_first == (size_t)-1) r->trace_first = j;
            }
            ndtgpu_status rc = build_pairs(set, off, p, st);
            if (rc != NDTGPU_OK) return rc;
            if (tracing) HIP_TRY(r->trace_ev[2 * (j % 64) + 1].record(st));
            if (mk) HIP_TRY(mk->e[1].record(st));
            if (r->stat_host.get() && r->stat_seq[slot] < 0 && j % 3u == 0u) {
                // (how many Gaussian cells the maps of this build hold: one small kernel behind it writes the sum to the host.
                //  Every third sub-batch: the launch costs the build stream a few microseconds -- 2 % of the bench's rate when
                //  every sub-batch had one -- and an odd period does not lock onto callers that alternate between two scenes)
                hipLaunchKernelGGL(ndt_reg_stats_kernel, dim3(1), dim3(256), 0, st, set->v.counters, (unsigned)(2 * p), (unsigned long long)j,
                                   r->stat_host.get() + 2 * slot);
                HIP_TRY(hipGetLastError());
                r->stat_seq[slot] = (long long)j;
                r->stat_maps[slot] = (unsigned)(2 * p);
            }
            HIP_TRY(r->built[slot].record(st));
            HIP_TRY(r->built[slot].order(r->pst.get()));
            hipError_t pe = ndt_stream_publish(r->queue.get(), set->v, T16_dev + off * 16, reinterpret_cast<NdtMatchResultDev *>(results_dev + off),
                                               pdev, (unsigned)p, (unsigned)j, r->pst.get(), with_cov ? cov_mode : -1,
                                               with_cov ? cov36_dev + off * 36 : nullptr, with_cov ? cov_flags_dev + off : nullptr);
            if (pe != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: publish", pe);
            HIP_TRY(r->pub_ev[slot].record(r->pst.get()));
            // every published batch is followed by an instance launch: it starts when the running instance has ended (and
            // then serves this batch and whatever is published while it runs), or finds the batch taken and leaves
            HIP_TRY(r->pub_ev[slot].order(r->mst.get()));
            pe = ndt_launch_match_stream(r->queue.get(), pdev.n_neighbours, r->stream_slots, r->stream_groups, r->mst.get(), r->stream_cov);
            if (pe != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: matcher launch", pe);
            r->submitted++;
            if (ticket) *ticket = (uint64_t)r->submitted;
        }
        return NDTGPU_OK;
    }
    if (with_cov && !r->cov_save.get()) {
        // (only grid-barrier / pool sub-batches read it -- sets of large maps, at most half as many pairs as CUs.  Made once and
        //  never replaced: nothing to wait for)
        const size_t n = std::min(r->per, (size_t)r->n_cu);
        HIP_TRY(r->cov_save.reserve((size_t)r->depth * n * 16));
        r->cov_save_pairs = n;
    }
    for (size_t off = 0; off < n_pairs; off += r->per) {
        const size_t p = std::min(r->per, n_pairs - off);
        const int slot = (int)(r->submitted % (size_t)r->depth);
        hipStream_t st = r->streams[slot].get();
        ndtgpu_mapset *set = r->sets[slot].get();
        HIP_TRY(r->in_ev.order(st));
        if (r->last_built >= 0 && r->last_built != slot) HIP_TRY(r->built[r->last_built].order(st));
        ndtgpu_registrar::ProfMark *mk = nullptr;
        if (r->profiling) { ndtgpu_status mrc = new_mark(-1, &mk); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk->e[0].record(st)); }
        ndtgpu_status rc = build_pairs(set, off, p, st);
        if (rc != NDTGPU_OK) return rc;
        if (mk) { HIP_TRY(mk->e[1].record(st)); HIP_TRY(mk->e[2].record(st)); }
        HIP_TRY(r->built[slot].record(st));
        r->last_built = slot;
        // `built` releases the next sub-batch's build AND, on this stream, this sub-batch's matcher.  The matcher's persistent
        // workgroups (one per CU, all registers and LDS of it) must not be placed first: the build would then only get the CUs
        // the matcher leaves, its end -- which releases the build after it -- moves out, and the pipeline loses a tenth of its
        // rate (measured: 430 k against 470 k registrations/s).  Two 4-byte fills keep this stream busy for the few
        // microseconds the next build's dispatch needs to get ahead (NDTGPU_REG_GAP: their number).
        if (r->depth > 1) {
            const int n_gap = env_int("NDTGPU_REG_GAP", 2);
            for (int g = 0; g < n_gap; g++) HIP_TRY(hipMemsetAsync(r->iota.get() + 2 * r->per, 0, 4, st));
        }
        rc = match_batch_device_ex(set, r->iota.get(), set, r->iota.get() + p, T16_dev + off * 16, p, prm, results_dev + off, st, cov_mode,
                                   with_cov ? cov36_dev + off * 36 : nullptr, with_cov ? cov_flags_dev + off : nullptr,
                                   with_cov && p <= r->cov_save_pairs ? r->cov_save.get() + (size_t)slot * r->cov_save_pairs * 16 : nullptr);
        if (rc != NDTGPU_OK) return rc;
        if (mk) HIP_TRY(mk->e[3].record(st));
        HIP_TRY(r->done[r->submitted % r->done.size()].record(st));
        r->submitted++;
        if (ticket) *ticket = (uint64_t)r->submitted;      // "every sub-batch before this count"
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_register_batch_device(ndtgpu_registrar *r, const void *targets_dev, const void *sources_dev, size_t n_points,
                                           size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                           const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                           const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev, ndtgpu_stream stream,
                                           uint64_t *ticket)
{
    return register_batch_core(r, targets_dev, sources_dev, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16_dev, n_pairs,
                               prm, results_dev, stream, ticket, -1, nullptr, nullptr);
}

ndtgpu_status ndtgpu_register_batch_cov_device(ndtgpu_registrar *r, const void *targets_dev, const void *sources_dev, size_t n_points,
                                               size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                               const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                               const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev, int covariance_mode,
                                               double *cov36_dev, int32_t *cov_flags_dev, ndtgpu_stream stream, uint64_t *ticket)
{
    if (covariance_mode != 0 && covariance_mode != 1) {
        if (ticket) *ticket = r ? (uint64_t)r->submitted : 0;
        return fail(NDTGPU_ERR_INVALID, "register_batch_cov_device: covariance_mode must be 0 or 1");
    }
    return register_batch_core(r, targets_dev, sources_dev, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16_dev, n_pairs,
                               prm, results_dev, stream, ticket, covariance_mode, cov36_dev, cov_flags_dev);
}

ndtgpu_status ndtgpu_registrar_wait_stream(ndtgpu_registrar *r, uint64_t ticket, ndtgpu_stream stream)
{
    if (!r || ticket > (uint64_t)r->submitted) return fail(NDTGPU_ERR_INVALID, "registrar_wait_stream: bad argument");
    const size_t end = ticket ? (size_t)ticket : r->submitted;
    if (r->queue.get()) {
        // The wait is a device-side kernel that ends when the running matcher instance has made the batch complete: it must not
        // sit in the hardware queue the instance launches go through.  The runtime keeps streams of different priorities on
        // different queues; a stream of the matcher stream's priority (the highest the device offers) is refused.
        if (stream) {
            int prio = 0;
            if (hipStreamGetPriority((hipStream_t)stream, &prio) == hipSuccess && prio == r->mst_prio)
                return fail(NDTGPU_ERR_INVALID, "registrar_wait_stream: a stream of the highest priority may share the matcher's hardware queue; "
                                                "wait on a stream of default priority (or use ndtgpu_registrar_sync)");
        }
        // the last `depth` sub-batches before `end` (a sub-batch is only published once the one `depth` before it is complete)
        for (size_t j = end > (size_t)r->depth ? end - (size_t)r->depth : 0; j < end; j++) {
            hipError_t we = ndt_stream_wait(r->queue.get(), (unsigned)r->depth, (unsigned)j, (hipStream_t)stream);
            if (we != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: wait launch", we);
        }
        return NDTGPU_OK;
    }
    // the newest sub-batch before `end` on every internal stream (earlier ones precede it in stream order)
    for (size_t j = end > (size_t)r->depth ? end - (size_t)r->depth : 0; j < end; j++)
        HIP_TRY(r->done[j % r->done.size()].order((hipStream_t)stream));
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_registrar_sync(ndtgpu_registrar *r)
{
    if (!r) return fail(NDTGPU_ERR_INVALID, "registrar_sync: null");
    if (r->queue.get()) {
        // Nothing more is coming before this call returns: once the last sub-batch has been published the CUs that were kept
        // for the builds are free, and a second instance on those takes its share of what is left to register.
        // (nothing more is coming before this call returns: instances do not linger behind the last published batch)
        if (r->submitted) {
            hipError_t fe = ndt_stream_final(r->queue.get(), (unsigned)r->submitted, r->pst.get());
            if (fe != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: final launch", fe);
        }
        if (r->submitted > r->helped && r->stream_groups && r->stream_nn >= 0 && !getenv("NDTGPU_REG_NO_HELPER")) {
            const int n_cu = r->n_cu;
            if ((unsigned)n_cu > r->stream_groups + 8u) {
                if (!r->hst.get()) HIP_TRY(r->hst.create(hipStreamNonBlocking));
                HIP_TRY(r->pub_ev[(r->submitted - 1) % (size_t)r->depth].order(r->hst.get()));
                hipError_t he = ndt_launch_match_stream(r->queue.get(), r->stream_nn, r->stream_slots, (unsigned)n_cu - r->stream_groups, r->hst.get(),
                                                        r->stream_cov);
                if (he != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: helper launch", he);
            }
            r->helped = r->submitted;
        }
        HIP_TRY(hipStreamSynchronize(r->bst.get()));
        if (r->bst2.get()) HIP_TRY(hipStreamSynchronize(r->bst2.get()));
        HIP_TRY(hipStreamSynchronize(r->pst.get()));
        HIP_TRY(hipStreamSynchronize(r->mst.get()));
        if (r->hst.get()) HIP_TRY(hipStreamSynchronize(r->hst.get()));
        if (getenv("NDTGPU_REG_TRACE") && r->submitted) {
            // (experiments: when the last batches were published -- their maps built -- and when their last registration finished,
            //  in microseconds after the first of them)
            const size_t nb = std::min<size_t>(r->submitted, ndt_stream_stamps());
            unsigned long long t0 = 0;
            for (size_t k = r->submitted - nb; k < r->submitted; k++) {
                unsigned long long st[2] = {0, 0};
                HIP_TRY(ndt_stream_read_stamps(r->queue.get(), (unsigned)k, st));
                if (!t0) t0 = st[0];
                float b0 = 0.f, b1 = 0.f;          // the build's start and end, against the end of the first listed build (~ its publication)
                const size_t kref = std::max(r->submitted - nb, r->trace_first);
                if (!r->trace_ev.empty() && k >= kref) {
                    (void)hipEventElapsedTime(&b0, r->trace_ev[2 * (kref % 64) + 1].get(), r->trace_ev[2 * (k % 64)].get());
                    (void)hipEventElapsedTime(&b1, r->trace_ev[2 * (kref % 64) + 1].get(), r->trace_ev[2 * (k % 64) + 1].get());
                    (void)hipGetLastError();
                }
                if (k == kref) t0 = st[0];
                fprintf(stderr, "[ndtgpu trace] batch %zu build %+.1f .. %+.1f us, published %+.1f us, done %+.1f us\n", k, 1e3 * b0, 1e3 * b1,
                        ((double)st[0] - (double)t0) * 0.01, ((double)st[1] - (double)t0) * 0.01);
            }
        }
        unsigned aborted = 0;
        HIP_TRY(hipMemcpy(&aborted, r->queue.get() + ndt_stream_abort_offset(), sizeof aborted, hipMemcpyDeviceToHost));
        if (aborted) {
            // Reported ONCE: the registrations of the batches that were cut short carry exit_code -4 (every result starts as
            // "not run" when its batch is published), the queue is put back to "everything submitted is over", and the
            // registrar can be used again.
            HIP_TRY(ndt_stream_reset(r->queue.get(), (unsigned)r->submitted, (unsigned)r->depth));
            return fail(NDTGPU_ERR_HIP, "registrar: the stream-fed matcher gave up (no work, or no progress behind a wait, for ~30 s); "
                                        "registrations that did not run report exit_code -4");
        }
        return NDTGPU_OK;
    }
    for (int k = 0; k < r->depth; k++) HIP_TRY(hipStreamSynchronize(r->streams[k].get()));
    for (int k = 0; k < r->depth && (size_t)k < r->submitted; k++) {
        int aborted = 0;
        ndtgpu_status rc = ndtgpu_match_aborted(r->sets[k].get(), &aborted);
        if (rc != NDTGPU_OK) return rc;
        if (aborted) return fail(NDTGPU_ERR_HIP, "registrar: a matcher launch gave up (a wave found no work for ~1 s)");
    }
    return NDTGPU_OK;
}

// Host clouds in, host poses out: the reference's call sites hold pcl::PointCloud objects in host memory.  Sub-batch after
// sub-batch the scans travel to a device staging area of the slot they will be built in (one copy stream; the copies of
// sub-batch j + 1 run under the builds and registrations of sub-batch j), then the device entry takes over; poses and results
// come back with one copy each when everything is done.  Synchronous.
static ndtgpu_status register_batch_host_core(ndtgpu_registrar *r, const void *targets_host, const void *sources_host, size_t n_points,
                                              size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                              const ndtgpu_cell_params *cell, double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                              ndtgpu_match_result *results, int cov_mode, double *cov36, int32_t *cov_flags)
{
    if (!r || (n_pairs && (!T16 || !results || (n_points && (!targets_host || !sources_host)))) || stride_bytes < 12 ||
        (stride_bytes & 3) || n_points > 0xFFFFFFFFull || (n_pairs > 1 && map_stride_bytes < n_points * stride_bytes))
        return fail(NDTGPU_ERR_INVALID, "register_batch_host: bad argument (clouds must not overlap: map_stride_bytes >= n_points * stride_bytes)");
    const bool with_cov = cov_mode >= 0;
    if (with_cov && n_pairs && (!cov36 || !cov_flags)) return fail(NDTGPU_ERR_INVALID, "register_batch_cov_host: bad argument (cov36 / cov_flags)");
    if (n_pairs == 0) return NDTGPU_OK;
    if (!r->hcopy.get()) HIP_TRY(r->hcopy.create(hipStreamNonBlocking));
    if (r->hstage.empty()) r->hstage.resize(r->depth);
    const size_t bT = n_pairs * 16 * sizeof(double), bR = n_pairs * sizeof(ndtgpu_match_result);
    // (with the covariance: 36 doubles and a flag word per pair behind the results)
    const size_t bC = with_cov ? n_pairs * 36 * sizeof(double) : 0, bF = with_cov ? n_pairs * sizeof(int32_t) : 0;
    StageLayout io;
    const size_t offT = io.take(bT), offR = io.take(bR), offC = io.take(bC);
    const size_t offF = offC + bC, need_io = with_cov ? offF + bF : offR + bR;
    if (r->hio.capacity() < need_io) {
        HIP_TRY(hipStreamSynchronize(r->hcopy.get()));          // (the last call's copies)
        HIP_TRY(r->hio.reserve(need_io));
    }
    double *T_dev = (double *)(r->hio.get() + offT);
    ndtgpu_match_result *R_dev = (ndtgpu_match_result *)(r->hio.get() + offR);
    double *C_dev = with_cov ? (double *)(r->hio.get() + offC) : nullptr;
    int32_t *F_dev = with_cov ? (int32_t *)(r->hio.get() + offF) : nullptr;
    HIP_TRY(hipMemcpyAsync(T_dev, T16, bT, hipMemcpyHostToDevice, r->hcopy.get()));
    const size_t cloud_bytes = n_points * stride_bytes;
    for (size_t off = 0; off < n_pairs; off += r->per) {
        const size_t p = std::min(r->per, n_pairs - off);
        const int slot = (int)(r->submitted % (size_t)r->depth);
        const size_t half = (p - 1) * map_stride_bytes + cloud_bytes, half_al = p * map_stride_bytes;   // targets, then sources
        const size_t need = half_al + half;
        // the staging area of this slot is read by the build of the sub-batch that used it last: wait for that build
        if (r->submitted >= (size_t)r->depth) HIP_TRY(r->built[slot].sync());
        HIP_TRY(r->hstage[slot].reserve(need));
        char *tg = r->hstage[slot].get(), *sc = tg + half_al;        // sources follow targets: ONE build launch per sub-batch
        if (n_points) {
            HIP_TRY(hipMemcpyAsync(tg, (const char *)targets_host + off * map_stride_bytes, half, hipMemcpyHostToDevice, r->hcopy.get()));
            HIP_TRY(hipMemcpyAsync(sc, (const char *)sources_host + off * map_stride_bytes, half, hipMemcpyHostToDevice, r->hcopy.get()));
        }
        // (p <= pairs_per_batch: ONE sub-batch, in this slot, behind these copies)
        ndtgpu_status rc = register_batch_core(r, tg, sc, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T_dev + off * 16, p,
                                               prm, R_dev + off, (ndtgpu_stream)r->hcopy.get(), nullptr, cov_mode,
                                               with_cov ? C_dev + off * 36 : nullptr, with_cov ? F_dev + off : nullptr);
        if (rc != NDTGPU_OK) return rc;
    }
    ndtgpu_status rc = ndtgpu_registrar_sync(r);
    if (rc != NDTGPU_OK) return rc;
    HIP_TRY(hipMemcpy(T16, T_dev, bT, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(results, R_dev, bR, hipMemcpyDeviceToHost));
    if (with_cov) {
        HIP_TRY(hipMemcpy(cov36, C_dev, bC, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cov_flags, F_dev, bF, hipMemcpyDeviceToHost));
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_register_batch_host(ndtgpu_registrar *r, const void *targets_host, const void *sources_host, size_t n_points,
                                         size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                         const ndtgpu_cell_params *cell, double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                         ndtgpu_match_result *results)
{
    return register_batch_host_core(r, targets_host, sources_host, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16,
                                    n_pairs, prm, results, -1, nullptr, nullptr);
}

ndtgpu_status ndtgpu_register_batch_cov_host(ndtgpu_registrar *r, const void *targets_host, const void *sources_host, size_t n_points,
                                             size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                             const ndtgpu_cell_params *cell, double *T16, size_t n_pairs, const ndtgpu_match_params *prm,
                                             ndtgpu_match_result *results, int covariance_mode, double *cov36, int32_t *cov_flags)
{
    if (covariance_mode != 0 && covariance_mode != 1)
        return fail(NDTGPU_ERR_INVALID, "register_batch_cov_host: covariance_mode must be 0 or 1");
    return register_batch_host_core(r, targets_host, sources_host, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16,
                                    n_pairs, prm, results, covariance_mode, cov36, cov_flags);
}

}  // extern "C"
