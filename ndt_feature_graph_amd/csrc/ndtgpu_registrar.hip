// ndtgpu_registrar.hip -- the registrar of the C-ABI (include/ndtgpu.h): scans in, poses out.
#include "ndtgpu_host.h"
#include "ndtgpu_split.h"

#include <atomic>

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

// the experiment switches of the submit path: read once, when the registrar is created
struct RegKnobs {
    bool verbose = false, trace = false, probe = true, no_helper = false;
    int gap = 2;
};

// what a call of ndtgpu_register_batch_device / ndtgpu_register_batch_cov_device (cov_mode 0 / 1; < 0: no covariance) was given
struct BatchCall {
    const void *targets_dev, *sources_dev;
    size_t n_points, stride_bytes, map_stride_bytes;
    double range_limit;
    const ndtgpu_cell_params *cell;
    double *T16_dev;
    size_t n_pairs;
    const ndtgpu_match_params *prm;
    ndtgpu_match_result *results_dev;
    int cov_mode;
    double *cov36_dev;
    int32_t *cov_flags_dev;
    ndtgpu_stream stream;
    uint64_t *ticket;
    NdtMatchParamsDev pdev;            // `prm` in its device form, checked (register_batch_core)
    bool with_cov() const { return cov_mode >= 0; }
    double *cov36(size_t off) const { return with_cov() ? cov36_dev + off * 36 : nullptr; }
    int32_t *cov_flags(size_t off) const { return with_cov() ? cov_flags_dev + off : nullptr; }
};

struct ndtgpu_registrar {
    size_t per = 0;
    int depth = 0;
    ndtgpu_registrar_params prm{};     // as given to ndtgpu_registrar_create_ex (zeros resolved)
    RegKnobs knobs;
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
    RecalWindow recal;                 // the cells per map the split stands for and those of the last sub-batches seen (ndtgpu_split.h)
    PinnedBuffer<unsigned long long> stat_host; // [depth][2]: {Gaussian cells of the slot's maps, sub-batch + 1} written by a
                                             // one-workgroup kernel behind the build (no copy engine, no event: a device-to-host
                                             // copy per sub-batch cost the pipeline a quarter of its rate, measured)
    std::vector<long long> stat_seq;   // sub-batch whose counters slot k was asked for (-1: none / consumed)
    std::vector<unsigned> stat_maps;
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
    ndtgpu_status drain(bool ignore_errors = false);
    ndtgpu_status new_mark(long long seq, ProfMark **out_mark);
    ndtgpu_status build_pairs(const BatchCall &c, ndtgpu_mapset *set, size_t off, size_t p, hipStream_t st);
    ndtgpu_status trace_record(size_t j, int end, hipStream_t st);
    ndtgpu_status poll_map_stats(size_t j, int slot);
    ndtgpu_status measure_clocks(const BatchCall &c, size_t off, size_t p, size_t j, int slot, hipStream_t st, SplitClocks &clk);
    ndtgpu_status time_build(const BatchCall &c, size_t off, size_t p, int slot, unsigned groups, double *ms);
    ndtgpu_status calibrate(const BatchCall &c, size_t off, size_t p, size_t j, int slot, hipStream_t st);
    ndtgpu_status submit_stream_fed(const BatchCall &c);
    ndtgpu_status submit_per_batch(const BatchCall &c);
    ndtgpu_status print_trace();
};

// The streams of the stream-fed form, waited for by the host -- the ONLY place that lists them: an instance change at submit, a
// re-measurement, ndtgpu_registrar_sync and (ignoring errors) ndtgpu_registrar_destroy.
ndtgpu_status ndtgpu_registrar::drain(bool ignore_errors)
{
    for (Stream *st : {&bst, &bst2, &pst, &mst, &hst}) {
        if (!st->get()) continue;
        const hipError_t e = hipStreamSynchronize(st->get());
        if (e != hipSuccess && !ignore_errors) return fail(NDTGPU_ERR_HIP, "registrar: hipStreamSynchronize", e);
    }
    return NDTGPU_OK;
}


ndtgpu_status ndtgpu_registrar_destroy(ndtgpu_registrar *r)
{
    if (!r) return NDTGPU_OK;
    // every stream drained before the first one goes (a device-side wait on one of them ends with the matcher's progress on another)
    for (Stream &st : r->streams) (void)hipStreamSynchronize(st.get());
    if (r->hcopy.get()) (void)hipStreamSynchronize(r->hcopy.get());
    // (the same streams as before drain() held the list, errors ignored; in drain()'s order, the matcher stream before the
    //  drain helper's, as ndtgpu_registrar_sync has always waited -- everything is submitted, so the order of the host's waits is free)
    (void)r->drain(true);
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
    r->knobs.verbose = getenv("NDTGPU_REG_VERBOSE") != nullptr;
    r->knobs.trace = getenv("NDTGPU_REG_TRACE") != nullptr;
    r->knobs.probe = env_int("NDTGPU_REG_PROBE", 1) != 0;
    r->knobs.no_helper = getenv("NDTGPU_REG_NO_HELPER") != nullptr;
    r->knobs.gap = env_int("NDTGPU_REG_GAP", 2);
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
    info->cells_per_map = r->recal.calib_cells;
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

ndtgpu_status ndtgpu_registrar::new_mark(long long seq, ProfMark **out_mark)
{
    ProfMark m{};
    m.seq = seq;
    for (int k = 0; k < (seq >= 0 ? 2 : 4); k++) HIP_TRY(m.e[k].create(hipEventDefault));
    marks.push_back(std::move(m));
    *out_mark = &marks.back();
    return NDTGPU_OK;
}

// the maps of the p pairs from `off` on: one build launch when the sources follow the targets in memory, else two
ndtgpu_status ndtgpu_registrar::build_pairs(const BatchCall &c, ndtgpu_mapset *set, size_t off, size_t p, hipStream_t st)
{
    const char *tg = (const char *)c.targets_dev + off * c.map_stride_bytes, *sc = (const char *)c.sources_dev + off * c.map_stride_bytes;
    if (sc == tg + p * c.map_stride_bytes)
        return ndtgpu_mapset_build(set, 0, 2 * p, tg, c.n_points, c.stride_bytes, c.map_stride_bytes, c.range_limit, nullptr, c.cell, st);
    ndtgpu_status rc = ndtgpu_mapset_build(set, 0, p, tg, c.n_points, c.stride_bytes, c.map_stride_bytes, c.range_limit, nullptr, c.cell, st);
    if (rc == NDTGPU_OK)
        rc = ndtgpu_mapset_build(set, p, p, sc, c.n_points, c.stride_bytes, c.map_stride_bytes, c.range_limit, nullptr, c.cell, st);
    return rc;
}

// NDTGPU_REG_TRACE: the start (end = 0) or the end of sub-batch j's build; the events are made on first use
ndtgpu_status ndtgpu_registrar::trace_record(size_t j, int end, hipStream_t st)
{
    if (trace_ev.empty()) {
        std::vector<Fence> ev(128);
        for (Fence &e : ev) HIP_TRY(e.create(hipEventDefault));
        trace_ev = std::move(ev);                                         // (all 128 or none)
    }
    HIP_TRY(trace_ev[2 * (j % 64) + (size_t)end].record(st));
    if (!end && trace_first == (size_t)-1) trace_first = j;
    return NDTGPU_OK;
}

// Have the maps changed?  The counters of earlier builds that have arrived on the host say how many Gaussian cells a map holds
// now; when the mean over the last sub-batches has left the figure the split was measured at by more than recalibrate_pct
// (RecalWindow, ndtgpu_split.h), the pipeline is drained once and sub-batch j measures the split again (a registrar that moves
// from halls to clutter would otherwise keep 128 matcher CUs where 200 are right).
ndtgpu_status ndtgpu_registrar::poll_map_stats(size_t j, int slot)
{
    if (!stat_host.get() || stream_groups == 0u) return NDTGPU_OK;
    // (back-pressure: the host runs at most `depth` sub-batches ahead of the builds -- without it a caller that
    //  never waits would have submitted everything before the first counters arrive)
    if (j >= (size_t)depth) HIP_TRY(built[slot].sync());
    for (int k = 0; k < depth; k++) {
        volatile unsigned long long *sh = stat_host.get() + 2 * k;
        if (stat_seq[k] < 0 || sh[1] != (unsigned long long)stat_seq[k] + 1ull) continue;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (stat_maps[k]) recal.sample((double)sh[0] / (double)stat_maps[k], depth);
        stat_seq[k] = -1;
    }
    double mean = 0;
    if (!recal.should_remeasure(j, depth, prm.recalibrate_pct, &mean)) return NDTGPU_OK;
    if (knobs.verbose)
        fprintf(stderr, "ndtgpu registrar: %.0f cells per map where the split was measured at %.0f: measuring again\n", mean, recal.calib_cells);
    ndtgpu_status drc = drain();
    if (drc != NDTGPU_OK) return drc;
    stream_groups = 0u;
    recal.recal_ref = mean;
    return NDTGPU_OK;
}

// The first half of a measurement: sub-batch j's maps are built and its pairs registered on `st` with nothing else on the device
// (the whole chip each; the same bits), its batch is marked as done in the queue, and the host reads the kernels' own clocks.
// Costs one synchronisation.
ndtgpu_status ndtgpu_registrar::measure_clocks(const BatchCall &c, size_t off, size_t p, size_t j, int slot, hipStream_t st, SplitClocks &clk)
{
    ndtgpu_mapset *set = sets[slot].get();
    ProfMark *mk0 = nullptr;
    if (profiling) { ndtgpu_status mrc = new_mark(-1, &mk0); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk0->e[0].record(st)); }
    ndtgpu_status rc0 = build_pairs(c, set, off, p, st);
    if (rc0 != NDTGPU_OK) return rc0;
    if (mk0) { HIP_TRY(mk0->e[1].record(st)); HIP_TRY(mk0->e[2].record(st)); }
    const unsigned saved_groups = set->match_groups;
    set->match_groups = 0;                            // (the whole chip)
    rc0 = match_batch_device_ex(set, iota.get(), set, iota.get() + p, c.T16_dev + off * 16, p, c.prm, c.results_dev + off, st, c.cov_mode,
                                c.cov36(off), c.cov_flags(off), nullptr);
    set->match_groups = saved_groups;
    if (rc0 != NDTGPU_OK) return rc0;
    if (mk0) HIP_TRY(mk0->e[3].record(st));
    hipError_t se = ndt_stream_skip(queue.get(), (unsigned)j, st);
    if (se != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: calibration", se);
    HIP_TRY(built[slot].record(st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<NdtMapCounters> ctr(2 * p);
    std::vector<ndtgpu_match_result> res(p);
    HIP_TRY(hipMemcpy(ctr.data(), set->v.counters, 2 * p * sizeof(NdtMapCounters), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(res.data(), c.results_dev + off, p * sizeof(ndtgpu_match_result), hipMemcpyDeviceToHost));
    for (const NdtMapCounters &m : ctr) clk.add_map(m.cyc, m.n_cells);
    for (const ndtgpu_match_result &q : res)
        if (!clk.add_result((long long)q.cycles_eval, (long long)q.cycles_solver) && knobs.verbose && clk.n_bad <= 4)
            fprintf(stderr, "ndtgpu registrar: calibration result %zu: cycles_eval %lld cycles_solver %lld iterations %d exit %d\n",
                    (size_t)(&q - res.data()), (long long)q.cycles_eval, (long long)q.cycles_solver, (int)q.iterations, (int)q.exit_code);
    clk.finish();
    return NDTGPU_OK;
}

// What the builds of the sub-batch take beside `groups` matcher CUs: built again (same maps, same bits) on a stream that owns
// exactly the other CUs (Stream::create_cu_mask: mask bits are dealt to the XCDs in turn, like the CUs a matcher instance
// leaves), timed with events.
ndtgpu_status ndtgpu_registrar::time_build(const BatchCall &c, size_t off, size_t p, int slot, unsigned groups, double *ms)
{
    hipStream_t ms_st = nullptr;
    ndtgpu_status prc = masked_stream((unsigned)n_cu - groups, &ms_st);
    if (prc != NDTGPU_OK) return prc;
    HIP_TRY(probe_ev[0].create(hipEventDefault));
    HIP_TRY(probe_ev[1].create(hipEventDefault));
    float best = 0.f;
    for (int rep = 0; rep < 2; rep++) {                    // (the first launch on a new stream pays for the stream)
        HIP_TRY(probe_ev[0].record(ms_st));
        prc = build_pairs(c, sets[slot].get(), off, p, ms_st);
        if (prc != NDTGPU_OK) return prc;
        HIP_TRY(probe_ev[1].record(ms_st));
        HIP_TRY(probe_ev[1].sync());
        float e = 0.f;
        HIP_TRY(hipEventElapsedTime(&e, probe_ev[0].get(), probe_ev[1].get()));
        if (rep == 0 || e < best) best = e;
    }
    *ms = (double)best;
    return NDTGPU_OK;
}

// A sub-batch that measures the split of the chip (the first of a registrar's life; later ones after a drain, poll_map_stats):
// from the clocks of its kernels -- CU-time of the builds B and of the registrations M -- a matcher instance gets n_cu M / (M + B)
// CUs from then on, refined by whole build rounds and, since 0.6.5, by timing the builds on the CUs they would be left: 128 of
// 256 on the bench's halls, 200 on a cluttered scene whose maps hold five times the cells.  Every decision is ndtgpu_split.h's;
// here is the device work.  A few build launches, once per measurement; NDTGPU_REG_PROBE=0 keeps the model.
ndtgpu_status ndtgpu_registrar::calibrate(const BatchCall &c, size_t off, size_t p, size_t j, int slot, hipStream_t st)
{
    SplitClocks clk;
    ndtgpu_status rc = measure_clocks(c, off, p, j, slot, st, clk);
    if (rc != NDTGPU_OK) return rc;
    stream_groups = split_model(clk.B, clk.M_raw, p, n_cu);
    if (clk.B > 0 && clk.M_raw > 0 && knobs.probe) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device) != hipSuccess) khz = 0;
        const SplitSearch s = split_probe_search(stream_groups, 2 * p, n_cu, clk.M_raw, split_clk_per_ms(khz),
                                                 [&](unsigned g, double *ms) { return time_build(c, off, p, slot, g, ms) == NDTGPU_OK; });
        if (!s.ok) {
            (void)hipGetLastError();                               // (no masked streams on this device / runtime: the model's split stands)
            g_err.clear();
        } else if (knobs.verbose) {
            for (const SplitCand &q : s.cand)
                fprintf(stderr, "ndtgpu registrar: %u matcher CUs: builds %.3f ms on the other %u, registrations %.3f ms -> %.3f ms per sub-batch%s\n",
                        q.g, q.build_ms, (unsigned)n_cu - q.g, q.match_ms, q.t_ms, q.g == s.groups ? "  <-" : "");
        }
        stream_groups = s.groups;
        // (the probe streams go at once: each is a hardware queue of its own and of no use until the next measurement;
        //  creating them is most of what a measurement costs, ~50 ms with three or four candidates)
        masked.clear();
        HIP_TRY(built[slot].record(st));               // (the maps were rebuilt: same contents)
    }
    calibrations++;
    const double cells_per_map = split_cells_per_map(clk.cells, p);
    if (prm.matcher_slots == 0) stream_slots = split_slots(cells_per_map);
    recal.measured(cells_per_map, j);
    for (long long &q : stat_seq) q = -1;
    if (knobs.verbose)
        fprintf(stderr, "ndtgpu registrar: build %.3g, registrations %.3g CU-clocks per sub-batch, %.0f cells per map -> matcher instances of %u workgroups\n",
                clk.B, split_matcher_clocks(clk.M_raw), recal.calib_cells, stream_groups);
    return NDTGPU_OK;
}

// Stream-fed form: builds on two streams in turn, batches published in order to the running matcher instance.
ndtgpu_status ndtgpu_registrar::submit_stream_fed(const BatchCall &c)
{
    // (an instance is compiled for one neighbourhood size, and with or without the covariance tail)
    if (stream_nn != c.pdev.n_neighbours || stream_cov != (c.with_cov() ? 1 : 0)) {
        if (stream_nn >= 0) { ndtgpu_status drc = drain(); if (drc != NDTGPU_OK) return drc; }
        stream_nn = c.pdev.n_neighbours;
        stream_cov = c.with_cov() ? 1 : 0;
    }
    for (size_t off = 0; off < c.n_pairs; off += per) {
        const size_t p = std::min(per, c.n_pairs - off);
        const size_t j = submitted;
        const int slot = (int)(j % (size_t)depth);
        ndtgpu_mapset *set = sets[slot].get();
        hipStream_t st = (bst2.get() && (j & 1u)) ? bst2.get() : bst.get();
        ndtgpu_status rc = poll_map_stats(j, slot);
        if (rc != NDTGPU_OK) return rc;
        HIP_TRY(in_ev.order(st));
        if (stream_groups == 0u) {
            rc = calibrate(c, off, p, j, slot, st);
            if (rc != NDTGPU_OK) return rc;
            submitted++;
            if (c.ticket) *c.ticket = (uint64_t)submitted;
            continue;
        }
        // This map set was last used by sub-batch j - depth: its registrations must be complete before it is rebuilt.
        // (Depth: a batch is complete 3-5 ms after its publication; with 8 map sets the builds never wait for that, 4 cost
        //  ~5 % on the bench -- include/ndtgpu.h.)
        if (j >= (size_t)depth) {
            hipError_t we = ndt_stream_wait(queue.get(), (unsigned)depth, (unsigned)(j - (size_t)depth), st);
            if (we != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: wait launch", we);
        }
        ProfMark *mk = nullptr;
        if (profiling) { ndtgpu_status mrc = new_mark((long long)j, &mk); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk->e[0].record(st)); }
        if (knobs.trace) { rc = trace_record(j, 0, st); if (rc != NDTGPU_OK) return rc; }
        rc = build_pairs(c, set, off, p, st);
        if (rc != NDTGPU_OK) return rc;
        if (knobs.trace) { rc = trace_record(j, 1, st); if (rc != NDTGPU_OK) return rc; }
        if (mk) HIP_TRY(mk->e[1].record(st));
        if (stat_host.get() && stat_seq[slot] < 0 && j % 3u == 0u) {
            // (how many Gaussian cells the maps of this build hold: one small kernel behind it writes the sum to the host.
            //  Every third sub-batch: the launch costs the build stream a few microseconds -- 2 % of the bench's rate when
            //  every sub-batch had one -- and an odd period does not lock onto callers that alternate between two scenes)
            hipLaunchKernelGGL(ndt_reg_stats_kernel, dim3(1), dim3(256), 0, st, set->v.counters, (unsigned)(2 * p), (unsigned long long)j,
                               stat_host.get() + 2 * slot);
            HIP_TRY(hipGetLastError());
            stat_seq[slot] = (long long)j;
            stat_maps[slot] = (unsigned)(2 * p);
        }
        HIP_TRY(built[slot].record(st));
        HIP_TRY(built[slot].order(pst.get()));
        hipError_t pe = ndt_stream_publish(queue.get(), set->v, c.T16_dev + off * 16, reinterpret_cast<NdtMatchResultDev *>(c.results_dev + off),
                                           c.pdev, (unsigned)p, (unsigned)j, pst.get(), c.with_cov() ? c.cov_mode : -1, c.cov36(off),
                                           c.cov_flags(off));
        if (pe != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: publish", pe);
        HIP_TRY(pub_ev[slot].record(pst.get()));
        // every published batch is followed by an instance launch: it starts when the running instance has ended (and
        // then serves this batch and whatever is published while it runs), or finds the batch taken and leaves
        HIP_TRY(pub_ev[slot].order(mst.get()));
        pe = ndt_launch_match_stream(queue.get(), c.pdev.n_neighbours, stream_slots, stream_groups, mst.get(), stream_cov);
        if (pe != hipSuccess) return fail(NDTGPU_ERR_HIP, "registrar: matcher launch", pe);
        submitted++;
        if (c.ticket) *c.ticket = (uint64_t)submitted;
    }
    return NDTGPU_OK;
}

// One matcher launch per sub-batch, on the stream of the sub-batch's map set.
ndtgpu_status ndtgpu_registrar::submit_per_batch(const BatchCall &c)
{
    if (c.with_cov() && !cov_save.get()) {
        // (only grid-barrier / pool sub-batches read it -- sets of large maps, at most half as many pairs as CUs.  Made once and
        //  never replaced: nothing to wait for)
        const size_t n = std::min(per, (size_t)n_cu);
        HIP_TRY(cov_save.reserve((size_t)depth * n * 16));
        cov_save_pairs = n;
    }
    for (size_t off = 0; off < c.n_pairs; off += per) {
        const size_t p = std::min(per, c.n_pairs - off);
        const int slot = (int)(submitted % (size_t)depth);
        hipStream_t st = streams[slot].get();
        ndtgpu_mapset *set = sets[slot].get();
        HIP_TRY(in_ev.order(st));
        if (last_built >= 0 && last_built != slot) HIP_TRY(built[last_built].order(st));
        ProfMark *mk = nullptr;
        if (profiling) { ndtgpu_status mrc = new_mark(-1, &mk); if (mrc != NDTGPU_OK) return mrc; HIP_TRY(mk->e[0].record(st)); }
        ndtgpu_status rc = build_pairs(c, set, off, p, st);
        if (rc != NDTGPU_OK) return rc;
        if (mk) { HIP_TRY(mk->e[1].record(st)); HIP_TRY(mk->e[2].record(st)); }
        HIP_TRY(built[slot].record(st));
        last_built = slot;
        // `built` releases the next sub-batch's build AND, on this stream, this sub-batch's matcher.  The matcher's persistent
        // workgroups (one per CU, all registers and LDS of it) must not be placed first: the build would then only get the CUs
        // the matcher leaves, its end -- which releases the build after it -- moves out, and the pipeline loses a tenth of its
        // rate (measured: 430 k against 470 k registrations/s).  Two 4-byte fills keep this stream busy for the few
        // microseconds the next build's dispatch needs to get ahead (NDTGPU_REG_GAP: their number).
        if (depth > 1)
            for (int g = 0; g < knobs.gap; g++) HIP_TRY(hipMemsetAsync(iota.get() + 2 * per, 0, 4, st));
        rc = match_batch_device_ex(set, iota.get(), set, iota.get() + p, c.T16_dev + off * 16, p, c.prm, c.results_dev + off, st, c.cov_mode,
                                   c.cov36(off), c.cov_flags(off),
                                   c.with_cov() && p <= cov_save_pairs ? cov_save.get() + (size_t)slot * cov_save_pairs * 16 : nullptr);
        if (rc != NDTGPU_OK) return rc;
        if (mk) HIP_TRY(mk->e[3].record(st));
        HIP_TRY(done[submitted % done.size()].record(st));
        submitted++;
        if (c.ticket) *c.ticket = (uint64_t)submitted;      // "every sub-batch before this count"
    }
    return NDTGPU_OK;
}

// ndtgpu_register_batch_device (cov_mode < 0) and ndtgpu_register_batch_cov_device (cov_mode 0 / 1): one code path
static ndtgpu_status register_batch_core(ndtgpu_registrar *r, BatchCall &c)
{
    if (c.ticket) *c.ticket = r ? (uint64_t)r->submitted : 0;
    if (!r || (c.n_pairs && (!c.T16_dev || !c.results_dev || (c.n_points && (!c.targets_dev || !c.sources_dev)))) || c.stride_bytes < 12 ||
        (c.stride_bytes & 3) || c.n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "register_batch_device: bad argument");
    if (c.with_cov() && c.n_pairs && (!c.cov36_dev || !c.cov_flags_dev))
        return fail(NDTGPU_ERR_INVALID, "register_batch_cov_device: bad argument (cov36_dev / cov_flags_dev)");
    if (c.n_pairs == 0) return NDTGPU_OK;
    { ndtgpu_status prc = match_params_dev(c.prm, 0, c.pdev); if (prc != NDTGPU_OK) return prc; }
    HIP_TRY(r->in_ev.record((hipStream_t)c.stream));
    return r->queue.get() ? r->submit_stream_fed(c) : r->submit_per_batch(c);
}

ndtgpu_status ndtgpu_register_batch_device(ndtgpu_registrar *r, const void *targets_dev, const void *sources_dev, size_t n_points,
                                           size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                           const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                           const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev, ndtgpu_stream stream,
                                           uint64_t *ticket)
{
    BatchCall c{targets_dev, sources_dev, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16_dev, n_pairs, prm, results_dev,
                -1, nullptr, nullptr, stream, ticket, {}};
    return register_batch_core(r, c);
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
    BatchCall c{targets_dev, sources_dev, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T16_dev, n_pairs, prm, results_dev,
                covariance_mode, cov36_dev, cov_flags_dev, stream, ticket, {}};
    return register_batch_core(r, c);
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

// NDTGPU_REG_TRACE, at a sync: what the queue and the trace events saw of the last batches
ndtgpu_status ndtgpu_registrar::print_trace()
{
    // (experiments: when the last batches were published -- their maps built -- and when their last registration finished,
    //  in microseconds after the first of them)
    const size_t nb = std::min<size_t>(submitted, ndt_stream_stamps());
    unsigned long long t0 = 0;
    for (size_t k = submitted - nb; k < submitted; k++) {
        unsigned long long st[2] = {0, 0};
        HIP_TRY(ndt_stream_read_stamps(queue.get(), (unsigned)k, st));
        if (!t0) t0 = st[0];
        float b0 = 0.f, b1 = 0.f;          // the build's start and end, against the end of the first listed build (~ its publication)
        const size_t kref = std::max(submitted - nb, trace_first);
        if (!trace_ev.empty() && k >= kref) {
            (void)hipEventElapsedTime(&b0, trace_ev[2 * (kref % 64) + 1].get(), trace_ev[2 * (k % 64)].get());
            (void)hipEventElapsedTime(&b1, trace_ev[2 * (kref % 64) + 1].get(), trace_ev[2 * (k % 64) + 1].get());
            (void)hipGetLastError();
        }
        if (k == kref) t0 = st[0];
        fprintf(stderr, "[ndtgpu trace] batch %zu build %+.1f .. %+.1f us, published %+.1f us, done %+.1f us\n", k, 1e3 * b0, 1e3 * b1,
                ((double)st[0] - (double)t0) * 0.01, ((double)st[1] - (double)t0) * 0.01);
    }
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
        if (r->submitted > r->helped && r->stream_groups && r->stream_nn >= 0 && !r->knobs.no_helper) {
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
        ndtgpu_status drc = r->drain();
        if (drc != NDTGPU_OK) return drc;
        if (r->knobs.trace && r->submitted) { drc = r->print_trace(); if (drc != NDTGPU_OK) return drc; }
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
        BatchCall c{tg, sc, n_points, stride_bytes, map_stride_bytes, range_limit, cell, T_dev + off * 16, p, prm, R_dev + off,
                    cov_mode, with_cov ? C_dev + off * 36 : nullptr, with_cov ? F_dev + off : nullptr, (ndtgpu_stream)r->hcopy.get(), nullptr, {}};
        ndtgpu_status rc = register_batch_core(r, c);
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
