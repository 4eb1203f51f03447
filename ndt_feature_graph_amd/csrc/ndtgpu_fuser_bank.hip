// ndtgpu_fuser_bank.hip -- the fuser bank of the C-ABI (include/ndtgpu.h).
#include "ndtgpu_featbank.h"
#include "ndt_fuserfeat.h"

extern "C" {

// ---- the fuser bank: NDTFeatureFuserHMT::update for a batch of independent fusers as ONE call (include/ndtgpu.h) ----------
// Per call and slot: [host] the odometry model, the soft-constraint covariance, the odometry cells, the scan frame and the scan
// map's centre (ndtgpu_fuser_prepare) -> ONE upload -> [device] scan into the node map's frame, scan map build, matchFusion
// against the slot's node map, the matcher's covariance, the post-registration step (pose, gates, accumulated covariance),
// scan into the frame of the new pose, ray-traced fuse-in.  No host round trip in between; the host looks at the poses when it
// asks for them (ndtgpu_fuser_poses) or at the next call, which needs them.
// With a feature bank attached the *_feat entries add the FLIRT feature path to the same call (:245-334, 497-502): RANSAC of the
// scan's interest points against the previous scan's (ndt_featmatch_kernel) -> gate and cell records IN FRONT of the odometry
// cells (csrc/ndt_fuserfeat.hip; the host uploads the odometry cells' values only) -> ... the steps above ... -> behind the post
// step: prev <- cur moved to the new pose, appended to the slot's feature map.  The plain entries share their body with them
// (fuser_initialize_core / fuser_update_core) and leave the feature state alone.

struct ndtgpu_fuser_bank {
    ndtgpu_fuser_params prm{};
    size_t n = 0;
    ndtgpu_mapset *nodes = nullptr;               // the node maps: the caller's (borrowed), or own_nodes (below)
    struct HostState {
        NdtFuserState s{};
        double Todom[16];
        bool is_init = false;
    };
    std::vector<HostState> st;
    DeviceBuffer<NdtFuserState> st_dev;
    DeviceBuffer<double> sensor_pose_dev;
    // staging of one call: a pinned block and its device twin
    //   [count] Tscan16 | Tmotion16 | Test16 | Q36 | origins3 | centres3 | feat cells (40 x 18) | feat offsets | idx | spose16 | fuse origins3 |
    //   match results | cov36 | cov flags | results
    PinnedBuffer<char> pin;
    DeviceBuffer<char> dev;
    DeviceBuffer<float> xyz_a, xyz_b;             // the scans in the node frame before / after the registration (packed xyz)
    DeviceBuffer<char> xyz_in;                    // host clouds (the *_host entries) on their way in
    Fence done;                                   // recorded behind the last call's launches; valid: that call is in flight
    size_t fl_first = 0, fl_count = 0;
    size_t off_res = 0, off_pin_res = 0;          // where the in-flight call's results sit in the staging block
    hipStream_t fl_stream = nullptr;
    // the feature path (ndtgpu_fuser_bank_attach_features): a borrowed feature bank, slot k's prev / map sets, per slot the
    // NDTFeatureMap counter and whether the last call moved prev into the map frame
    ndtgpu_featbank *fb = nullptr;
    size_t prev_first = 0, map_first = 0;
    ndtgpu_fuser_feat_params fprm{};
    std::vector<uint32_t> feat_counter;
    std::vector<unsigned char> prev_moved;
    size_t ff_first = 0, ff_count = 0, off_pin_frec = 0;      // the last _feat call's records in the pinned block
    size_t cl_first = 0, cl_count = 0, off_foff = 0, off_cells = 0;   // the last update call's cell records in the device block
    // the owned map sets after the buffers: they go first, and ndtgpu_mapset_destroy's hipDeviceSynchronize covers the buffers
    // above too, also after a call that failed midway on a stream of the caller's and never recorded `done`
    MapsetOwner own_nodes, scans;
    Stream own_st;                                // the *_host entries' stream (last: ndtgpu_resource.h)
};

namespace {
struct FuserLayout {
    size_t Tscan, Tmotion, Test, Q, origin, centre, feat, foff, idx, spose, forigin, match, cov, covflag, res, total;
};
FuserLayout fuser_layout(size_t count, bool feat)
{
    FuserLayout L;
    StageLayout S;
    L.Tscan = S.take(count * 16 * sizeof(double));
    L.Tmotion = S.take(count * 16 * sizeof(double));
    L.Test = S.take(count * 16 * sizeof(double));
    L.Q = S.take(count * 36 * sizeof(double));
    L.origin = S.take(count * 3 * sizeof(double));
    L.centre = S.take(count * 3 * sizeof(double));
    L.feat = S.take(feat ? count * 40 * 18 * sizeof(double) : 0);
    L.foff = S.take((count + 1) * sizeof(uint32_t));
    L.idx = S.take(count * sizeof(uint32_t));
    L.spose = S.take(count * 16 * sizeof(double));
    L.forigin = S.take(count * 3 * sizeof(double));
    L.match = S.take(count * sizeof(NdtMatchResultDev));
    L.cov = S.take(count * 36 * sizeof(double));
    L.covflag = S.take(count * sizeof(int));
    L.res = S.take(count * sizeof(NdtFuserResultDev));
    L.total = S.at;
    return L;
}
// what a _feat call adds behind the plain call's block: [count] cur | prev | map set indices | slot flags | odometry cell values
// (18) || RANSAC records | T16 | corr (max_points x 2) | feature records | cell offsets | cells (64 x 18); the part before ||
// is uploaded
struct FuserFeatLayout {
    size_t cur, prev, map, flags, odom, upload_end, ransac, T16, corr, rec, foff, cells, total;
};
FuserFeatLayout fuser_feat_layout(size_t at, size_t count, size_t max_points, bool cells)
{
    FuserFeatLayout F;
    StageLayout S;
    S.at = at;
    F.cur = S.take(count * sizeof(uint32_t));
    F.prev = S.take(count * sizeof(uint32_t));
    F.map = S.take(count * sizeof(uint32_t));
    F.flags = S.take(count * sizeof(uint32_t));
    F.odom = S.take(count * 18 * sizeof(double));
    F.upload_end = S.at;
    F.ransac = S.take(count * sizeof(ndtgpu_featmatch_result));
    F.T16 = S.take(count * 16 * sizeof(double));
    F.corr = S.take(cells ? count * max_points * 2 * sizeof(uint32_t) : 0);
    F.rec = S.take(count * sizeof(ndtgpu_fuser_feat_result));
    F.foff = S.take((count + 1) * sizeof(uint32_t));
    F.cells = S.take(cells ? count * NDT_FUSERFEAT_MAX_CELLS * 18 * sizeof(double) : 0);
    F.total = S.at;
    return F;
}
void pose_identity(double *T) { for (int q = 0; q < 16; q++) T[q] = (q % 5 == 0) ? 1.0 : 0.0; }
}  // namespace

static_assert(sizeof(ndtgpu_fuser_result) == sizeof(NdtFuserResultDev), "fuser result layouts must agree");

void ndtgpu_default_fuser_params(ndtgpu_fuser_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    // NDTFeatureFuserHMT::Params() (ndt_feature_fuser_hmt.h:58-101)
    p->resolution = 1.0;
    p->map_size_x = 40.0; p->map_size_y = 40.0; p->map_size_z = 10.0;
    p->sensor_range = 3.0;
    p->max_translation_norm = 1.0;
    p->max_rotation_norm = M_PI / 4.0;
    p->check_consistency = 0;
    p->fuse_incomplete = 0;
    p->use_odom = 1;
    p->neighbours = 0;
    p->stepcontrol = 1;
    p->itr_max = 30;
    p->delta_score = 10e-4;
    p->force_odom_as_est = 0;
    p->fusion2d = 0;
    p->all_matches_valid = 0;
    p->use_soft_constraints = 1;
    p->compute_cov = 1;
    p->step_control_fusion = 1;
    p->use_tikhonov = 1;
    p->covariance_mode = 0;
    // MotionModel2d::Params() (motion_model.hpp:128-136)
    p->motion_Cd = 0.001; p->motion_Ct = 0.001; p->motion_Dd = 0.005; p->motion_Dt = 0.005; p->motion_Td = 0.001; p->motion_Tt = 0.001;
    pose_identity(p->sensor_pose);
    p->max_cells = 0;
}

ndtgpu_status ndtgpu_fuser_prepare(const ndtgpu_fuser_params *prm, const double Tnow16[16], const double Tmotion16[16],
                                   const double node_centre[3], ndtgpu_fuser_prepared *out)
{
    if (!prm || !Tnow16 || !Tmotion16 || !node_centre || !out) return fail(NDTGPU_ERR_INVALID, "fuser_prepare: null argument");
    if (!(prm->resolution > 0)) return fail(NDTGPU_ERR_INVALID, "fuser_prepare: resolution");
    // fuser_hmt.cpp:124-146 -- the odometry "constraints" (MotionModel2d::getMeasurementCov, motion_model.cpp:190-207)
    double e3[3];
    ndt_euler012(Tmotion16, e3);
    const double rx = Tmotion16[12], ry = Tmotion16[13], rot = e3[2];
    const double dist = std::sqrt(rx * rx + ry * ry);
    const double R00 = prm->motion_Dd * dist * dist + prm->motion_Dt * rot * rot;
    const double R11 = prm->motion_Cd * dist * dist + prm->motion_Ct * rot * rot;
    const double R22 = prm->motion_Td * dist * dist + prm->motion_Tt * rot * rot;
    for (double &v : out->odom_cov) v = 0.0;
    out->odom_cov[0] = R00; out->odom_cov[4] = R11;
    out->odom_cov[8] = 0.01;                       // "the height in the ndt feature vec and not rotational variance"
    for (double &v : out->Tcov) v = 0.0;
    for (int a = 0; a < 6; a++) out->Tcov[a * 6 + a] = 1.0;
    out->Tcov[0] = R00; out->Tcov[7] = R11; out->Tcov[35] = R22;     // getCovMatrix6; (2,2) = (3,3) = (4,4) = 1 (:144-146)
    // :166-190 (globalTransf): the scan goes to the node map's frame by Tinit * sensor_pose, Tinit = Tnow
    ndt_pose_mul(Tnow16, prm->sensor_pose, out->Tscan);
    for (int a = 0; a < 3; a++) {
        out->range_origin[a] = out->Tscan[12 + a];
        // loadPointCloudCentroid (:201-202): the scan map's centre on the lattice of the node map's
        const double diff = out->range_origin[a] - node_centre[a];
        out->scan_centre[a] = node_centre[a] + std::floor(diff / prm->resolution) * prm->resolution;
    }
    // :291-334 -- the odometry cells: a pair (previous pose + motion | current pose), both moved into the node map's frame
    // by Tnow (pseudoTransformNDTMap: mean' = T mean, cov' = R cov R^T); the LAST current cell keeps the un-rotated covariance
    double RC[9], RCRt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s2 = 0;
            for (int k = 0; k < 3; k++) s2 += Tnow16[k * 4 + i] * out->odom_cov[k * 3 + j];
            RC[i * 3 + j] = s2;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s2 = 0;
            for (int k = 0; k < 3; k++) s2 += RC[i * 3 + k] * Tnow16[k * 4 + j];
            RCRt[i * 3 + j] = s2;
        }
    const int ij[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int k = 0; k < 6; k++) {
        out->feat_cov_rotated[k] = RCRt[ij[k][0] * 3 + ij[k][1]];
        out->feat_cov_plain[k] = out->odom_cov[ij[k][0] * 3 + ij[k][1]];
    }
    for (int a = 0; a < 3; a++) {
        out->feat_src_mean[a] = Tnow16[12 + a];                                                        // Tinit * 0
        out->feat_tgt_mean[a] = Tnow16[a] * Tmotion16[12] + Tnow16[4 + a] * Tmotion16[13] + Tnow16[8 + a] * Tmotion16[14] + Tnow16[12 + a];
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_bank_destroy(ndtgpu_fuser_bank *b)
{
    if (!b) return NDTGPU_OK;
    (void)b->done.sync();                         // (the call in flight, on whatever stream)
    delete b;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_bank_create(const ndtgpu_fuser_params *prm, size_t n_fusers, ndtgpu_mapset *node_maps, ndtgpu_fuser_bank **out)
{
    if (!prm || !out || n_fusers == 0) return fail(NDTGPU_ERR_INVALID, "fuser_bank_create: bad argument");
    if (!(prm->resolution > 0) || !(prm->sensor_range > 0) || prm->neighbours < 0 || prm->neighbours > 3 || prm->itr_max < 0)
        return fail(NDTGPU_ERR_INVALID, "fuser_bank_create: resolution / sensor_range must be positive, neighbours 0..3");
    if (!have_device()) return fail(NDTGPU_ERR_NO_DEVICE, "fuser_bank_create: no HIP device");
    if (node_maps && node_maps->n_maps < n_fusers) return fail(NDTGPU_ERR_INVALID, "fuser_bank_create: node_maps holds fewer maps than fusers");
    if (node_maps && node_maps->v.grid.res != prm->resolution) return fail(NDTGPU_ERR_INVALID, "fuser_bank_create: node_maps has another cell size");
    ndtgpu_fuser_bank *b = new (std::nothrow) ndtgpu_fuser_bank();
    if (!b) return fail(NDTGPU_ERR_ALLOC, "fuser_bank_create: host alloc");
    b->prm = *prm;
    b->n = n_fusers;
    b->st.resize(n_fusers);
    for (auto &h : b->st) { pose_identity(h.s.Tnow); pose_identity(h.s.Tlast_fuse); pose_identity(h.Todom); }
    ndtgpu_status rc = NDTGPU_OK;
    if (node_maps) {
        b->nodes = node_maps;
    } else {
        ndtgpu_grid_params g{};
        g.res = prm->resolution;
        g.size[0] = prm->map_size_x; g.size[1] = prm->map_size_y; g.size[2] = prm->map_size_z;
        g.max_cells = prm->max_cells;
        rc = mapset_create_owned(&g, n_fusers, b->own_nodes);
        b->nodes = b->own_nodes.get();
    }
    if (rc == NDTGPU_OK) rc = ndtgpu_mapset_enable_occupancy(b->nodes);
    if (rc == NDTGPU_OK) {
        // the scan maps: localMapSize (ndt_feature_fuser_hmt.h:224-226), centres set per update
        ndtgpu_grid_params g{};
        g.res = prm->resolution;
        g.size[0] = g.size[1] = prm->sensor_range + 3.0 * prm->resolution;
        g.size[2] = prm->map_size_z;
        g.max_cells = prm->max_cells;
        rc = mapset_create_owned(&g, n_fusers, b->scans);
    }
    if (rc != NDTGPU_OK) { delete b; return rc; }
#define TRY(expr) CREATE_TRY(b, NDTGPU_ERR_HIP, "fuser_bank_create", expr)
    TRY(b->st_dev.alloc(n_fusers));
    TRY(b->sensor_pose_dev.alloc(16));
    TRY(hipMemcpy(b->sensor_pose_dev.get(), prm->sensor_pose, 16 * sizeof(double), hipMemcpyHostToDevice));
    TRY(b->done.create());
#undef TRY
    *out = b;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_bank_mapsets(ndtgpu_fuser_bank *b, ndtgpu_mapset **node_maps, ndtgpu_mapset **scan_maps)
{
    if (!b) return fail(NDTGPU_ERR_INVALID, "fuser_bank_mapsets: null");
    if (node_maps) *node_maps = b->nodes;
    if (scan_maps) *scan_maps = b->scans.get();
    return NDTGPU_OK;
}

// the host's copy of the pose state catches up with the device: waits for the call in flight
static ndtgpu_status fuser_catch_up(ndtgpu_fuser_bank *b)
{
    if (!b->done.valid()) return NDTGPU_OK;
    HIP_TRY(b->done.sync());
    b->done.clear();
    if (b->fl_count) {
        std::vector<NdtFuserState> tmp(b->fl_count);
        HIP_TRY(hipMemcpy(tmp.data(), b->st_dev.get() + b->fl_first, b->fl_count * sizeof(NdtFuserState), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < b->fl_count; k++) b->st[b->fl_first + k].s = tmp[k];
    }
    return NDTGPU_OK;
}

// room for a call's staging block and moved scans (no launch uses the old blocks: every caller has caught up with the call in flight)
static ndtgpu_status fuser_stage(ndtgpu_fuser_bank *b, size_t bytes, size_t count, size_t n_points)
{
    HIP_TRY(b->pin.reserve(bytes));
    HIP_TRY(b->dev.reserve(bytes));
    HIP_TRY(b->xyz_a.reserve(count * n_points * 3));
    HIP_TRY(b->xyz_b.reserve(count * n_points * 3));
    return NDTGPU_OK;
}

// the checks of a _feat call that need no device: the bank has features attached and every cur index names a set of the feature
// bank outside the prev / map ranges
static ndtgpu_status fuser_feat_check(const char *what, const ndtgpu_fuser_bank *b, size_t count, const uint32_t *cur_set_idx)
{
    if (!b->fb) return fail_in(NDTGPU_ERR_INVALID, what, "no feature bank attached (ndtgpu_fuser_bank_attach_features)");
    if (count && !cur_set_idx) return fail_in(NDTGPU_ERR_INVALID, what, "cur_set_idx is NULL");
    for (size_t k = 0; k < count; k++) {
        const size_t c = cur_set_idx[k];
        if (c >= b->fb->v.n_sets || (c >= b->prev_first && c < b->prev_first + b->n) || (c >= b->map_first && c < b->map_first + b->n))
            return fail_in(NDTGPU_ERR_INVALID, what, "a cur set index is outside the feature bank or inside the prev / map ranges");
    }
    return NDTGPU_OK;
}

// what a _feat call uploads per slot: the three set indices and the flags (the odometry cell values: the caller)
static void fuser_feat_fill(ndtgpu_fuser_bank *b, char *pin, const FuserFeatLayout &F, size_t first, size_t count, const uint32_t *cur_set_idx,
                            unsigned call_flags, bool advance)
{
    uint32_t *cur = (uint32_t *)(pin + F.cur), *prev = (uint32_t *)(pin + F.prev), *map = (uint32_t *)(pin + F.map),
             *flags = (uint32_t *)(pin + F.flags);
    const uint32_t every = b->fprm.map_every > 0 ? (uint32_t)b->fprm.map_every : 1u;
    for (size_t k = 0; k < count; k++) {
        const size_t slot = first + k;
        cur[k] = cur_set_idx[k];
        prev[k] = (uint32_t)(b->prev_first + slot);
        map[k] = (uint32_t)(b->map_first + slot);
        unsigned f = call_flags | (b->prev_moved[slot] ? NDT_FUSERFEAT_PREV_MOVED : 0);
        if (advance) {                                          // NDTFeatureMap::update (ndt_feature_map.h:62-68)
            if (b->feat_counter[slot] % every == 0) f |= NDT_FUSERFEAT_APPEND;
            b->feat_counter[slot]++;
        }
        flags[k] = f;
        b->prev_moved[slot] = (call_flags & NDT_FUSERFEAT_MOVE) ? 1 : 0;
    }
}

static NdtFuserFeatPolicy fuser_feat_policy(const ndtgpu_fuser_params *prm, const ndtgpu_fuser_feat_params *fprm)
{
    NdtFuserFeatPolicy pol;
    pol.max_translation_norm = prm->max_translation_norm; pol.max_rotation_norm = prm->max_rotation_norm;
    for (int q = 0; q < 3; q++) pol.feat_cov[q] = fprm->feat_cov[q];
    pol.check_consistency = prm->check_consistency; pol.use_feat = fprm->use_feat ? 1 : 0; pol.use_odom = prm->use_odom ? 1 : 0;
    pol.fusion2d = prm->fusion2d ? 1 : 0; pol.prev_in_map_frame = fprm->prev_in_map_frame ? 1 : 0;
    return pol;
}

static NdtFuserFeatArgs fuser_feat_args(ndtgpu_fuser_bank *b, char *dev, const FuserFeatLayout &F, size_t first, size_t count)
{
    NdtFuserFeatArgs a{};
    a.pol = fuser_feat_policy(&b->prm, &b->fprm);
    a.count = (unsigned)count; a.n_sets = b->fb->v.n_sets; a.max_points = b->fb->v.max_points; a.desc_len = b->fb->v.desc_len;
    a.cur_idx = (const uint32_t *)(dev + F.cur); a.prev_idx = (const uint32_t *)(dev + F.prev); a.map_idx = (const uint32_t *)(dev + F.map);
    a.slot_flags = (const uint32_t *)(dev + F.flags);
    a.ransac = nullptr;
    a.T16 = (const double *)(dev + F.T16);
    a.corr = (const uint32_t *)(dev + F.corr);
    a.state = b->st_dev.get() + first;
    a.sensor_pose16 = b->sensor_pose_dev.get();
    a.odom18 = (const double *)(dev + F.odom);
    a.bank_count = b->fb->count.get(); a.bank_pos = b->fb->pos.get(); a.bank_desc = b->fb->desc.get();
    a.foff = (uint32_t *)(dev + F.foff);
    a.cells = (double *)(dev + F.cells);
    a.rec = (ndtgpu_fuser_feat_result *)(dev + F.rec);
    return a;
}

// ndtgpu_fuser_initialize_batch; cur_set_idx: the feature path as well (ndtgpu_fuser_initialize_batch_feat), else NULL
static ndtgpu_status fuser_initialize_core(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *initPose16, const void *xyz_dev,
                                           size_t n_points, size_t stride_bytes, size_t map_stride_bytes, const uint32_t *cur_set_idx,
                                           ndtgpu_stream stream)
{
    if (!b || first + count > b->n || (count && (!initPose16 || (n_points && !xyz_dev))) || stride_bytes < 12 || (stride_bytes & 3) ||
        n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "fuser_initialize: bad argument");
    if (count == 0) return NDTGPU_OK;
    ndtgpu_status rc = fuser_catch_up(b);
    if (rc != NDTGPU_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const FuserLayout L = fuser_layout(count, false);
    const FuserFeatLayout F = fuser_feat_layout(L.total, count, cur_set_idx ? b->fb->v.max_points : 0, false);
    rc = fuser_stage(b, cur_set_idx ? F.total : L.total, count, n_points);
    if (rc != NDTGPU_OK) return rc;
    // fuser_hmt.cpp:65-102: the first cloud goes through the sensor pose, then through the initial pose (two roundings to float);
    // Tnow = initPos; the map is centred on it (z = 0) and receives the cloud from where the sensor stood
    rc = ndtgpu_mapset_clear(b->nodes, first, count);
    if (rc != NDTGPU_OK) return rc;
    double *Tinit = (double *)(b->pin.get() + L.Tscan), *orig = (double *)(b->pin.get() + L.forigin), *Tsens = (double *)(b->pin.get() + L.Tmotion);
    for (size_t k = 0; k < count; k++) {
        ndtgpu_fuser_bank::HostState &h = b->st[first + k];
        const double *T0 = initPose16 + 16 * k;
        memcpy(h.s.Tnow, T0, sizeof h.s.Tnow);
        memcpy(h.s.Tlast_fuse, T0, sizeof h.s.Tlast_fuse);
        memcpy(h.Todom, T0, sizeof h.Todom);
        for (double &v : h.s.cov_mean) v = 0.0;
        for (double &v : h.s.cov) v = 0.0;
        h.is_init = true;
        const double centre[3] = {T0[12], T0[13], 0.0};
        rc = ndtgpu_mapset_set_centre(b->nodes, first + k, centre);
        if (rc != NDTGPU_OK) return rc;
        memcpy(Tinit + 16 * k, T0, 16 * sizeof(double));
        memcpy(Tsens + 16 * k, b->prm.sensor_pose, 16 * sizeof(double));
        double Ts[16];
        ndt_pose_mul(T0, b->prm.sensor_pose, Ts);              // Tnow_sensor: the origin the readings were taken from
        for (int a = 0; a < 3; a++) orig[3 * k + a] = Ts[12 + a];
        memcpy(b->pin.get() + L.spose + 16 * k * sizeof(double), Ts, sizeof Ts);    // (the feature path moves the points by it)
    }
    if (cur_set_idx) {
        for (size_t k = 0; k < count; k++) b->feat_counter[first + k] = 0;
        fuser_feat_fill(b, b->pin.get(), F, first, count, cur_set_idx, NDT_FUSERFEAT_MOVE | NDT_FUSERFEAT_RESET_MAP, true);
        HIP_TRY(hipMemcpyAsync(b->dev.get() + F.cur, b->pin.get() + F.cur, F.upload_end - F.cur, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(b->dev.get(), b->pin.get(), L.total, hipMemcpyHostToDevice, st));
    {
        std::vector<NdtFuserState> tmp(count);
        for (size_t k = 0; k < count; k++) tmp[k] = b->st[first + k].s;
        HIP_TRY(hipMemcpy(b->st_dev.get() + first, tmp.data(), count * sizeof(NdtFuserState), hipMemcpyHostToDevice));
    }
    hipError_t e = ndt_launch_cloud_transform(xyz_dev, count, n_points, stride_bytes, map_stride_bytes, (const double *)(b->dev.get() + L.Tmotion),
                                              (const double *)(b->dev.get() + L.Tscan), 16, b->xyz_b.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_initialize: transform", e);
    NdtFuseParams fp;
    fp.maxz = 100.0; fp.sensor_noise = 0.1; fp.maxnumpoints = 1e5; fp.occupancy_limit = 255.0; fp.eval_factor = 1000.0; fp.n_min = 3;   // :92-94
    e = ndt_launch_fuse(b->nodes->v, first, count, b->xyz_b.get(), n_points, 12, n_points * 12, (const double *)(b->dev.get() + L.forigin), fp,
                        b->nodes->nice_range(first, count), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_initialize: fuse launch", e);
    { ndtgpu_status trc = b->nodes->touch(st); if (trc != NDTGPU_OK) return trc; }
    b->ff_count = 0;
    if (cur_set_idx) {
        // :78-85 -- ptsPrev = pts moved by initPos * sensor_pose, featuremap.update(ptsPrev)
        NdtFuserFeatArgs a = fuser_feat_args(b, b->dev.get(), F, first, count);
        a.Tmove16 = (const double *)(b->dev.get() + L.spose);
        HIP_TRY(b->fb->used.order(st));                        // (a match or an extraction on another stream may still use the sets)
        HIP_TRY(hipMemsetAsync(b->dev.get() + F.rec, 0, count * sizeof(ndtgpu_fuser_feat_result), st));
        e = ndt_launch_fuserfeat_commit(a, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_initialize: feature commit launch", e);
        HIP_TRY(b->fb->used.record(st));
        HIP_TRY(hipMemcpyAsync(b->pin.get() + F.rec, b->dev.get() + F.rec, count * sizeof(ndtgpu_fuser_feat_result), hipMemcpyDeviceToHost, st));
        b->ff_first = first; b->ff_count = count; b->off_pin_frec = F.rec;
    }
    b->cl_count = 0;
    HIP_TRY(b->done.record(st));
    b->fl_first = first; b->fl_count = 0;                      // (the host state is already what the device holds)
    b->fl_stream = st;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_initialize_batch(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *initPose16,
                                            const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                            ndtgpu_stream stream)
{
    return fuser_initialize_core(b, first, count, initPose16, xyz_dev, n_points, stride_bytes, map_stride_bytes, nullptr, stream);
}

ndtgpu_status ndtgpu_fuser_initialize_batch_feat(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *initPose16,
                                                 const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                 const uint32_t *cur_set_idx, ndtgpu_stream stream)
{
    if (!b || first + count > b->n) return fail(NDTGPU_ERR_INVALID, "fuser_initialize_feat: bad argument");
    ndtgpu_status rc = fuser_feat_check("fuser_initialize_feat", b, count, cur_set_idx);
    if (rc != NDTGPU_OK) return rc;
    return fuser_initialize_core(b, first, count, initPose16, xyz_dev, n_points, stride_bytes, map_stride_bytes, cur_set_idx, stream);
}

// ndtgpu_fuser_update_batch; cur_set_idx: with the feature path (ndtgpu_fuser_update_batch_feat), else NULL
static ndtgpu_status fuser_update_core(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *Tmotion16, const void *xyz_dev,
                                       size_t n_points, size_t stride_bytes, size_t map_stride_bytes, const uint32_t *cur_set_idx,
                                       int update_feature_map, int update_ndt_map, ndtgpu_stream stream)
{
    if (!b || first + count > b->n || (count && (!Tmotion16 || (n_points && !xyz_dev))) || stride_bytes < 12 || (stride_bytes & 3) ||
        n_points > 0xFFFFFFFFull)
        return fail(NDTGPU_ERR_INVALID, "fuser_update: bad argument");
    if (count == 0) return NDTGPU_OK;
    ndtgpu_status rc = fuser_catch_up(b);          // this call starts from the poses the previous one left
    if (rc != NDTGPU_OK) return rc;
    for (size_t k = 0; k < count; k++)
        if (!b->st[first + k].is_init) return fail(NDTGPU_ERR_INVALID, "fuser_update: call ndtgpu_fuser_initialize_batch first (NDT-FuserHMT: Call Initialize first!!)");
    const ndtgpu_fuser_params &P = b->prm;
    hipStream_t st = (hipStream_t)stream;
    const bool fpath = cur_set_idx != nullptr;                 // the cells come from the device (ndt_fuserfeat_cells_kernel)
    const bool feat = P.use_odom != 0 && !P.fusion2d && !fpath;   // ... or, the 40 odometry cells, from this function
    const bool dev_cells = fpath && !P.fusion2d;
    const int flags = P.fusion2d ? 0 : ((P.use_soft_constraints ? 1 : 0) | (P.use_tikhonov ? 2 : 0));
    const FuserLayout L = fuser_layout(count, feat);
    const FuserFeatLayout F = fuser_feat_layout(L.total, count, fpath ? b->fb->v.max_points : 0, fpath);
    NdtFeatMatchParamsDev fmd{};
    if (fpath && b->fprm.use_feat) {
        rc = featmatch_params_dev("fuser_update_feat", &b->fprm.match, fmd);
        if (rc != NDTGPU_OK) return rc;
    }
    rc = fuser_stage(b, fpath ? F.total : L.total, count, n_points);
    if (rc != NDTGPU_OK) return rc;
    // ---- host: what depends on the odometry increment and the current pose only -----------------------------------------
    double *Tscan = (double *)(b->pin.get() + L.Tscan), *Tm = (double *)(b->pin.get() + L.Tmotion), *Te = (double *)(b->pin.get() + L.Test),
           *Q = (double *)(b->pin.get() + L.Q), *orig = (double *)(b->pin.get() + L.origin), *cen = (double *)(b->pin.get() + L.centre),
           *fc = (double *)(b->pin.get() + L.feat);
    uint32_t *foff = (uint32_t *)(b->pin.get() + L.foff), *idx = (uint32_t *)(b->pin.get() + L.idx);
    for (size_t k = 0; k < count; k++) {
        ndtgpu_fuser_bank::HostState &h = b->st[first + k];
        const double *T = Tmotion16 + 16 * k;
        ndtgpu_fuser_prepared pp;
        rc = ndtgpu_fuser_prepare(&P, h.s.Tnow, T, &b->nodes->centres_host[(first + k) * 3], &pp);
        if (rc != NDTGPU_OK) return rc;
        memcpy(Tscan + 16 * k, pp.Tscan, sizeof pp.Tscan);
        memcpy(Tm + 16 * k, T, 16 * sizeof(double));
        memcpy(Te + 16 * k, T, 16 * sizeof(double));          // Tmotion_est starts as the odometry increment (:166-170)
        if (flags && !invert6(pp.Tcov, Q + 36 * k)) return fail(NDTGPU_ERR_INVALID, "fuser_update: singular odometry covariance");
        for (int a = 0; a < 3; a++) { orig[3 * k + a] = pp.range_origin[a]; cen[3 * k + a] = pp.scan_centre[a]; }
        if (feat) {
            for (int i = 0; i < 40; i++) {
                double *c = fc + (k * 40 + i) * 18;          // {source mean, cov | target mean, cov}: NDTMatcherFeatureD2D pairs (i, i)
                for (int a = 0; a < 3; a++) { c[a] = pp.feat_src_mean[a]; c[9 + a] = pp.feat_tgt_mean[a]; }
                for (int a = 0; a < 6; a++) { c[3 + a] = i == 39 ? pp.feat_cov_plain[a] : pp.feat_cov_rotated[a]; c[12 + a] = pp.feat_cov_rotated[a]; }
            }
        }
        if (fpath) {                                           // (the odometry cells' values: the kernel lays them out behind the FLIRT cells)
            double *o = (double *)(b->pin.get() + F.odom) + 18 * k;
            for (int a = 0; a < 3; a++) { o[a] = pp.feat_src_mean[a]; o[3 + a] = pp.feat_tgt_mean[a]; }
            for (int a = 0; a < 6; a++) { o[6 + a] = pp.feat_cov_rotated[a]; o[12 + a] = pp.feat_cov_plain[a]; }
        }
        foff[k] = (uint32_t)(40 * k);
        idx[k] = (uint32_t)(first + k);
        double To[16];
        ndt_pose_mul(h.Todom, T, To);                          // "we track this only for display purposes!"
        memcpy(h.Todom, To, sizeof To);
        // the scan map's centre: the launcher picks its kernel by what the host knows of the centres
        for (int a = 0; a < 3; a++) b->scans->centres_host[(first + k) * 3 + a] = pp.scan_centre[a];
        b->scans->nice_host[first + k] = ndt_grid_is_nice(b->scans->v.grid, pp.scan_centre) ? 1 : 0;
    }
    foff[count] = (uint32_t)(40 * count);
    HIP_TRY(hipMemcpyAsync(b->dev.get(), b->pin.get(), L.res, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b->scans->v.centres + first * 3, b->dev.get() + L.centre, count * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    NdtFuserFeatArgs fa{};
    if (fpath) {
        // ---- the feature term (:245-334): RANSAC of (prev, cur), the gate, the cell records in front of the odometry cells.
        // The slots' poses on the device are still the ones this call starts from: ndt_fuser_post_kernel advances them below.
        fuser_feat_fill(b, b->pin.get(), F, first, count, cur_set_idx, update_feature_map ? NDT_FUSERFEAT_MOVE : 0, update_feature_map != 0);
        HIP_TRY(hipMemcpyAsync(b->dev.get() + F.cur, b->pin.get() + F.cur, F.upload_end - F.cur, hipMemcpyHostToDevice, st));
        fa = fuser_feat_args(b, b->dev.get(), F, first, count);
        fa.Tmotion16 = (const double *)(b->dev.get() + L.Tmotion);
        fa.Tmove16 = (const double *)(b->dev.get() + L.spose);
        HIP_TRY(b->fb->used.order(st));                        // (an extraction or a match on another stream may still use the sets)
        if (b->fprm.use_feat) {
            fa.ransac = (const ndtgpu_featmatch_result *)(b->dev.get() + F.ransac);
            hipError_t fe = ndt_featmatch_launch(b->fb->v, fa.prev_idx, fa.cur_idx, count, fmd, (ndtgpu_featmatch_result *)(b->dev.get() + F.ransac),
                                                 (double *)(b->dev.get() + F.T16), (uint32_t *)(b->dev.get() + F.corr), st);
            if (fe != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update_feat: RANSAC launch", fe);
        }
        hipError_t fe = ndt_launch_fuserfeat_cells(fa, st);
        if (fe != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update_feat: cells launch", fe);
        HIP_TRY(b->fb->used.record(st));
    }
    // ---- device -------------------------------------------------------------------------------------------------------
    // the scan in the node map's frame (:190), its NDT map on the node map's lattice (:201-227)
    hipError_t e = ndt_launch_cloud_transform(xyz_dev, count, n_points, stride_bytes, map_stride_bytes, (const double *)(b->dev.get() + L.Tscan),
                                              nullptr, 16, b->xyz_a.get(), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: transform", e);
    rc = mapset_build_core(b->scans.get(), first, count, b->xyz_a.get(), n_points, 12, n_points * 12, P.sensor_range, (const double *)(b->dev.get() + L.origin),
                           nullptr, st);
    if (rc != NDTGPU_OK) return rc;
    if (P.discard_cells && n_points > 0) {
        // :229-232 -- ndt_feature::discardCell(ndglobal, cloud.front()) and (.., cloud.back()): the cells of the scan map that hold the
        // first and the last point of the (moved) scan lose their Gaussian
        for (size_t k = 0; k < count; k++) {
            const float *c0 = b->xyz_a.get() + k * n_points * 3;
            e = ndt_launch_discard(b->scans->v, first + k, c0, 1, st);
            if (e == hipSuccess) e = ndt_launch_discard(b->scans->v, first + k, c0 + (n_points - 1) * 3, 1, st);
            if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: discard launch", e);
        }
    }
    // matchFusion / matchFusion2d of the scan map against the slot's node map (:353-357)
    ndtgpu_match_params mp;
    ndtgpu_default_match_params(&mp);
    mp.n_neighbours = P.neighbours; mp.itr_max = P.itr_max; mp.delta_score = P.delta_score; mp.step_control = P.stepcontrol ? 1 : 0;
    mp.dof_mask = P.fusion2d ? 0x23 : 0x3f;
    mp.use_initial_guess = 1;
    NdtMatchParamsDev pd = to_dev(&mp);
    // (a slot whose offsets are equal has no cells: the matcher runs it with useFeat = false, whatever bit 2 says)
    pd.fusion_flags = (feat || dev_cells) ? (flags | (P.step_control_fusion ? 4 : 0)) : flags;
    const uint32_t *idx_dev = (const uint32_t *)(b->dev.get() + L.idx);
    const unsigned *foff_dev = dev_cells ? (const unsigned *)(b->dev.get() + F.foff) : feat ? (const unsigned *)(b->dev.get() + L.foff) : nullptr;
    const double *cells_dev = dev_cells ? (const double *)(b->dev.get() + F.cells) : feat ? (const double *)(b->dev.get() + L.feat) : nullptr;
    rc = match_device_core(b->nodes, idx_dev, b->scans.get(), idx_dev, (double *)(b->dev.get() + L.Test), count, pd,
                           (ndtgpu_match_result *)(b->dev.get() + L.match), flags ? (const double *)(b->dev.get() + L.Q) : nullptr, st,
                           foff_dev, cells_dev);
    if (rc != NDTGPU_OK) return rc;
    // NDTMatcherD2D::covariance at the registered pose (:403-405; a default-constructed matcher: n_neighbours 2)
    if (P.compute_cov) {
        ndtgpu_match_params cp;
        ndtgpu_default_match_params(&cp);
        e = ndt_launch_covariance(b->nodes->v, idx_dev, b->scans->v, idx_dev, (const double *)(b->dev.get() + L.Test), count, cp.n_neighbours,
                                  cp.lfd1, cp.lfd2, P.covariance_mode, (double *)(b->dev.get() + L.cov), (int *)(b->dev.get() + L.covflag), st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: covariance launch", e);
    }
    // the post-registration step (:361-480), the scan in the frame of the new pose, the fuse-in (:485-486)
    NdtFuserPolicy pol;
    pol.max_translation_norm = P.max_translation_norm; pol.max_rotation_norm = P.max_rotation_norm;
    pol.translation_fuse_delta = 0.05; pol.rotation_fuse_delta = 0.01;                   // ndt_feature_fuser_hmt.h:222-223
    pol.check_consistency = P.check_consistency; pol.fuse_incomplete = P.fuse_incomplete; pol.all_matches_valid = P.all_matches_valid;
    pol.force_odom_as_est = P.force_odom_as_est; pol.compute_cov = P.compute_cov;
    e = ndt_launch_fuser_post(pol, b->sensor_pose_dev.get(), b->st_dev.get() + first, (const double *)(b->dev.get() + L.Tmotion), (const double *)(b->dev.get() + L.Test),
                              (const NdtMatchResultDev *)(b->dev.get() + L.match), P.compute_cov ? (const double *)(b->dev.get() + L.cov) : nullptr,
                              P.compute_cov ? (const int *)(b->dev.get() + L.covflag) : nullptr, count, (double *)(b->dev.get() + L.spose),
                              (double *)(b->dev.get() + L.forigin), (NdtFuserResultDev *)(b->dev.get() + L.res), st);
    if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: post launch", e);
    if (fpath) {
        // :497-502 -- ptsPrev = pts; with updateFeatureMap moved by Tnow * sensor_pose and appended to the feature map
        HIP_TRY(b->fb->used.order(st));
        e = ndt_launch_fuserfeat_commit(fa, st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update_feat: commit launch", e);
        HIP_TRY(b->fb->used.record(st));
        HIP_TRY(hipMemcpyAsync(b->pin.get() + F.rec, b->dev.get() + F.rec, count * sizeof(ndtgpu_fuser_feat_result), hipMemcpyDeviceToHost, st));
    }
    b->ff_first = first; b->ff_count = fpath ? count : 0; b->off_pin_frec = F.rec;
    b->cl_first = first; b->cl_count = (feat || dev_cells) ? count : 0;
    b->off_foff = dev_cells ? F.foff : L.foff; b->off_cells = dev_cells ? F.cells : L.feat;
    if (update_ndt_map) {
        e = ndt_launch_cloud_transform(xyz_dev, count, n_points, stride_bytes, map_stride_bytes, (const double *)(b->dev.get() + L.spose), nullptr, 16,
                                       b->xyz_b.get(), st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: transform", e);
        NdtFuseParams fp;
        fp.maxz = 25.0; fp.sensor_noise = 0.06; fp.maxnumpoints = 1e5; fp.occupancy_limit = 255.0; fp.eval_factor = 1000.0; fp.n_min = 3;   // :485-486
        e = ndt_launch_fuse(b->nodes->v, first, count, b->xyz_b.get(), n_points, 12, n_points * 12, (const double *)(b->dev.get() + L.forigin), fp,
                            b->nodes->nice_range(first, count), st);
        if (e != hipSuccess) return fail(NDTGPU_ERR_HIP, "fuser_update: fuse launch", e);
        { ndtgpu_status trc = b->nodes->touch(st); if (trc != NDTGPU_OK) return trc; }
    }
    HIP_TRY(hipMemcpyAsync(b->pin.get() + L.res, b->dev.get() + L.res, count * sizeof(NdtFuserResultDev), hipMemcpyDeviceToHost, st));
    HIP_TRY(b->done.record(st));
    b->fl_first = first; b->fl_count = count;
    b->off_pin_res = L.res;
    b->fl_stream = st;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_update_batch(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *Tmotion16, const void *xyz_dev,
                                        size_t n_points, size_t stride_bytes, size_t map_stride_bytes, int update_ndt_map,
                                        ndtgpu_stream stream)
{
    return fuser_update_core(b, first, count, Tmotion16, xyz_dev, n_points, stride_bytes, map_stride_bytes, nullptr, 0, update_ndt_map, stream);
}

ndtgpu_status ndtgpu_fuser_update_batch_feat(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *Tmotion16, const void *xyz_dev,
                                             size_t n_points, size_t stride_bytes, size_t map_stride_bytes, const uint32_t *cur_set_idx,
                                             int update_feature_map, int update_ndt_map, ndtgpu_stream stream)
{
    if (!b || first + count > b->n) return fail(NDTGPU_ERR_INVALID, "fuser_update_feat: bad argument");
    ndtgpu_status rc = fuser_feat_check("fuser_update_feat", b, count, cur_set_idx);
    if (rc != NDTGPU_OK) return rc;
    return fuser_update_core(b, first, count, Tmotion16, xyz_dev, n_points, stride_bytes, map_stride_bytes, cur_set_idx, update_feature_map,
                             update_ndt_map, stream);
}

void ndtgpu_default_fuser_feat_params(ndtgpu_fuser_feat_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->use_feat = 1;                               // Params(): useFeat = true (ndt_feature_fuser_hmt.h:58-101)
    p->prev_in_map_frame = 0;
    p->map_every = 4;                              // ndt_feature_map.h:64
    p->feat_cov[0] = 0.0002; p->feat_cov[1] = 0.0002; p->feat_cov[2] = 0.0001;      // :249
    ndtgpu_default_featmatch_params(&p->match);    // ndt_feature_fuser_hmt.h:213
}

ndtgpu_status ndtgpu_fuser_feat_prepare(const ndtgpu_fuser_params *prm, const ndtgpu_fuser_feat_params *fprm, const double Tnow16[16],
                                        const double Tmotion16[16], const ndtgpu_featmatch_result *ransac, const uint32_t *corr,
                                        const double *cur_pos3, size_t n_cur, const double *prev_pos3, size_t n_prev, int prev_moved,
                                        ndtgpu_fuser_feat_result *rec, double *cells18, uint32_t *n_cells)
{
    if (!prm || !fprm || !Tnow16 || !Tmotion16 || !rec || !cells18 || !n_cells) return fail(NDTGPU_ERR_INVALID, "fuser_feat_prepare: null argument");
    *n_cells = 0;
    if ((n_cur && !cur_pos3) || (n_prev && !prev_pos3)) return fail(NDTGPU_ERR_INVALID, "fuser_feat_prepare: positions are required");
    if (ransac && (ransac->n_inliers < 0 || (size_t)ransac->n_inliers > n_cur || (ransac->n_inliers > 0 && !corr)))
        return fail(NDTGPU_ERR_INVALID, "fuser_feat_prepare: n_inliers / corr");
    const double centre[3] = {0.0, 0.0, 0.0};
    ndtgpu_fuser_prepared pp;
    ndtgpu_status rc = ndtgpu_fuser_prepare(prm, Tnow16, Tmotion16, centre, &pp);
    if (rc != NDTGPU_OK) return rc;
    const NdtFuserFeatPolicy pol = fuser_feat_policy(prm, fprm);
    const bool run = ransac && fprm->use_feat;
    double T16[16] = {0};
    if (run) ndt_fuserfeat_T16(*ransac, T16);
    ndt_fuserfeat_gate(pol, run ? ransac : nullptr, T16, prm->sensor_pose, Tnow16, Tmotion16, *rec);
    for (int l = 0; l < rec->n_feat_cells; l++)
        if (corr[2 * l] >= n_cur || corr[2 * l + 1] >= n_prev) return fail(NDTGPU_ERR_INVALID, "fuser_feat_prepare: a correspondence names no point");
    double odom18[18];
    for (int a = 0; a < 3; a++) { odom18[a] = pp.feat_src_mean[a]; odom18[3 + a] = pp.feat_tgt_mean[a]; }
    for (int a = 0; a < 6; a++) { odom18[6 + a] = pp.feat_cov_rotated[a]; odom18[12 + a] = pp.feat_cov_plain[a]; }
    const bool as_is = pol.prev_in_map_frame && prev_moved;
    for (int l = 0; l < rec->n_feat_cells; l++)
        ndt_fuserfeat_cell_pair(pol, prm->sensor_pose, Tnow16, cur_pos3 + 3 * (size_t)corr[2 * l], prev_pos3 + 3 * (size_t)corr[2 * l + 1], as_is,
                                cells18 + 18 * (size_t)l);
    for (int l = 0; l < rec->n_odom_cells; l++)
        ndt_fuserfeat_odom_cell(odom18, l == rec->n_odom_cells - 1, cells18 + 18 * (size_t)(rec->n_feat_cells + l));
    *n_cells = (uint32_t)(rec->n_feat_cells + rec->n_odom_cells);
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_feat_move(const double T16[16], const double *pos3_in, size_t n, double *pos3_out)
{
    if (!T16 || (n && (!pos3_in || !pos3_out))) return fail(NDTGPU_ERR_INVALID, "fuser_feat_move: null argument");
    for (size_t i = 0; i < n; i++) {
        double q[3];
        ndt_fuserfeat_move_point(T16, pos3_in + 3 * i, q);
        for (int a = 0; a < 3; a++) pos3_out[3 * i + a] = q[a];
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_bank_attach_features(ndtgpu_fuser_bank *b, ndtgpu_featbank *fb, size_t prev_set_first, size_t map_set_first,
                                                const ndtgpu_fuser_feat_params *prm)
{
    if (!b || !fb) return fail(NDTGPU_ERR_INVALID, "fuser_bank_attach_features: null handle");
    const ndtgpu_fuser_feat_params p = params_or_default(prm, ndtgpu_default_fuser_feat_params);
    if (p.map_every < 1 || !(p.feat_cov[0] > 0) || !(p.feat_cov[1] > 0) || !(p.feat_cov[2] > 0))
        return fail(NDTGPU_ERR_INVALID, "fuser_bank_attach_features: map_every must be >= 1, feat_cov positive");
    NdtFeatMatchParamsDev d;
    ndtgpu_status rc = featmatch_params_dev("fuser_bank_attach_features", &p.match, d);
    if (rc != NDTGPU_OK) return rc;
    const size_t ns = fb->v.n_sets, n = b->n;
    if (prev_set_first > ns || n > ns - prev_set_first || map_set_first > ns || n > ns - map_set_first)
        return fail(NDTGPU_ERR_INVALID, "fuser_bank_attach_features: the prev / map ranges must lie inside the feature bank");
    if (prev_set_first < map_set_first + n && map_set_first < prev_set_first + n)
        return fail(NDTGPU_ERR_INVALID, "fuser_bank_attach_features: the prev and map ranges overlap");
    rc = fuser_catch_up(b);
    if (rc != NDTGPU_OK) return rc;
    b->fb = fb;
    b->prev_first = prev_set_first; b->map_first = map_set_first;
    b->fprm = p;
    b->feat_counter.assign(n, 0);
    b->prev_moved.assign(n, 0);
    b->ff_count = 0;
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_feat_results(ndtgpu_fuser_bank *b, size_t first, size_t count, ndtgpu_fuser_feat_result *out)
{
    if (!b || first + count > b->n || (count && !out)) return fail(NDTGPU_ERR_INVALID, "fuser_feat_results: bad argument");
    ndtgpu_status rc = fuser_catch_up(b);
    if (rc != NDTGPU_OK) return rc;
    memset(out, 0, count * sizeof *out);
    for (size_t k = 0; k < count; k++) {
        const size_t slot = first + k;
        if (slot >= b->ff_first && slot < b->ff_first + b->ff_count)
            memcpy(&out[k], b->pin.get() + b->off_pin_frec + (slot - b->ff_first) * sizeof *out, sizeof *out);
    }
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_feat_cells(ndtgpu_fuser_bank *b, size_t first, size_t count, uint32_t *offsets, double *cells18, size_t capacity)
{
    if (!b || first + count > b->n || !offsets || (capacity && !cells18)) return fail(NDTGPU_ERR_INVALID, "fuser_feat_cells: bad argument");
    ndtgpu_status rc = fuser_catch_up(b);
    if (rc != NDTGPU_OK) return rc;
    for (size_t k = 0; k <= count; k++) offsets[k] = 0;
    if (!b->cl_count || !count) return NDTGPU_OK;
    if (first < b->cl_first || first + count > b->cl_first + b->cl_count)
        return fail(NDTGPU_ERR_INVALID, "fuser_feat_cells: slots [first, first + count) are not of the last update call");
    std::vector<uint32_t> off(count + 1);
    HIP_TRY(hipMemcpy(off.data(), b->dev.get() + b->off_foff + (first - b->cl_first) * sizeof(uint32_t), (count + 1) * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    const size_t total = off[count] - off[0];
    if (total > capacity) return fail(NDTGPU_ERR_CAPACITY, "fuser_feat_cells: more cell records than `capacity`");
    if (total)
        HIP_TRY(hipMemcpy(cells18, b->dev.get() + b->off_cells + (size_t)off[0] * 18 * sizeof(double), total * 18 * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k <= count; k++) offsets[k] = off[k] - off[0];
    return NDTGPU_OK;
}

// the clouds of a *_host entry travel to a device buffer of the bank on a stream of its own; the device entry follows there
static ndtgpu_status fuser_clouds_in(ndtgpu_fuser_bank *b, size_t count, const void *xyz_host, size_t n_points, size_t stride_bytes,
                                     size_t map_stride_bytes, const void **xyz_dev)
{
    *xyz_dev = nullptr;
    if (!count || !n_points) return NDTGPU_OK;
    if (count > 1 && map_stride_bytes < n_points * stride_bytes) return fail(NDTGPU_ERR_INVALID, "fuser: clouds must not overlap");
    ndtgpu_status rc = fuser_catch_up(b);          // (the previous call may still read the buffer)
    if (rc != NDTGPU_OK) return rc;
    if (!b->own_st.get()) HIP_TRY(b->own_st.create(hipStreamNonBlocking));
    const size_t bytes = (count - 1) * map_stride_bytes + n_points * stride_bytes;
    HIP_TRY(b->xyz_in.reserve(bytes));             // (nothing reads the old block: caught up above)
    HIP_TRY(hipMemcpyAsync(b->xyz_in.get(), xyz_host, bytes, hipMemcpyHostToDevice, b->own_st.get()));
    *xyz_dev = b->xyz_in.get();
    return NDTGPU_OK;
}

ndtgpu_status ndtgpu_fuser_initialize_batch_host(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *initPose16,
                                                 const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes)
{
    if (!b || (count && n_points && !xyz_host)) return fail(NDTGPU_ERR_INVALID, "fuser_initialize_host: bad argument");
    const void *dev = nullptr;
    ndtgpu_status rc = fuser_clouds_in(b, count, xyz_host, n_points, stride_bytes, map_stride_bytes, &dev);
    if (rc != NDTGPU_OK) return rc;
    return ndtgpu_fuser_initialize_batch(b, first, count, initPose16, dev, n_points, stride_bytes, map_stride_bytes, (ndtgpu_stream)b->own_st.get());
}

ndtgpu_status ndtgpu_fuser_update_batch_host(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *Tmotion16,
                                             const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                             int update_ndt_map)
{
    if (!b || (count && n_points && !xyz_host)) return fail(NDTGPU_ERR_INVALID, "fuser_update_host: bad argument");
    const void *dev = nullptr;
    ndtgpu_status rc = fuser_clouds_in(b, count, xyz_host, n_points, stride_bytes, map_stride_bytes, &dev);
    if (rc != NDTGPU_OK) return rc;
    return ndtgpu_fuser_update_batch(b, first, count, Tmotion16, dev, n_points, stride_bytes, map_stride_bytes, update_ndt_map,
                                     (ndtgpu_stream)b->own_st.get());
}

ndtgpu_status ndtgpu_fuser_initialize_batch_feat_host(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *initPose16,
                                                      const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                      const uint32_t *cur_set_idx)
{
    if (!b || first + count > b->n || (count && n_points && !xyz_host)) return fail(NDTGPU_ERR_INVALID, "fuser_initialize_feat_host: bad argument");
    ndtgpu_status rc = fuser_feat_check("fuser_initialize_feat_host", b, count, cur_set_idx);
    if (rc != NDTGPU_OK) return rc;
    const void *dev = nullptr;
    rc = fuser_clouds_in(b, count, xyz_host, n_points, stride_bytes, map_stride_bytes, &dev);
    if (rc != NDTGPU_OK) return rc;
    return fuser_initialize_core(b, first, count, initPose16, dev, n_points, stride_bytes, map_stride_bytes, cur_set_idx,
                                 (ndtgpu_stream)b->own_st.get());
}

ndtgpu_status ndtgpu_fuser_update_batch_feat_host(ndtgpu_fuser_bank *b, size_t first, size_t count, const double *Tmotion16,
                                                  const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                  const uint32_t *cur_set_idx, int update_feature_map, int update_ndt_map)
{
    if (!b || first + count > b->n || (count && n_points && !xyz_host)) return fail(NDTGPU_ERR_INVALID, "fuser_update_feat_host: bad argument");
    ndtgpu_status rc = fuser_feat_check("fuser_update_feat_host", b, count, cur_set_idx);
    if (rc != NDTGPU_OK) return rc;
    const void *dev = nullptr;
    rc = fuser_clouds_in(b, count, xyz_host, n_points, stride_bytes, map_stride_bytes, &dev);
    if (rc != NDTGPU_OK) return rc;
    return fuser_update_core(b, first, count, Tmotion16, dev, n_points, stride_bytes, map_stride_bytes, cur_set_idx, update_feature_map,
                             update_ndt_map, (ndtgpu_stream)b->own_st.get());
}

ndtgpu_status ndtgpu_fuser_poses(ndtgpu_fuser_bank *b, size_t first, size_t count, double *Tnow16, ndtgpu_fuser_result *results)
{
    if (!b || first + count > b->n || (count && !Tnow16)) return fail(NDTGPU_ERR_INVALID, "fuser_poses: bad argument");
    const size_t f0 = b->fl_first, fc = b->fl_count, off = b->off_pin_res;
    ndtgpu_status rc = fuser_catch_up(b);
    if (rc != NDTGPU_OK) return rc;
    for (size_t k = 0; k < count; k++) memcpy(Tnow16 + 16 * k, b->st[first + k].s.Tnow, 16 * sizeof(double));
    if (results) {
        // the records of the LAST update call, for the slots it covered (zeroes elsewhere)
        memset(results, 0, count * sizeof *results);
        if (fc)
            for (size_t k = 0; k < count; k++) {
                const size_t slot = first + k;
                if (slot >= f0 && slot < f0 + fc) memcpy(&results[k], b->pin.get() + off + (slot - f0) * sizeof(NdtFuserResultDev), sizeof(NdtFuserResultDev));
            }
    }
    return NDTGPU_OK;
}

}  // extern "C"
