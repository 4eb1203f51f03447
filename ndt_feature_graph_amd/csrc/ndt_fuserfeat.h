// ndt_fuserfeat.h -- the arithmetic of the fuser bank's feature path (include/ndtgpu.h "the fuser bank's feature path", steps 2-6),
// shared by the kernels (csrc/ndt_fuserfeat.hip) and the pure host entries (ndtgpu_fuser_feat_prepare, ndtgpu_fuser_feat_move in
// csrc/ndtgpu_fuser_bank.hip): the consistency gate (ndt_feature_fuser_hmt.cpp:252-289), one FLIRT cell pair (:294-325;
// conversions.h:52-83), one odometry cell pair (:312-334) and one moved interest point (:500).  Like ndt_pose.h: the same loops in
// the same order on both sides, contraction off, so that tests/fuserfeat_model.py can restate them operation for operation.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_pose.h"

#define NDT_FUSERFEAT_MAX_CELLS 64        // correspondences the matcher takes per registration (ndt_match.hip)
#define NDT_FUSERFEAT_ODOM_CELLS 40       // "Quick HACK HERE" (:315)
#define NDT_FUSERFEAT_COMMIT_THREADS 256

// what the gate and the cells read of ndtgpu_fuser_params / ndtgpu_fuser_feat_params
struct NdtFuserFeatPolicy {
    double max_translation_norm, max_rotation_norm;
    double feat_cov[3];
    int check_consistency, use_feat, use_odom, fusion2d, prev_in_map_frame;
};

// per-slot flags of a call (host-known)
enum {
    NDT_FUSERFEAT_PREV_MOVED = 1,         // the previous call moved prev into the map frame
    NDT_FUSERFEAT_APPEND = 2,             // NDTFeatureMap::update appends this time (counter % map_every == 0)
    NDT_FUSERFEAT_MOVE = 4,               // update_feature_map: the points are moved
    NDT_FUSERFEAT_RESET_MAP = 8           // initialize: the map set starts empty
};

// Steps 2, 3 and 5's counts: fills rec up to `truncated`, zeroes the rest.  ransac == NULL: RANSAC was not run.  T16: Tfeat_sensor.
NDT_HD void ndt_fuserfeat_gate(const NdtFuserFeatPolicy &pol, const ndtgpu_featmatch_result *ransac, const double *T16,
                               const double *sensor_pose, const double *Tnow, const double *Tmotion, ndtgpu_fuser_feat_result &rec)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    rec.ransac_run = 0; rec.consistent = 0; rec.n_feat_cells = 0; rec.truncated = 0;
    rec.n_prev = 0; rec.n_map = 0; rec.map_appended = 0; rec.map_overflow = 0; rec.pad_ = 0;
    rec.n_odom_cells = (pol.use_odom && !pol.fusion2d) ? NDT_FUSERFEAT_ODOM_CELLS : 0;
    for (int q = 0; q < 16; q++) rec.Tfeat[q] = 0.0;
    if (!ransac) {
        rec.ransac.score = 0.0; rec.ransac.x = 0.0; rec.ransac.y = 0.0; rec.ransac.theta = 0.0; rec.ransac.c = 0.0; rec.ransac.s = 0.0;
        rec.ransac.n_candidates = 0; rec.ransac.n_hypotheses = 0; rec.ransac.n_tested = 0; rec.ransac.best_hypothesis = 0;
        rec.ransac.n_inliers = 0; rec.ransac.status = 0;
        return;
    }
    rec.ransac = *ransac;
    rec.ransac_run = 1;
    double Sinv[16];
    ndt_pose_inverse(sensor_pose, Sinv);
    ndt_pose_mul(T16, Sinv, rec.Tfeat);                        // :255
    bool consistent = ransac->status == NDTGPU_FEATMATCH_OK && ransac->n_inliers > 0;        // (matches.size() > 0, :271)
    if (consistent && pol.check_consistency) {                 // :279-285
        double P[16], Pinv[16], diff[16], e3[3];
        ndt_pose_mul(Tnow, Tmotion, P);
        ndt_pose_inverse(P, Pinv);
        ndt_pose_mul(Pinv, rec.Tfeat, diff);
        ndt_euler012(diff, e3);
        const double dt = sqrt(diff[12] * diff[12] + diff[13] * diff[13] + diff[14] * diff[14]);
        const double dr = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
        if (dt > pol.max_translation_norm / 10. || dr > pol.max_rotation_norm / 4.) consistent = false;
    }
    rec.consistent = consistent ? 1 : 0;
    if (pol.use_feat && consistent && !pol.fusion2d) {         // :299
        const int room = NDT_FUSERFEAT_MAX_CELLS - rec.n_odom_cells;
        rec.n_feat_cells = ransac->n_inliers < room ? ransac->n_inliers : room;
        rec.truncated = ransac->n_inliers > room ? 1 : 0;
    }
}

// the 4x4 of ndtgpu_featbank_match_device's T16 from the record's (c, s, x, y)
NDT_HD void ndt_fuserfeat_T16(const ndtgpu_featmatch_result &r, double *T16)
{
    for (int k = 0; k < 16; k++) T16[k] = 0.0;
    T16[0] = r.c; T16[1] = r.s; T16[4] = -r.s; T16[5] = r.c; T16[10] = 1.0;
    T16[12] = r.x; T16[13] = r.y; T16[15] = 1.0;
}

// pseudoTransformNDTMap on one Gaussian: mean' = T mean, cov' = R cov R^T (9 doubles, row-major), the loops of ndtgpu_fuser_prepare
NDT_HD void ndt_fuserfeat_pseudo(const double *T, double *mean3, double *cov9)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double m[3], RC[9];
    for (int a = 0; a < 3; a++) m[a] = T[a] * mean3[0] + T[4 + a] * mean3[1] + T[8 + a] * mean3[2] + T[12 + a];
    for (int a = 0; a < 3; a++) mean3[a] = m[a];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s2 = 0;
            for (int k = 0; k < 3; k++) s2 += T[k * 4 + i] * cov9[k * 3 + j];
            RC[i * 3 + j] = s2;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s2 = 0;
            for (int k = 0; k < 3; k++) s2 += RC[i * 3 + k] * T[k * 4 + j];
            cov9[i * 3 + j] = s2;
        }
}

NDT_HD void ndt_fuserfeat_half(const double *mean3, const double *cov9, double *out9)
{
    out9[0] = mean3[0]; out9[1] = mean3[1]; out9[2] = mean3[2];
    out9[3] = cov9[0]; out9[4] = cov9[1]; out9[5] = cov9[2]; out9[6] = cov9[4]; out9[7] = cov9[5]; out9[8] = cov9[8];
}

// Step 4 for one correspondence: cur3 / prev3 the two points (x, y, theta); prev_as_is: prev_in_map_frame and the point was moved.
// cell18: {source mean[3], cov[6] | target mean[3], cov[6]}
NDT_HD void ndt_fuserfeat_cell_pair(const NdtFuserFeatPolicy &pol, const double *sensor_pose, const double *Tnow, const double *cur3,
                                    const double *prev3, bool prev_as_is, double *cell18)
{
    double m[3], C[9];
    for (int side = 0; side < 2; side++) {
        const double *p = side == 0 ? cur3 : prev3;
        m[0] = p[0]; m[1] = p[1]; m[2] = 0.0;
        for (int q = 0; q < 9; q++) C[q] = 0.0;
        C[0] = pol.feat_cov[0]; C[4] = pol.feat_cov[1]; C[8] = pol.feat_cov[2];
        if (side == 0 || !prev_as_is) {
            ndt_fuserfeat_pseudo(sensor_pose, m, C);           // :307-309
            ndt_fuserfeat_pseudo(Tnow, m, C);                  // :324-325
        }
        ndt_fuserfeat_half(m, C, cell18 + 9 * side);
    }
}

// one of the 40 odometry cell pairs from ndtgpu_fuser_prepared's values: odom18 = {feat_src_mean[3], feat_tgt_mean[3],
// feat_cov_rotated[6], feat_cov_plain[6]}; last: the source cell that keeps the un-rotated covariance (:328-333)
NDT_HD void ndt_fuserfeat_odom_cell(const double *odom18, bool last, double *cell18)
{
    for (int a = 0; a < 3; a++) { cell18[a] = odom18[a]; cell18[9 + a] = odom18[3 + a]; }
    for (int a = 0; a < 6; a++) { cell18[3 + a] = last ? odom18[12 + a] : odom18[6 + a]; cell18[12 + a] = odom18[6 + a]; }
}

// Step 6 for one point: pose2d(x, y, theta) as a 4x4, moved by T
NDT_HD void ndt_fuserfeat_move_point(const double *T, const double *p3, double *out3)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double P[16], M[16], e3[3];
    const double c = cos(p3[2]), s = sin(p3[2]);
    for (int q = 0; q < 16; q++) P[q] = (q % 5 == 0) ? 1.0 : 0.0;
    P[0] = c; P[1] = s; P[4] = -s; P[5] = c; P[12] = p3[0]; P[13] = p3[1];
    ndt_pose_mul(T, P, M);
    ndt_euler012(M, e3);
    out3[0] = M[12]; out3[1] = M[13]; out3[2] = e3[2];
}

// what the kernels of a call receive
struct NdtFuserFeatArgs {
    NdtFuserFeatPolicy pol;
    unsigned count, n_sets, max_points, desc_len;
    const uint32_t *cur_idx, *prev_idx, *map_idx;     // [count] sets of the bank (checked by the host)
    const uint32_t *slot_flags;                       // [count] NDT_FUSERFEAT_*
    const ndtgpu_featmatch_result *ransac;            // [count] step 1's outputs, or NULL: not run
    const double *T16;                                // [count][16]
    const uint32_t *corr;                             // [count][max_points][2]
    const NdtFuserState *state;                       // [count] the slots' poses BEFORE the update
    const double *Tmotion16;                          // [count][16]
    const double *sensor_pose16;                      // [16]
    const double *odom18;                             // [count][18]
    const double *Tmove16;                            // [count][16] commit: Tnow_new * sensor_pose
    uint32_t *bank_count;                             // the feature bank's arrays (NdtFeatBankView's, writable)
    double *bank_pos, *bank_desc;
    uint32_t *foff;                                   // [count + 1]
    double *cells;                                    // [count * 64][18]
    ndtgpu_fuser_feat_result *rec;                    // [count]
};

// csrc/ndt_fuserfeat.hip
hipError_t ndt_launch_fuserfeat_cells(const NdtFuserFeatArgs &a, hipStream_t st);
hipError_t ndt_launch_fuserfeat_commit(const NdtFuserFeatArgs &a, hipStream_t st);
