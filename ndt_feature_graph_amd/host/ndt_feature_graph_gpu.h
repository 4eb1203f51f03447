// ndt_feature_graph_gpu.h -- host front door of the ndt_feature classes that drive the hot path, over the C-ABI of libndtgpu.so:
//   ndt_feature::MotionModel2d        motion_model.hpp:123-163, motion_model.cpp:166-207
//   ndt_feature::matchFusion / matchFusion2d   ndt_matcher_d2d_fusion.h:797-1155, 1159-1176
//   ndt_feature::NDTFeatureFuserHMT   ndt_feature_fuser_hmt.h:36-334 (Params, initialize, update)
//   ndt_feature::NDTFeatureLink / NDTFeatureNode / overlapNDTOccupancyScore   ndt_feature_link.h:9-56, ndt_feature_node.h:38-252
//   ndt_feature::NDTFeatureGraph      ndt_feature_graph.h:20-280 (initialize, update, updateLink[s]UsingNDTRegistration, ...)
//   ndt_feature::optimizeGraphUsingISAM   ndt_offline_mapper.h:8-26, 40-107 (on the device: ndtgpu_pgo_*)
//   ndt_feature::optimizeGraph3D          (added) the same for 6-DoF links and their cov_3d, without force2D (ndtgpu_pgo3_*)
//   ndt_feature::assembleWorldMap         the graph's node maps under their poses as ONE map (ndt_feature_graph.h:149-152 fuse(),
//                                         ndt_feature2d_fuser.cpp:425-432; on the device: ndtgpu_world_assemble)
// Class, member and parameter names are the reference's, so that its callers compile against this header.  What is behind them
// is not the reference's control flow retyped but the batched device entries:
//   * NDTFeatureFuserHMT::initialize / update are ONE C-ABI call each (ndtgpu_fuser_initialize_batch / ndtgpu_fuser_update_batch
//     on the fuser's slot of a ndtgpu_host::FuserBank): scan -> scan map -> matchFusion -> covariance -> pose -> ray-traced
//     fuse-in run on the device without a host round trip.  A graph's node fusers are the slots of one bank over the pool its
//     node maps live in, so several graphs / robots / bags can also be stepped with one call (FuserBank::update).
//   * NDTFeatureGraph::updateLinksUsingNDTRegistration registers ALL links in one batched call each for the matcher, the
//     covariance and the overlap score (three calls per batch instead of three per link), never blocks on stdin
//     (graph.cpp:318-328) and reports non-convergence in NDTFeatureLink::converged.
//   * the FLIRT feature path (useFeat): initialize / update overloads that take ndt_feature::InterestPointGPUVec
//     (ndt_feature_map_gpu.h) stage the points into the bank's feature sets and run ndtgpu_fuser_*_batch_feat_host: RANSAC
//     against the previous scan, the consistency gate, the FLIRT cells in front of the odometry cells, the points moved and
//     appended to the node's feature map (ndt_feature_fuser_hmt.cpp:245-334, 497-502), all in the same device call.
//     getFeatureMap() reads a node's map back; NDTFeatureGraph::matchNodesUsingFeatureMap (ndt_feature_node.h:254-256) matches
//     two nodes' maps on the device.  computeLink itself is not rewired.  The overloads that take the empty placeholder
//     InterestPointVec stay and run without features.
// Configurations the device path does not cover are rejected loudly (ndtgpu_host::Error), never silently ignored:
// globalTransf = false, loadCentroid = false.  In a catkin build that needs those the reference's own ndt_feature_fuser_hmt.cpp runs against
// lslgeneric_gpu.h instead.
#pragma once
#include "lslgeneric_gpu.h"
#include "ndt_feature_map_gpu.h"

#include <cstdlib>
#include <iostream>
#include <sstream>

namespace ndt_feature {

struct InterestPointVec {};   // flirtlib's InterestPoint container: the feature front-end is out of scope (useFeat = false)

typedef Eigen::Vector3d Pose2d;
struct Pose2dCov {
    Pose2d mean;
    Eigen::Matrix3d cov;
};

// getRobustYawFromAffine3d (utils.h:30-41).  `clamped`: the cosine is brought into [-1, 1] first -- upstream does not, so a
// rotation whose (0, 0) entry is a rounding above 1 yields NaN there: kept as written where it only rejects a link
// (distanceBetweenAffine3d -> getValidLinks), not where it would turn a pose into NaN (force2D).
inline double getRobustYawFromAffine3d(const Eigen::Affine3d &a, bool clamped = true)
{
    const double c = clamped ? std::fmax(-1.0, std::fmin(1.0, a(0, 0))) : a(0, 0);   // x axis . rotated x axis, in the xy plane
    const double angle = std::acos(c);
    return (a(1, 0) > 0) ? angle : -angle;
}
// distanceBetweenAffine3d (utils.h:43-48)
inline void distanceBetweenAffine3d(const Eigen::Affine3d &p1, const Eigen::Affine3d &p2, double &dist, double &angularDist)
{
    Eigen::Affine3d tmp = p1.inverse() * p2;
    dist = tmp.translation().norm();
    angularDist = std::fabs(getRobustYawFromAffine3d(tmp, false));
}
// forceEigenAffine3dTo2dInPlace (utils.h:50-72)
inline void forceEigenAffine3dTo2dInPlace(Eigen::Affine3d &a3d)
{
    const double yaw = getRobustYawFromAffine3d(a3d);
    const Eigen::Vector3d t = a3d.translation();
    a3d = ndtgpu_host::affine_from_pose(t(0), t(1), 0., 0., 0., yaw);
}
// pose2dFromAffine3d, cov6toCov3, pose2dClearDependence (motion_model.cpp:128-165)
inline Pose2d pose2dFromAffine3d(const Eigen::Affine3d &T)
{
    return Pose2d(T.translation()(0), T.translation()(1), T.rotation().eulerAngles(0, 1, 2)(2));
}
inline Eigen::Matrix3d cov6toCov3(const Eigen::MatrixXd &cov6)
{
    Eigen::Matrix3d c;
    c(0, 0) = cov6(0, 0); c(1, 1) = cov6(1, 1); c(2, 2) = cov6(5, 5);
    c(0, 1) = cov6(0, 1); c(1, 0) = cov6(1, 0);
    c(0, 2) = cov6(0, 5); c(1, 2) = cov6(1, 5); c(2, 0) = cov6(5, 0); c(2, 1) = cov6(5, 1);
    return c;
}
inline void pose2dClearDependence(Pose2dCov &p)
{
    p.cov(0, 1) = p.cov(1, 0) = p.cov(0, 2) = p.cov(1, 2) = p.cov(2, 0) = p.cov(2, 1) = 0.;
}
// discardCell (utils.h:229-236)
inline bool discardCell(lslgeneric::NDTMap &map, const pcl::PointXYZ &pt) { return map.discardCellAtPoint(pt); }
// computeLocalCentroid (utils.h:213-227)
inline Eigen::Vector3d computeLocalCentroid(const Eigen::Vector3d &map_centroid, const Eigen::Vector3d &local_pos, double resolution)
{
    Eigen::Vector3d diff = map_centroid - local_pos, local_centroid;
    for (int i = 0; i < 3; i++) local_centroid(i) = diff(i) - std::floor(diff(i) / resolution) * resolution;
    return local_centroid;
}

// Eliazar-style odometry covariance (motion_model.hpp:123-163; motion_model.cpp:166-207)
class MotionModel2d {
public:
    class Params {
    public:
        Params() { Cd = 0.001; Ct = 0.001; Dd = 0.005; Dt = 0.005; Td = 0.001; Tt = 0.001; }
        double Cd, Ct, Dd, Dt, Td, Tt;
    };
    MotionModel2d() {}
    MotionModel2d(const MotionModel2d::Params &p) : params(p) {}
    void setParams(const MotionModel2d::Params &p) { params = p; }
    Pose2dCov getPose2dCov(const Pose2d &rel) const
    {
        Pose2dCov ret;
        ret.mean = rel;
        ret.cov = getMeasurementCov(rel);
        return ret;
    }
    Eigen::MatrixXd getCovMatrix6(const Pose2d &rel) const
    {
        Eigen::MatrixXd cov(6, 6);
        cov.setIdentity();
        Eigen::Matrix3d c2 = getMeasurementCov(rel);
        cov(0, 0) = c2(0, 0); cov(1, 0) = c2(1, 0); cov(0, 1) = c2(0, 1); cov(1, 1) = c2(1, 1);
        cov(0, 5) = c2(0, 2); cov(1, 5) = c2(1, 2);
        cov(5, 0) = c2(2, 0); cov(5, 1) = c2(2, 1); cov(5, 5) = c2(2, 2);
        return cov;
    }
    MotionModel2d::Params params;

private:
    Eigen::Matrix3d getMeasurementCov(const Eigen::Vector3d &rel) const
    {
        const double dist = std::sqrt(rel[0] * rel[0] + rel[1] * rel[1]), rot = rel[2];
        Eigen::Matrix3d R;
        R.setZero();                        // motion_model.cpp:202 (with the real Eigen an unset matrix is garbage)
        R(0, 0) = params.Dd * dist * dist + params.Dt * rot * rot;
        R(1, 1) = params.Cd * dist * dist + params.Ct * rot * rot;
        R(2, 2) = params.Td * dist * dist + params.Tt * rot * rot;
        return R;
    }
};

// ndt_feature::matchFusion (ndt_matcher_d2d_fusion.h:797-1155) -- the reference's full signature.  The whole Newton /
// More-Thuente loop runs on the device (ndtgpu_match_fusion_batch / ndtgpu_match_fusion_feat_batch); the feature maps
// are CellVector maps whose cells correspond through corr_feat (NDTMatcherFeatureD2D).
inline bool matchFusion(lslgeneric::NDTMap &targetNDT, lslgeneric::NDTMap &sourceNDT, lslgeneric::NDTMap &targetNDT_feat,
                        lslgeneric::NDTMap &sourceNDT_feat, const std::vector<std::pair<int, int> > &corr_feat,
                        Eigen::Affine3d &T, const Eigen::MatrixXd &Tcov, bool useInitialGuess, bool useNDT, bool useFeat,
                        bool step_control, int ITR_MAX = 30, int n_neighbours = 2, double DELTA_SCORE = 10e-4,
                        bool useSoftConstraints = true, bool step_control_fusion = true, bool useTikhonovRegularization = false,
                        ndtgpu_match_result *result = nullptr)
{
    if (!useNDT) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "matchFusion: useNDT == false leaves nothing to match");
    lslgeneric::NDTMatcherD2D m;
    m.n_neighbours = n_neighbours;
    m.ITR_MAX = ITR_MAX;
    m.DELTA_SCORE = DELTA_SCORE;
    m.step_control = step_control;
    ndtgpu_match_params p = m.params(0x3f, useInitialGuess);
    ndtgpu_match_result r;
    uint32_t ti = (uint32_t)targetNDT.slot(), si = (uint32_t)sourceNDT.slot();
    double c36[36];
    const int flags = (useSoftConstraints ? 1 : 0) | (useTikhonovRegularization ? 2 : 0);
    if (flags) {
        if (Tcov.rows() != 6 || Tcov.cols() != 6) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "matchFusion: Tcov must be 6x6");
        for (int a = 0; a < 6; a++)
            for (int b = 0; b < 6; b++) c36[a * 6 + b] = Tcov(a, b);
    }
    // the feature / odometry-cell maps: NDTMatcherFeatureD2D(corr_feat) pairs source cell corr.second with target cell corr.first
    std::vector<double> sm, sc, tm, tc;
    uint32_t off[2] = {0, 0};
    if (useFeat) {
        lslgeneric::CellVector *cvt = targetNDT_feat.getMyIndex(), *cvs = sourceNDT_feat.getMyIndex();
        if (!cvt || !cvs) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "matchFusion: the feature maps must be CellVector maps");
        for (const auto &c : corr_feat) {
            const lslgeneric::NDTCell *t = cvt->getCellIdx((unsigned)c.first), *s_ = cvs->getCellIdx((unsigned)c.second);
            if (!t || !s_) continue;                    // (targetNDT.getCellIdx fails: the pair is skipped)
            const Eigen::Vector3d mt = t->getMean(), ms = s_->getMean();
            const Eigen::Matrix3d Ct = t->getCov(), Cs = s_->getCov();
            for (int a = 0; a < 3; a++) { tm.push_back(mt(a)); sm.push_back(ms(a)); }
            const int ij[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
            for (int k = 0; k < 6; k++) { tc.push_back(Ct(ij[k][0], ij[k][1])); sc.push_back(Cs(ij[k][0], ij[k][1])); }
        }
        off[1] = (uint32_t)(tm.size() / 3);
    }
    if (off[1]) {
        ndtgpu_feat_pairs fp = {off, sm.data(), sc.data(), tm.data(), tc.data()};
        ndtgpu_host::check(ndtgpu_match_fusion_feat_batch(targetNDT.handle(), &ti, sourceNDT.handle(), &si, T.data(), flags ? c36 : nullptr, &fp,
                                                          1, &p, flags | (step_control_fusion ? 4 : 0), &r, nullptr),
                           "ndtgpu_match_fusion_feat_batch");
    } else {
        ndtgpu_host::check(ndtgpu_match_fusion_batch(targetNDT.handle(), &ti, sourceNDT.handle(), &si, T.data(), flags ? c36 : nullptr, 1,
                                                     &p, flags, &r, nullptr), "ndtgpu_match_fusion_batch");
    }
    if (result) *result = r;
    return r.converged != 0;
}
// ndt_feature::addNDTCellToMap (utils.h): a copy of the cell joins the map's cell list
inline void addNDTCellToMap(lslgeneric::NDTMap *map, lslgeneric::NDTCell *cell)
{
    lslgeneric::CellVector *cl = map->getMyIndex();
    if (!cl) return;
    lslgeneric::NDTCell *c = new lslgeneric::NDTCell();
    c->setMean(cell->getMean()); c->setCov(cell->getCov()); c->setN(cell->getN());
    cl->addCell(c);
}
// ndt_feature::matchFusion2d (ndt_matcher_d2d_fusion.h:1159-1176): NDTMatcherD2D_2D on the NDT maps
inline bool matchFusion2d(lslgeneric::NDTMap &targetNDT, lslgeneric::NDTMap &sourceNDT, lslgeneric::NDTMap & /*targetNDT_feat*/,
                          lslgeneric::NDTMap & /*sourceNDT_feat*/, const std::vector<std::pair<int, int> > & /*corr_feat*/,
                          Eigen::Affine3d &T, bool useInitialGuess, bool /*useNDT*/, bool /*useFeat*/, bool step_control, int ITR_MAX = 30,
                          int n_neighbours = 2, double DELTA_SCORE = 10e-4)
{
    lslgeneric::NDTMatcherD2D_2D matcher_d2d_2d;
    matcher_d2d_2d.n_neighbours = n_neighbours;
    matcher_d2d_2d.step_control = step_control;
    matcher_d2d_2d.ITR_MAX = ITR_MAX;
    matcher_d2d_2d.DELTA_SCORE = DELTA_SCORE;
    return matcher_d2d_2d.match(targetNDT, sourceNDT, T, useInitialGuess);
}

}  // namespace ndt_feature

namespace ndtgpu_host {

// B independent fusers stepped by ONE call (ndtgpu_fuser_bank): the slots' node maps are the maps of a MapPool.
class FuserBank {
public:
    FuserBank(const ndtgpu_fuser_params &p, std::shared_ptr<MapPool> pool) : pool_(std::move(pool)), prm_(p)
    {
        check(ndtgpu_fuser_bank_create(&p, pool_->size(), pool_->handle(), &bank_), "ndtgpu_fuser_bank_create");
    }
    ~FuserBank()
    {
        ndtgpu_fuser_bank_destroy(bank_);              // (waits for its last call, which may still use the feature bank)
        if (feat_) ndtgpu_featbank_destroy(feat_);
    }
    FuserBank(const FuserBank &) = delete;
    FuserBank &operator=(const FuserBank &) = delete;
    const ndtgpu_fuser_params &params() const { return prm_; }
    const std::shared_ptr<MapPool> &pool() const { return pool_; }

    // slots [first, first + clouds.size()): poses and first clouds (sensor frame)
    void initialize(size_t first, const std::vector<Eigen::Affine3d> &initPos, const std::vector<const pcl::PointCloud<pcl::PointXYZ> *> &clouds)
    {
        pack(clouds);
        std::vector<double> T = flat(initPos);
        check(ndtgpu_fuser_initialize_batch_host(bank_, first, clouds.size(), T.data(), pts_.data(), np_, 16, np_ * 16), "ndtgpu_fuser_initialize_batch_host");
    }
    // one update of every slot of the range; returns the records of the call (pose, registered increment, matcher report)
    std::vector<ndtgpu_fuser_result> update(size_t first, const std::vector<Eigen::Affine3d> &Tmotion,
                                            const std::vector<const pcl::PointCloud<pcl::PointXYZ> *> &clouds, bool updateNDTMap = true)
    {
        if (Tmotion.size() != clouds.size()) throw Error(NDTGPU_ERR_INVALID, "FuserBank::update: one odometry increment per cloud");
        pack(clouds);
        std::vector<double> T = flat(Tmotion);
        check(ndtgpu_fuser_update_batch_host(bank_, first, clouds.size(), T.data(), pts_.data(), np_, 16, np_ * 16, updateNDTMap ? 1 : 0),
              "ndtgpu_fuser_update_batch_host");
        std::vector<ndtgpu_fuser_result> res(clouds.size());
        std::vector<double> now(16 * clouds.size());
        check(ndtgpu_fuser_poses(bank_, first, clouds.size(), now.data(), res.data()), "ndtgpu_fuser_poses");
        return res;
    }
    Eigen::Affine3d pose(size_t slot)
    {
        Eigen::Affine3d T;
        check(ndtgpu_fuser_poses(bank_, slot, 1, T.data(), nullptr), "ndtgpu_fuser_poses");
        return T;
    }

    // ---- the feature path (include/ndtgpu.h "the fuser bank's feature path"): a feature bank of the bank's own with three sets
    // per slot -- [0, n) the scans' points (cur), [n, 2n) ptsPrev, [2n, 3n) the feature maps
    void attachFeatures(size_t max_points = 256, size_t desc_len = 48, const ndtgpu_fuser_feat_params *prm = nullptr)
    {
        if (feat_) throw Error(NDTGPU_ERR_INVALID, "FuserBank::attachFeatures: already attached");
        const size_t n = pool_->size();
        check(ndtgpu_featbank_create(3 * n, max_points, desc_len, &feat_), "ndtgpu_featbank_create");
        feat_max_points_ = max_points;
        feat_desc_len_ = desc_len;
        check(ndtgpu_fuser_bank_attach_features(bank_, feat_, n, 2 * n, prm), "ndtgpu_fuser_bank_attach_features");
    }
    ndtgpu_featbank *features() const { return feat_; }
    size_t featMaxPoints() const { return feat_max_points_; }
    size_t curSet(size_t slot) const { return slot; }
    size_t prevSet(size_t slot) const { return pool_->size() + slot; }
    size_t mapSet(size_t slot) const { return 2 * pool_->size() + slot; }
    // initialize / update with the scans' interest points: staged into the cur sets with ndtgpu_featbank_set, then ONE call
    void initialize(size_t first, const std::vector<Eigen::Affine3d> &initPos, const std::vector<const pcl::PointCloud<pcl::PointXYZ> *> &clouds,
                    const std::vector<const ndt_feature::InterestPointGPUVec *> &pts)
    {
        const std::vector<uint32_t> cur = stage(first, clouds.size(), pts);
        pack(clouds);
        std::vector<double> T = flat(initPos);
        check(ndtgpu_fuser_initialize_batch_feat_host(bank_, first, clouds.size(), T.data(), pts_.data(), np_, 16, np_ * 16, cur.data()),
              "ndtgpu_fuser_initialize_batch_feat_host");
    }
    std::vector<ndtgpu_fuser_result> update(size_t first, const std::vector<Eigen::Affine3d> &Tmotion,
                                            const std::vector<const pcl::PointCloud<pcl::PointXYZ> *> &clouds,
                                            const std::vector<const ndt_feature::InterestPointGPUVec *> &pts, bool updateFeatureMap = true,
                                            bool updateNDTMap = true)
    {
        if (Tmotion.size() != clouds.size()) throw Error(NDTGPU_ERR_INVALID, "FuserBank::update: one odometry increment per cloud");
        const std::vector<uint32_t> cur = stage(first, clouds.size(), pts);
        pack(clouds);
        std::vector<double> T = flat(Tmotion);
        check(ndtgpu_fuser_update_batch_feat_host(bank_, first, clouds.size(), T.data(), pts_.data(), np_, 16, np_ * 16, cur.data(),
                                                  updateFeatureMap ? 1 : 0, updateNDTMap ? 1 : 0),
              "ndtgpu_fuser_update_batch_feat_host");
        std::vector<ndtgpu_fuser_result> res(clouds.size());
        std::vector<double> now(16 * clouds.size());
        check(ndtgpu_fuser_poses(bank_, first, clouds.size(), now.data(), res.data()), "ndtgpu_fuser_poses");
        return res;
    }
    std::vector<ndtgpu_fuser_feat_result> featResults(size_t first, size_t count)
    {
        std::vector<ndtgpu_fuser_feat_result> res(count);
        check(ndtgpu_fuser_feat_results(bank_, first, count, res.data()), "ndtgpu_fuser_feat_results");
        return res;
    }
    // a set of the feature bank read back (a slot's feature map: mapSet(slot))
    ndt_feature::InterestPointGPUVec readSet(size_t set)
    {
        if (!feat_) throw Error(NDTGPU_ERR_INVALID, "FuserBank::readSet: no feature bank attached");
        std::vector<double> pos(3 * feat_max_points_), desc(feat_max_points_ * feat_desc_len_);
        size_t m = 0;
        check(ndtgpu_featbank_get(feat_, set, &m, pos.data(), desc.data()), "ndtgpu_featbank_get");
        ndt_feature::InterestPointGPUVec out(m);
        for (size_t i = 0; i < m; i++) {
            out[i].x = pos[3 * i]; out[i].y = pos[3 * i + 1]; out[i].theta = pos[3 * i + 2];
            out[i].descriptor.assign(desc.begin() + i * feat_desc_len_, desc.begin() + (i + 1) * feat_desc_len_);
        }
        return out;
    }

private:
    std::vector<uint32_t> stage(size_t first, size_t count, const std::vector<const ndt_feature::InterestPointGPUVec *> &pts)
    {
        if (!feat_) throw Error(NDTGPU_ERR_INVALID, "FuserBank: call attachFeatures first");
        if (pts.size() != count) throw Error(NDTGPU_ERR_INVALID, "FuserBank: one set of interest points per cloud");
        std::vector<uint32_t> cur(count);
        std::vector<double> pos, desc;
        for (size_t k = 0; k < count; k++) {
            pos.clear();
            desc.clear();
            for (const ndt_feature::InterestPointGPU &p : *pts[k]) {
                if (p.descriptor.size() != feat_desc_len_) throw Error(NDTGPU_ERR_INVALID, "FuserBank: a descriptor of another length than the bank's");
                pos.push_back(p.x); pos.push_back(p.y); pos.push_back(p.theta);
                desc.insert(desc.end(), p.descriptor.begin(), p.descriptor.end());
            }
            cur[k] = (uint32_t)curSet(first + k);
            check(ndtgpu_featbank_set(feat_, cur[k], pts[k]->size(), pos.data(), desc.data()), "ndtgpu_featbank_set");
        }
        return cur;
    }
    static std::vector<double> flat(const std::vector<Eigen::Affine3d> &T)
    {
        std::vector<double> o(16 * T.size());
        for (size_t k = 0; k < T.size(); k++)
            for (int e = 0; e < 16; e++) o[16 * k + e] = T[k].data()[e];
        return o;
    }
    // clouds of unequal length side by side, padded with NaN points (which the binning drops)
    void pack(const std::vector<const pcl::PointCloud<pcl::PointXYZ> *> &clouds)
    {
        static_assert(sizeof(pcl::PointXYZ) == 16, "pcl::PointXYZ is four floats");
        np_ = 0;
        for (const auto *c : clouds) np_ = std::max(np_, c->size());
        pts_.assign(clouds.size() * np_ * 4, std::nanf(""));
        for (size_t k = 0; k < clouds.size(); k++)
            for (size_t i = 0; i < clouds[k]->size(); i++) {
                const pcl::PointXYZ &q = clouds[k]->points[i];
                float *o = &pts_[(k * np_ + i) * 4];
                o[0] = q.x; o[1] = q.y; o[2] = q.z;
            }
    }
    std::shared_ptr<MapPool> pool_;
    ndtgpu_fuser_params prm_;
    ndtgpu_fuser_bank *bank_ = nullptr;
    ndtgpu_featbank *feat_ = nullptr;
    size_t feat_max_points_ = 0, feat_desc_len_ = 0;
    std::vector<float> pts_;
    size_t np_ = 0;
};

}  // namespace ndtgpu_host

namespace ndt_feature {

class NDTFeatureFuserHMT {
public:
    Eigen::Affine3d Tnow, Tlast_fuse, Todom;   ///< current pose
    lslgeneric::NDTMap *map;                   ///< da map

    //! ndt_feature_fuser_hmt.h:58-207: all 30 fields, the reference's defaults
    class Params {
    public:
        Params()
        {
            checkConsistency = false;
            resolution = 1.;
            map_size_x = 40.; map_size_y = 40.; map_size_z = 10.;
            sensor_range = 3.;
            max_translation_norm = 1;
            max_rotation_norm = M_PI / 4.;
            fuseIncomplete = false;
            beHMT = true;
            prefix = "";
            hmt_map_dir = "map";
            useNDT = true; useFeat = true; useOdom = true;
            neighbours = 0;
            stepcontrol = true;
            ITR_MAX = 30;
            DELTA_SCORE = 10e-4;
            globalTransf = true;
            loadCentroid = true;
            forceOdomAsEst = false;
            visualizeLocalCloud = false;
            fusion2d = false;
            allMatchesValid = false;
            discardCells = false;
            useSoftConstraints = true;
            computeCov = true;
            stepControlFusion = true;
            useTikhonovRegularization = true;
        }
        bool checkConsistency;
        double resolution, map_size_x, map_size_y, map_size_z, sensor_range, max_translation_norm, max_rotation_norm;
        bool fuseIncomplete, beHMT;
        std::string prefix, hmt_map_dir;
        bool useNDT, useFeat, useOdom;
        int neighbours;
        bool stepcontrol;
        int ITR_MAX;
        double DELTA_SCORE;
        bool globalTransf, loadCentroid, forceOdomAsEst, visualizeLocalCloud, fusion2d, allMatchesValid, discardCells,
            useSoftConstraints, computeCov, stepControlFusion, useTikhonovRegularization;
        std::string getDescString() const
        {
            std::ostringstream os;
            os << "resolution" << resolution << "loadCentroid" << loadCentroid << "discardCells" << discardCells << "neighbours" << neighbours
               << "forceOdomAsEst" << forceOdomAsEst << "useSoftConstraints" << useSoftConstraints;
            return os.str();
        }
    };

    Params params_;
    MotionModel2d::Params motion_params_;
    ndtgpu_match_result last_match{};        // (added) what the device matcher reported for the last update
    ndtgpu_fuser_result last_update{};       // (added) the whole record of the last update

    // the fields of Params / MotionModel2d::Params / the sensor pose that the device path reads, as the C-ABI wants them.
    // Throws for the configurations it does not cover.
    static ndtgpu_fuser_params bankParams(const Params &p, const MotionModel2d::Params &m, const Eigen::Affine3d &sensor_pose)
    {
        if (!p.globalTransf || !p.loadCentroid)
            throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "NDTFeatureFuserHMT: the device path covers globalTransf = loadCentroid = true (the "
                                                         "defaults); run the reference's own update against lslgeneric_gpu.h for the others");
        if (!p.useNDT) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "NDTFeatureFuserHMT: useNDT == false leaves nothing to match");
        ndtgpu_fuser_params q;
        ndtgpu_default_fuser_params(&q);
        q.resolution = p.resolution;
        q.map_size_x = p.map_size_x; q.map_size_y = p.map_size_y; q.map_size_z = p.map_size_z;
        q.sensor_range = p.sensor_range;
        q.max_translation_norm = p.max_translation_norm; q.max_rotation_norm = p.max_rotation_norm;
        q.check_consistency = p.checkConsistency; q.fuse_incomplete = p.fuseIncomplete;
        q.use_odom = p.useOdom;               // (useFeat: without FLIRT interest points there are no feature matches to add)
        q.neighbours = p.neighbours; q.stepcontrol = p.stepcontrol; q.itr_max = p.ITR_MAX; q.delta_score = p.DELTA_SCORE;
        q.force_odom_as_est = p.forceOdomAsEst; q.fusion2d = p.fusion2d; q.all_matches_valid = p.allMatchesValid;
        q.use_soft_constraints = p.useSoftConstraints; q.compute_cov = p.computeCov; q.step_control_fusion = p.stepControlFusion;
        q.use_tikhonov = p.useTikhonovRegularization; q.discard_cells = p.discardCells;
        q.motion_Cd = m.Cd; q.motion_Ct = m.Ct; q.motion_Dd = m.Dd; q.motion_Dt = m.Dt; q.motion_Td = m.Td; q.motion_Tt = m.Tt;
        for (int e = 0; e < 16; e++) q.sensor_pose[e] = sensor_pose.data()[e];
        return q;
    }

    NDTFeatureFuserHMT(const NDTFeatureFuserHMT::Params &params) : map(NULL), params_(params), isInit(false) {}
    // a fuser that is slot `slot` of a bank shared with other fusers (the node fusers of a graph)
    NDTFeatureFuserHMT(const NDTFeatureFuserHMT::Params &params, std::shared_ptr<ndtgpu_host::FuserBank> bank, size_t slot)
        : map(NULL), params_(params), isInit(false), bank_(std::move(bank)), slot_(slot) {}
    ~NDTFeatureFuserHMT()
    {
        if (map != NULL) delete map;
    }
    NDTFeatureFuserHMT(const NDTFeatureFuserHMT &) = delete;
    NDTFeatureFuserHMT &operator=(const NDTFeatureFuserHMT &) = delete;

    void setMotionParams(const MotionModel2d::Params &params) { motion_params_ = params; }
    void setSensorPose(Eigen::Affine3d spose) { sensor_pose = spose; }
    bool wasInit() { return isInit; }
    const NDTFeatureFuserHMT::Params &getParam() const { return params_; }
    Eigen::Matrix3d &getCov() { return current_posecov.cov; }

    /** initialize(initPos, cloud, pts, preLoad) -- ndt_feature_fuser_hmt.cpp:65-102 -- as ONE device call */
    void initialize(Eigen::Affine3d initPos, const pcl::PointCloud<pcl::PointXYZ> &cloudOrig, const InterestPointVec & /*pts*/, bool /*preLoad*/ = false)
    {
        if (!bank_) {     // a fuser on its own: a bank of one over a pool of one
            const double c[3] = {0, 0, 0}, sz[3] = {params_.map_size_x, params_.map_size_y, params_.map_size_z};
            auto pool = std::make_shared<ndtgpu_host::MapPool>(params_.resolution, c, sz, 1);
            bank_ = std::make_shared<ndtgpu_host::FuserBank>(bankParams(params_, motion_params_, sensor_pose), pool);
            slot_ = 0;
        }
        if (map != NULL) delete map;
        map = new lslgeneric::NDTMap(bank_->pool(), slot_);
        // (the host object learns where the map sits; the device call below fills it)
        map->initialize(initPos.translation()(0), initPos.translation()(1), 0., params_.map_size_x, params_.map_size_y, params_.map_size_z);
        bank_->initialize(slot_, {initPos}, {&cloudOrig});
        Tnow = Tlast_fuse = Todom = initPos;
        isInit = true;
    }

    /** update(Tmotion, cloud, pts, updateFeatureMap, updateNDTMap) -- ndt_feature_fuser_hmt.cpp:108-512 -- as ONE device call */
    Eigen::Affine3d update(Eigen::Affine3d Tmotion, const pcl::PointCloud<pcl::PointXYZ> &cloudOrig, const InterestPointVec & /*pts*/,
                           bool /*updateFeatureMap*/ = true, bool updateNDTMap = true)
    {
        if (!isInit) {
            fprintf(stderr, "NDT-FuserHMT: Call Initialize first!!\n");
            return Tnow;
        }
        absorb(bank_->update(slot_, {Tmotion}, {&cloudOrig}, updateNDTMap)[0], Tmotion);
        return Tnow;
    }
    // ---- with the scans' interest points (ndt_feature_map_gpu.h: InterestPointGPUVec): the feature path of the device call --
    // RANSAC against the previous scan's points, the consistency gate, the FLIRT cells in front of the odometry cells
    // (ndt_feature_fuser_hmt.cpp:245-334), the points moved and appended to the feature map (:497-502).  The bank gets a feature
    // bank on first use (max 256 points per set, descriptors of the first point's length).
    void initialize(Eigen::Affine3d initPos, const pcl::PointCloud<pcl::PointXYZ> &cloudOrig, const InterestPointGPUVec &pts, bool /*preLoad*/ = false)
    {
        if (!bank_) {
            const double c[3] = {0, 0, 0}, sz[3] = {params_.map_size_x, params_.map_size_y, params_.map_size_z};
            auto pool = std::make_shared<ndtgpu_host::MapPool>(params_.resolution, c, sz, 1);
            bank_ = std::make_shared<ndtgpu_host::FuserBank>(bankParams(params_, motion_params_, sensor_pose), pool);
            slot_ = 0;
        }
        ensureFeatures(pts);
        if (map != NULL) delete map;
        map = new lslgeneric::NDTMap(bank_->pool(), slot_);
        map->initialize(initPos.translation()(0), initPos.translation()(1), 0., params_.map_size_x, params_.map_size_y, params_.map_size_z);
        bank_->initialize(slot_, {initPos}, {&cloudOrig}, {&pts});
        last_feat = bank_->featResults(slot_, 1)[0];
        Tnow = Tlast_fuse = Todom = initPos;
        isInit = true;
    }
    Eigen::Affine3d update(Eigen::Affine3d Tmotion, const pcl::PointCloud<pcl::PointXYZ> &cloudOrig, const InterestPointGPUVec &pts,
                           bool updateFeatureMap = true, bool updateNDTMap = true)
    {
        if (!isInit) {
            fprintf(stderr, "NDT-FuserHMT: Call Initialize first!!\n");
            return Tnow;
        }
        ensureFeatures(pts);
        absorb(bank_->update(slot_, {Tmotion}, {&cloudOrig}, {&pts}, updateFeatureMap, updateNDTMap)[0], Tmotion);
        last_feat = bank_->featResults(slot_, 1)[0];
        return Tnow;
    }
    // featuremap (ndt_feature_fuser_hmt.h): the slot's map set read back
    NDTFeatureMapGPU getFeatureMap()
    {
        NDTFeatureMapGPU m;
        if (bank_ && bank_->features()) m.map = bank_->readSet(bank_->mapSet(slot_));
        return m;
    }
    ndtgpu_fuser_feat_result last_feat{};    // (added) the feature record of the last call with interest points
    // (added) what a batched caller does after FuserBank::update on this fuser's slot
    void absorb(const ndtgpu_fuser_result &r, const Eigen::Affine3d &Tmotion)
    {
        last_update = r;
        last_match = r.match;
        for (int e = 0; e < 16; e++) Tnow.data()[e] = r.Tnow[e];
        Todom = Todom * Tmotion;
        for (int a = 0; a < 3; a++) current_posecov.mean(a) = r.posecov_mean[a];
        for (int e = 0; e < 9; e++) current_posecov.cov.data()[e] = r.posecov[e];
    }
    const std::shared_ptr<ndtgpu_host::FuserBank> &bank() const { return bank_; }
    size_t slot() const { return slot_; }

private:
    void ensureFeatures(const InterestPointGPUVec &pts)
    {
        if (bank_->features()) return;
        ndtgpu_fuser_feat_params fp;
        ndtgpu_default_fuser_feat_params(&fp);
        fp.use_feat = params_.useFeat ? 1 : 0;
        bank_->attachFeatures(256, pts.empty() ? 48 : pts[0].descriptor.size(), &fp);
    }
    bool isInit;
    Eigen::Affine3d sensor_pose;
    Pose2dCov current_posecov;
    std::shared_ptr<ndtgpu_host::FuserBank> bank_;
    size_t slot_ = 0;
};

// interfaces.h:10-48 -- what the iSAM layer consumes (ndt_offline_mapper.h:40 takes NDTFeatureGraphInterface&)
class NDTFeatureNodeInterface {
public:
    virtual ~NDTFeatureNodeInterface() {}
    virtual const Eigen::Affine3d &getPose() const = 0;
    virtual const Eigen::Matrix3d &getCov() const = 0;
    virtual void setPose(const Eigen::Affine3d &pose) = 0;
    virtual void setCov(const Eigen::Matrix3d &cov) = 0;
};
class NDTFeatureLinkInterface {
public:
    virtual ~NDTFeatureLinkInterface() {}
    virtual const Eigen::Affine3d &getRelPose() const = 0;
    virtual const Eigen::Matrix3d &getRelCov() const = 0;
    virtual double getScore() const = 0;
    virtual size_t getRefIdx() const = 0;
    virtual size_t getMovIdx() const = 0;
    friend std::ostream &operator<<(std::ostream &os, const NDTFeatureLinkInterface &obj)
    {
        os << "\n[" << obj.getRefIdx() << "<->" << obj.getMovIdx() << "] T: " << "[" << obj.getRelPose().translation()[0] << ","
           << obj.getRelPose().translation()[1] << "](" << obj.getRelPose().rotation().eulerAngles(0, 1, 2)[2] << ")";
        os << "\n score : " << obj.getScore();
        return os;
    }
};
class NDTFeatureGraphInterface {
public:
    virtual ~NDTFeatureGraphInterface() {}
    virtual size_t getNbNodes() const = 0;
    virtual NDTFeatureNodeInterface &getNodeInterface(size_t idx) = 0;
    virtual const NDTFeatureNodeInterface &getNodeInterface(size_t idx) const = 0;
    virtual size_t getNbLinks() const = 0;
    virtual NDTFeatureLinkInterface &getLinkInterface(size_t idx) = 0;
    virtual const NDTFeatureLinkInterface &getLinkInterface(size_t idx) const = 0;
};

class NDTFeatureLink : public NDTFeatureLinkInterface {
public:
    NDTFeatureLink() : ref_idx(0), mov_idx(0), cov_3d(6, 6), score(0.) {}
    NDTFeatureLink(size_t ref, size_t mov) : ref_idx(ref), mov_idx(mov), cov_3d(6, 6), score(0.) {}
    size_t ref_idx, mov_idx;   // Vector idx...
    Eigen::Affine3d T;         // From ref->mov.
    Eigen::Matrix3d cov;
    Eigen::MatrixXd cov_3d;    // the covariance returned by NDTMatcherD2D::covariance (graph.cpp:296-310, 330)
    double score;
    bool converged = true;     // (added) replaces the stdin pause of graph.cpp:318-323
    int iterations = 0;
    // Interfaces.
    virtual const Eigen::Affine3d &getRelPose() const { return T; }
    virtual const Eigen::Matrix3d &getRelCov() const { return cov; }
    virtual double getScore() const { return score; }
    virtual size_t getRefIdx() const { return ref_idx; }
    virtual size_t getMovIdx() const { return mov_idx; }
    void force2D() { forceEigenAffine3dTo2dInPlace(this->T); }
};

class NDTFeatureNode : public NDTFeatureNodeInterface {
public:
    NDTFeatureNode() : map(NULL), nbUpdates(0), time_last_update(0) {}
    NDTFeatureFuserHMT *map;   // owned by the graph (ndt_feature_graph.h:78-88); node copies are shallow like the reference's
    Eigen::Affine3d T;
    Eigen::Matrix3d cov;
    Eigen::Affine3d Tlocal_odom;   // Incremental odometry between successive local maps.
    Eigen::Affine3d Tlocal_fuse;   // Incremental fuse estimates between sucessive local maps.
    pcl::PointCloud<pcl::PointXYZ> pts;   // Only for visualizaion purposes...
    int nbUpdates;
    double time_last_update;
    // ndt_feature_node.h:81-96
    void addCloud(Eigen::Affine3d &T_, const pcl::PointCloud<pcl::PointXYZ> &pc)
    {
        pcl::PointCloud<pcl::PointXYZ> moved(pc);
        ndtgpu_host::transformPointCloudInPlace(T_, moved);
        for (const auto &p : moved.points) this->pts.push_back(p);
    }
    pcl::PointCloud<pcl::PointXYZ> getGlobalPointCloud()
    {
        pcl::PointCloud<pcl::PointXYZ> out(this->pts);
        ndtgpu_host::transformPointCloudInPlace(this->T, out);
        return out;
    }
    pcl::PointCloud<pcl::PointXYZ> getLocalPointCloud() { return this->pts; }
    lslgeneric::NDTMap &getNDTMap() { return *(map->map); }
    NDTFeatureFuserHMT &getFuser() { return *map; }
    // Interfaces.
    virtual const Eigen::Affine3d &getPose() const { return T; }
    virtual void setPose(const Eigen::Affine3d &pose) { T = pose; }
    virtual const Eigen::Matrix3d &getCov() const { return cov; }
    virtual void setCov(const Eigen::Matrix3d &c) { cov = c; }
    void force2D()
    {
        forceEigenAffine3dTo2dInPlace(this->T);
        forceEigenAffine3dTo2dInPlace(this->Tlocal_odom);
        forceEigenAffine3dTo2dInPlace(this->Tlocal_fuse);
    }
};

// ndt_feature::overlapNDTOccupancyScore(ref, mov, T)  (ndt_feature_node.h:213-252), on the device
inline double overlapNDTOccupancyScore(NDTFeatureNode &ref, NDTFeatureNode &mov, const Eigen::Affine3d &T)
{
    uint32_t ri = (uint32_t)ref.getNDTMap().slot(), mi = (uint32_t)mov.getNDTMap().slot();
    double score = 1.;
    ndtgpu_host::check(ndtgpu_overlap_score_batch(ref.getNDTMap().handle(), &ri, mov.getNDTMap().handle(), &mi, T.data(), 1, &score, nullptr, nullptr),
                       "ndtgpu_overlap_score_batch");
    return score;
}

class NDTFeatureGraph : public NDTFeatureGraphInterface {
public:
    class Params {   // ndt_feature_graph.h:24-56
    public:
        Params()
        {
            newNodeNumberOfFrames = 20;
            newNodeTranslDist = 1.;
            storePtsInNodes = false;
            storePtsInNodesIncr = 8;
            popNodes = false;
            maxNodes = 256;
        }
        int newNodeNumberOfFrames;
        double newNodeTranslDist;
        bool storePtsInNodes;
        int storePtsInNodesIncr;
        bool popNodes;
        size_t maxNodes;   // (added) capacity of the device pool the node maps live in
    };

    NDTFeatureGraph() : distance_moved_in_last_node_(0.) {}
    NDTFeatureGraph(const NDTFeatureGraph::Params &params, const NDTFeatureFuserHMT::Params &fuserParams)
        : params_(params), fuser_params_(fuserParams), distance_moved_in_last_node_(0.) {}
    virtual ~NDTFeatureGraph()
    {
        for (auto it = nodes_.begin(); it != nodes_.end(); ++it)
            if (it->map != NULL) delete it->map;
    }
    NDTFeatureGraph(const NDTFeatureGraph &) = delete;
    NDTFeatureGraph &operator=(const NDTFeatureGraph &) = delete;

    // Interfaces (ndt_feature_graph.h: the graph IS-A NDTFeatureGraphInterface)
    virtual size_t getNbNodes() const { return nodes_.size(); }
    virtual NDTFeatureNodeInterface &getNodeInterface(size_t idx) { return nodes_[idx]; }
    virtual const NDTFeatureNodeInterface &getNodeInterface(size_t idx) const { return nodes_[idx]; }
    virtual size_t getNbLinks() const { return links_.size(); }
    virtual NDTFeatureLinkInterface &getLinkInterface(size_t idx) { return links_[idx]; }
    virtual const NDTFeatureLinkInterface &getLinkInterface(size_t idx) const { return links_[idx]; }
    NDTFeatureNode &getNode(size_t i) { return nodes_[i]; }
    const NDTFeatureNode &getNode(size_t i) const { return nodes_[i]; }
    NDTFeatureLink &getLink(size_t i) { return links_[i]; }
    lslgeneric::NDTMap *getMap(int i) { return nodes_[i].map->map; }
    Eigen::Affine3d getT() { return Tnow; }
    void setFuserParams(const NDTFeatureFuserHMT::Params &p) { fuser_params_ = p; }
    void setMotionParams(const MotionModel2d::Params &p) { motion_params_ = p; }
    void setSensorPose(const Eigen::Affine3d &p) { sensor_pose_ = p; }
    void clearAllLinks() { links_.clear(); }
    void setLinks(const std::vector<NDTFeatureLink> &l) { links_ = l; }
    void appendLinks(const std::vector<NDTFeatureLink> &l) { links_.insert(links_.end(), l.begin(), l.end()); }
    const std::vector<NDTFeatureLink> &getCurrentLinks() { return links_; }
    void force2D()
    {
        for (auto &n : nodes_) n.force2D();
        for (auto &l : links_) l.force2D();
    }
    bool fullInit()
    {
        for (size_t i = 0; i < getNbNodes(); ++i)
            if (nodes_[i].map->wasInit() == false) return false;
        return true;
    }

    // initialize(initPose, cloud, pts, preLoad) -- ndt_feature_graph.cpp:24-55: the first node.  A node keeps its map in its
    // own frame (node.T places it in the world), so its fuser starts at the identity.
    void initialize(Eigen::Affine3d initPose, pcl::PointCloud<pcl::PointXYZ> &cloud, const InterestPointVec &pts, bool preLoad = false)
    {
        open_node(initPose, cloud, pts, preLoad);
        Tnow = initPose;
    }
    // ... and update with the scans' interest points: they go through to the node's fuser (its feature path)
    void initialize(Eigen::Affine3d initPose, pcl::PointCloud<pcl::PointXYZ> &cloud, const InterestPointGPUVec &pts, bool preLoad = false)
    {
        open_node(initPose, cloud, pts, preLoad);
        Tnow = initPose;
    }
    Eigen::Affine3d update(Eigen::Affine3d Tmotion, pcl::PointCloud<pcl::PointXYZ> &cloud, const InterestPointGPUVec &pts)
    {
        return update_with(Tmotion, cloud, pts);
    }
    // matchNodesUsingFeatureMap(ref, mov, matches, T) (ndt_feature_node.h:254-256): the RANSAC of two nodes' feature maps where
    // they are, in the bank's device sets, without reading them back.  Returns matchFeatureMap's score (ndt_feature_map.h:104-122).
    double matchNodesUsingFeatureMap(size_t idx_ref, size_t idx_mov, CorrespondencesGPU &matches, Eigen::Affine3d &T,
                                     const ndtgpu_featmatch_params *params = nullptr)
    {
        if (!bank_ || !bank_->features()) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "matchNodesUsingFeatureMap: the nodes have no feature maps");
        const uint32_t ref = (uint32_t)bank_->mapSet(nodes_[idx_ref].map->slot()), mov = (uint32_t)bank_->mapSet(nodes_[idx_mov].map->slot());
        const ndtgpu_fuser_feat_result r = nodes_[idx_ref].map->last_feat, m = nodes_[idx_mov].map->last_feat;
        if (r.n_map == 0 || m.n_map == 0) return std::numeric_limits<double>::max();
        ndtgpu_featbank *h = bank_->features();
        ndtgpu_host::check(ndtgpu_featbank_match(h, &ref, &mov, 1, params, nullptr), "ndtgpu_featbank_match");
        ndtgpu_featmatch_result res;
        double T16[16];
        std::vector<uint32_t> corr(2 * bank_->featMaxPoints());
        ndtgpu_host::check(ndtgpu_featbank_results(h, 0, 1, &res, T16, corr.data()), "ndtgpu_featbank_results");
        matches.clear();
        for (int k = 0; k < res.n_inliers; k++) matches.emplace_back(corr[2 * k], corr[2 * k + 1]);
        if (res.status == NDTGPU_FEATMATCH_NO_HYPOTHESIS) return std::numeric_limits<double>::max();
        for (int e = 0; e < 16; e++) T.data()[e] = T16[e];
        return res.score;
    }

    // update(Tmotion, cloud, pts) -- ndt_feature_graph.cpp:60-144: the scan goes to the current node's fuser; once the robot
    // has moved newNodeTranslDist inside a node, the scan is only LOCALISED there (no fuse-in) and becomes the first scan of
    // a new node at the pose that localisation gave.  Returns the pose in world coordinates.
    Eigen::Affine3d update(Eigen::Affine3d Tmotion, pcl::PointCloud<pcl::PointXYZ> &cloud, const InterestPointVec &pts)
    {
        return update_with(Tmotion, cloud, pts);
    }

private:
    template <class Pts>
    Eigen::Affine3d update_with(Eigen::Affine3d Tmotion, pcl::PointCloud<pcl::PointXYZ> &cloud, const Pts &pts)
    {
        distance_moved_in_last_node_ += Tmotion.translation().norm();
        const bool leave = distance_moved_in_last_node_ > params_.newNodeTranslDist;
        NDTFeatureNode &cur = nodes_.back();
        const Eigen::Affine3d local = cur.map->update(Tmotion, cloud, pts, !leave, !leave);
        Tnow = cur.T * local;
        cur.Tlocal_odom = cur.Tlocal_odom * Tmotion;
        cur.Tlocal_fuse = local;
        if (leave) {
            distance_moved_in_last_node_ = 0.;
            if (params_.popNodes) {          // (only the newest node is kept)
                delete nodes_.back().map;
                nodes_.pop_back();
                pool_->release_last();
            }
            open_node(Tnow, cloud, pts, false);
            return Tnow;
        }
        if (params_.storePtsInNodes && cur.nbUpdates % params_.storePtsInNodesIncr == 0) {
            Eigen::Affine3d in_node = local * sensor_pose_;
            cur.addCloud(in_node, cloud);
        }
        cur.nbUpdates++;
        return Tnow;
    }

public:

    // computeLink (graph.cpp:162-177) without the FLIRT feature match that seeds link.T upstream (out of scope): the
    // relative pose of the node estimates, scored by the occupancy overlap like the reference
    NDTFeatureLink computeLink(size_t idx_ref, size_t idx_mov)
    {
        NDTFeatureLink m(idx_ref, idx_mov);
        m.T = nodes_[idx_ref].T.inverse() * nodes_[idx_mov].T;
        m.score = overlapNDTOccupancyScore(nodes_[idx_ref], nodes_[idx_mov], m.T);
        return m;
    }
    // computeAllPossibleLinks (graph.cpp:395-405); the overlap scores of all links in ONE device call
    std::vector<NDTFeatureLink> computeAllPossibleLinks()
    {
        std::vector<NDTFeatureLink> ret;
        for (size_t i = 0; i < nodes_.size(); i++)
            for (size_t j = i + 1; j < nodes_.size(); j++) {
                NDTFeatureLink m(i, j);
                m.T = nodes_[i].T.inverse() * nodes_[j].T;
                ret.push_back(m);
            }
        score_links(ret);
        return ret;
    }
    std::vector<NDTFeatureLink> getIncrementalLinks() const   // graph.cpp:180-204
    {
        std::vector<NDTFeatureLink> ret;
        for (size_t i = 0; i + 1 < nodes_.size(); i++) {
            NDTFeatureLink m(i, i + 1);
            m.T = nodes_[i].T.inverse() * nodes_[i + 1].T;
            m.score = -1.;
            ret.push_back(m);
        }
        return ret;
    }

    // updateLinkUsingNDTRegistration (graph.cpp:260-345): one link
    void updateLinkUsingNDTRegistration(NDTFeatureLink &link, int nb_neighbours, bool keepScore)
    {
        std::vector<NDTFeatureLink> one(1, link);
        updateLinksUsingNDTRegistration(one, nb_neighbours, keepScore);
        link = one[0];
    }
    // updateLinksUsingNDTRegistration (graph.cpp:347-353): every link's match, covariance and overlap score in three
    // batched device calls
    void updateLinksUsingNDTRegistration(std::vector<NDTFeatureLink> &links, int nb_neighbours, bool keepScore)
    {
        const size_t n = links.size();
        if (!n) return;
        std::vector<uint32_t> ti(n), si(n);
        std::vector<double> T(16 * n), before(16 * n), cov(36 * n);
        std::vector<ndtgpu_match_result> res(n);
        std::vector<int32_t> singular(n);
        for (size_t k = 0; k < n; k++) {
            ti[k] = (uint32_t)nodes_[links[k].ref_idx].getNDTMap().slot();
            si[k] = (uint32_t)nodes_[links[k].mov_idx].getNDTMap().slot();
            const double *m = links[k].T.data();
            for (int q = 0; q < 16; q++) T[16 * k + q] = before[16 * k + q] = m[q];
        }
        lslgeneric::NDTMatcherD2D matcher_d2d;          // default-constructed, graph.cpp:261
        matcher_d2d.n_neighbours = nb_neighbours;       // graph.cpp:262
        ndtgpu_match_params p = matcher_d2d.params(0x3f, true);
        ndtgpu_mapset *pool = pool_->handle();
        ndtgpu_host::check(ndtgpu_match_batch(pool, ti.data(), pool, si.data(), T.data(), n, &p, res.data(), nullptr), "ndtgpu_match_batch");
        ndtgpu_host::check(ndtgpu_covariance_batch(pool, ti.data(), pool, si.data(), T.data(), n, &p, matcher_d2d.covariance_mode, cov.data(),
                                                   singular.data(), nullptr), "ndtgpu_covariance_batch");
        for (size_t k = 0; k < n; k++) {
            double *m = links[k].T.data();
            bool same = true;
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) same = same && (before[16 * k + c * 4 + r] == T[16 * k + c * 4 + r]);
            for (int q = 0; q < 16; q++) m[q] = T[16 * k + q];
            links[k].converged = res[k].converged != 0;
            links[k].iterations = res[k].iterations;
            if (links[k].cov_3d.rows() != 6) links[k].cov_3d.resize(6, 6);
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++)   // "NOTHING HAPPENED": 0.02 * identity, graph.cpp:300-310
                    links[k].cov_3d(a, b) = same ? ((a == b) ? 0.02 : 0.0) : cov[36 * k + a * 6 + b];
        }
        if (!keepScore) score_links(links);             // graph.cpp:335-341
    }
    void updateAllGraphLinksUsingNDTRegistration(int nb_neighbours, bool keepScore)
    {
        // (the reference updates COPIES of its links here, graph.cpp:249-258: the results are lost; the stored links are
        //  updated instead)
        updateLinksUsingNDTRegistration(links_, nb_neighbours, keepScore);
    }

    // getValidLinks (graph.cpp:527-556)
    std::vector<NDTFeatureLink> getValidLinks(const std::vector<NDTFeatureLink> &links, double maxScore, double maxDist,
                                              double maxAngularDist, int minIdxDist) const
    {
        std::vector<NDTFeatureLink> ret;
        for (size_t i = 0; i < links.size(); i++) {
            if (links[i].getScore() > maxScore) continue;
            if (std::abs((int)links[i].getMovIdx() - (int)links[i].getRefIdx()) < minIdxDist) continue;
            const NDTFeatureNode &ref_node = nodes_[links[i].getRefIdx()];
            const NDTFeatureNode &mov_node = nodes_[links[i].getMovIdx()];
            Eigen::Affine3d Tlink = ref_node.T * links[i].T;
            double dist, angular_dist;
            distanceBetweenAffine3d(mov_node.T, Tlink, dist, angular_dist);
            if (dist < maxDist && angular_dist < maxAngularDist) ret.push_back(links[i]);
        }
        return ret;
    }

    Params params_;
    NDTFeatureFuserHMT::Params fuser_params_;
    MotionModel2d::Params motion_params_;

protected:
    // the node fusers are the slots of ONE bank over the pool the node maps live in
    NDTFeatureFuserHMT *new_fuser()
    {
        if (!pool_) {
            const double c[3] = {0, 0, 0}, s[3] = {fuser_params_.map_size_x, fuser_params_.map_size_y, fuser_params_.map_size_z};
            pool_ = std::make_shared<ndtgpu_host::MapPool>(fuser_params_.resolution, c, s, params_.maxNodes);
            bank_ = std::make_shared<ndtgpu_host::FuserBank>(NDTFeatureFuserHMT::bankParams(fuser_params_, motion_params_, sensor_pose_), pool_);
        }
        return new NDTFeatureFuserHMT(fuser_params_, bank_, pool_->allocate());
    }
    // a new node at world pose `at`, its map started from `cloud`
    template <class Pts>
    void open_node(const Eigen::Affine3d &at, pcl::PointCloud<pcl::PointXYZ> &cloud, const Pts &pts, bool preLoad)
    {
        NDTFeatureNode node;
        node.T = at;
        node.map = new_fuser();
        node.map->setMotionParams(motion_params_);
        node.map->setSensorPose(sensor_pose_);
        node.map->initialize(Eigen::Affine3d::Identity(), cloud, pts, preLoad);
        if (params_.storePtsInNodes && nodes_.empty()) {
            Eigen::Affine3d in_node = sensor_pose_;
            node.addCloud(in_node, cloud);
        }
        nodes_.push_back(node);
    }
    void score_links(std::vector<NDTFeatureLink> &links)
    {
        const size_t n = links.size();
        if (!n) return;
        std::vector<uint32_t> ri(n), mi(n);
        std::vector<double> T(16 * n), score(n);
        for (size_t k = 0; k < n; k++) {
            ri[k] = (uint32_t)nodes_[links[k].ref_idx].getNDTMap().slot();
            mi[k] = (uint32_t)nodes_[links[k].mov_idx].getNDTMap().slot();
            const double *m = links[k].T.data();
            for (int q = 0; q < 16; q++) T[16 * k + q] = m[q];
        }
        ndtgpu_host::check(ndtgpu_overlap_score_batch(pool_->handle(), ri.data(), pool_->handle(), mi.data(), T.data(), n, score.data(), nullptr, nullptr),
                           "ndtgpu_overlap_score_batch");
        for (size_t k = 0; k < n; k++) links[k].score = score[k];
    }

    std::shared_ptr<ndtgpu_host::MapPool> pool_;
    std::shared_ptr<ndtgpu_host::FuserBank> bank_;
    std::vector<NDTFeatureNode> nodes_;
    std::vector<NDTFeatureLink> links_;
    Eigen::Affine3d sensor_pose_, Tnow;
    double distance_moved_in_last_node_;
};

// convertEigenAffine3dToIsamPose2d / convertIsamPose2dToEigenAffine3d (ndt_offline_mapper.h:8-26); isam::Pose2d is (x, y, t)
inline Pose2d convertEigenAffine3dToIsamPose2d(const Eigen::Affine3d &a)
{
    return Pose2d(a.translation()(0), a.translation()(1), getRobustYawFromAffine3d(a));
}
inline Eigen::Affine3d convertIsamPose2dToEigenAffine3d(const Pose2d &p)
{
    return ndtgpu_host::affine_from_pose(p(0), p(1), 0., 0., 0., p(2));
}

// optimizeGraphUsingISAM (ndt_offline_mapper.h:40-107; called at ndt_feature_graph_opt.cpp:164) on the device: one graph of a
// ndtgpu_pgo bank (include/ndtgpu.h gives the factors, the Gauss-Newton stop rule and what differs from iSAM).  As upstream: node
// 0's pose is the prior (:59-63), the links with score < 0 are added first (:74-82) and then EVERY link, those again (:86-93),
// every factor at the information 100 * I3 (:45), and the poses go back with setPose (:101-104).  `params` / `result` are
// additions: the stop rule's parameters (NULL: the defaults), the optimiser's report, and `wide`: the chip-wide form
// (ndtgpu_pgo_optimize_wide: one launch per pass over the whole device), the one to ask for above some 600 nodes -- the mapper's
// graph of thousands of nodes -- where the one-workgroup form leaves the chip idle.
namespace pgo_detail {
// the body of optimizeGraphUsingISAM and of optimizeGraphUsingISAMWithCov: `marginals` (NULL: none) receives the nodes' records and
// makes the call ask for every node's 3x3 block behind the optimisation, on the same handle, and hand it over with setCov
inline void optimize_graph_se2(NDTFeatureGraphInterface &graph, const ndtgpu_pgo_params *params, ndtgpu_pgo_result *result, bool wide,
                               std::vector<ndtgpu_pgo_marginal_result> *marginals)
{
    const size_t n = graph.getNbNodes();
    if (n == 0) return;
    std::vector<double> pose(3 * n), meas;
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < n; i++) {
        const Pose2d p = convertEigenAffine3dToIsamPose2d(graph.getNodeInterface(i).getPose());
        for (int a = 0; a < 3; a++) pose[3 * i + a] = p(a);
    }
    for (int pass = 0; pass < 2; pass++)
        for (size_t i = 0; i < graph.getNbLinks(); i++) {
            const NDTFeatureLinkInterface &link = graph.getLinkInterface(i);
            if (pass == 0 && !(link.getScore() < 0.)) continue;
            const Pose2d z = convertEigenAffine3dToIsamPose2d(link.getRelPose());
            ref.push_back((uint32_t)link.getRefIdx());
            mov.push_back((uint32_t)link.getMovIdx());
            for (int a = 0; a < 3; a++) meas.push_back(z(a));
        }
    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(1, n, ref.size(), &h), "ndtgpu_pgo_create");
    ndtgpu_status rc = ndtgpu_pgo_set_graph(h, 0, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr);
    if (rc == NDTGPU_OK) rc = wide ? ndtgpu_pgo_optimize_wide(h, 0, params, nullptr, nullptr) : ndtgpu_pgo_optimize(h, 0, 1, params, nullptr);
    ndtgpu_pgo_result r;
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo_poses(h, 0, pose.data(), nullptr, &r);
    std::vector<double> cov9;
    if (rc == NDTGPU_OK && marginals) {
        std::vector<uint32_t> g(n, 0), q(n);
        for (size_t i = 0; i < n; i++) q[i] = (uint32_t)i;
        cov9.resize(9 * n);
        marginals->resize(n);
        rc = ndtgpu_pgo_marginals(h, n, g.data(), q.data(), nullptr, params, nullptr, cov9.data(), nullptr, marginals->data());
    }
    const std::string err = rc == NDTGPU_OK ? "" : ndtgpu_last_error();
    ndtgpu_pgo_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "optimizeGraphUsingISAM: " + err);
    if (result) *result = r;
    for (size_t i = 0; i < n; i++) {
        graph.getNodeInterface(i).setPose(convertIsamPose2dToEigenAffine3d(Pose2d(pose[3 * i], pose[3 * i + 1], pose[3 * i + 2])));
        if (marginals) {
            Eigen::Matrix3d C;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) C(a, b) = cov9[9 * i + 3 * a + b];
            graph.getNodeInterface(i).setCov(C);
        }
    }
}
}   // namespace pgo_detail

inline void optimizeGraphUsingISAM(NDTFeatureGraphInterface &graph, const ndtgpu_pgo_params *params = nullptr,
                                   ndtgpu_pgo_result *result = nullptr, bool wide = false)
{
    pgo_detail::optimize_graph_se2(graph, params, result, wide, nullptr);
}

// optimizeGraphUsingISAM, and what it leaves out upstream (ndt_offline_mapper.h:101-104 only ever calls setPose): the same
// optimisation -- the same poses, bit for bit -- and then every node's marginal covariance through setCov
// (NDTFeatureNodeInterface, interfaces.h:16): the 3x3 block of (x, y, yaw) in the graph's frame (include/ndtgpu.h "Marginal
// covariances").  The link doubling above is part of the cost, so the covariances reflect it: a link with score < 0 counts twice.
// `params` is used for both steps, as the marginals need the prior the graph was optimised with; `marginals` (NULL: not wanted)
// receives a record per node.
inline void optimizeGraphUsingISAMWithCov(NDTFeatureGraphInterface &graph, const ndtgpu_pgo_params *params = nullptr,
                                          ndtgpu_pgo_result *result = nullptr, std::vector<ndtgpu_pgo_marginal_result> *marginals = nullptr,
                                          bool wide = false)
{
    std::vector<ndtgpu_pgo_marginal_result> own;
    pgo_detail::optimize_graph_se2(graph, params, result, wide, marginals ? marginals : &own);
}

// optimizeGraphUsingISAM(graph, wide): the defaults, in the form asked for
inline void optimizeGraphUsingISAM(NDTFeatureGraphInterface &graph, bool wide) { optimizeGraphUsingISAM(graph, nullptr, nullptr, wide); }

// The 6-DoF back end the reference does not have (it calls graph.force2D() before iSAM, ndt_feature_graph_opt.cpp:147): one graph
// of a ndtgpu_pgo3 bank (include/ndtgpu.h "SE(3) pose-graph optimisation").  Node poses and link.T go in as they are, WITHOUT
// force2D; a link's information is the inverse of its cov_3d (ndt_feature_graph.cpp:296-330) by
// ndtgpu_pgo3_link_from_registration -- 50 * I6 where it does not invert, 100 * I6 for a link whose cov_3d is not 6x6; node 0's
// pose is the prior; every link is taken once; the poses go back with setPose.  `links` are NDTFeatureLink because cov_3d is not
// part of NDTFeatureLinkInterface.  `wide`: the chip-wide form (ndtgpu_pgo3_optimize_wide: one launch per pass over the whole
// device), the one to ask for for the mapper's one large graph; include/ndtgpu.h says where the two forms cross.
namespace pgo_detail {
// the body of optimizeGraph3D and of optimizeGraph3DWithCov: `cov36` (NULL: none) receives every node's 6x6 block, row-major, asked
// for behind the optimisation on the same handle, `marginals` (may be NULL) the nodes' records
inline void optimize_graph_se3(NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links, const ndtgpu_pgo3_params *params,
                               ndtgpu_pgo_result *result, bool wide, std::vector<double> *cov36, std::vector<ndtgpu_pgo_marginal_result> *marginals)
{
    const size_t n = graph.getNbNodes(), m = links.size();
    if (n == 0) return;
    std::vector<double> T16(16 * n), Z16(16 * m), W36(36 * m);
    std::vector<uint32_t> ref(m), mov(m);
    for (size_t i = 0; i < n; i++) std::copy_n(graph.getNodeInterface(i).getPose().data(), 16, &T16[16 * i]);
    for (size_t k = 0; k < m; k++) {
        const NDTFeatureLink &l = links[k];
        ref[k] = (uint32_t)l.ref_idx;
        mov[k] = (uint32_t)l.mov_idx;
        double cov[36];
        const bool has_cov = l.cov_3d.rows() == 6 && l.cov_3d.cols() == 6;
        if (has_cov)
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) cov[6 * a + b] = l.cov_3d(a, b);
        ndtgpu_host::check(ndtgpu_pgo3_link_from_registration(l.T.data(), has_cov ? cov : nullptr, 0, &Z16[16 * k], &W36[36 * k]),
                           "ndtgpu_pgo3_link_from_registration");
    }
    ndtgpu_pgo3 *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo3_create(1, n, m, &h), "ndtgpu_pgo3_create");
    ndtgpu_status rc = ndtgpu_pgo3_set_graph(h, 0, n, T16.data(), m, ref.data(), mov.data(), Z16.data(), W36.data());
    if (rc == NDTGPU_OK) rc = wide ? ndtgpu_pgo3_optimize_wide(h, 0, params, nullptr, nullptr) : ndtgpu_pgo3_optimize(h, 0, 1, params, nullptr);
    ndtgpu_pgo_result r;
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo3_poses(h, 0, T16.data(), &r);
    if (rc == NDTGPU_OK && cov36) {
        std::vector<uint32_t> g(n, 0), q(n);
        for (size_t i = 0; i < n; i++) q[i] = (uint32_t)i;
        std::vector<ndtgpu_pgo_marginal_result> own;
        std::vector<ndtgpu_pgo_marginal_result> &mr = marginals ? *marginals : own;
        cov36->resize(36 * n);
        mr.resize(n);
        rc = ndtgpu_pgo3_marginals(h, n, g.data(), q.data(), nullptr, params, nullptr, cov36->data(), nullptr, mr.data());
    }
    const std::string err = rc == NDTGPU_OK ? "" : ndtgpu_last_error();
    ndtgpu_pgo3_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "optimizeGraph3D: " + err);
    if (result) *result = r;
    for (size_t i = 0; i < n; i++) {
        Eigen::Affine3d T;
        std::copy_n(&T16[16 * i], 16, T.data());
        graph.getNodeInterface(i).setPose(T);
    }
}
}   // namespace pgo_detail

inline void optimizeGraph3D(NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links,
                            const ndtgpu_pgo3_params *params = nullptr, ndtgpu_pgo_result *result = nullptr, bool wide = false)
{
    pgo_detail::optimize_graph_se3(graph, links, params, result, wide, nullptr, nullptr);
}

// optimizeGraph3D, and beside it the nodes' 6x6 marginal covariances: cov36 receives n_nodes x 36 doubles, node i's block row-major
// in (rho, phi) of the node's OWN tangent frame (include/ndtgpu.h "Marginal covariances"; NDTFeatureNodeInterface has no place for
// a 6x6, so setCov is not called).  The poses are those of optimizeGraph3D, bit for bit; `params` is used for both steps.
inline void optimizeGraph3DWithCov(NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links, std::vector<double> &cov36,
                                   const ndtgpu_pgo3_params *params = nullptr, ndtgpu_pgo_result *result = nullptr,
                                   std::vector<ndtgpu_pgo_marginal_result> *marginals = nullptr, bool wide = false)
{
    pgo_detail::optimize_graph_se3(graph, links, params, result, wide, &cov36, marginals);
}

// optimizeGraph3D(graph): the graph's own current links
inline void optimizeGraph3D(NDTFeatureGraph &graph, const ndtgpu_pgo3_params *params = nullptr, ndtgpu_pgo_result *result = nullptr,
                            bool wide = false)
{
    optimizeGraph3D(graph, graph.getCurrentLinks(), params, result, wide);
}

// optimizeGraphUsingISAM with a robust cost (include/ndtgpu.h "robust loop-closure weighting": Huber, Cauchy or DCS by iteratively
// re-weighted least squares round the same optimiser), for the wrong loop closure that getValidLinks lets through.  The factors
// are those of optimizeGraphUsingISAM, the doubling included; links between nodes closer than robust->min_index_gap -- the
// incremental links -- are never re-weighted.  link_weights_out (NULL: not wanted) receives one weight per link of the graph, in
// the graph's order: 1 for a link the optimisation trusted, towards 0 for one it weighted down.  `robust` NULL: the defaults (DCS,
// Phi = 1); `result` the robust call's report.
inline void optimizeGraphUsingISAMRobust(NDTFeatureGraphInterface &graph, const ndtgpu_pgo_robust_params *robust = nullptr,
                                         std::vector<double> *link_weights_out = nullptr, const ndtgpu_pgo_params *params = nullptr,
                                         ndtgpu_pgo_robust_result *result = nullptr, bool wide = false)
{
    const size_t n = graph.getNbNodes(), m = graph.getNbLinks();
    if (n == 0) return;
    std::vector<double> pose(3 * n), meas;
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < n; i++) {
        const Pose2d p = convertEigenAffine3dToIsamPose2d(graph.getNodeInterface(i).getPose());
        for (int a = 0; a < 3; a++) pose[3 * i + a] = p(a);
    }
    for (int pass = 0; pass < 2; pass++)
        for (size_t i = 0; i < m; i++) {
            const NDTFeatureLinkInterface &link = graph.getLinkInterface(i);
            if (pass == 0 && !(link.getScore() < 0.)) continue;
            const Pose2d z = convertEigenAffine3dToIsamPose2d(link.getRelPose());
            ref.push_back((uint32_t)link.getRefIdx());
            mov.push_back((uint32_t)link.getMovIdx());
            for (int a = 0; a < 3; a++) meas.push_back(z(a));
        }
    const ndtgpu_pgo_wide_params wide_defaults = {32, 0};
    std::vector<double> weight(ref.size());
    ndtgpu_pgo *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo_create(1, n, ref.size(), &h), "ndtgpu_pgo_create");
    ndtgpu_status rc = ndtgpu_pgo_set_graph(h, 0, n, pose.data(), ref.size(), ref.data(), mov.data(), meas.data(), nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo_optimize_robust(h, 0, 1, params, robust, wide ? &wide_defaults : nullptr, nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo_poses(h, 0, pose.data(), nullptr, nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo_robust_links(h, 0, nullptr, weight.data(), nullptr, result);
    const std::string err = rc == NDTGPU_OK ? "" : ndtgpu_last_error();
    ndtgpu_pgo_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "optimizeGraphUsingISAMRobust: " + err);
    for (size_t i = 0; i < n; i++)
        graph.getNodeInterface(i).setPose(convertIsamPose2dToEigenAffine3d(Pose2d(pose[3 * i], pose[3 * i + 1], pose[3 * i + 2])));
    if (link_weights_out) link_weights_out->assign(weight.end() - (std::ptrdiff_t)m, weight.end());      // (the second pass: every link, in order)
}

// optimizeGraph3D with a robust cost: the factors of optimizeGraph3D, the weighting of optimizeGraphUsingISAMRobust; one weight
// per link of `links`
inline void optimizeGraph3DRobust(NDTFeatureGraphInterface &graph, const std::vector<NDTFeatureLink> &links,
                                  const ndtgpu_pgo_robust_params *robust = nullptr, std::vector<double> *link_weights_out = nullptr,
                                  const ndtgpu_pgo3_params *params = nullptr, ndtgpu_pgo_robust_result *result = nullptr, bool wide = false)
{
    const size_t n = graph.getNbNodes(), m = links.size();
    if (n == 0) return;
    std::vector<double> T16(16 * n), Z16(16 * m), W36(36 * m), weight(m);
    std::vector<uint32_t> ref(m), mov(m);
    for (size_t i = 0; i < n; i++) std::copy_n(graph.getNodeInterface(i).getPose().data(), 16, &T16[16 * i]);
    for (size_t k = 0; k < m; k++) {
        const NDTFeatureLink &l = links[k];
        ref[k] = (uint32_t)l.ref_idx;
        mov[k] = (uint32_t)l.mov_idx;
        double cov[36];
        const bool has_cov = l.cov_3d.rows() == 6 && l.cov_3d.cols() == 6;
        if (has_cov)
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) cov[6 * a + b] = l.cov_3d(a, b);
        ndtgpu_host::check(ndtgpu_pgo3_link_from_registration(l.T.data(), has_cov ? cov : nullptr, 0, &Z16[16 * k], &W36[36 * k]),
                           "ndtgpu_pgo3_link_from_registration");
    }
    const ndtgpu_pgo_wide_params wide_defaults = {32, 0};
    ndtgpu_pgo3 *h = nullptr;
    ndtgpu_host::check(ndtgpu_pgo3_create(1, n, m, &h), "ndtgpu_pgo3_create");
    ndtgpu_status rc = ndtgpu_pgo3_set_graph(h, 0, n, T16.data(), m, ref.data(), mov.data(), Z16.data(), W36.data());
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo3_optimize_robust(h, 0, 1, params, robust, wide ? &wide_defaults : nullptr, nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo3_poses(h, 0, T16.data(), nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_pgo3_robust_links(h, 0, nullptr, weight.data(), nullptr, result);
    const std::string err = rc == NDTGPU_OK ? "" : ndtgpu_last_error();
    ndtgpu_pgo3_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "optimizeGraph3DRobust: " + err);
    for (size_t i = 0; i < n; i++) {
        Eigen::Affine3d T;
        std::copy_n(&T16[16 * i], 16, T.data());
        graph.getNodeInterface(i).setPose(T);
    }
    if (link_weights_out) *link_weights_out = weight;
}

// The product of the mapper: ONE map from the graph's node maps under the node poses T -- graph->getMap() moved by getT()
// (ndt_feature2d_fuser.cpp:425-432), the combination NDTFeatureGraph::fuse() (ndt_feature_graph.h:149-152) declares but leaves
// empty, the single map ndt_feature_mcl_node.cpp:174 localises in.  On the device in one call: ndtgpu_world_assemble
// (include/ndtgpu.h "world-map assembly": pseudoTransformNDT of every cell, binned by the world's LazyGrid, cells that share a
// world cell merged as pooled sample statistics).  `world` has its geometry (guessSize or initialize) and a resolution not below
// the nodes'; its previous content is replaced.  `node_maps` live in one pool.  Returns the call's report.
inline ndtgpu_world_result assembleWorldMap(const std::vector<lslgeneric::NDTMap *> &node_maps, const std::vector<Eigen::Affine3d> &poses,
                                            lslgeneric::NDTMap &world, const ndtgpu_world_params *params = nullptr)
{
    if (node_maps.size() != poses.size()) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "assembleWorldMap: one pose per node map");
    const uint32_t off[2] = {0u, (uint32_t)node_maps.size()};
    std::vector<uint32_t> idx(node_maps.size() + 1, 0u);
    std::vector<double> T16(16 * (node_maps.size() + 1), 0.);
    ndtgpu_mapset *src = world.handle();               // (no nodes: any set will do, nothing of it is read)
    for (size_t i = 0; i < node_maps.size(); i++) {
        if (i == 0) src = node_maps[0]->handle();
        else if (node_maps[i]->handle() != src) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "assembleWorldMap: the node maps must live in one pool");
        idx[i] = (uint32_t)node_maps[i]->slot();
        for (int q = 0; q < 16; q++) T16[16 * i + q] = poses[i].data()[q];
    }
    ndtgpu_world_result r;
    ndtgpu_host::check(ndtgpu_world_assemble(world.handle(), world.slot(), 1, src, off, idx.data(), T16.data(), params, &r, nullptr),
                       "ndtgpu_world_assemble");
    return r;
}
// every node's map under the node's pose T, in one call
inline ndtgpu_world_result assembleWorldMap(const NDTFeatureGraph &graph, lslgeneric::NDTMap &world, const ndtgpu_world_params *params = nullptr)
{
    std::vector<lslgeneric::NDTMap *> maps;
    std::vector<Eigen::Affine3d> poses;
    for (size_t i = 0; i < graph.getNbNodes(); i++) {
        maps.push_back(graph.getNode(i).map->map);
        poses.push_back(graph.getNode(i).T);
    }
    return assembleWorldMap(maps, poses, world, params);
}

}  // namespace ndt_feature
