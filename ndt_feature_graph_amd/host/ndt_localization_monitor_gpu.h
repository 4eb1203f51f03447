// ndt_localization_monitor_gpu.h -- host C++ mirror of the reference's localisation monitor (flirtlib_ros) over the
// ndtgpu_locmon_* calls of libndtgpu.so (include/ndtgpu.h, "localisation monitor": the field, the badness, the winner's rule and
// what deviates from the reference are stated there).
//   flirtlib_ros::ScanPoseEvaluatorGPU        ScanPoseEvaluator (localization_monitor.h:41-63, localization_monitor.cpp:41-120):
//                                             the constructor builds the distance field, operator()(scan, pose) is the badness,
//                                             adjustPose(scan, init, pos_range, dpos, dtheta) the lattice search -- ONE device
//                                             call for the whole lattice
//   flirtlib_ros::LocalizationMonitorGPU      update(scan, pose) follows scanCB (localization_monitor_node.cpp:498-537):
//                                             localised -> updateLocalized's box test (:439-440) decides whether the scan's
//                                             features become a reference set; otherwise updateUnlocalized (:331-413): match
//                                             against every reference set, pick, compose, evaluate, verdict
// OccupancyGridGPU (ndt_occupancy_grid_gpu.h) stands where nav_msgs::OccupancyGrid stands, ndt_feature::LaserScanGPU where
// sensor_msgs::LaserScan stands, OccupancyGridGPU's Pose where geometry_msgs::Pose stands.
// Left out, as in the C-ABI: the scan database (the reference sets live in the object), the one-day expiry, the navigation counter,
// odometry compensation.  This header owns no device memory, so relocalisation reads the match records back and applies the pick
// rule of ndtgpu_locmon_pick_device to them on the host (ndtgpu_locmon_compose makes the pose); a caller that holds device
// buffers keeps extract -> match -> pick -> evaluate on the device with the C-ABI.
// There is no CPU fallback: a failed C-ABI call throws ndtgpu_host::Error.
#pragma once
#include "ndt_feature_map_gpu.h"
#include "ndt_occupancy_grid_gpu.h"

#include <cmath>
#include <limits>

namespace flirtlib_ros {

using PoseGPU = OccupancyGridGPU::MapMetaData::Pose;
using ndt_feature::LaserScanGPU;

// the pose as the library carries it: (x, y, cos yaw, sin yaw), the yaw that of tf::getYaw -- the heading of the rotated x axis
inline void locmonPose4(const PoseGPU &p, double out[4])
{
    const Eigen::Affine3d T = ndtgpu_host::pose_msg_to_affine(p);
    const double c = T(0, 0), s = T(1, 0), n = std::sqrt(c * c + s * s);
    out[0] = p.position.x;
    out[1] = p.position.y;
    out[2] = n > 0 ? c / n : 1.0;
    out[3] = n > 0 ? s / n : 0.0;
}
// makePose (common.cpp:47-54) from the cosine and sine of the yaw: the quaternion (0, 0, sin(yaw / 2), cos(yaw / 2))
inline PoseGPU locmonMakePose(double x, double y, double c, double s)
{
    PoseGPU p;
    const double yaw = std::atan2(s, c);
    p.position.x = x;
    p.position.y = y;
    p.orientation.z = std::sin(0.5 * yaw);
    p.orientation.w = std::cos(0.5 * yaw);
    return p;
}

class ScanPoseEvaluatorGPU {
public:
    // ScanPoseEvaluator(g, threshold): threshold is the field's reach (the node passes badness_threshold * 1.5)
    ScanPoseEvaluatorGPU(const OccupancyGridGPU &g, double threshold, int occupied_min = 55, size_t max_beams = 8192,
                         size_t max_candidates = (size_t)1 << 20)
    {
        ndtgpu_default_locmon_params(&prm_);
        prm_.max_dist = threshold;
        prm_.occupied_min = occupied_min;
        const size_t w = g.info.width, hgt = g.info.height;
        if (g.data.size() != w * hgt) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "ScanPoseEvaluatorGPU: data is not width x height");
        ndtgpu_host::check(ndtgpu_locmon_check(1, w, hgt, g.info.resolution, 1, 0.0, 0.0, 1, 0, &prm_), "ndtgpu_locmon_check");
        ndtgpu_host::check(ndtgpu_locmon_create(1, w * hgt, max_beams, max_candidates, &h_), "ndtgpu_locmon_create");
        const double origin[2] = {g.info.origin.position.x, g.info.origin.position.y};
        const ndtgpu_status rc = ndtgpu_locmon_set_grids(h_, g.data.data(), 1, w, hgt, g.info.resolution, origin, &prm_);
        if (rc != NDTGPU_OK) {
            const std::string err = ndtgpu_last_error();
            ndtgpu_locmon_destroy(h_);
            throw ndtgpu_host::Error(rc, "ndtgpu_locmon_set_grids: " + err);
        }
    }
    ~ScanPoseEvaluatorGPU() { ndtgpu_locmon_destroy(h_); }
    ScanPoseEvaluatorGPU(const ScanPoseEvaluatorGPU &) = delete;
    ScanPoseEvaluatorGPU &operator=(const ScanPoseEvaluatorGPU &) = delete;

    // the range gate of every later call (an addition: the reference has none)
    void setRangeGate(double r_min, double r_max) { prm_.r_min = r_min; prm_.r_max = r_max; }

    // the whole record of a (scan, pose)
    ndtgpu_locmon_result evaluate(const LaserScanGPU &scan, const PoseGPU &pose)
    {
        beams(scan);
        ndtgpu_locmon_query q;
        double p4[4];
        locmonPose4(pose, p4);
        q.x = p4[0]; q.y = p4[1]; q.c = p4[2]; q.s = p4[3];
        q.scan = 0;
        q.grid = 0;
        ndtgpu_locmon_result res;
        ndtgpu_host::check(ndtgpu_locmon_evaluate(h_, scan.ranges.data(), 1, &q, 1, &prm_, &res), "ndtgpu_locmon_evaluate");
        return res;
    }
    // float operator()(scan, pose) (:87-120): the median distance of the scan's endpoints to the nearest obstacle
    float operator()(const LaserScanGPU &scan, const PoseGPU &pose) { return (float)evaluate(scan, pose).badness; }

    // adjustPose (:48-85).  `result` and `volume` are additions: the winner's record and every candidate's key in loop order.
    PoseGPU adjustPose(const LaserScanGPU &scan, const PoseGPU &initial_pose, double pos_range, double dpos, double dtheta,
                       ndtgpu_locmon_adjust_result *result = nullptr, std::vector<uint32_t> *volume = nullptr)
    {
        beams(scan);
        double p4[4];
        locmonPose4(initial_pose, p4);
        const double theta0 = std::atan2(p4[3], p4[2]);
        size_t cnt[3];
        ndtgpu_host::check(ndtgpu_calib_lattice(p4[0], p4[1], theta0, pos_range, pos_range, 3.14, dpos, dtheta, cnt, nullptr, nullptr, nullptr,
                                                nullptr, nullptr, 0), "ndtgpu_calib_lattice");
        const size_t room = std::max(cnt[0], std::max(cnt[1], cnt[2]));
        std::vector<double> xs(room), ys(room), yaws(room), cs(room), sn(room);
        ndtgpu_host::check(ndtgpu_calib_lattice(p4[0], p4[1], theta0, pos_range, pos_range, 3.14, dpos, dtheta, cnt, xs.data(), ys.data(),
                                                yaws.data(), cs.data(), sn.data(), room), "ndtgpu_calib_lattice");
        const size_t n = cnt[0] * cnt[1] * cnt[2];
        if (volume) volume->assign(n, 0u);
        ndtgpu_locmon_adjust_result res;
        ndtgpu_host::check(ndtgpu_locmon_adjust(h_, scan.ranges.data(), 1, 0, 0, xs.data(), cnt[0], ys.data(), cnt[1], cs.data(), sn.data(), cnt[2],
                                                &prm_, &res, volume ? volume->data() : nullptr), "ndtgpu_locmon_adjust");
        if (result) *result = res;
        const size_t ix = res.index / (cnt[1] * cnt[2]), iy = (res.index / cnt[2]) % cnt[1], iyaw = res.index % cnt[2];
        return locmonMakePose(xs[ix], ys[iy], cs[iyaw], sn[iyaw]);
    }

    ndtgpu_locmon *handle() const { return h_; }
    const ndtgpu_locmon_params &params() const { return prm_; }

private:
    // the beam table follows the scanner's geometry: installed when it changes
    void beams(const LaserScanGPU &scan)
    {
        if (scan.ranges.size() == n_beams_ && scan.angle_min == angle_min_ && scan.angle_increment == angle_increment_) return;
        ndtgpu_host::check(ndtgpu_locmon_set_beams(h_, scan.ranges.size(), scan.angle_min, scan.angle_increment, nullptr), "ndtgpu_locmon_set_beams");
        n_beams_ = scan.ranges.size();
        angle_min_ = scan.angle_min;
        angle_increment_ = scan.angle_increment;
    }
    ndtgpu_locmon *h_ = nullptr;
    ndtgpu_locmon_params prm_;
    size_t n_beams_ = 0;
    double angle_min_ = 0., angle_increment_ = 0.;
};

// RefScan (localization_monitor_node.cpp): the pose a scan was taken at and its features
struct RefScanGPU {
    PoseGPU pose;
    ndt_feature::InterestPointGPUVec raw_pts;
};

struct LocalizationVerdictGPU {
    bool localised = false;          // badness of the given pose below the threshold
    double badness = 0.;             // of the given pose
    bool added_reference = false;    // the scan's features became a reference set
    bool relocalised = false;        // not localised, a reference scan qualified and its pose's badness is below the threshold
    int ref_scan = -1;               // the picked reference scan, -1 where none qualified
    int n_matches = 0;               // its matches
    double match_badness = 0.;       // of the picked pose (1e9 where none qualified)
    PoseGPU pose;                    // the picked pose
};

class LocalizationMonitorGPU {
public:
    LocalizationMonitorGPU(const OccupancyGridGPU &g, double badness_threshold = 0.25, int min_num_matches = 8, double post_x = -0.275,
                           double post_y = 0.0)
        : evaluator_(g, badness_threshold * 1.5), threshold_(badness_threshold), min_num_matches_(min_num_matches)
    {
        post_[0] = post_x;
        post_[1] = post_y;
    }

    LocalizationVerdictGPU update(const LaserScanGPU &scan, const PoseGPU &pose)
    {
        LocalizationVerdictGPU v;
        v.badness = evaluator_.evaluate(scan, pose).badness;
        v.localised = v.badness < threshold_;
        v.match_badness = 1e9;
        if (v.localised) {
            if (!nearReference(pose)) {
                RefScanGPU r;
                r.pose = pose;
                r.raw_pts = ndt_feature::detectAndDescribe({scan})[0];
                ref_scans.push_back(r);
                v.added_reference = true;
            }
            return v;
        }
        if (ref_scans.empty()) return v;
        // updateUnlocalized: the scan's features against every reference set, the set with the most matches above min_num_matches
        std::vector<ndt_feature::NDTFeatureMapGPU> maps(ref_scans.size() + 1);
        std::vector<const ndt_feature::NDTFeatureMapGPU *> ptrs;
        for (size_t k = 0; k < ref_scans.size(); k++) maps[k].map = ref_scans[k].raw_pts;
        maps.back().map = ndt_feature::detectAndDescribe({scan})[0];
        for (const auto &m : maps) ptrs.push_back(&m);
        std::vector<uint32_t> ref, mov;
        for (size_t k = 0; k < ref_scans.size(); k++) {
            ref.push_back((uint32_t)k);
            mov.push_back((uint32_t)ref_scans.size());
        }
        const ndt_feature::detail::FeatBank bank(ptrs);
        const std::vector<ndt_feature::NDTFeatureMatchLink> links = bank.match(ref, mov, nullptr);
        int best = -1, best_n = 0;
        for (size_t k = 0; k < links.size(); k++) {
            const ndtgpu_featmatch_result &m = links[k].report;
            if (m.status == NDTGPU_FEATMATCH_OK && m.n_inliers > min_num_matches_ && m.n_inliers > best_n) {
                best = (int)k;
                best_n = m.n_inliers;
            }
        }
        if (best < 0) return v;
        const ndtgpu_featmatch_result &m = links[(size_t)best].report;
        double ref4[4], out4[4];
        const double m4[4] = {m.x, m.y, m.c, m.s};
        locmonPose4(ref_scans[(size_t)best].pose, ref4);
        ndtgpu_host::check(ndtgpu_locmon_compose(ref4, m4, post_, out4), "ndtgpu_locmon_compose");
        v.ref_scan = best;
        v.n_matches = best_n;
        v.pose = locmonMakePose(out4[0], out4[1], out4[2], out4[3]);
        v.match_badness = evaluator_.evaluate(scan, v.pose).badness;
        v.relocalised = v.match_badness < threshold_;
        return v;
    }

    ScanPoseEvaluatorGPU &evaluator() { return evaluator_; }
    std::vector<RefScanGPU> ref_scans;

private:
    // updateLocalized's query (:439-440): a reference scan within 0.7 m along x and along y and within 1 rad of the pose
    bool nearReference(const PoseGPU &pose) const
    {
        double p[4], q[4];
        locmonPose4(pose, p);
        for (const RefScanGPU &r : ref_scans) {
            locmonPose4(r.pose, q);
            const double dth = std::atan2(p[3] * q[2] - p[2] * q[3], p[2] * q[2] + p[3] * q[3]);
            if (std::fabs(p[0] - q[0]) < 0.7 && std::fabs(p[1] - q[1]) < 0.7 && std::fabs(dth) < 1.0) return true;
        }
        return false;
    }
    ScanPoseEvaluatorGPU evaluator_;
    double threshold_, post_[2];
    int min_num_matches_;
};

}   // namespace flirtlib_ros
