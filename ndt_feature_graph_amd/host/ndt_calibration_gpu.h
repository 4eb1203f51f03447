// ndt_calibration_gpu.h -- host C++ mirror of the reference's laser-to-base calibration program
// (ndt_feature/src/laser2d_extrinsic_calibration.cpp) over the ndtgpu_calib_* calls of libndtgpu.so (include/ndtgpu.h, "extrinsic
// calibration": the score, the lattice, the winner's rule and what deviates from the reference are stated there).
//   ndt_feature::ScanPairGPU                  ScanPair (:40-125): two clouds with the base poses they were taken at; scoreICP(Ts)
//   ndt_feature::errorFunction                :146-152: the sum of scoreICP over the pairs
//   ndt_feature::bruteForceOptimization       :176-204: the lattice walk -- ONE device call for the whole lattice; it RETURNS the
//                                             winning offset and score, where the reference prints them
//   ndt_feature::CalibrationPairCollector     the callback's anchor and gate walk (:312-349): add(scan cloud, base pose)
// Every search is one device call (ndtgpu_calib_search); scoreICP and errorFunction are searches over a lattice of one node.
// There is no CPU fallback: a failed C-ABI call throws ndtgpu_host::Error.
#pragma once
#include "lslgeneric_gpu.h"

#include <cmath>
#include <limits>

namespace ndt_feature {

// getAsAffine(x, y, yaw) of the reference's utilities
inline Eigen::Affine3d calibGetAsAffine(double x, double y, double yaw)
{
    Eigen::Affine3d T = Eigen::Affine3d::Identity();
    const double c = std::cos(yaw), s = std::sin(yaw);
    T(0, 0) = c; T(0, 1) = -s; T(1, 0) = s; T(1, 1) = c;
    T(0, 3) = x; T(1, 3) = y;
    return T;
}

struct ScanPairGPU {
    pcl::PointCloud<pcl::PointXYZ> cloud1, cloud2;
    Eigen::Affine3d pose1, pose2;
    ScanPairGPU() {}
    ScanPairGPU(const pcl::PointCloud<pcl::PointXYZ> &c1, const Eigen::Affine3d &p1, const pcl::PointCloud<pcl::PointXYZ> &c2,
                const Eigen::Affine3d &p2) : cloud1(c1), cloud2(c2), pose1(p1), pose2(p2) {}
    inline double scoreICP(const Eigen::Affine3d &Ts, const ndtgpu_calib_params *params = nullptr) const;
};

struct CalibrationResultGPU {
    Eigen::Affine3d T;               // the winning sensor offset
    double x = 0., y = 0., yaw = 0.; // ... as the lattice node
    double score = 0.;
    size_t index = 0, n_candidates = 0;
    bool found = false;              // false where the score is >= 1e6: the reference reports nothing then
    uint32_t n_skipped = 0;
    std::vector<double> volume;      // every candidate's score, in loop order (x outer, y middle, yaw inner), where asked for
};

namespace calib_detail {

// one device call over the lattice tables: the clouds of pair k are scans 2k and 2k + 1 of the bank
inline ndtgpu_calib_result search(const std::vector<ScanPairGPU> &pairs, const std::vector<double> &xs, const std::vector<double> &ys,
                                  const std::vector<double> &cs, const std::vector<double> &sn, const ndtgpu_calib_params *params,
                                  std::vector<double> *volume)
{
    if (pairs.empty()) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "calibration: no scan pairs");
    size_t n_points = 1;
    for (const ScanPairGPU &p : pairs) n_points = std::max(n_points, std::max(p.cloud1.size(), p.cloud2.size()));
    const size_t n_scans = 2 * pairs.size(), stride = sizeof(pcl::PointXYZ);
    pcl::PointXYZ pad;
    pad.x = pad.y = pad.z = std::numeric_limits<float>::quiet_NaN();
    std::vector<pcl::PointXYZ> rows(n_scans * n_points, pad);
    std::vector<uint32_t> n_kept(n_scans), idx(n_scans);
    std::vector<double> poses(4 * n_scans);
    for (size_t k = 0; k < n_scans; k++) {
        const ScanPairGPU &p = pairs[k / 2];
        const pcl::PointCloud<pcl::PointXYZ> &c = k % 2 ? p.cloud2 : p.cloud1;
        const Eigen::Affine3d &T = k % 2 ? p.pose2 : p.pose1;
        for (size_t i = 0; i < c.size(); i++) rows[k * n_points + i] = c.points[i];
        n_kept[k] = (uint32_t)c.size();
        idx[k] = (uint32_t)k;
        poses[4 * k] = T(0, 3); poses[4 * k + 1] = T(1, 3); poses[4 * k + 2] = T(0, 0); poses[4 * k + 3] = T(1, 0);
    }
    const size_t n_candidates = xs.size() * ys.size() * cs.size();
    // (the checks first: a bad argument is refused with the library's message, not by the handle's capacity)
    ndtgpu_host::check(ndtgpu_calib_check(n_scans, n_points, stride, n_points * stride, pairs.size(), xs.size(), ys.size(), cs.size(), params),
                       "ndtgpu_calib_check");
    ndtgpu_calib *h = nullptr;
    ndtgpu_host::check(ndtgpu_calib_create(pairs.size(), n_points, n_candidates, &h), "ndtgpu_calib_create");
    if (volume) volume->assign(n_candidates, 0.0);
    ndtgpu_calib_result res;
    const ndtgpu_status rc = ndtgpu_calib_search(h, rows.data(), n_scans, n_points, stride, n_points * stride, n_kept.data(), poses.data(),
                                                 idx.data(), pairs.size(), xs.data(), xs.size(), ys.data(), ys.size(), cs.data(), sn.data(),
                                                 cs.size(), params, &res, volume ? volume->data() : nullptr);
    const std::string err = rc == NDTGPU_OK ? std::string() : std::string(ndtgpu_last_error());
    ndtgpu_calib_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "calibration: " + err);
    return res;
}

}   // namespace calib_detail

// errorFunction (:146-152): the candidate Ts alone -- a lattice of one node whose cosine and sine are Ts's own
inline double errorFunction(const std::vector<ScanPairGPU> &pairs, const Eigen::Affine3d &Ts, const ndtgpu_calib_params *params = nullptr)
{
    return calib_detail::search(pairs, {Ts(0, 3)}, {Ts(1, 3)}, {Ts(0, 0)}, {Ts(1, 0)}, params, nullptr).score;
}

inline double ScanPairGPU::scoreICP(const Eigen::Affine3d &Ts, const ndtgpu_calib_params *params) const
{
    return errorFunction(std::vector<ScanPairGPU>(1, *this), Ts, params);
}

// bruteForceOptimization (:176-204): ix, iy, iyaw the initial guess, x_s, y_s, yaw_s the search region around it, t_r and yaw_r the
// increments.  `params` and `want_volume` are additions.
inline CalibrationResultGPU bruteForceOptimization(const std::vector<ScanPairGPU> &pairs, double ix, double iy, double iyaw, double x_s,
                                                   double y_s, double yaw_s, double t_r, double yaw_r,
                                                   const ndtgpu_calib_params *params = nullptr, bool want_volume = false)
{
    size_t cnt[3];
    ndtgpu_host::check(ndtgpu_calib_lattice(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r, cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0),
                       "ndtgpu_calib_lattice");
    const size_t room = std::max(cnt[0], std::max(cnt[1], cnt[2]));
    std::vector<double> xs(room), ys(room), yaws(room), cs(room), sn(room);
    ndtgpu_host::check(ndtgpu_calib_lattice(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r, cnt, xs.data(), ys.data(), yaws.data(), cs.data(),
                                            sn.data(), room), "ndtgpu_calib_lattice");
    xs.resize(cnt[0]); ys.resize(cnt[1]); yaws.resize(cnt[2]); cs.resize(cnt[2]); sn.resize(cnt[2]);
    CalibrationResultGPU out;
    const ndtgpu_calib_result res = calib_detail::search(pairs, xs, ys, cs, sn, params, want_volume ? &out.volume : nullptr);
    out.n_candidates = cnt[0] * cnt[1] * cnt[2];
    out.index = res.index;
    out.x = xs[res.index / (cnt[1] * cnt[2])];
    out.y = ys[(res.index / cnt[2]) % cnt[1]];
    out.yaw = yaws[res.index % cnt[2]];
    out.T = calibGetAsAffine(out.x, out.y, out.yaw);
    out.score = res.score;
    out.found = !(res.flags & NDTGPU_CALIB_NO_RESULT);
    out.n_skipped = res.n_skipped;
    return out;
}

// The callback (:250-353) from the cloud on: the first scan becomes the anchor; a scan more than max_translation from the anchor
// replaces it without a pair; a scan that has turned by less than min_yaw is dropped; any other scan forms the pair (anchor, scan)
// and becomes the anchor.  The rule itself is the library's (ndtgpu_calib_select_pairs).
class CalibrationPairCollector {
public:
    explicit CalibrationPairCollector(double max_translation = 1.0, double min_yaw = 25.0 * M_PI / 180.0)
        : max_translation_(max_translation), min_yaw_(min_yaw) {}
    // true where the scan completed a pair
    bool add(const pcl::PointCloud<pcl::PointXYZ> &cloud, const Eigen::Affine3d &Tgt)
    {
        if (first_) {
            first_ = false;
            Told_ = Tgt;
            cloud_old_ = cloud;
            return false;
        }
        const double poses[8] = {Told_(0, 3), Told_(1, 3), Told_(0, 0), Told_(1, 0), Tgt(0, 3), Tgt(1, 3), Tgt(0, 0), Tgt(1, 0)};
        uint32_t pr[2];
        size_t n = 0, turned = 0;
        ndtgpu_host::check(ndtgpu_calib_select_pairs(poses, 2, max_translation_, min_yaw_, pr, 1, &n), "ndtgpu_calib_select_pairs");
        if (n == 0) {
            // too far (the anchor is replaced) or not turned enough (keep waiting): without the yaw gate only the first remains
            ndtgpu_host::check(ndtgpu_calib_select_pairs(poses, 2, max_translation_, 0.0, pr, 1, &turned), "ndtgpu_calib_select_pairs");
            if (turned == 0) { Told_ = Tgt; cloud_old_ = cloud; }
            return false;
        }
        pairs.push_back(ScanPairGPU(cloud_old_, Told_, cloud, Tgt));
        Told_ = Tgt;
        cloud_old_ = cloud;
        return true;
    }
    std::vector<ScanPairGPU> pairs;

private:
    double max_translation_, min_yaw_;
    bool first_ = true;
    Eigen::Affine3d Told_;
    pcl::PointCloud<pcl::PointXYZ> cloud_old_;
};

}   // namespace ndt_feature
