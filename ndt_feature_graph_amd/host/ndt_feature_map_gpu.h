// ndt_feature_map_gpu.h -- host C++ mirror of the feature map and its matcher (ndt_feature/include/ndt_feature/ndt_feature_map.h)
// over the ndtgpu_featbank_* calls of libndtgpu.so (include/ndtgpu.h, "feature-set RANSAC matching": the algorithm, its provenance
// and what deviates from flirtlib's RansacFeatureSetMatcher are stated there).
//   ndt_feature::InterestPointGPU                 flirtlib's InterestPoint as the matcher sees it: a pose and a descriptor
//   ndt_feature::NDTFeatureMapGPU                 NDTFeatureMap: update (ndt_feature_map.h:62-68), getMap
//   ndt_feature::matchFeatureMap                  ndt_feature_map.h:104-122 (called through ndt_feature_node.h:256 by computeLink,
//                                                 ndt_feature_graph.cpp:162-177, and by the fuser, ndt_feature_fuser_hmt.cpp:251)
//   ndt_feature::computeAllPossibleFeatureLinks   the feature step of computeAllPossibleLinks (ndt_feature_graph.cpp:395-405): every
//                                                 pair i < j, all of them in ONE device call
//   ndt_feature::LaserScanGPU                     the reading flirtlib_ros::fromRos builds (conversions.cpp:69-82): angle_min,
//                                                 angle_increment and the ranges, the sensor at the origin
//   ndt_feature::detectAndDescribe                the detect + describe loop of the fuser (ndt_feature2d_fuser.cpp:772-776) for a
//                                                 batch of scans in ONE device call (include/ndtgpu.h, "laser-scan feature
//                                                 extraction": the detector and descriptor are restated there, with what
//                                                 deviates from flirtlib's CurvatureDetector and BetaGridGenerator)
//   ndt_feature::projectLaserGPU                  projector_.projectLaser, the range gate and the z jitter of every consumer of a
//                                                 scan (ndt_feature2d_fuser.cpp:747-765) for a batch of scans in ONE device call:
//                                                 the pcl_cloud of every scan (include/ndtgpu.h, "laser-scan projection")
// A caller may also fill InterestPointGPU from flirtlib's own points (position, BetaGrid histogram flattened row by row:
// flirtlib_utils.h:32-42 gives bin_rho 4 x bin_phi 12).
// WIRED: host/ndt_feature_graph_gpu.h takes InterestPointGPUVec in NDTFeatureFuserHMT / NDTFeatureGraph initialize and update (the
// fuser bank's feature path: the feature term of the registration and the node feature maps, on the device), reads a node's
// feature map back as an NDTFeatureMapGPU (getFeatureMap) and matches two nodes' maps where they are
// (matchNodesUsingFeatureMap).  Its InterestPointVec overloads remain an empty placeholder without features.
// NOT WIRED: NDTFeatureGraph::computeLink still seeds link.T from the node poses; a caller that wants the RANSAC seed calls
// matchNodesUsingFeatureMap (or computeAllPossibleFeatureLinks on maps it read back) itself.
// There is no CPU fallback: a failed C-ABI call throws ndtgpu_host::Error.
#pragma once
#include "lslgeneric_gpu.h"

#include <limits>
#include <utility>

namespace ndt_feature {

struct InterestPointGPU {
    double x = 0., y = 0., theta = 0.;        // OrientedPoint2D
    std::vector<double> descriptor;           // the histogram, flattened
};
using InterestPointGPUVec = std::vector<InterestPointGPU>;
// flirtlib's Correspondences are pairs of InterestPoint pointers; here pairs of indices (mov, ref) into the two maps
using CorrespondencesGPU = std::vector<std::pair<size_t, size_t>>;

class NDTFeatureMapGPU {
public:
    // appends the points of every 4th call, the first included (ndt_feature_map.h:62-68)
    void update(const InterestPointGPUVec &pts)
    {
        if (counter_ % 4 == 0) map.insert(map.end(), pts.begin(), pts.end());
        counter_++;
    }
    InterestPointGPUVec &getMap() { return map; }
    const InterestPointGPUVec &getMap() const { return map; }
    InterestPointGPUVec map;

private:
    int counter_ = 0;
};

// sensor_msgs/LaserScan as flirtlib_ros::fromRos reads it (conversions.cpp:69-82): beam i looks along
// angle_min + i * angle_increment
struct LaserScanGPU {
    double angle_min = 0., angle_increment = 0.;
    std::vector<double> ranges;
};

struct NDTFeatureMatchLink {
    size_t ref_idx = 0, mov_idx = 0;
    Eigen::Affine3d T;                        // maps mov into ref: computeLink's link.T
    double score = std::numeric_limits<double>::max();
    CorrespondencesGPU matches;
    ndtgpu_featmatch_result report;           // (an addition: the matcher's record of the pair)
};

namespace detail {

// a bank with one set per map, filled
struct FeatBank {
    ndtgpu_featbank *h = nullptr;
    size_t max_points = 1;
    FeatBank(const std::vector<const NDTFeatureMapGPU *> &maps)
    {
        size_t desc_len = 0;
        for (const NDTFeatureMapGPU *m : maps) {
            max_points = std::max(max_points, m->map.size());
            for (const InterestPointGPU &p : m->map) {
                if (desc_len == 0) desc_len = p.descriptor.size();
                if (p.descriptor.size() != desc_len || desc_len == 0)
                    throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "matchFeatureMap: every descriptor must have the same, non-zero length");
            }
        }
        if (desc_len == 0) desc_len = 1;      // (every map is empty)
        ndtgpu_host::check(ndtgpu_featbank_create(maps.size(), max_points, desc_len, &h), "ndtgpu_featbank_create");
        std::vector<double> pos, desc;
        for (size_t k = 0; k < maps.size(); k++) {
            const InterestPointGPUVec &v = maps[k]->map;
            pos.clear();
            desc.clear();
            for (const InterestPointGPU &p : v) {
                pos.push_back(p.x);
                pos.push_back(p.y);
                pos.push_back(p.theta);
                desc.insert(desc.end(), p.descriptor.begin(), p.descriptor.end());
            }
            const ndtgpu_status rc = ndtgpu_featbank_set(h, k, v.size(), pos.data(), desc.data());
            if (rc != NDTGPU_OK) {
                const std::string err = ndtgpu_last_error();
                ndtgpu_featbank_destroy(h);
                throw ndtgpu_host::Error(rc, "ndtgpu_featbank_set: " + err);
            }
        }
    }
    ~FeatBank() { ndtgpu_featbank_destroy(h); }
    FeatBank(const FeatBank &) = delete;
    FeatBank &operator=(const FeatBank &) = delete;

    std::vector<NDTFeatureMatchLink> match(const std::vector<uint32_t> &ref, const std::vector<uint32_t> &mov,
                                           const ndtgpu_featmatch_params *params) const
    {
        const size_t n = ref.size();
        std::vector<NDTFeatureMatchLink> links(n);
        if (n == 0) return links;
        ndtgpu_host::check(ndtgpu_featbank_match(h, ref.data(), mov.data(), n, params, nullptr), "ndtgpu_featbank_match");
        std::vector<ndtgpu_featmatch_result> res(n);
        std::vector<double> T16(16 * n);
        std::vector<uint32_t> corr(n * max_points * 2);
        ndtgpu_host::check(ndtgpu_featbank_results(h, 0, n, res.data(), T16.data(), corr.data()), "ndtgpu_featbank_results");
        for (size_t p = 0; p < n; p++) {
            NDTFeatureMatchLink &l = links[p];
            l.ref_idx = ref[p];
            l.mov_idx = mov[p];
            l.report = res[p];
            for (int e = 0; e < 16; e++) l.T.data()[e] = T16[16 * p + e];
            // upstream: max() for an empty map and for the NaN transform of a run without a hypothesis; a run with too few
            // candidates returns matchSets' 1e17 with the transform untouched
            l.score = res[p].status == NDTGPU_FEATMATCH_NO_HYPOTHESIS || res[p].status == NDTGPU_FEATMATCH_BAD_INDEX
                          ? std::numeric_limits<double>::max() : res[p].score;
            for (int k = 0; k < res[p].n_inliers; k++)
                l.matches.emplace_back(corr[(p * max_points + k) * 2], corr[(p * max_points + k) * 2 + 1]);
        }
        return links;
    }
};

}  // namespace detail

// ndt_feature_map.h:104-122.  `matches` and T are written as upstream writes them: not at all where max() is returned for an
// empty map.  `params` is an addition (NULL: upstream's constructor arguments).
inline double matchFeatureMap(const NDTFeatureMapGPU &ref, const NDTFeatureMapGPU &mov, CorrespondencesGPU &matches, Eigen::Affine3d &T,
                              const ndtgpu_featmatch_params *params = nullptr)
{
    if (ref.map.empty() || mov.map.empty()) return std::numeric_limits<double>::max();
    const detail::FeatBank bank({&ref, &mov});
    const NDTFeatureMatchLink l = bank.match({0}, {1}, params)[0];
    matches = l.matches;
    if (l.report.status == NDTGPU_FEATMATCH_NO_HYPOTHESIS) return std::numeric_limits<double>::max();
    T = l.T;
    return l.score;
}

// ndt_feature2d_fuser.cpp:772-776 (detector_->detect(*reading, pts), then descriptor_->describe(*p, *reading) for every point) for
// a batch of scans in one device call: the interest points of scan b, in ascending beam order, with their BetaGrid descriptors.
// Every scan must have the first scan's angle_min, angle_increment and number of beams (one call reads one kind of laser).
// `params` is an addition (NULL: flirtlib_utils.h:15-42); `max_points` is the most a scan may give (more: the first max_points in
// beam order), `records` the device's record of every scan.
inline std::vector<InterestPointGPUVec> detectAndDescribe(const std::vector<LaserScanGPU> &scans,
                                                          const ndtgpu_featextract_params *params = nullptr, size_t max_points = 256,
                                                          std::vector<ndtgpu_featextract_result> *records = nullptr)
{
    std::vector<InterestPointGPUVec> out(scans.size());
    if (scans.empty()) return out;
    ndtgpu_featextract_params prm;
    ndtgpu_default_featextract_params(&prm);
    if (params) prm = *params;
    const size_t n = scans.size(), n_beams = scans[0].ranges.size(), desc_len = (size_t)prm.bin_rho * (size_t)prm.bin_phi;
    std::vector<double> ranges;
    std::vector<uint32_t> idx(n);
    for (size_t b = 0; b < n; b++) {
        if (scans[b].ranges.size() != n_beams || scans[b].angle_min != scans[0].angle_min || scans[b].angle_increment != scans[0].angle_increment)
            throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "detectAndDescribe: every scan must have the same angles and number of beams");
        ranges.insert(ranges.end(), scans[b].ranges.begin(), scans[b].ranges.end());
        idx[b] = (uint32_t)b;
    }
    ndtgpu_featbank *h = nullptr;
    ndtgpu_host::check(ndtgpu_featbank_create(n, max_points, desc_len ? desc_len : 1, &h), "ndtgpu_featbank_create");
    std::vector<ndtgpu_featextract_result> res(n);
    std::vector<double> pos(max_points * 3), desc(max_points * (desc_len ? desc_len : 1));
    ndtgpu_status rc = ndtgpu_featbank_extract(h, idx.data(), ranges.data(), n, n_beams, scans[0].angle_min, scans[0].angle_increment, &prm,
                                               nullptr);
    if (rc == NDTGPU_OK) rc = ndtgpu_featbank_extract_results(h, 0, n, res.data(), nullptr, nullptr, nullptr);
    for (size_t b = 0; b < n && rc == NDTGPU_OK; b++) {
        size_t m = 0;
        rc = ndtgpu_featbank_get(h, b, &m, pos.data(), desc.data());
        if (rc != NDTGPU_OK) break;
        out[b].resize(m);
        for (size_t i = 0; i < m; i++) {
            InterestPointGPU &p = out[b][i];
            p.x = pos[3 * i];
            p.y = pos[3 * i + 1];
            p.theta = pos[3 * i + 2];
            p.descriptor.assign(desc.begin() + i * desc_len, desc.begin() + (i + 1) * desc_len);
        }
    }
    const std::string err = rc == NDTGPU_OK ? std::string() : std::string(ndtgpu_last_error());
    ndtgpu_featbank_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "detectAndDescribe: " + err);
    if (records) *records = res;
    return out;
}

// projector_.projectLaser(*msg_in, cloud), the range gate and the z jitter (ndt_feature2d_fuser.cpp:747-765, publish_graph_message.cpp:
// 1356-1381 and the other call sites include/ndtgpu.h "laser-scan projection" lists) for a batch of scans in one device call: scan
// b's pcl_cloud, the kept points in beam order, cut to its n_kept points.  Every scan must have the first scan's angle_min,
// angle_increment and number of beams.  `params` is an addition (NULL: gustav_laser_tf.launch:20-23); `scan_ids` names the z
// draws of every scan (empty: scan b has id b).
inline std::vector<pcl::PointCloud<pcl::PointXYZ>> projectLaserGPU(const std::vector<LaserScanGPU> &scans,
                                                                   const ndtgpu_scanproject_params *params = nullptr,
                                                                   const std::vector<uint64_t> &scan_ids = {})
{
    std::vector<pcl::PointCloud<pcl::PointXYZ>> out(scans.size());
    if (scans.empty()) return out;
    const size_t n = scans.size(), n_beams = scans[0].ranges.size();
    if (!scan_ids.empty() && scan_ids.size() != n) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "projectLaserGPU: one scan id per scan");
    std::vector<double> ranges;
    for (size_t b = 0; b < n; b++) {
        if (scans[b].ranges.size() != n_beams || scans[b].angle_min != scans[0].angle_min || scans[b].angle_increment != scans[0].angle_increment)
            throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "projectLaserGPU: every scan must have the same angles and number of beams");
        ranges.insert(ranges.end(), scans[b].ranges.begin(), scans[b].ranges.end());
    }
    // (the checks first: a scan without beams is refused with the library's message, not by the handle's capacity)
    ndtgpu_host::check(ndtgpu_scanproj_check(n, n_beams, scans[0].angle_min, scans[0].angle_increment, sizeof(pcl::PointXYZ),
                                             n_beams * sizeof(pcl::PointXYZ), params), "ndtgpu_scanproj_check");
    ndtgpu_scanproj *h = nullptr;
    ndtgpu_host::check(ndtgpu_scanproj_create(n, n_beams, &h), "ndtgpu_scanproj_create");
    std::vector<pcl::PointXYZ> rows(n * n_beams);
    std::vector<uint32_t> n_kept(n);
    const ndtgpu_status rc = ndtgpu_scanproj_project(h, ranges.data(), scan_ids.empty() ? nullptr : scan_ids.data(), n, n_beams,
                                                     scans[0].angle_min, scans[0].angle_increment, params, rows.data(), sizeof(pcl::PointXYZ),
                                                     n_beams * sizeof(pcl::PointXYZ), n_kept.data());
    const std::string err = rc == NDTGPU_OK ? std::string() : std::string(ndtgpu_last_error());
    ndtgpu_scanproj_destroy(h);
    if (rc != NDTGPU_OK) throw ndtgpu_host::Error(rc, "projectLaserGPU: " + err);
    for (size_t b = 0; b < n; b++)
        for (size_t k = 0; k < n_kept[b]; k++) out[b].push_back(rows[b * n_beams + k]);
    return out;
}

// every pair i < j of `maps` (ref = i, mov = j, in computeAllPossibleLinks' order) in one device call; a pair with an empty map
// comes back with score max(), the identity and no matches
inline std::vector<NDTFeatureMatchLink> computeAllPossibleFeatureLinks(const std::vector<NDTFeatureMapGPU> &maps,
                                                                       const ndtgpu_featmatch_params *params = nullptr)
{
    std::vector<const NDTFeatureMapGPU *> ptrs;
    for (const NDTFeatureMapGPU &m : maps) ptrs.push_back(&m);
    std::vector<uint32_t> ref, mov;
    for (size_t i = 0; i < maps.size(); i++)
        for (size_t j = i + 1; j < maps.size(); j++) {
            ref.push_back((uint32_t)i);
            mov.push_back((uint32_t)j);
        }
    if (ref.empty()) return {};
    const detail::FeatBank bank(ptrs);
    std::vector<NDTFeatureMatchLink> links = bank.match(ref, mov, params);
    for (NDTFeatureMatchLink &l : links)
        if (maps[l.ref_idx].map.empty() || maps[l.mov_idx].map.empty()) l.score = std::numeric_limits<double>::max();
    return links;
}

}  // namespace ndt_feature
