// ndt_scan_simulator_gpu.h -- host C++ mirror of the scan simulation flirtlib_ros takes from occupancy_grid_utils, over the
// ndtgpu_scansim_* calls of libndtgpu.so (include/ndtgpu.h, "scan simulation": the ray, the stop rule, the lattice and what deviates
// from upstream are stated there).
//   flirtlib_ros::simulateRangeScanGPU(grid, pose, scanner_info, unknown_cells_are_obstacles)
//                                             gu::simulateRangeScan as place_rec_test.cpp:242 and simulate_scans.cpp:131 call it
//   flirtlib_ros::generateRefScansGPU(...)    the three loops of generateRefScans (place_rec_test.cpp:218-237) and the simulated scan
//                                             of every kept pose (:242) -- ONE device call for the lattice and one for all scans
//   flirtlib_ros::ScanSimulatorGPU            the object behind both: a grid installed once, many poses
// OccupancyGridGPU (ndt_occupancy_grid_gpu.h) stands where nav_msgs::OccupancyGrid stands, ScannerInfoGPU where the sensor_msgs::
// LaserScan of getScannerParams stands, ndt_feature::LaserScanGPU where the returned scan stands.  The features of :245-254 are the
// feature bank's (ndt_feature_map_gpu.h); a caller that holds device buffers keeps lattice -> simulate -> extract -> match -> pick on
// the device with the C-ABI.
// There is no CPU fallback: a failed C-ABI call throws ndtgpu_host::Error.
#pragma once
#include "ndt_localization_monitor_gpu.h"

#include <cmath>
#include <vector>

namespace flirtlib_ros {

// the fields of the scanner's sensor_msgs::LaserScan that the simulation reads
struct ScannerInfoGPU {
    double angle_min = -M_PI / 2, angle_max = M_PI / 2, angle_increment = M_PI / 180;
    double range_max = 10.0;
    // beams at angle_min + i * angle_increment up to angle_max (half an increment of slack for the rounding of the sum)
    size_t beams() const { return angle_increment > 0 ? (size_t)std::floor((angle_max - angle_min) / angle_increment + 0.5) + 1 : 1; }
};

struct SimulatedRefScanGPU {
    LaserScanGPU scan;
    PoseGPU pose;
    uint32_t lattice_index = 0;               // (an addition: ((x / skip) * ny + y / skip) * n_headings + heading)
    ndtgpu_scansim_result report{};           // (an addition: hits and flags)
};

class ScanSimulatorGPU {
public:
    ScanSimulatorGPU(const OccupancyGridGPU &g, const ScannerInfoGPU &info, bool unknown_cells_are_obstacles = true, int occupied_min = 55,
                     size_t max_poses = (size_t)1 << 16)
        : info_(info), res_(g.info.resolution), w_(g.info.width), hgt_(g.info.height), max_poses_(max_poses)
    {
        ndtgpu_default_scansim_params(&prm_);
        prm_.range_max = info.range_max;
        prm_.miss = info.range_max + 1.0;         // upstream's out-of-range value
        prm_.occupied_min = occupied_min;
        prm_.unknown_is_obstacle = unknown_cells_are_obstacles ? 1 : 0;
        nb_ = info.beams();
        if (g.data.size() != w_ * hgt_) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "ScanSimulatorGPU: data is not width x height");
        ndtgpu_host::check(ndtgpu_scansim_check(1, w_, hgt_, res_, nb_, info.angle_min, info.angle_increment, 1, &prm_), "ndtgpu_scansim_check");
        ndtgpu_host::check(ndtgpu_scansim_create(1, nb_, max_poses, &h_), "ndtgpu_scansim_create");
        const double origin[2] = {g.info.origin.position.x, g.info.origin.position.y};
        ndtgpu_status rc = ndtgpu_scansim_set_grids(h_, g.data.data(), 1, w_, hgt_, res_, origin);
        if (rc == NDTGPU_OK) rc = ndtgpu_scansim_set_beams(h_, nb_, info.angle_min, info.angle_increment, nullptr);
        if (rc != NDTGPU_OK) {
            const std::string err = ndtgpu_last_error();
            ndtgpu_scansim_destroy(h_);
            throw ndtgpu_host::Error(rc, "ScanSimulatorGPU: " + err);
        }
    }
    ~ScanSimulatorGPU() { ndtgpu_scansim_destroy(h_); }
    ScanSimulatorGPU(const ScanSimulatorGPU &) = delete;
    ScanSimulatorGPU &operator=(const ScanSimulatorGPU &) = delete;

    size_t beams() const { return nb_; }

    // the scans of many poses in one call; reports (may be NULL): hits and flags per pose
    std::vector<LaserScanGPU> simulate(const std::vector<PoseGPU> &poses, std::vector<ndtgpu_scansim_result> *reports = nullptr)
    {
        std::vector<double> p4(4 * poses.size());
        for (size_t k = 0; k < poses.size(); k++) locmonPose4(poses[k], &p4[4 * k]);
        return simulate4(p4, reports);
    }

    // gu::simulateRangeScan(grid, pose, scanner_info, unknown_cells_are_obstacles)
    LaserScanGPU simulate(const PoseGPU &pose, ndtgpu_scansim_result *report = nullptr)
    {
        std::vector<ndtgpu_scansim_result> rep;
        LaserScanGPU out = simulate(std::vector<PoseGPU>(1, pose), &rep)[0];
        if (report) *report = rep[0];
        return out;
    }

    // generateRefScans' poses and their scans: skip = (unsigned)(ref_pos_resolution / resolution), headings from 0 by
    // ref_angle_resolution while below 6.28, free cells whose centre lies in [x0, x1] x [y0, y1]
    std::vector<SimulatedRefScanGPU> generateRefScans(double ref_pos_resolution, double ref_angle_resolution, double x0 = -1e9, double x1 = 1e9,
                                             double y0 = -1e9, double y1 = 1e9)
    {
        uint32_t skip = 0;
        ndtgpu_host::check(ndtgpu_scansim_skip(ref_pos_resolution, res_, &skip), "ndtgpu_scansim_skip");
        size_t nyaw = 0;
        ndtgpu_host::check(ndtgpu_scansim_headings(ref_angle_resolution, &nyaw, nullptr, nullptr, 0), "ndtgpu_scansim_headings");
        std::vector<double> cs(nyaw), sn(nyaw);
        ndtgpu_host::check(ndtgpu_scansim_headings(ref_angle_resolution, &nyaw, cs.data(), sn.data(), nyaw), "ndtgpu_scansim_headings");
        const size_t nodes = ((w_ + skip - 1) / skip) * ((hgt_ + skip - 1) / skip) * nyaw, cap = nodes < max_poses_ ? nodes : max_poses_;
        const double box[4] = {x0, y0, x1, y1};
        std::vector<double> p4(4 * cap);
        std::vector<uint32_t> index(cap);
        uint32_t counts[2] = {0, 0};
        ndtgpu_host::check(ndtgpu_scansim_lattice(h_, 0, skip, cs.data(), sn.data(), nyaw, box, cap, p4.data(), index.data(), counts),
                           "ndtgpu_scansim_lattice");
        if (counts[1] > counts[0]) throw ndtgpu_host::Error(NDTGPU_ERR_CAPACITY, "generateRefScansGPU: more reference poses than max_poses");
        p4.resize(4 * (size_t)counts[0]);
        std::vector<SimulatedRefScanGPU> out(counts[0]);
        if (out.empty()) return out;
        std::vector<ndtgpu_scansim_result> rep;
        std::vector<LaserScanGPU> scans = simulate4(p4, &rep);
        for (size_t k = 0; k < out.size(); k++) {
            out[k].scan = std::move(scans[k]);
            out[k].pose = locmonMakePose(p4[4 * k], p4[4 * k + 1], p4[4 * k + 2], p4[4 * k + 3]);
            out[k].lattice_index = index[k];
            out[k].report = rep[k];
        }
        return out;
    }

private:
    std::vector<LaserScanGPU> simulate4(const std::vector<double> &p4, std::vector<ndtgpu_scansim_result> *reports)
    {
        const size_t n = p4.size() / 4;
        std::vector<LaserScanGPU> out(n);
        if (n == 0) return out;
        std::vector<double> ranges(n * nb_);
        std::vector<ndtgpu_scansim_result> rep(n);
        ndtgpu_host::check(ndtgpu_scansim_simulate(h_, p4.data(), nullptr, n, &prm_, ranges.data(), rep.data()), "ndtgpu_scansim_simulate");
        for (size_t k = 0; k < n; k++) {
            out[k].angle_min = info_.angle_min;
            out[k].angle_increment = info_.angle_increment;
            out[k].ranges.assign(ranges.begin() + k * nb_, ranges.begin() + (k + 1) * nb_);
        }
        if (reports) *reports = rep;
        return out;
    }

    ndtgpu_scansim *h_ = nullptr;
    ndtgpu_scansim_params prm_;
    ScannerInfoGPU info_;
    double res_;
    size_t w_, hgt_, nb_ = 0, max_poses_;
};

// gu::simulateRangeScan's call shape: one grid, one pose (a caller with many poses keeps a ScanSimulatorGPU)
inline LaserScanGPU simulateRangeScanGPU(const OccupancyGridGPU &grid, const PoseGPU &pose, const ScannerInfoGPU &scanner_info,
                                         bool unknown_cells_are_obstacles = true)
{
    ScanSimulatorGPU sim(grid, scanner_info, unknown_cells_are_obstacles, 55, 1);
    return sim.simulate(pose);
}

// generateRefScans' call shape, the parameters it reads from the server as arguments
inline std::vector<SimulatedRefScanGPU> generateRefScansGPU(const OccupancyGridGPU &grid, const ScannerInfoGPU &scanner_info, double ref_pos_resolution,
                                                   double ref_angle_resolution, double x0 = -1e9, double x1 = 1e9, double y0 = -1e9,
                                                   double y1 = 1e9, size_t max_poses = (size_t)1 << 20)
{
    ScanSimulatorGPU sim(grid, scanner_info, true, 55, max_poses);
    return sim.generateRefScans(ref_pos_resolution, ref_angle_resolution, x0, x1, y0, y1);
}

}   // namespace flirtlib_ros
