// ndt_occupancy_grid_gpu.h -- host C++ mirror of the occupancy-grid export the reference's mapper publishes on a timer:
//   lslgeneric::toOccupancyGrid(map, omap, occ_map_resolution_, frame)   ndt_feature/src/ndt_feature2d_fuser.cpp:428-433, 450-454
//   moveOccupancyMap(omap, graph->getT())                                 ndt_feature/include/ndt_feature/ros_utils.h:12-18
// over the C-ABI (include/ndtgpu.h "occupancy-grid export": ndtgpu_mapset_occupancy_grid, ndtgpu_occgrid_move).  The two
// functions have the reference's names, namespaces and argument lists; OccupancyGridGPU stands where nav_msgs::OccupancyGrid
// stands there and has that message's members.  The functions are templates over the message type: in a catkin build the call
// sites pass nav_msgs::OccupancyGrid itself.
// Everything that computes lives on the GPU; there is no CPU fallback: a failed C-ABI call throws ndtgpu_host::Error.
#pragma once
#include "lslgeneric_gpu.h"

#include <cstdint>
#include <string>
#include <vector>

// nav_msgs::OccupancyGrid, member for member, as far as the two functions touch it
struct OccupancyGridGPU {
    struct Header {
        std::string frame_id;
    } header;
    struct MapMetaData {
        float resolution = 0.f;                  // [m / pixel] (float32 in the message)
        uint32_t width = 0, height = 0;          // [pixels]
        struct Pose {
            struct Point { double x = 0, y = 0, z = 0; } position;
            struct Quaternion { double x = 0, y = 0, z = 0, w = 1; } orientation;
        } origin;                                // pose of pixel (0, 0)'s lower corner
    } info;
    std::vector<int8_t> data;                    // row-major from (0, 0): -1 unknown, 0 free, 55..100 occupied
};

namespace ndtgpu_host {

// tf::poseMsgToEigen / tf::poseEigenToMsg on the message's Pose
template <class Pose>
inline Eigen::Affine3d pose_msg_to_affine(const Pose &p)
{
    const double x = p.orientation.x, y = p.orientation.y, z = p.orientation.z, w = p.orientation.w;
    Eigen::Affine3d T = Eigen::Affine3d::Identity();
    double *m = T.data();                        // column-major
    m[0] = 1 - 2 * (y * y + z * z); m[4] = 2 * (x * y - z * w);     m[8] = 2 * (x * z + y * w);
    m[1] = 2 * (x * y + z * w);     m[5] = 1 - 2 * (x * x + z * z); m[9] = 2 * (y * z - x * w);
    m[2] = 2 * (x * z - y * w);     m[6] = 2 * (y * z + x * w);     m[10] = 1 - 2 * (x * x + y * y);
    m[12] = p.position.x; m[13] = p.position.y; m[14] = p.position.z;
    return T;
}
template <class Pose>
inline void affine_to_pose_msg(const Eigen::Affine3d &T, Pose &p)
{
    const double *m = T.data();
    const double r00 = m[0], r01 = m[4], r02 = m[8], r10 = m[1], r11 = m[5], r12 = m[9], r20 = m[2], r21 = m[6], r22 = m[10];
    const double tr = r00 + r11 + r22;
    double x, y, z, w;
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        w = 0.25 * s; x = (r21 - r12) / s; y = (r02 - r20) / s; z = (r10 - r01) / s;
    } else if (r00 > r11 && r00 > r22) {
        const double s = std::sqrt(1.0 + r00 - r11 - r22) * 2;
        w = (r21 - r12) / s; x = 0.25 * s; y = (r01 + r10) / s; z = (r02 + r20) / s;
    } else if (r11 > r22) {
        const double s = std::sqrt(1.0 + r11 - r00 - r22) * 2;
        w = (r02 - r20) / s; x = (r01 + r10) / s; y = 0.25 * s; z = (r12 + r21) / s;
    } else {
        const double s = std::sqrt(1.0 + r22 - r00 - r11) * 2;
        w = (r10 - r01) / s; x = (r02 + r20) / s; y = (r12 + r21) / s; z = 0.25 * s;
    }
    p.orientation.x = x; p.orientation.y = y; p.orientation.z = z; p.orientation.w = w;
    p.position.x = m[12]; p.position.y = m[13]; p.position.z = m[14];
}

}  // namespace ndtgpu_host

namespace lslgeneric {

// toOccupancyGrid(ndt_map, occ_grid, resolution, frame_id) (perception_oru ndt_map/ndt_conversions.h; called at
// ndt_feature2d_fuser.cpp:430, 452): ONE device call rasterises the map; params NULL: the defaults (z 0, a cell that is
// occupied without a Gaussian counts 100).  `counts`, when given, receives the grid's geometry and its unknown / free / occupied
// pixel counts.
template <class OccupancyGrid>
inline bool toOccupancyGrid(NDTMap *ndt_map, OccupancyGrid &occ_grid, double resolution, std::string frame_id,
                            const ndtgpu_occgrid_params *params = nullptr, ndtgpu_occgrid_info *counts = nullptr)
{
    if (!ndt_map) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "toOccupancyGrid: null map");
    int32_t cpa[3], width = 0, height = 0;
    double centre[3], origin[3];
    ndtgpu_host::check(ndtgpu_mapset_info(ndt_map->handle(), nullptr, cpa, nullptr), "mapset_info");
    ndt_map->getCentroid(centre[0], centre[1], centre[2]);
    ndtgpu_host::check(ndtgpu_occgrid_dims(ndt_map->resolution(), cpa, centre, resolution, &width, &height, origin), "ndtgpu_occgrid_dims");
    ndtgpu_host::check(ndtgpu_occgrid_check(ndt_map->slot() + 1, ndt_map->slot(), 1, width, height), "ndtgpu_occgrid_check");
    occ_grid.data.assign((size_t)width * (size_t)height, (int8_t)-1);
    ndtgpu_occgrid_info info;
    ndtgpu_host::check(ndtgpu_mapset_occupancy_grid(ndt_map->handle(), ndt_map->slot(), 1, resolution, params, occ_grid.data.data(), &info, nullptr),
                       "ndtgpu_mapset_occupancy_grid");
    occ_grid.info.resolution = (float)resolution;
    occ_grid.info.width = (uint32_t)info.width;
    occ_grid.info.height = (uint32_t)info.height;
    occ_grid.info.origin.position.x = info.origin[0];
    occ_grid.info.origin.position.y = info.origin[1];
    occ_grid.info.origin.position.z = info.origin[2];
    occ_grid.info.origin.orientation.x = occ_grid.info.origin.orientation.y = occ_grid.info.origin.orientation.z = 0.0;
    occ_grid.info.origin.orientation.w = 1.0;
    occ_grid.header.frame_id = frame_id;
    if (counts) *counts = info;
    return true;
}

}  // namespace lslgeneric

// moveOccupancyMap(occ_grid, pose) (ros_utils.h:12-18): origin <- pose * origin.  The data is not resampled, as in the reference.
template <class OccupancyGrid>
inline void moveOccupancyMap(OccupancyGrid &occ_grid, const Eigen::Affine3d &pose)
{
    const Eigen::Affine3d map_origin = ndtgpu_host::pose_msg_to_affine(occ_grid.info.origin);
    Eigen::Affine3d new_map_origin = Eigen::Affine3d::Identity();
    ndtgpu_occgrid_move(pose.data(), map_origin.data(), new_map_origin.data());
    ndtgpu_host::affine_to_pose_msg(new_map_origin, occ_grid.info.origin);
}
