// ndt_rviz_gpu.h -- host C++ mirror of the marker functions of ndt_feature/include/ndt_feature/ndt_rviz.h (assignDefault, assignColor,
// markerNDTCells, markerNDTCells2, markerParticlesNDTMCL3D: :1032-1088, 1163-1233, 1277-1297) and of ndt_feature_rviz.h:282-313
// (markerNDTFeatureLinks), over the marker export of libndtgpu.so (include/ndtgpu.h "marker export": the semantics and the deviations
// are stated there).  Each function is ONE device call: the cells stay on the device, the eigen-pairs are computed there, and only the
// marker's points come back.  With this header the publish timers of ndt_feature2d_fuser.cpp:425-433, 448-454,
// ndt_feature_fuser.cpp:253 and ndt_feature_mcl_node.cpp:274, 287 compile against the project.
//
// MarkerGPU stands in for visualization_msgs::Marker (this build has no ROS): the fields the functions set, with the points as
// geometry_msgs/Point (three doubles).  Without a HIP device the functions throw ndtgpu_host::Error (NDTGPU_ERR_NO_DEVICE): there is no
// CPU fallback.
#pragma once
#include "lslgeneric_gpu.h"
#include "ndt_feature_graph_gpu.h"
#include "ndt_mcl_gpu.h"

#include <string>
#include <vector>

namespace ndt_visualisation {

struct PointGPU {              // geometry_msgs/Point
    double x, y, z;
};

struct MarkerGPU {             // visualization_msgs/Marker: what the marker functions set
    enum { ARROW = 0, LINE_LIST = 5 };
    int type = ARROW;
    std::string frame_id;
    double scale_x = 0.0, scale_y = 0.0, scale_z = 0.0;
    double color[4] = {0.0, 0.0, 0.0, 0.0};   // r, g, b, a
    double lifetime = 0.0;     // seconds
    std::string ns;
    int id = 0;
    std::vector<PointGPU> points;
};

inline void assignDefault(MarkerGPU &m)
{
    m.frame_id = "/world";
    m.scale_x = m.scale_y = m.scale_z = 1.0;
    m.lifetime = 60.0;
}

// red, green, blue by color % 3 at alpha 0.3; opaque white for a negative color
inline void assignColor(MarkerGPU &m, int color)
{
    const int mod = color % 3;
    m.color[0] = mod == 0 ? 1.0 : (mod == 1 || mod == 2 ? 0.0 : 0.5);
    m.color[1] = mod == 1 ? 1.0 : (mod == 0 || mod == 2 ? 0.0 : 0.5);
    m.color[2] = mod == 2 ? 1.0 : (mod == 0 || mod == 1 ? 0.0 : 0.5);
    m.color[3] = 0.3;
    if (color < 0) m.color[0] = m.color[1] = m.color[2] = m.color[3] = 1.0;
}

namespace detail {

// a marker handle for the lifetime of one call
struct MarkerHandle {
    ndtgpu_marker *h = nullptr;
    MarkerHandle(size_t max_maps, size_t max_links) { ndtgpu_host::check(ndtgpu_marker_create(max_maps, max_links, &h), "ndtgpu_marker_create"); }
    ~MarkerHandle() { if (h) ndtgpu_marker_destroy(h); }
    MarkerHandle(const MarkerHandle &) = delete;
    MarkerHandle &operator=(const MarkerHandle &) = delete;
};

inline void append(MarkerGPU &m, const std::vector<double> &rows, size_t n_segments)
{
    m.points.reserve(m.points.size() + 2 * n_segments);
    for (size_t k = 0; k < 2 * n_segments; k++) m.points.push_back(PointGPU{rows[3 * k], rows[3 * k + 1], rows[3 * k + 2]});
}

// the cell markers of one map under `pose` (NULL: none) appended to m.points: one device call
inline void cells(lslgeneric::NDTMap &map, const Eigen::Affine3d *pose, MarkerGPU &m)
{
    m.type = MarkerGPU::LINE_LIST;
    m.scale_x = 0.02;
    const size_t capacity = 3 * (size_t)map.numberOfActiveCells();
    MarkerHandle mk(1, 0);
    std::vector<double> rows(6 * capacity + 6);
    size_t n = 0;
    int32_t overflow = 0;
    ndtgpu_host::check(ndtgpu_mapset_markers(mk.h, map.handle(), map.slot(), 1, pose ? pose->data() : nullptr, nullptr, rows.data(), nullptr, capacity, &n,
                                             &overflow, nullptr),
                       "ndtgpu_mapset_markers");
    if (overflow) throw ndtgpu_host::Error(NDTGPU_ERR_CAPACITY, "markerNDTCells: the map changed during the call");
    append(m, rows, n);
}

}  // namespace detail

// markerNDTCells(map, id, name) (ndt_rviz.h:1163-1175)
inline MarkerGPU markerNDTCells(lslgeneric::NDTMap &map, int id, const std::string &name)
{
    MarkerGPU m;
    assignDefault(m);
    assignColor(m, id);
    m.id = id;
    m.ns = name;
    detail::cells(map, nullptr, m);
    return m;
}

// markerNDTCells(map, pose, id, name) (ndt_rviz.h:1177-1189)
inline MarkerGPU markerNDTCells(lslgeneric::NDTMap &map, const Eigen::Affine3d &pose, int id, const std::string &name)
{
    MarkerGPU m;
    assignDefault(m);
    assignColor(m, id);
    m.id = id;
    m.ns = name;
    detail::cells(map, &pose, m);
    return m;
}

// markerNDTCells(map, id) (ndt_rviz.h:1191-1194)
inline MarkerGPU markerNDTCells(lslgeneric::NDTMap &map, int id) { return markerNDTCells(map, id, std::string("NDTMap")); }

// markerNDTCells2(map, pose, id, name, m) (ndt_rviz.h:1223-1233): into the caller's marker, behind the points it holds
inline void markerNDTCells2(lslgeneric::NDTMap &map, const Eigen::Affine3d &pose, int id, const std::string &name, MarkerGPU &m)
{
    assignDefault(m);
    assignColor(m, id);
    m.id = id;
    m.ns = name;
    detail::cells(map, &pose, m);
}

// markerParticlesNDTMCL3D(mcl, color, ns) (ndt_rviz.h:1277-1297): read from the device filter in place
inline MarkerGPU markerParticlesNDTMCL3D(const NDTMCL3D &mcl, int color, const std::string &ns)
{
    MarkerGPU m;
    assignDefault(m);
    m.ns = ns;
    m.id = 0;
    m.type = MarkerGPU::LINE_LIST;
    m.scale_x = 0.005;
    m.color[0] = 0.6;
    m.color[1] = 1.0;
    m.color[2] = 0.8;
    m.color[3] = 1.0;
    if (color >= 0) assignColor(m, color);
    const size_t n = mcl.pf.size();
    if (n == 0) return m;
    if (!mcl.handle()) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "markerParticlesNDTMCL3D: the filter is not initialized");
    std::vector<double> rows(6 * n);
    ndtgpu_host::check(ndtgpu_mcl_markers(mcl.handle(), 0, 1, nullptr, rows.data()), "ndtgpu_mcl_markers");
    detail::append(m, rows, n);
    return m;
}

}  // namespace ndt_visualisation

namespace ndt_feature {

// markerNDTFeatureLinks(graph, id, color, frame, skipOdom) (ndt_feature_rviz.h:282-313)
// A link that is drawn must name two nodes of the graph (ndtgpu_host::Error, NDTGPU_ERR_INVALID, where upstream indexes out of bounds);
// a link that skipOdom skips is not looked at, as upstream.
inline ndt_visualisation::MarkerGPU markerNDTFeatureLinks(const NDTFeatureGraphInterface &graph, const int id, const int color, const std::string &frame,
                                                          bool skipOdom)
{
    ndt_visualisation::MarkerGPU m;
    ndt_visualisation::assignDefault(m);
    ndt_visualisation::assignColor(m, color);
    m.ns = frame;
    m.id = id;
    m.type = ndt_visualisation::MarkerGPU::LINE_LIST;
    m.scale_x = 0.02;
    m.color[0] = m.color[3] = 1.0;
    m.color[1] = 0.65;
    const size_t n_nodes = graph.getNbNodes(), n_links = graph.getNbLinks();
    if (n_links == 0) return m;
    std::vector<double> T16(16 * n_nodes), score(n_links), rows(6 * n_links);
    std::vector<uint32_t> ref(n_links), mov(n_links);
    for (size_t i = 0; i < n_nodes; i++) {
        const double *p = graph.getNodeInterface(i).getPose().data();
        for (int e = 0; e < 16; e++) T16[16 * i + e] = p[e];
    }
    for (size_t i = 0; i < n_links; i++) {
        ref[i] = (uint32_t)graph.getLinkInterface(i).getRefIdx();
        mov[i] = (uint32_t)graph.getLinkInterface(i).getMovIdx();
        score[i] = graph.getLinkInterface(i).getScore();
    }
    ndtgpu_marker_params prm;
    ndtgpu_default_marker_params(&prm);
    prm.skip_negative = skipOdom ? 1 : 0;
    ndt_visualisation::detail::MarkerHandle mk(1, n_links);
    size_t n = 0;
    ndtgpu_host::check(ndtgpu_marker_links(mk.h, T16.data(), n_nodes, ref.data(), mov.data(), score.data(), n_links, &prm, rows.data(), n_links, &n, nullptr),
                       "ndtgpu_marker_links");
    ndt_visualisation::detail::append(m, rows, n);
    return m;
}

}  // namespace ndt_feature
