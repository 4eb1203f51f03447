// ndt_mcl_gpu.h -- host C++ mirror of perception_oru's NDTMCL3D (ndt_mcl/3d_ndt_mcl.h), the members that
// ndt_feature/src/ndt_feature_mcl_node.cpp touches: the constructor from an lslgeneric::NDTMap (:174), the public parameters
// (:175-184), initializeFilter (:335), updateAndPredictEff (:361), pf.size(), pf.pcloud[i].T / .p / getXYZ and pf.getMean()
// (:377-396).  A thin wrapper over one filter of the C-ABI bank (include/ndtgpu.h, "NDT Monte Carlo localisation"): the
// semantics, the recalled defaults and the deviations are stated there.  With this header the node's body compiles against the
// project instead of ndt_mcl/3d_ndt_mcl.h.
//
// The map is borrowed, not copied (the header's DEVIATION): nd_map must outlive the filter, and its cells must be computed
// (computeNDTCells) before the first update.  The parameters are read when initializeFilter creates the device filter, as the
// node sets them between the constructor and initializeFilter; changing them later takes effect at the next initializeFilter.
// Without a HIP device initializeFilter throws ndtgpu_host::Error (NDTGPU_ERR_NO_DEVICE): there is no CPU fallback.
#pragma once
#include "lslgeneric_gpu.h"

#include <cmath>
#include <cstring>
#include <vector>

class NDTMCL3D;

namespace mcl {

// ParticleFilter3D's PoseParticle: pose, weight, the last likelihood
struct PoseParticle {
    Eigen::Affine3d T;
    double p = 0.0;
    double lik = 0.0;
    void getXYZ(double &x, double &y, double &z) const
    {
        x = T(0, 3);
        y = T(1, 3);
        z = T(2, 3);
    }
};

// ParticleFilter3D: pcloud is a copy of the device particles, refreshed after every initializeFilter / updateAndPredictEff
class ParticleFilter3D {
public:
    std::vector<PoseParticle> pcloud;
    size_t size() const { return pcloud.size(); }
    // pf.getMean(): computed on the device (ndtgpu_mcl_mean)
    Eigen::Affine3d getMean() const
    {
        Eigen::Affine3d M;
        if (!h_) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "ParticleFilter3D::getMean: the filter is not initialized");
        ndtgpu_host::check(ndtgpu_mcl_mean(h_, 0, 1, M.data(), nullptr), "ndtgpu_mcl_mean");
        return M;
    }
    // the record of the last update (var_p, resampled, since_sir, terms, ...)
    ndtgpu_mcl_result lastResult() const
    {
        ndtgpu_mcl_result r{};
        if (h_) ndtgpu_host::check(ndtgpu_mcl_mean(h_, 0, 1, nullptr, &r), "ndtgpu_mcl_mean");
        return r;
    }

private:
    ndtgpu_mcl *h_ = nullptr;
    void refresh(size_t n)
    {
        std::vector<double> T(16 * n), w(n), lik(n);
        ndtgpu_host::check(ndtgpu_mcl_particles(h_, 0, 1, T.data(), w.data(), lik.data()), "ndtgpu_mcl_particles");
        pcloud.resize(n);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(pcloud[i].T.data(), &T[16 * i], 16 * sizeof(double));
            pcloud[i].p = w[i];
            pcloud[i].lik = lik[i];
        }
    }
    friend class ::NDTMCL3D;
};

}  // namespace mcl

class NDTMCL3D {
public:
    // the public members the node sets (:175-184); defaults: ndtgpu_default_mcl_params
    bool forceSIR;
    double SIR_varP_threshold;
    int SIR_max_iters_wo_resampling;
    std::vector<double> motion_model;          // 36 values, row-major 6x6
    std::vector<double> motion_model_offset;   // 6 values
    double resolution, resolution_sensor, zfilt_min;
    // (added; fixed upstream) the local scan map's extent, range limit and cell capacity, and the random-number seed
    double scan_size[3];
    double range_limit;
    uint32_t max_scan_cells;
    uint64_t seed;
    mcl::ParticleFilter3D pf;

    // NDTMCL3D(map_resolution, nd_map, zfilter) (:174)
    NDTMCL3D(double map_resolution, lslgeneric::NDTMap &nd_map, double zfilter) : map_(&nd_map)
    {
        ndtgpu_mcl_params p;
        ndtgpu_default_mcl_params(&p);
        forceSIR = p.force_sir != 0;
        SIR_varP_threshold = p.sir_varp_threshold;
        SIR_max_iters_wo_resampling = p.sir_max_iters_wo_resampling;
        motion_model.assign(p.motion_model, p.motion_model + 36);
        motion_model_offset.assign(p.motion_model_offset, p.motion_model_offset + 6);
        resolution = resolution_sensor = map_resolution;
        zfilt_min = zfilter;
        for (int a = 0; a < 3; a++) scan_size[a] = p.scan_size[a];
        range_limit = p.range_limit;
        max_scan_cells = p.max_scan_cells;
        seed = p.seed;
    }
    ~NDTMCL3D() { release(); }
    NDTMCL3D(const NDTMCL3D &) = delete;
    NDTMCL3D &operator=(const NDTMCL3D &) = delete;

    // the device filter's parameters as the members now hold them
    ndtgpu_mcl_params params() const
    {
        ndtgpu_mcl_params p;
        ndtgpu_default_mcl_params(&p);
        if (motion_model.size() != 36 || motion_model_offset.size() != 6)
            throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "NDTMCL3D: motion_model needs 36 values and motion_model_offset 6");
        p.map_res = resolution;
        p.sensor_res = resolution_sensor;
        for (int a = 0; a < 3; a++) p.scan_size[a] = scan_size[a];
        p.range_limit = range_limit;
        p.zfilt_min = zfilt_min;
        std::memcpy(p.motion_model, motion_model.data(), 36 * sizeof(double));
        std::memcpy(p.motion_model_offset, motion_model_offset.data(), 6 * sizeof(double));
        p.force_sir = forceSIR ? 1 : 0;
        p.sir_max_iters_wo_resampling = SIR_max_iters_wo_resampling;
        p.sir_varp_threshold = SIR_varP_threshold;
        p.max_scan_cells = max_scan_cells;
        p.seed = seed;
        return p;
    }

    // initializeFilter(x, y, z, r, p, t, cov_x, cov_y, cov_z, cov_r, cov_p, cov_t, numParticles) (:335): a fresh device filter
    void initializeFilter(double x, double y, double z, double r, double p, double t, double cov_x, double cov_y, double cov_z,
                          double cov_r, double cov_p, double cov_t, unsigned int numParticles)
    {
        release();
        const ndtgpu_mcl_params prm = params();
        const uint32_t idx = (uint32_t)map_->slot();
        ndtgpu_host::check(ndtgpu_mcl_create(map_->handle(), &idx, &prm, 1, numParticles, &pf.h_), "ndtgpu_mcl_create");
        const double pose6[6] = {x, y, z, r, p, t}, sigma6[6] = {cov_x, cov_y, cov_z, cov_r, cov_p, cov_t};
        ndtgpu_host::check(ndtgpu_mcl_initialize(pf.h_, 0, 1, pose6, sigma6), "ndtgpu_mcl_initialize");
        n_ = numParticles;
        pf.refresh(n_);
    }

    // updateAndPredictEff(Tmotion, cloud, subsample_level) (:361): the cloud in the base frame
    void updateAndPredictEff(const Eigen::Affine3d &Tmotion, const pcl::PointCloud<pcl::PointXYZ> &cloud, double subsample_level)
    {
        if (!pf.h_) throw ndtgpu_host::Error(NDTGPU_ERR_INVALID, "NDTMCL3D::updateAndPredictEff: initializeFilter first");
        ndtgpu_host::check(ndtgpu_mcl_update_host(pf.h_, 0, 1, Tmotion.data(), subsample_level, cloud.size() ? &cloud.points[0] : nullptr,
                                                  cloud.size(), sizeof(pcl::PointXYZ), cloud.size() * sizeof(pcl::PointXYZ)),
                           "ndtgpu_mcl_update_host");
        pf.refresh(n_);
    }

    // the device filter (a bank of one)
    ndtgpu_mcl *handle() const { return pf.h_; }

private:
    lslgeneric::NDTMap *map_;
    size_t n_ = 0;
    void release()
    {
        if (pf.h_) ndtgpu_mcl_destroy(pf.h_);
        pf.h_ = nullptr;
        pf.pcloud.clear();
    }
};
