/*
 * ndtgpu.h -- C-ABI of the MI355X-native NDT scan-matching front-end.
 *
 * Drop-in boundary for the lslgeneric:: classes that MalcolmMielle/ndt_feature_graph calls
 * on its hot path (there is no FFI layer in the reference: the path sits behind the C++
 * class API of perception_oru's ndt_map / ndt_registration).  Each
 * entry point cites the reference interface it replaces (paths relative to the reference
 * root).  Plain pointers and sizes only; handles are opaque; outputs are caller-owned.
 *
 * Conventions
 *   - 4x4 poses are 16 doubles, COLUMN-major, exactly Eigen::Affine3d::data().
 *   - points are float xyz records, `stride_bytes` apart (12 = packed, 16 = pcl::PointXYZ).
 *   - a "mapset" is B NDT maps that share one grid geometry (cell size, extent in cells) and
 *     live in one device arena; a single lslgeneric::NDTMap is a mapset with B = 1.
 *   - every call returns ndtgpu_status; convergence is reported in the result struct, never
 *     as an error (reference: match() returns bool, fusion.h:1075-1079).
 *   - handles are not thread-safe; distinct handles may be used from distinct threads.
 *   - the library never falls back to the CPU: without a HIP device every compute entry
 *     point returns NDTGPU_ERR_NO_DEVICE.
 */
#ifndef NDTGPU_H
#define NDTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int ndtgpu_status;
enum {
    NDTGPU_OK = 0,
    NDTGPU_ERR_INVALID = -1,   /* bad argument */
    NDTGPU_ERR_HIP = -2,       /* HIP runtime error (see ndtgpu_last_error) */
    NDTGPU_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    NDTGPU_ERR_CAPACITY = -4,  /* a map needed more cells than max_cells */
    NDTGPU_ERR_ALLOC = -5
};

typedef struct ndtgpu_mapset ndtgpu_mapset;
typedef void *ndtgpu_stream; /* hipStream_t; NULL = default stream */

/* lslgeneric::LazyGrid(res) + NDTMap::initialize(cx,cy,cz,sx,sy,sz) / guessSize(...)
 * (ndt_feature/src/ndt_feature_src/ndt_feature_fuser_hmt.cpp:87-89, 195-196, 222). */
typedef struct {
    double res;        /* cubic cell size [m] (params_.resolution) */
    double centre[3];  /* grid centre [m]; per-map override: ndtgpu_mapset_set_centre */
    double size[3];    /* extent [m]; cells per axis = |ceil(size/res)| (LazyGrid::initialize) */
    uint32_t max_cells; /* capacity of occupied cells per map; 0 = min(slots, 16384) */
} ndtgpu_grid_params;

/* NDTCell::computeGaussian / rescaleCovariance knobs.
 * PROVENANCE: both constants live in perception_oru's ndt_map (un-vendored, no version pinned by the reference).
 *   n_min        the reference never passes it; the perception_oru revisions of the reference's era test
 *                `hasGaussian_ == false && points_.size() < 3` in the 5-argument computeGaussian that
 *                ndt_feature_fuser_hmt.cpp:94, 227, 486 reach (older / "simple" variants use 6).  Default 3;
 *                it decides which cells exist, so a deployment against a different perception_oru sets it here.
 *   eval_factor  EVAL_FACTOR of NDTCell; the reference itself passes 1000 when it builds cells by hand
 *                (ndt_feature/include/ndt_feature/utils.h:200). */
typedef struct {
    int32_t n_min;       /* points needed for a first Gaussian (default 3, see above) */
    double eval_factor;  /* EVAL_FACTOR, eigenvalue floor lambda_max/eval_factor (default 1000) */
} ndtgpu_cell_params;

/* NDTMatcherD2D members set by the callers (ndt_feature_graph.cpp:261-262;
 * ndt_feature_fuser_hmt.cpp:356-357; ndt_matcher_d2d_fusion.h:1170-1174).
 * PROVENANCE of the defaults (ndtgpu_default_match_params): the "fuser" preset -- what matchFusion is called with
 * in production: n_neighbours 2, ITR_MAX 30, DELTA_SCORE 1e-6 (launch/gustav_laser_tf.launch:56-59,
 * ndt_graph_offline.cpp:310-313), step_control on, lfd1 1, lfd2 0.05 (NDTMatcherD2D constructor, perception_oru).
 * The EDGE matcher of ndt_feature_graph.cpp:261 is default-constructed with only n_neighbours overridden; its
 * DELTA_SCORE is perception_oru's constructor value `10e-3 * current_resolution` with current_resolution = 0.1,
 * i.e. 1e-3 -- recalled, not readable in the reference: the host mirror
 * (host/lslgeneric_gpu.h NDTMatcherD2D::DELTA_SCORE) exposes it as a member like upstream does. */
typedef struct {
    int32_t n_neighbours;      /* matcher.n_neighbours */
    int32_t itr_max;           /* ITR_MAX */
    double delta_score;        /* DELTA_SCORE */
    int32_t step_control;      /* More-Thuente line search on/off */
    double lfd1, lfd2;         /* 1.0, 0.05 */
    int32_t dof_mask;          /* bit a = pose dof a active: 0x3f NDTMatcherD2D, 0x23 NDTMatcherD2D_2D */
    int32_t use_initial_guess; /* match(..., useInitialGuess) */
} ndtgpu_match_params;

typedef struct {
    int32_t converged;  /* return value of match(): 0 = iteration cap hit */
    int32_t iterations; /* itr_ctr at exit */
    int32_t fevals;     /* derivativesNDT evaluations */
    int32_t exit_code;  /* 0 step<delta, 1 gradient vanished, 2 wrong direction, 3 iteration cap;
                         * not run (device-pointer batches): -2 map index out of range, -3 a map overflowed max_cells,
                         * -4 the grid barrier of a small batch gave up (foreign work held CUs for seconds) */
    double score;       /* score at the returned pose */
    int32_t n_source;   /* Gaussian cells in the source map */
    int32_t n_target;
    int64_t cycles_eval;   /* shader clocks spent in derivative evaluations (profiling aid) */
    int64_t cycles_solver; /* shader clocks spent in the serial Newton / line-search code */
    int64_t pair_terms_g;  /* (source cell, target cell) terms summed in gradient-only evaluations */
    int64_t pair_terms_h;  /* ... and in evaluations with the Hessian (k-bar = terms / (fevals * n_source)) */
} ndtgpu_match_result;

/* ---- library ------------------------------------------------------------------------- */
const char *ndtgpu_version(void);
const char *ndtgpu_last_error(void);
/* number of usable devices (0 on a box without a GPU; never an error) */
int ndtgpu_device_count(void);
void ndtgpu_default_cell_params(ndtgpu_cell_params *p);
void ndtgpu_default_match_params(ndtgpu_match_params *p);

/* ---- maps ---------------------------------------------------------------------------- */
/* new NDTMap(new LazyGrid(res)) x n_maps + initialize()  (fuser_hmt.cpp:87-89, 195-196) */
ndtgpu_status ndtgpu_mapset_create(const ndtgpu_grid_params *grid, size_t n_maps, ndtgpu_mapset **out);
/* NDTMap destructor (ndt_feature_graph.h:78-88 deletes node maps) */
ndtgpu_status ndtgpu_mapset_destroy(ndtgpu_mapset *set);
/* LazyGrid::setCenter -- e.g. the snapped centroid of loadPointCloudCentroid
 * (fuser_hmt.cpp:201-217; ndt_odom_debug.cpp:191) or the node pose (fuser_hmt.cpp:89) */
ndtgpu_status ndtgpu_mapset_set_centre(ndtgpu_mapset *set, size_t map, const double centre[3]);
ndtgpu_status ndtgpu_mapset_info(const ndtgpu_mapset *set, size_t *n_maps, int32_t cells_per_axis[3],
                                 uint32_t *max_cells);

/* NDTMap::loadPointCloud(cloud, range) + computeNDTCells(CELL_UPDATE_MODE_SAMPLE_VARIANCE)
 * (fuser_hmt.cpp:225-227; ndt_odom_debug.cpp:178-179) for maps [first, first+count).
 * xyz_dev: DEVICE pointer; map k reads n_points records from
 *   (char*)xyz_dev + k*map_stride_bytes, records stride_bytes apart.
 * range_limit <= 0 disables the range filter; range_origins (HOST, 3 doubles per map, may be
 * NULL = sensor at the frame origin) gives the origin the range is measured from
 * (loadPointCloudCentroid, fuser_hmt.cpp:201-202).  Replaces the maps' content.
 * Asynchronous on `stream`. */
ndtgpu_status ndtgpu_mapset_build(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_dev,
                                  size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                  double range_limit, const double *range_origins,
                                  const ndtgpu_cell_params *cell, ndtgpu_stream stream);
/* same, points in HOST memory (one H2D copy; the reference hands over host PointClouds) */
ndtgpu_status ndtgpu_mapset_build_host(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_host,
                                       size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                       double range_limit, const double *range_origins,
                                       const ndtgpu_cell_params *cell);
/* The same with an explicit stream: returns as soon as the caller's memory has been read (it may be reused); the maps are
 * complete when `stream` is.  Both forms cut batches of >= 24 MB into chunks of clouds that travel through a ring of
 * pinned slots filled by host threads: the copy of chunk k + 1 runs under the build of chunk k, and nothing waits for the
 * whole device (the synchronous form waits for a stream of its own). */
ndtgpu_status ndtgpu_mapset_build_host_async(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_host,
                                             size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                             double range_limit, const double *range_origins,
                                             const ndtgpu_cell_params *cell, ndtgpu_stream stream);

/* NDTMap::numberOfActiveCells / getAllCells (fuser_hmt.cpp:234; ndtgraph_conversion.h:34-43):
 * Gaussian cells in slot order (x-major, y, z).  Synchronises the build stream.
 * Any output pointer may be NULL.  cov9 row-major 3x3, idx3 = LazyGrid cell indices. */
ndtgpu_status ndtgpu_mapset_num_cells(ndtgpu_mapset *set, size_t map, uint32_t *n);
ndtgpu_status ndtgpu_mapset_export_cells(ndtgpu_mapset *set, size_t map, double *mean3, double *cov9,
                                         int32_t *idx3, uint32_t *npts);
/* installs ready-made Gaussians (CellVector::addNDTCell / a node map received from elsewhere;
 * ndt_odom_debug.cpp:217-229); the cell index is LazyGrid::getIndexForPoint(mean). */
ndtgpu_status ndtgpu_mapset_set_cells(ndtgpu_mapset *set, size_t map, const double *mean3, const double *cov9,
                                      size_t n_cells);

/* ndt_feature::discardCell(map, pt) (utils.h:229-236; ndt_feature_fuser_hmt.cpp:229-232, ndt_odom_debug.cpp:194-198): the cells that
 * hold the given points (HOST, n x packed float xyz) lose their Gaussian (hasGaussian_ = false).  Synchronous. */
ndtgpu_status ndtgpu_mapset_discard_cells(ndtgpu_mapset *set, size_t map, const float *xyz, size_t n_points);

/* ---- incremental (fused) node maps ------------------------------------------------------------- */
/* NDTMap::initialize(cx,cy,cz,sx,sy,sz) on every map of the set (fuser_hmt.cpp:89): every cell of the grid exists
 * and carries an occupancy (log-odds, 0 = no reading).  Allocates the per-slot occupancy arrays and the second cell
 * array an incremental update needs (12 bytes per slot + 80 bytes per cell and map).  Idempotent.  Plain builds
 * (ndtgpu_mapset_build*) on such a set also leave the occupancies NDTCell::computeGaussian would. */
ndtgpu_status ndtgpu_mapset_enable_occupancy(ndtgpu_mapset *set);

/* NDTMap::addPointCloud(origin, cloud, classifierTh, maxz, sensor_noise, occupancy_limit) immediately followed by
 * NDTMap::computeNDTCells(CELL_UPDATE_MODE_SAMPLE_VARIANCE, maxnumpoints, occupancy_limit, origin, noise): the two
 * calls the reference always makes together (fuser_hmt.cpp:92-94: (.., 0.1, 100.0, 0.1) + (.., 1e5, 255, ..);
 * :485-486: (.., 0.06, 25) + (.., 1e5, 255, ..)).  classifierTh, and origin / noise of computeNDTCells, are unused
 * upstream on this path and have no counterpart here. */
typedef struct {
    double maxz;            /* addPointCloud: points above it are dropped (100.0 / 25) */
    double sensor_noise;    /* addPointCloud: 0.1 / 0.06 */
    double maxnumpoints;    /* computeNDTCells: N saturates here ("sliding average"; 1e5); <= 0: never */
    double occupancy_limit; /* both: occupancy is clamped to +-limit (255) */
    int32_t n_min;          /* see ndtgpu_cell_params */
    double eval_factor;
} ndtgpu_fuse_params;
void ndtgpu_default_fuse_params(ndtgpu_fuse_params *p);   /* the values of fuser_hmt.cpp:485-486 */
/* Maps [first, first+count) each receive one cloud (map k: n_points records at xyz + k*map_stride_bytes, in the map's
 * frame) taken from sensor position origins[3*k..] (HOST).  Per beam the cells between sensor and hit receive
 * emptiness evidence, the hit joins its cell; cells merge the new points into their Gaussian (N, mean, covariance),
 * Gaussians whose occupancy falls to <= 0 disappear.  Needs ndtgpu_mapset_enable_occupancy.  xyz_dev: DEVICE pointer;
 * asynchronous on `stream`. */
ndtgpu_status ndtgpu_mapset_add_cloud(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_dev,
                                      size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                      const double *origins, const ndtgpu_fuse_params *prm, ndtgpu_stream stream);
/* same, points in HOST memory; synchronous */
ndtgpu_status ndtgpu_mapset_add_cloud_host(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_host,
                                           size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                           const double *origins, const ndtgpu_fuse_params *prm);
/* (asynchronous form of the host entry, like ndtgpu_mapset_build_host_async) */
ndtgpu_status ndtgpu_mapset_add_cloud_host_async(ndtgpu_mapset *set, size_t first, size_t count, const void *xyz_host,
                                                 size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                 const double *origins, const ndtgpu_fuse_params *prm,
                                                 ndtgpu_stream stream);
/* a fresh NDTMap in slots [first, first+count): no Gaussians, occupancy 0 (a new graph node, graph.cpp:87-101) */
ndtgpu_status ndtgpu_mapset_clear(ndtgpu_mapset *set, size_t first, size_t count);
/* NDTCell::getOccupancy of every cell of one map, slot order (x-major, y, z): cells_per_axis[0]*[1]*[2] floats */
ndtgpu_status ndtgpu_mapset_export_occupancy(ndtgpu_mapset *set, size_t map, float *occ_out);

/* the inverse of export_occupancy: installs NDTCell::occ of every cell of one map (a map received as a message,
 * ndtgraph_conversion.h:129-158).  Needs ndtgpu_mapset_enable_occupancy. */
ndtgpu_status ndtgpu_mapset_import_occupancy(ndtgpu_mapset *set, size_t map, const float *occ);

/* ndt_feature::overlapNDTOccupancyScore(ref, mov, T) (ndt_feature_node.h:213-252; used at ndt_feature_graph.cpp:175,
 * 338-340) for n_links (ref, mov, T) triples.  Both sets need ndtgpu_mapset_enable_occupancy.  T16: HOST, n_links x 16
 * column-major.  score: HOST n_links doubles (1.0 when no cell pair overlaps); nb_sum (may be NULL): HOST, the number
 * of compared cell pairs.  Synchronous. */
ndtgpu_status ndtgpu_overlap_score_batch(ndtgpu_mapset *ref_set, const uint32_t *ref_idx, ndtgpu_mapset *mov_set,
                                         const uint32_t *mov_idx, const double *T16, size_t n_links, double *score,
                                         int64_t *nb_sum, ndtgpu_stream stream);

/* ---- matcher ---------------------------------------------------------------------------- */
/* NDTMatcherD2D::derivativesNDT(sourceCells, targetMap, g, H, computeHessian)
 * (ndt_matcher_d2d_fusion.h:80, 238, 444, 617, 856, 1085): lets the in-repo matchFusion host
 * loop run unchanged.  src_* are HOST arrays of m cells already in the target frame.
 * g[6]; H[36] row-major (untouched when compute_hessian == 0). */
ndtgpu_status ndtgpu_derivatives(ndtgpu_mapset *target, size_t target_map, const double *src_mean3,
                                 const double *src_cov9, size_t m, int n_neighbours, int compute_hessian,
                                 double lfd1, double lfd2, double *score, double g[6], double H[36]);

/* NDTMatcherD2D::match(target, source, T, useInitialGuess) (ndt_feature_graph.cpp:273) and
 * NDTMatcherD2D_2D::match (ndt_matcher_d2d_fusion.h:1175) for n_pairs independent pairs --
 * the loop of NDTFeatureGraph::updateLinksUsingNDTRegistration (ndt_feature_graph.cpp:347-353).
 * Pair k matches target_set[target_idx[k]] (fixed) against source_set[source_idx[k]] (moving).
 * T16: HOST, n_pairs x 16 doubles, in: initial guess, out: result.  results: HOST, n_pairs.
 * The whole Newton / More-Thuente loop runs on the device: persistent workgroups pulling pairs from a ticket
 * counter when the batch fills the chip, one grid-barrier launch with several workgroups per registration when it
 * does not (<= 8 pairs, or <= 128 pairs of large maps; the one-link-at-a-time call of ndt_feature_graph.cpp:273 is
 * n_pairs = 1).
 * Synchronous (returns after the results are on the host). */
ndtgpu_status ndtgpu_match_batch(ndtgpu_mapset *target_set, const uint32_t *target_idx, ndtgpu_mapset *source_set,
                                 const uint32_t *source_idx, double *T16, size_t n_pairs,
                                 const ndtgpu_match_params *prm, ndtgpu_match_result *results,
                                 ndtgpu_stream stream);
/* device-resident variant for pipelines: T16_dev / results_dev are DEVICE buffers, idx arrays
 * DEVICE uint32.  ONE launch, ALWAYS asynchronous on `stream`: no host synchronisation.
 * Batches that fill the chip (and every batch on sets of small maps): persistent workgroups that pull pairs from a
 * ticket counter; safe under stream capture.  At most half as many pairs as CUs on a source set with room for >= 16384
 * cells per map (3D maps): several workgroups per registration -- static teams at a grid barrier up to 8 pairs, beyond
 * that a pool of (registration, evaluation, chunk) tasks that any workgroup serves (32 pairs of 12 k-cell maps: 7 instead
 * of 65 ms) -- ordered behind the previous launch of its kind, on whatever stream, by an event (not while `stream` is
 * being captured: the persistent kernel then).  Environment
 * NDTGPU_DEVICE_COOP=0 (read per call) keeps every batch on the persistent kernel.  Either way a registration's result
 * does not depend on its batch; the shapes agree to 1e-8 (another summation order).  A launch that gives up (a grid
 * barrier starved by a foreign process for seconds) reports exit_code -4, converged = 0 and leaves the pose untouched.
 * The indices are range-checked on the device and a map whose build overflowed max_cells is refused: such a pair gets
 * converged = 0 and exit_code -2 / -3, its pose stays untouched.  The work area (ticket counters, parked solver
 * states) belongs to the TARGET set: calls on different streams with the same target set -- through this entry or the
 * host-pointer ones -- are ordered by an event; builds of the involved maps must be ordered before the call by the
 * caller (same stream, or an event). */
ndtgpu_status ndtgpu_match_batch_device(ndtgpu_mapset *target_set, const uint32_t *target_idx_dev,
                                        ndtgpu_mapset *source_set, const uint32_t *source_idx_dev,
                                        double *T16_dev, size_t n_pairs, const ndtgpu_match_params *prm,
                                        ndtgpu_match_result *results_dev, ndtgpu_stream stream);
/* The persistent kernel's safety valve: a wave that finds no work for ~2 s raises a word in the target set's work area
 * and every workgroup leaves; registrations that were never drawn then keep whatever results_dev held.  The
 * host-pointer entries read the word themselves (NDTGPU_ERR_HIP); after a device batch the caller asks here (waits for
 * the set's last stream).  No counterpart in the reference: graph.cpp:347-353 is a serial host loop. */
ndtgpu_status ndtgpu_match_aborted(ndtgpu_mapset *target_set, int *aborted);
/* ndt_feature::matchFusion(target, source, <empty feature maps>, T, Tcov, useInitialGuess, useNDT = true,
 * useFeat = false, step_control, ITR_MAX, n_neighbours, DELTA_SCORE, useSoftConstraints, ...,
 * useTikhonovRegularization = false)  (ndt_matcher_d2d_fusion.h:797-1155; call site
 * ndt_feature_fuser_hmt.cpp:356-357): the D2D matcher plus the odometry soft constraint
 * x^T Tcov^-1 x on the accumulated pose increment (fusion.h:875-890, 1098-1110).
 * Tcov36: HOST, n_pairs x 36 doubles, row-major 6x6 covariance of (x,y,z,roll,pitch,yaw).
 * use_soft_constraints is a bit set: bit 0 = useSoftConstraints, bit 1 = useTikhonovRegularization (fusion.h:894-911,
 * 1113-1115: g <- H^T g + Q x0, H <- H^T H + Q, score += x0^T Q x0 with x0 the 2D pose vector of T Tinit^-1 and
 * Q = Tcov^-1); 0 degenerates to ndtgpu_match_batch.  Feature / odometry-cell maps: ndtgpu_match_fusion_feat_batch. */
ndtgpu_status ndtgpu_match_fusion_batch(ndtgpu_mapset *target_set, const uint32_t *target_idx,
                                        ndtgpu_mapset *source_set, const uint32_t *source_idx, double *T16,
                                        const double *Tcov36, size_t n_pairs, const ndtgpu_match_params *prm,
                                        int use_soft_constraints, ndtgpu_match_result *results, ndtgpu_stream stream);
/* The feature / odometry-cell maps of ndt_feature::matchFusion (targetNDT_feat, sourceNDT_feat, corr_feat;
 * ndt_matcher_d2d_fusion.h:797-801): two CellVector maps whose cells correspond one to one.  The fuser fills them with
 * FLIRT matches and / or 40 copies of an odometry cell pair (ndt_feature_fuser_hmt.cpp:291-334: target mean
 * Tnow * Tmotion.translation(), source mean Tinit * 0, covariance odom_cov, the last source cell un-rotated).
 * Correspondence i of registration k is entry offsets[k] + i of the four arrays (corr_feat[i] = (i, i)); at most 64 per
 * registration.  All arrays HOST. */
typedef struct ndtgpu_feat_pairs {
    const uint32_t *offsets;     /* [n_pairs + 1], non-decreasing */
    const double *src_mean;      /* [total][3]   cells of sourceNDT_feat: moved by T like the source map */
    const double *src_cov;       /* [total][6]   xx xy xz yy yz zz */
    const double *tgt_mean;      /* [total][3]   cells of targetNDT_feat */
    const double *tgt_cov;       /* [total][6] */
} ndtgpu_feat_pairs;
/* ndt_feature::matchFusion with useFeat (ndt_matcher_d2d_fusion.h:797-1155; call site ndt_feature_fuser_hmt.cpp:353-357
 * with use_odom_or_features): per Newton iteration the sums of NDTMatcherFeatureD2D::derivativesNDT over the
 * correspondences (the same pair term as the D2D matcher, known correspondence) are added to the NDT sums (fusion.h:858-
 * 871); with step control NDTMatcherD2D::lineSearchMT runs on the NDT maps, then NDTMatcherFeatureD2D::lineSearchMT on
 * the feature maps with the (possibly negated) increment the first one left, and the step is the smaller of the two, the
 * larger one when either is 0 (fusion.h:1013-1023); the final score includes the feature score (fusion.h:1085-1096).
 * flags: bit 0 useSoftConstraints, bit 1 useTikhonovRegularization, bit 2 step_control_fusion.  With bit 2 set and bit 0
 * clear the reference runs the JOINT line search lineSearchMTFusion (fusion.h:1004-1006, 390-793) instead: one search
 * on f_ndt(trial) + f_feat -- where, as written upstream, the feature maps are evaluated on the UN-stepped cells in every
 * trial (fusion.h:619), so their score and gradient at the current pose enter as constants.  Restated as written.
 * `fevals` counts derivative evaluations of the NDT maps.  feat == NULL: ndtgpu_match_fusion_batch.
 * A registration WITHOUT correspondences (offsets[k + 1] == offsets[k]) inside such a batch is run with useFeat = false, i.e.
 * by the rules of ndtgpu_match_fusion_batch: the reference's only call site passes useFeat = true together with at least
 * one correspondence (FLIRT matches that passed the consistency check, or the 40 odometry cells:
 * ndt_feature_fuser_hmt.cpp:296-320, 341-347).  What upstream's feature line search would do on EMPTY maps -- a zero
 * directional derivative, hence the in-place negation of the increment and the recovery step -- is deliberately not
 * restated, neither here nor in oracle/ndt_oracle.c (match_common: use_feat = n_feat > 0). */
ndtgpu_status ndtgpu_match_fusion_feat_batch(ndtgpu_mapset *target_set, const uint32_t *target_idx,
                                             ndtgpu_mapset *source_set, const uint32_t *source_idx, double *T16,
                                             const double *Tcov36, const ndtgpu_feat_pairs *feat, size_t n_pairs,
                                             const ndtgpu_match_params *prm, int flags, ndtgpu_match_result *results,
                                             ndtgpu_stream stream);
/* NDTMatcherD2D::covariance(target, source, T, cov) for n_links registered links (ndt_feature_graph.cpp:296-298;
 * ndt_feature_fuser_hmt.cpp:403-405): cov = H^-1 (0.03^2 J^T J) H^-1, H = D2D Hessian at T (prm->n_neighbours, lfd1,
 * lfd2), one row of J per source cell that falls into a Gaussian target cell.  PROVENANCE: perception_oru, restated from
 * memory (the least certain part of the path); `mode` selects what the row formula uses for the
 * pose Jacobians: 0 = those of the source cell itself (computeDerivativesLocal), 1 = the matcher's constructor values
 * (j = [I 0], Z = 0), which is what revisions whose derivativesNDT works on thread-local copies effectively compute.
 * T16: HOST n_links x 16 column-major (the registered poses); cov36: HOST n_links x 36 row-major.  A singular Hessian
 * gives an all-zero matrix for that link and NDTGPU_ERR_INVALID is NOT raised: singular[k] (may be NULL) is set to 1. */
ndtgpu_status ndtgpu_covariance_batch(ndtgpu_mapset *target_set, const uint32_t *target_idx, ndtgpu_mapset *source_set,
                                      const uint32_t *source_idx, const double *T16, size_t n_links,
                                      const ndtgpu_match_params *prm, int mode, double *cov36, int32_t *singular,
                                      ndtgpu_stream stream);
/* ---- exchange records of cell maps (multi-GPU graph replay, SURVEY.md 8e phases A-B) --------------------------------
 * With the node maps of a replay built data-parallel (node k on rank k mod world), every rank needs every node map before
 * it refines its share of the links: ndt_feature_graph.cpp:273 reads nodes_[ref].map and nodes_[mov].map (the loop
 * :347-353; candidate enumeration :395-405; caller ndt_feature_graph_opt.cpp:131-160).  pack writes ONE fixed-stride
 * record per map into a DEVICE buffer -- what one all_gather then moves --, unpack installs records into maps of a set
 * with the same grid geometry (cells, rank map, counters; occupancies when both sides carry them): an unpacked map is
 * indistinguishable from the packed one (same matcher bits).  Record = ndtgpu_packed_header, cells_cap cell records
 * (80 bytes each, the first n_cells valid, in LazyGrid slot order), then cells-per-grid floats when with_occupancy
 * (NDTCell::occ of every cell, for overlapNDTOccupancyScore, ndt_feature_node.h:213-252).  A map with more cells than
 * cells_cap is cut and flagged (flags bit 0), as is one that overflowed max_cells where it was built.  Asynchronous on
 * `stream`; no counterpart in the reference, whose graph lives in one process. */
typedef struct ndtgpu_packed_header { uint32_t n_cells, flags, n_dropped, cells_cap; } ndtgpu_packed_header;
typedef struct ndtgpu_cell_record {            /* 80 bytes */
    double mean[3];
    double cov[6];                             /* xx xy xz yy yz zz */
    uint32_t n;                                /* points behind the Gaussian */
    uint32_t slot;                             /* (ix * size_y + iy) * size_z + iz */
} ndtgpu_cell_record;
size_t ndtgpu_mapset_pack_bytes(const ndtgpu_mapset *set, uint32_t cells_cap, int with_occupancy);   /* bytes per record */
ndtgpu_status ndtgpu_mapset_pack_cells_device(ndtgpu_mapset *set, size_t first, size_t count, void *buf_dev,
                                              size_t record_stride_bytes, uint32_t cells_cap, int with_occupancy,
                                              ndtgpu_stream stream);
ndtgpu_status ndtgpu_mapset_unpack_cells_device(ndtgpu_mapset *set, size_t first, size_t count, const void *buf_dev,
                                                size_t record_stride_bytes, int with_occupancy, ndtgpu_stream stream);
/* The SPARSE form of the occupancy block: {uint32 n_occ, uint32 occ_cap} + occ_cap x {uint32 slot, float occ}, the cells
 * that have a reading (occupancy != 0, i.e. not the 0.5 of "initialised, no readings", ndt_feature_node.h:213-252) in slot
 * order; flags bit 2 marks it and ndtgpu_mapset_unpack_cells_device installs either form (every other cell gets "no
 * reading").  A fused node map of the replay has readings in 2-3 % of its 80 000 slots: 22 KB instead of 320 KB per node,
 * the exchange record 50 KB instead of 371 KB.  ndtgpu_mapset_occupied_cells_max: the largest number of such cells over
 * maps [first, first + count) -- what occ_cap must hold (host result: synchronises `stream`; with several ranks take the
 * maximum over ranks: the record stride is common).  A map with more readings than occ_cap is cut and flagged like one with
 * more cells than cells_cap. */
size_t ndtgpu_mapset_pack_bytes_sparse(const ndtgpu_mapset *set, uint32_t cells_cap, uint32_t occ_cap);
ndtgpu_status ndtgpu_mapset_occupied_cells_max(ndtgpu_mapset *set, size_t first, size_t count, uint32_t *max_occupied,
                                               ndtgpu_stream stream);
ndtgpu_status ndtgpu_mapset_pack_cells_sparse_device(ndtgpu_mapset *set, size_t first, size_t count, void *buf_dev,
                                                     size_t record_stride_bytes, uint32_t cells_cap, uint32_t occ_cap,
                                                     ndtgpu_stream stream);

/* ---- scans in, poses out: the whole path as ONE call ------------------------------------------------------------------
 * The reference reaches the path through calls that do everything for their inputs at once:
 * NDTFeatureGraph::updateLinksUsingNDTRegistration (ndt_feature_graph.cpp:347-353: every link of the list) and the fuser's
 * loadPointCloud + computeNDTCells + match of ndt_feature_fuser_hmt.cpp:195-227, 353-357 (raw scan -> NDT map -> pose).
 * A registrar is that call shape for batches of scan pairs: it owns `depth` internal map sets (2 x pairs_per_batch maps of
 * one grid geometry each), one stream per map set and the index arrays, and every submitted batch travels
 *     grid build of all target and source scans of a sub-batch (ONE launch)  ->  D2D matcher (ONE launch)
 * on the next internal stream, released when the previous sub-batch's builds are done: the builds of sub-batch k + 1 run on
 * the CUs that the long registrations of sub-batch k do not occupy (the pipeline that bench.py drove by hand until round 4).
 * Results are bit for bit those of ndtgpu_mapset_build + ndtgpu_match_batch_device on the same scans. */
typedef struct ndtgpu_registrar ndtgpu_registrar;
/* What a caller may decide about a registrar -- one POD struct, defaults from
 * ndtgpu_default_registrar_params; a field left at 0 means "the library's choice".  (The NDTGPU_REG_* environment variables of
 * earlier rounds survive as EXPERIMENT switches only: they fill in fields the caller left at 0.) */
enum { NDTGPU_MATCHER_AUTO = 0,        /* stream-fed where it applies (2 <= depth <= 8, max_cells < 16384, a device with more than
                                        * one stream priority), else one launch per sub-batch */
       NDTGPU_MATCHER_PER_BATCH = 1,   /* one matcher launch per sub-batch on the sub-batch's stream, ordered by events */
       NDTGPU_MATCHER_STREAM_FED = 2   /* ONE running matcher instance serves batch after batch from a queue in device memory;
                                        * create fails with NDTGPU_ERR_INVALID where it cannot be had */ };
typedef struct {
    size_t pairs_per_batch;   /* registrations per internal sub-batch (1024 fills an MI355X: two registrations per CU in flight) */
    int32_t depth;            /* internal map sets in flight, 1 .. 16 (the stream-fed matcher serves up to 8; a batch is complete
                               * 3-5 ms after its publication and its set is busy until then: 8 keeps the builds from waiting for
                               * that, 4 costs ~5 % on the bench; memory: ndtgpu_mapset_create x 2 x pairs_per_batch maps each) */
    int32_t matcher_form;     /* NDTGPU_MATCHER_* */
    uint32_t matcher_groups;  /* CUs (workgroups) the matcher side holds while builds run beside it; 0 = MEASURED: the first
                               * sub-batch runs alone on the chip, the kernels' own clocks give the CU-time of builds and
                               * registrations, and the chip is split in that proportion */
    int32_t build_streams;    /* stream-fed form: 1 or 2 build streams that take the sub-batches in turn; 0 = 2 when depth >= 3 */
    uint32_t linger_us;       /* stream-fed form: how long a matcher instance that has worked stays when it runs dry (0 = 1000: where
                               * the builds are the slower side an instance that leaves has to be placed again among build
                               * workgroups that keep arriving; ndtgpu_registrar_sync does not wait for it) */
    int32_t recalibrate_pct;  /* measured split only: when the mean number of Gaussian cells per map over the last sub-batches
                               * differs from the figure the split was measured at by more than this many percent, the pipeline is
                               * drained once and the split measured again (a registrar that moves from halls to clutter).
                               * 0 = 25; negative = never */
    int32_t matcher_slots;    /* stream-fed form: registrations in flight per workgroup of a matcher instance, 2 (hit lists of 1024 entries
                               * per share) or 3 (512: maps of up to ~450 cells; the one-lane solver steps of a registration are then covered
                               * by two others, +8 % on the bench); 0 = chosen with the split by the measured cells per map (2 with a
                               * forced split).  The same bits either way. */
} ndtgpu_registrar_params;
void ndtgpu_default_registrar_params(ndtgpu_registrar_params *p);
typedef struct {
    int32_t matcher_form;     /* the form in use: NDTGPU_MATCHER_PER_BATCH or NDTGPU_MATCHER_STREAM_FED */
    uint32_t matcher_groups;  /* current CUs of the matcher side (0: stream-fed and not measured yet) */
    int32_t build_streams;
    int32_t calibrations;     /* how often the split has been measured */
    uint64_t submitted;       /* sub-batches so far */
    double cells_per_map;     /* mean Gaussian cells per map of the sub-batch the split was last measured on */
    int32_t matcher_slots;    /* registrations in flight per workgroup of a matcher instance */
    int32_t resident_groups;  /* workgroups of matcher instances on the device at the time of the call (stream-fed form; a 4-byte
                               * device read on the null stream) */
} ndtgpu_registrar_info;
/* grid: as ndtgpu_mapset_create (grid->max_cells applies per scan). */
ndtgpu_status ndtgpu_registrar_create_ex(const ndtgpu_grid_params *grid, const ndtgpu_registrar_params *params,
                                         ndtgpu_registrar **out);
/* ... with the default parameters but for the two that every caller has to think about */
ndtgpu_status ndtgpu_registrar_create(const ndtgpu_grid_params *grid, size_t pairs_per_batch, int depth,
                                      ndtgpu_registrar **out);
ndtgpu_status ndtgpu_registrar_get_info(const ndtgpu_registrar *reg, ndtgpu_registrar_info *info);
/* TEST AID (stream-fed form): raises the matcher's abort word, as a workgroup that found no work for ~30 s would -- the give-up
 * protocol (results "not run", map sets held until the instances have left, one error from ndtgpu_registrar_sync, a registrar
 * that works again afterwards) is otherwise only reachable by starving the device for half a minute. */
ndtgpu_status ndtgpu_registrar_inject_abort(ndtgpu_registrar *reg);
ndtgpu_status ndtgpu_registrar_destroy(ndtgpu_registrar *reg);
/* n_pairs registrations: pair k builds the target map from cloud k of targets_dev and the source map from cloud k of
 * sources_dev (DEVICE pointers; n_points records each, stride_bytes apart, clouds map_stride_bytes apart; range filter as
 * ndtgpu_mapset_build with the sensor at the frame origin) and runs NDTMatcherD2D::match(target, source, T, prm).
 * T16_dev: DEVICE, n_pairs x 16 doubles column-major, in: initial guess, out: registered pose; results_dev: DEVICE.
 * ASYNCHRONOUS: the inputs must be complete in `stream` order at the time of the call (the library records an event there);
 * the work itself runs on the registrar's own streams, n_pairs > pairs_per_batch in sub-batches on successive streams.
 * The call neither waits for the device nor makes `stream` wait: successive calls overlap (whatever streams they name).
 * *ticket (may be NULL) names the call: its outputs are complete -- and its input and output buffers may be reused -- once
 * ndtgpu_registrar_wait_stream(reg, ticket, s) has made a stream wait for it, or ndtgpu_registrar_sync has returned.  A pair
 * whose map overflowed grid->max_cells reports exit_code -3 like ndtgpu_match_batch_device. */
ndtgpu_status ndtgpu_register_batch_device(ndtgpu_registrar *reg, const void *targets_dev, const void *sources_dev,
                                           size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                           const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                           const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev,
                                           ndtgpu_stream stream, uint64_t *ticket);
/* The same with the scans, the poses and the results in HOST memory -- what the reference's call sites hold (pcl::PointCloud,
 * Eigen::Affine3d).  Sub-batch after sub-batch the clouds are copied to the device under the builds and registrations of the
 * sub-batch before; clouds must not overlap (map_stride_bytes >= n_points * stride_bytes).  Synchronous: returns with T16
 * and results filled in (and everything submitted earlier through the device entry complete). */
ndtgpu_status ndtgpu_register_batch_host(ndtgpu_registrar *reg, const void *targets_host, const void *sources_host,
                                         size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                         const ndtgpu_cell_params *cell, double *T16, size_t n_pairs,
                                         const ndtgpu_match_params *prm, ndtgpu_match_result *results);
/* ndtgpu_register_batch_device + NDTMatcherD2D::covariance(target, source, T, cov) of every pair at its registered pose
 * (ndt_feature_graph.cpp:283-310; ndt_feature_fuser_hmt.cpp:399-413): what the reference's link update produces per link besides
 * the pose (the link covariance cov_3d).  Poses and the deterministic result fields (converged, iterations, fevals, exit_code,
 * score, n_source, n_target, pair_terms_g / _h) are the bits ndtgpu_register_batch_device gives for the same call: the
 * covariance's evaluation is not counted.  covariance_mode: `mode` of ndtgpu_covariance_batch (0 or 1; else NDTGPU_ERR_INVALID),
 * with prm->n_neighbours, lfd1, lfd2.  cov36_dev: DEVICE, n_pairs x 36 doubles, row-major 6x6 over (x, y, z, roll, pitch, yaw) --
 * always the full 6x6, whatever prm->dof_mask is; cov_flags_dev: DEVICE, one NDTGPU_COV_* bit set per pair.  Tickets,
 * ndtgpu_registrar_wait_stream and ndtgpu_registrar_sync cover these outputs as they cover poses and results.
 * How: a registration that is done does not release its slot -- it asks for one more evaluation with the Hessian at the final
 * pose, through the same shares, sums J^T J over its source cells (one target lookup each) and solves
 * H^-1 (0.03^2 J^T J) H^-1 on the solver lane, then writes cov, flags, pose and result together.  Sub-batches that go to the
 * grid-barrier / pool matcher (at most half as many pairs as CUs on 3D sets, max_cells >= 16384) get their covariance from a
 * follow-on ndtgpu_covariance_batch launch on the same stream instead.  Stream-fed form: a running matcher instance is compiled
 * with or without the covariance tail, so a call that switches between this entry and ndtgpu_register_batch_device drains the
 * pipeline first, as a change of n_neighbours does: the host waits for everything submitted, and the next sub-batch's build no
 * longer overlaps the previous sub-batch's registrations -- about one sub-batch of pipeline overlap lost per switch.  Measured
 * (tools/registrar_covariance_cost.py, the bench's workload, 100 steps): 663 k registrations/s with the covariance against
 * 722 k without, +8.9 % per step. */
enum {
    NDTGPU_COV_SINGULAR = 1,       /* the Hessian is singular: cov is all zeros (ndtgpu_covariance_batch's `singular`) */
    NDTGPU_COV_POSE_UNCHANGED = 2, /* the registered pose equals the initial guess bit for bit -- the reference's "NOTHING HAPPENED"
                                    * test (graph.cpp:283-291), after which the graph uses 0.02 I; cov is still the matcher's */
    NDTGPU_COV_NOT_COMPUTED = 4    /* exit_code -2, -3 or -4: the registration did not run; cov is all zeros */
};
ndtgpu_status ndtgpu_register_batch_cov_device(ndtgpu_registrar *reg, const void *targets_dev, const void *sources_dev,
                                               size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                               const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                               const ndtgpu_match_params *prm, ndtgpu_match_result *results_dev,
                                               int covariance_mode, double *cov36_dev, int32_t *cov_flags_dev,
                                               ndtgpu_stream stream, uint64_t *ticket);
/* the same in HOST memory, synchronous like ndtgpu_register_batch_host: cov36 (n_pairs x 36) and cov_flags come back with the poses */
ndtgpu_status ndtgpu_register_batch_cov_host(ndtgpu_registrar *reg, const void *targets_host, const void *sources_host,
                                             size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                             const ndtgpu_cell_params *cell, double *T16, size_t n_pairs,
                                             const ndtgpu_match_params *prm, ndtgpu_match_result *results,
                                             int covariance_mode, double *cov36, int32_t *cov_flags);
/* `stream` waits (on the device, the host does not) for the call `ticket` names and every call before it; ticket 0: for
 * every call submitted so far.  Stream-fed form: the wait is a device-side kernel that ends when the running matcher instance
 * has completed the batch, so `stream` must not share the matcher stream's hardware queue -- a stream created with the HIGHEST
 * priority the device offers is refused (NDTGPU_ERR_INVALID); streams of default priority and the null stream are fine. */
ndtgpu_status ndtgpu_registrar_wait_stream(ndtgpu_registrar *reg, uint64_t ticket, ndtgpu_stream stream);
/* the host waits for every batch submitted so far; NDTGPU_ERR_HIP if a matcher launch gave up (ndtgpu_match_aborted).  In the
 * stream-fed form that is reported once: registrations of the batches that were cut short carry exit_code -4 (every result of a
 * batch is set to "not run" when the batch is published), and the registrar can be used again afterwards. */
ndtgpu_status ndtgpu_registrar_sync(ndtgpu_registrar *reg);
/* Profiling: when enabled every sub-batch's build launch is bracketed by HIP events on the internal stream it runs on, and so
 * is its matcher launch in the per-batch form.  In the stream-fed form there is no launch per batch: mean_ms[1] is then what
 * the queue saw of the batch -- from its publication (maps built) until its last registration finished, on the device's 100 MHz
 * clock -- for the last 64 sub-batches.  ndtgpu_registrar_kernel_ms waits for the recorded sub-batches (stream-fed: for
 * everything submitted), returns their number and the mean durations (mean_ms[0] build, mean_ms[1] matcher side; under a
 * pipeline these include the time the work shares the chip with its neighbours), and forgets them. */
ndtgpu_status ndtgpu_registrar_profiling(ndtgpu_registrar *reg, int on);
ndtgpu_status ndtgpu_registrar_kernel_ms(ndtgpu_registrar *reg, float mean_ms[2], int32_t *launches);
/* the internal map set a sub-batch slot uses (tests: cell-by-cell parity of what the registrar built; slot < depth).  Owned by
 * the registrar. */
ndtgpu_status ndtgpu_registrar_mapset(ndtgpu_registrar *reg, int slot, ndtgpu_mapset **set);

/* ---- the fuser's call as ONE entry: NDTFeatureFuserHMT::update for a batch of independent fusers ---------------------------
 * NDTFeatureFuserHMT::update (ndt_feature/src/ndt_feature_src/ndt_feature_fuser_hmt.cpp:108-512) is, per scan: move the scan
 * into the node map's frame (:186-190), build its NDT map on the node map's lattice (:201-227), matchFusion against the node
 * map with the odometry soft constraint / Tikhonov term / odometry cells (:291-357), the matcher's covariance (:399-413), the
 * consistency gate and the pose update (:415-474), move the raw scan by the new pose and ray-trace it into the node map
 * (:479-486) -- three host-synchronous C-ABI calls (build, match, add_cloud) with host arithmetic in between.  A fuser bank
 * holds B independent fusers (robots, bags, the node fusers of a graph: they share nothing) and does all of it for a range of
 * its slots in ONE asynchronous call: one upload of what the host derives from the odometry increments, then device work only --
 * the pose a registration yields goes into the fuse-in without visiting the host.  Results are bit for bit those of the calls
 * it replaces on the same inputs (tests/test_gpu_fuser_bank.py).
 * Covers the production configuration of the fuser -- globalTransf and loadCentroid (their defaults; the launch files never
 * change them), beHMT / visualisation outside the path.  The FLIRT feature term and the node feature maps
 * (useFeat) are the *_feat entries at the end of this header ("the fuser bank's feature path"); the entries below run without them,
 * also on a bank that has a feature bank attached, and leave its feature state untouched. */
typedef struct ndtgpu_fuser_bank ndtgpu_fuser_bank;
typedef struct {
    /* NDTFeatureFuserHMT::Params (ndt_feature_fuser_hmt.h:58-207): the fields the path reads, same names in snake case */
    double resolution, map_size_x, map_size_y, map_size_z, sensor_range;
    double max_translation_norm, max_rotation_norm;
    int32_t check_consistency, fuse_incomplete;
    int32_t use_odom;              /* the 40 odometry cell pairs (:322-334) join the registration (matchFusion's useFeat) */
    int32_t neighbours, stepcontrol, itr_max;
    double delta_score;
    int32_t force_odom_as_est, fusion2d, all_matches_valid, use_soft_constraints, compute_cov, step_control_fusion, use_tikhonov;
    int32_t covariance_mode;       /* `mode` of ndtgpu_covariance_batch */
    int32_t discard_cells;         /* the scan map's cells that hold the scan's first and last point lose their Gaussian (:229-232) */
    int32_t pad_;
    /* MotionModel2d::Params (motion_model.hpp:123-136) */
    double motion_Cd, motion_Ct, motion_Dd, motion_Dt, motion_Td, motion_Tt;
    double sensor_pose[16];        /* setSensorPose: column-major like every pose of this header */
    uint32_t max_cells;            /* cell capacity of the node and scan maps (ndtgpu_grid_params.max_cells) */
} ndtgpu_fuser_params;
void ndtgpu_default_fuser_params(ndtgpu_fuser_params *p);   /* Params() and MotionModel2d::Params() of the reference, sensor at the origin */
/* What the host derives from (current pose, odometry increment) before the device takes over -- a pure function, exposed so
 * that a caller (or a test) can drive the three separate calls with exactly the inputs the bank uses. */
typedef struct {
    double Tscan[16];            /* Tinit * sensor_pose: raw scan -> node map frame (:186-190) */
    double scan_centre[3];       /* loadPointCloudCentroid's grid centre (:201-202) */
    double range_origin[3];      /* the sensor position the range limit is measured from */
    double Tcov[36];             /* TmotionCov, row-major (:137-146) */
    double odom_cov[9];          /* covariance of the odometry cells (:127-130) */
    double feat_src_mean[3];     /* the 40 correspondences of ndtgpu_match_fusion_feat_batch: source cell i ... */
    double feat_tgt_mean[3];     /* ... target cell i, */
    double feat_cov_rotated[6];  /* the covariance of all of them (xx xy xz yy yz zz) */
    double feat_cov_plain[6];    /* but the LAST source cell, which keeps the un-rotated one (:336-339) */
} ndtgpu_fuser_prepared;
ndtgpu_status ndtgpu_fuser_prepare(const ndtgpu_fuser_params *prm, const double Tnow16[16], const double Tmotion16[16],
                                   const double node_centre[3], ndtgpu_fuser_prepared *out);
typedef struct {
    double Tnow[16];             /* the fuser's pose after the update: what update() returns */
    double Tmotion_est[16];      /* the registered increment */
    double spose[16];            /* Tnow * sensor_pose: the frame the raw scan was fused in at */
    ndtgpu_match_result match;
    int32_t match_ok;            /* converged, or fuseIncomplete / allMatchesValid */
    int32_t registration_failure;/* the consistency gate fired: the pose is the odometry's */
    int32_t cov_singular, pad_;
    double posecov_mean[3];      /* current_posecov */
    double posecov[9];           /* column-major 3x3 */
} ndtgpu_fuser_result;
/* node_maps: the map set whose maps [0, n_fusers) are the fusers' node maps (a graph's pool: the caller keeps ownership), or
 * NULL: the bank makes its own with prm's map sizes.  Enables occupancy on it. */
ndtgpu_status ndtgpu_fuser_bank_create(const ndtgpu_fuser_params *prm, size_t n_fusers, ndtgpu_mapset *node_maps,
                                       ndtgpu_fuser_bank **out);
ndtgpu_status ndtgpu_fuser_bank_destroy(ndtgpu_fuser_bank *bank);
/* the node maps and the scan maps of the last update (borrowed) */
ndtgpu_status ndtgpu_fuser_bank_mapsets(ndtgpu_fuser_bank *bank, ndtgpu_mapset **node_maps, ndtgpu_mapset **scan_maps);
/* NDTFeatureFuserHMT::initialize(initPos, cloud, ...) (:65-102) for slots [first, first + count): pose initPose16[k] (HOST), the
 * node map centred on it, the first cloud (DEVICE, sensor frame; n_points records `stride_bytes` apart, clouds
 * `map_stride_bytes` apart) ray-traced in.  Asynchronous on `stream`. */
ndtgpu_status ndtgpu_fuser_initialize_batch(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *initPose16,
                                            const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                            ndtgpu_stream stream);
/* NDTFeatureFuserHMT::update(Tmotion, cloud, pts, updateFeatureMap, updateNDTMap) for slots [first, first + count): Tmotion16
 * HOST (count x 16), clouds DEVICE in the sensor frame.  Asynchronous on `stream`; a call waits (on the host) for the bank's
 * previous call first: it starts from the poses that one left.  Scans of unequal length: pad with NaN points. */
ndtgpu_status ndtgpu_fuser_update_batch(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *Tmotion16,
                                        const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                        int update_ndt_map, ndtgpu_stream stream);
/* the same with the clouds in HOST memory (pcl::PointCloud: 16-byte records), copied to the device on a stream of the bank's own;
 * asynchronous once the caller's memory has been read */
ndtgpu_status ndtgpu_fuser_initialize_batch_host(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *initPose16,
                                                 const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes);
ndtgpu_status ndtgpu_fuser_update_batch_host(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *Tmotion16,
                                             const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                             int update_ndt_map);
/* waits for the bank's last call; Tnow16: HOST, count x 16; results (may be NULL): the records of the last update call for the
 * slots it covered, zeroes for the others */
ndtgpu_status ndtgpu_fuser_poses(ndtgpu_fuser_bank *bank, size_t first, size_t count, double *Tnow16, ndtgpu_fuser_result *results);

/* ---- coarse to fine: multi-resolution D2D registration of raw scan pairs ----------------------------------------------------
 * NDTMatcherD2D(isIrregularGrid, useDefaultGridResolutions, resolutions).match(target_pc, source_pc, T, useInitialGuess), the
 * raw-cloud overload (ndt_feature/src/ndt_odom_debug.cpp:159-165: matcher.match(static_pc, moving_pc, T_p2p, true);
 * ndt_feature/src/ndt_feature_pcl_eval.cpp:620-642: matcher.match(moving_pc, static_pc, T_p2p)).
 * PROVENANCE: the body lives in perception_oru (ndt_registration/src/ndt_matcher_d2d.cpp), which the reference does not vendor;
 * restated from memory:
 *   - useDefaultGridResolutions: the list is {0.2, 0.5, 1, 2} (ndtgpu_default_resolutions); else the caller's.  isIrregularGrid
 *     (OctTree maps) has no counterpart here.
 *   - useInitialGuess: the source cloud is moved by T (transformPointCloudInPlace: a double-precision product, stored back as
 *     float) and Tinit = T; else Tinit = I.  Then T = I.
 *   - for r = n_levels - 1 down to 0 -- in LIST order, the list is not sorted: build the target map and the source map (from the
 *     moved cloud) on a fresh LazyGrid(resolutions[r]); Temp = I; ret = match(targetNDT, sourceNDT, Temp) (the map overload,
 *     from the identity); move the source cloud by Temp, again rounded to float; T = Temp * T.
 *   - finally T = T * Tinit; the call returns the last level's ret.
 *   - n_neighbours, ITR_MAX, DELTA_SCORE, lfd1 / lfd2 and step_control are the same at every level (DELTA_SCORE is not rescaled).
 * DEVIATION: upstream's un-sized LazyGrid centres each map on the centroid of its cloud (guess_size_).  Here every map of a level
 * sits on the caller's grid -- ndtgpu_grid_params' centre and size, with res replaced by the level's cell size -- as the
 * registrar places its maps.  grid->res is ignored.
 * range_limit <= 0: no range filter (upstream's overload).  A positive value filters each RAW scan around its own origin
 * (NDTMap::loadPointCloud's test), the source before it is moved.
 * Outputs: T16 the final T; results[k * n_levels + j] the result of pair k at list position j.  A level that does not run stops
 * its pair -- a map over max_cells (exit_code -3), or a grid barrier that gave up (-4): every level after it is not run either
 * and reports the same exit_code, T16 gets the levels that did complete times Tinit.
 * Work per sub-batch of pairs_per_batch pairs, in turn, asynchronous on `stream`; a call's work waits (on the device) for the
 * previous call on the same handle, whatever stream that one named -- the handle's map sets and buffers are reused.  The target maps of
 * a level are built with the library's build kernels; the source build moves each cloud on load (an instance of the flat-grid
 * kernel, ndt_build_flat_kernel<SD, true>, with a per-map rigid transform that is uniform per workgroup, which also writes the
 * moved cloud for the next level; levels whose build ndtgpu_mapset_build would not give to the flat kernel -- max_cells <= 4096,
 * even cell counts, fp32 cell centres, and >= 256 maps per sub-batch unless NDTGPU_FLAT=2 -- ndt_cloud_transform_kernel, then
 * ndtgpu_mapset_build's own choice of kernel: the maps are those ndtgpu_mapset_build makes of the moved clouds, bit for bit,
 * either way); the matcher runs in the per-batch
 * form of ndtgpu_match_batch_device; a small kernel composes the poses between levels.  Each level has its own pair of
 * internal map sets (2 x pairs_per_batch maps).  Environment NDTGPU_MR_FUSED=0 (read per call): never the fused source build
 * (A/B measurements, tools/multires_cost.py).  Measured there on MI355X (1024 pairs x 100 k points, the bench's 2D scenes,
 * max_cells 4096): 84 k registrations/s with the default list (the 0.2 m match is 10.7 of 12.2 ms), 108 k with {0.5, 1, 2, 4};
 * fused source builds 12.2 / 9.45 ms per call against 12.4 / 9.67 ms for a separate move plus build.  (Holding the transform
 * costs the fused instances register room: 13 VGPR and 111-113 SGPR spills, 56 bytes of scratch, against 11, 52-60 and 48 for the
 * plain build.)  ndtgpu_multires_get_info counts the source builds of each kind. */
typedef struct ndtgpu_multires ndtgpu_multires;
#define NDTGPU_MAX_LEVELS 8
void ndtgpu_default_resolutions(double res[4], int *n_levels);    /* {0.2, 0.5, 1, 2}, 4 */
/* n_levels in 1 .. NDTGPU_MAX_LEVELS and every resolution > 0, else NDTGPU_ERR_INVALID */
ndtgpu_status ndtgpu_multires_create(const ndtgpu_grid_params *grid, const double *resolutions, int n_levels,
                                     size_t pairs_per_batch, ndtgpu_multires **out);
ndtgpu_status ndtgpu_multires_destroy(ndtgpu_multires *mr);
/* targets_dev / sources_dev: DEVICE clouds as ndtgpu_register_batch_device takes them; T16_dev: DEVICE n_pairs x 16 (in: the
 * initial guess when use_initial_guess, out: the registered pose); results_dev: DEVICE n_pairs x n_levels.  prm's
 * use_initial_guess is not read (the argument decides; every level matches from the identity).  Asynchronous on `stream`. */
ndtgpu_status ndtgpu_register_multires_device(ndtgpu_multires *mr, const void *targets_dev, const void *sources_dev,
                                              size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                              const ndtgpu_cell_params *cell, double *T16_dev, size_t n_pairs,
                                              const ndtgpu_match_params *prm, int use_initial_guess,
                                              ndtgpu_match_result *results_dev, ndtgpu_stream stream);
typedef struct {
    int32_t n_levels;
    size_t pairs_per_batch;
    uint64_t levels_fused;     /* source builds so far that moved the clouds on load (one per sub-batch and level) */
    uint64_t levels_unfused;   /* ... and that moved them first (ndt_cloud_transform_kernel), then built */
} ndtgpu_multires_info;
ndtgpu_status ndtgpu_multires_get_info(const ndtgpu_multires *mr, ndtgpu_multires_info *info);
/* the same with clouds, poses and results in HOST memory; synchronous */
ndtgpu_status ndtgpu_register_multires_host(ndtgpu_multires *mr, const void *targets_host, const void *sources_host,
                                            size_t n_points, size_t stride_bytes, size_t map_stride_bytes, double range_limit,
                                            const ndtgpu_cell_params *cell, double *T16, size_t n_pairs,
                                            const ndtgpu_match_params *prm, int use_initial_guess,
                                            ndtgpu_match_result *results);

/* ---- NDT Monte Carlo localisation in a built map: a bank of NDTMCL3D particle filters ----------------------------------------
 * ndt_feature/src/ndt_feature_mcl_node.cpp localises a robot in a saved NDT map with perception_oru's NDTMCL3D (:48 includes
 * ndt_mcl/3d_ndt_mcl.h; :174 `new NDTMCL3D(resolution, ndmap, -5)`; :175-184 its public parameters; :335 initializeFilter(x, y,
 * z, r, p, t, 0.5, 0.5, 0.1, 2 deg, 2 deg, 2 deg, numParticles); :361 updateAndPredictEff(Tm, cloud, subsample_level) per
 * odometry step; :377-396 reads pf.pcloud[i], pf.size() and pf.getMean()).  A bank holds n_filters independent filters of
 * n_particles particles each (robots, bags, hypotheses); filter k localises in map map_idx[k] of a BORROWED map set.
 * PROVENANCE: NDTMCL3D and mcl::ParticleFilter3D live in perception_oru's ndt_mcl, which the reference does not vendor;
 * restated from memory:
 *   - constructor: the map at map_resolution, zfilt_min = zfilter, resolution_sensor = map_resolution, sinceSIR = 0.
 *   - initializeFilter: N particles T = Translation(x + sx n1, y + sy n2, z + sz n3) * AngleAxis(r + sr n4, X) *
 *     AngleAxis(p + sp n5, Y) * AngleAxis(t + st n6, Z) (n standard normal), every weight p = 1/N.
 *   - updateAndPredictEff(Tmotion, cloud, subsample_level):
 *     1. subsample_level outside [0, 1] becomes 1.
 *     2. the local map: NDTMap(new LazyGrid(resolution_sensor)), guessSize(0,0,0, 100,100,8), loadPointCloud(cloud),
 *        computeNDTCells(SAMPLE_VARIANCE) -- the cloud in the base frame (the node applies sensorPoseT first, :357).
 *     3. tr = Tmotion.translation(), rot = Tmotion.rotation().eulerAngles(0,1,2) (Eigen: first angle in [0, pi]),
 *        sigma = motion_model * (|tr|, |rot|) + motion_model_offset.
 *     4. predict: T <- T * (Translation(tr + sigma[0..2] n) * AngleAxis(rot0 + sigma3 n, X) * AngleAxis(rot1 + sigma4 n, Y) *
 *        AngleAxis(rot2 + sigma5 n, Z)).
 *     5. the local map's Gaussian cells; when subsample_level < 1 each is kept with probability subsample_level (the same cells
 *        for every particle of the filter).
 *     6. per particle lik = sum over kept cells c of 0.1 + 0.9 exp(-0.05 l / 2), l = (mu - m)^T (C + R c.cov R^T)^-1 (mu - m),
 *        m = T c.mean, (mu, C) the map cell at pcl::PointXYZ(m) (float coordinates); a cell is skipped when m.z < zfilt_min,
 *        when m falls outside the grid or in a cell without a Gaussian, when computeInverseAndDetWithCheck fails
 *        (|det| <= 1e-12), or when l is not finite.
 *     7. pf.normalize(): p_i <- p_i lik_i, then p_i /= sum p; when sum p <= 0 every p_i = 1/N.
 *     8. forceSIR: SIRUpdate().  Else varP = sqrt(sum (p_i - 1/N)^2 / N); varP > SIR_varP_threshold or sinceSIR >
 *        SIR_max_iters_wo_resampling: SIRUpdate(), sinceSIR = 0; else sinceSIR++.  SIRUpdate is systematic (low-variance)
 *        resampling with one uniform offset; afterwards every p = 1/N.
 *   - pf.getMean(): translation sum p_i t_i; rotation AngleAxis(atan2(sum p sin r, sum p cos r), X) * (.. Y) * (.. Z) over
 *     each particle's T.rotation().eulerAngles(0,1,2).
 * DEVIATIONS:
 *   - random numbers: a counter-based generator -- synth.hash_uniform / hash_normal (SplitMix64, Box-Muller) keyed by (seed,
 *     filter slot, the filter's draw counter, particle or cell, draw index); a filter's draws do not depend on the batch it runs
 *     in.  Upstream uses rand() (srand(time(NULL))).  The draw counter counts the filter's initialize and update calls.  SIR's
 *     thresholds are (u0 + k) / N with one u0 ~ U[0, 1) per update.
 *   - the map is read in place, not copied into a LazyGrid of the filter's resolution: ndtgpu_mcl_create refuses a map set whose
 *     cell size differs from params->map_res (NDTGPU_ERR_INVALID).
 *   - resampling sums: cumulative weights are exact 64-bit fixed-point sums (units of 2^-52), so resampling is order-free.
 *   - updateAndPredict (the non-Eff variant) and the OctTree are not ported.
 * Calls on one handle are ordered (each waits, on the device, for the previous one, whatever stream that one named); the
 * borrowed map set is read by the update's likelihood kernel: the caller orders any rebuild of it before or after an update,
 * as for the matcher.  Scans of unequal length: pad with NaN points. */
typedef struct ndtgpu_mcl ndtgpu_mcl;
typedef struct {
    double map_res;                      /* NDTMCL3D(map_resolution, ..) (:174 `resolution`); 0 = the map set's cell size */
    double sensor_res;                   /* resolution_sensor of the local scan map (= map_resolution upstream); 0 = map_res */
    double scan_size[3];                 /* local map extent guessSize(0,0,0, 100,100,8) [m] (recalled); every 2D scan is served by
                                          * a planar extent, e.g. {60, 60, 1}: 100 x 100 x 8 m costs 40 MB of build scratch per
                                          * filter at 0.2 m */
    double range_limit;                  /* loadPointCloud's range limit; <= 0: none (recalled: upstream passes none) */
    double zfilt_min;                    /* NDTMCL3D(.., zfilter) (:174: -5) */
    double motion_model[36];             /* row-major 6x6 (:183 getParam("motion_model"); defaults recalled) */
    double motion_model_offset[6];       /* (:184 getParam("motion_model_offset"); defaults recalled) */
    int32_t force_sir;                   /* forceSIR (:175-176, default false) */
    int32_t sir_max_iters_wo_resampling; /* SIR_max_iters_wo_resampling (:179, 25) */
    double sir_varp_threshold;           /* SIR_varP_threshold (:178, 0.006) */
    uint32_t max_scan_cells;             /* cell capacity of each local scan map (ndtgpu_grid_params.max_cells; 0 = default) */
    uint32_t pad_;
    uint64_t seed;                       /* the random-number key (see DEVIATIONS) */
} ndtgpu_mcl_params;
void ndtgpu_default_mcl_params(ndtgpu_mcl_params *p);
typedef struct {
    double var_p;            /* varP of the last update (computed also when force_sir) */
    double lik_sum;          /* sum of the particles' lik */
    int64_t terms;           /* (particle, scan cell) terms scored */
    uint64_t draws;          /* the filter's draw counter (initialize and update calls so far) */
    int32_t resampled;       /* the last update ran SIRUpdate */
    int32_t since_sir;       /* sinceSIR after it */
    int32_t n_scan_cells;    /* Gaussian cells of the local scan map */
    int32_t overflow;        /* the local scan map needed more than max_scan_cells cells (the rest were not scored) */
} ndtgpu_mcl_result;
/* n_particles 1 .. 65536 per filter, n_filters * n_particles <= 2^24; map_idx: HOST, n_filters map indices of map_set */
ndtgpu_status ndtgpu_mcl_create(ndtgpu_mapset *map_set, const uint32_t *map_idx, const ndtgpu_mcl_params *params, size_t n_filters,
                                size_t n_particles, ndtgpu_mcl **out);
ndtgpu_status ndtgpu_mcl_destroy(ndtgpu_mcl *h);
/* initializeFilter for filters [first, first + count): pose6 / sigma6 HOST, count x (x, y, z, r, p, t).  Synchronous. */
ndtgpu_status ndtgpu_mcl_initialize(ndtgpu_mcl *h, size_t first, size_t count, const double *pose6, const double *sigma6);
/* installs particle sets (pf.pcloud[i].T / .p): T16 HOST count x n_particles x 16 (column-major), weights HOST count x n_particles
 * (NULL: 1/N).  Synchronous. */
ndtgpu_status ndtgpu_mcl_set_particles(ndtgpu_mcl *h, size_t first, size_t count, const double *T16, const double *weights);
/* updateAndPredictEff(Tmotion, cloud, subsample_level) for filters [first, first + count): Tmotion16 HOST count x 16; clouds
 * DEVICE, n_points records `stride_bytes` apart, clouds `map_stride_bytes` apart (base frame).  subsample_level is a per-call
 * argument as upstream's is.  Asynchronous on `stream`: local-map build, predict, likelihood, normalise and SIR, no host
 * synchronisation. */
ndtgpu_status ndtgpu_mcl_update(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, double subsample_level,
                                const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                ndtgpu_stream stream);
/* the same with the clouds in HOST memory; synchronous */
ndtgpu_status ndtgpu_mcl_update_host(ndtgpu_mcl *h, size_t first, size_t count, const double *Tmotion16, double subsample_level,
                                     const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes);
/* pf.pcloud after the handle's last call: T16 count x n_particles x 16, weights and lik count x n_particles (HOST; any may be
 * NULL; lik: the last update's likelihoods).  Waits for the handle. */
ndtgpu_status ndtgpu_mcl_particles(ndtgpu_mcl *h, size_t first, size_t count, double *T16, double *weights, double *lik);
/* pf.getMean() of filters [first, first + count): T16_mean HOST count x 16; results (may be NULL) the records of each filter's
 * last update.  Waits for the handle. */
ndtgpu_status ndtgpu_mcl_mean(ndtgpu_mcl *h, size_t first, size_t count, double *T16_mean, ndtgpu_mcl_result *results);

/* ---- SE(2) pose-graph optimisation of registered links: a bank of graphs ---------------------------------------------------
 * The offline mapper (ndt_feature/src/ndt_feature_graph_opt.cpp) ends in :147 graph.force2D() and the loop :152-164 --
 * clearAllLinks, appendLinks(incremental_links), getValidLinks, appendLinks(links), optimizeGraphUsingISAM(graph) -- whose last
 * call (ndt_offline_mapper.h:40-107) turns the links into node poses with iSAM.  ndtgpu_pgo_* is that call for a bank of
 * n_graphs independent graphs (the same nodes under several getValidLinks thresholds, several robots or bags, the replay's
 * 5000 nodes), and it takes the registrar's poses and covariances where they are, in device memory.
 * Semantics (restated):
 *   - a graph has n_nodes unknowns p_i = (x, y, t).  Poses enter as (x, y, yaw) with yaw = getRobustYawFromAffine3d
 *     (utils.h:30-40; convertEigenAffine3dToIsamPose2d, ndt_offline_mapper.h:8-15) and leave the same way; T16_out is
 *     convertIsamPose2dToEigenAffine3d (ndt_offline_mapper.h:17-26): Translation(x, y, 0) * Rz(t).
 *   - the prior (Pose2d_Factor, :61) acts on node 0: e = p_0 - origin, the angle wrapped to (-pi, pi]; origin is node 0's pose
 *     when the graph is set (:59).
 *   - each link (ref, mov, z) (Pose2d_Pose2d_Factor, :79, :90): e = (p_mov ominus p_ref) - z, the angle wrapped, with
 *     ominus = (c dx + s dy, -s dx + c dy, wrap(t_mov - t_ref)), c / s the cosine / sine of t_ref, (dx, dy) the translation
 *     difference (Pose2d::ominus).
 *   - the cost is sum e^T W e, W an information matrix per factor (its symmetric part is used); W = NULL is 100 * I3, which is
 *     what :45, :61, :79 and :90 give every factor.
 *   - slam.batch_optimization() (:97) is Gauss-Newton on this cost, iSAM's default method; after each step the angles are
 *     wrapped to (-pi, pi].  The Jacobians here are analytic.
 * PROVENANCE: iSAM (isam/isam.h) is not vendored by the reference; the factors' errors and the batch method are restated from
 * memory.
 * DEVIATIONS:
 *   - the stop rule and its defaults are OURS and explicit (ndtgpu_pgo_params), not iSAM's: stop when the largest absolute
 *     component of a Gauss-Newton update is <= eps_step, or after max_iterations updates.
 *   - each linear system is solved by conjugate gradients preconditioned with the inverses of the 3x3 diagonal blocks, from
 *     zero, to the relative residual eps_linear or max_linear_iterations -- not by sparse QR.  A solve that stops at the cap
 *     still gives its iterate as the step.
 *   - upstream adds every link with score < 0 twice (:74-82 and again in :86-93).  The entries here take an edge list as
 *     given; the host mirror's optimizeGraphUsingISAM (host/ndt_feature_graph_gpu.h) reproduces the doubling.
 * Device form (csrc/ndt_pgo.hip, ndt_pgo_kernel): one workgroup of 1024 threads optimises one graph from start to finish, `count`
 * graphs are `count` workgroups of one launch.  Nothing but the workgroup barrier orders its passes: no grid barrier, no queue,
 * no spin on memory, no atomics; every sum has one fixed order, so a graph's poses and result are the same bits whichever
 * batch it runs in, whatever first / count are.  The multi-workgroup form for ONE large graph is ndtgpu_pgo_optimize_wide
 * (the section below).
 * Measured on MI355X (tools/pgo_cost.py; grid-world graphs of 0.5 m cells, start 0.2 m / 0.1 rad off, defaults): 500 nodes and
 * 1886 links: 5 updates, 1082 inner iterations, 13.8 ms; 256 such graphs in one launch: 25.8 ms (0.10 ms per graph; 5-6 updates,
 * at most 1306 inner iterations); the replay's size, 5000 nodes and 43.5 k links: 5 updates, 2506 inner iterations, 740 ms,
 * converged -- no inner solve reached max_linear_iterations.  The NumPy model (dense solve) takes 0.18 s at 500 nodes on one
 * core. */
typedef struct ndtgpu_pgo ndtgpu_pgo;
typedef struct {
    int32_t max_iterations;          /* Gauss-Newton updates at most (ours: 50) */
    int32_t max_linear_iterations;   /* conjugate-gradient iterations per update at most (ours: 2000) */
    double eps_step;                 /* stop when the largest |component| of the update is <= this (ours: 1e-8; m and rad) */
    double eps_linear;               /* the inner solve's relative residual |r| / |b| (ours: 1e-8) */
    double prior_information[9];     /* the prior's W, row-major (100 * I3: ndt_offline_mapper.h:45, :61) */
} ndtgpu_pgo_params;
/* the defaults above: max_iterations, max_linear_iterations, eps_step and eps_linear are OURS, not iSAM's */
void ndtgpu_default_pgo_params(ndtgpu_pgo_params *p);
enum {
    NDTGPU_PGO_CONVERGED = 0,        /* the last update was within eps_step */
    NDTGPU_PGO_MAX_ITERATIONS = 1,   /* max_iterations updates without meeting eps_step */
    NDTGPU_PGO_LINEAR_CAP = 2,       /* in place of 0 or 1: an inner solve of the run stopped at max_linear_iterations */
    NDTGPU_PGO_NOT_FINITE = 3        /* an input or the cost is not finite: the poses are the last iterate with a finite cost
                                      * (the poses as set where the input is at fault) */
};
typedef struct {
    int32_t exit_code;               /* NDTGPU_PGO_* */
    int32_t iterations;              /* Gauss-Newton updates taken */
    int32_t linear_iterations;       /* conjugate-gradient iterations, all updates together */
    int32_t pad_;
    double cost_initial;             /* sum e^T W e at the poses as set */
    double cost_final;               /* ... at the poses returned */
    double max_step;                 /* the largest |component| of the last update */
    int32_t n_nodes;
    int32_t n_edges;
} ndtgpu_pgo_result;
/* room for n_graphs graphs of up to max_nodes nodes and max_edges links each (n_graphs, max_nodes >= 1; max_nodes <= 2^24,
 * max_edges <= 2^27) */
ndtgpu_status ndtgpu_pgo_create(size_t n_graphs, size_t max_nodes, size_t max_edges, ndtgpu_pgo **out);
ndtgpu_status ndtgpu_pgo_destroy(ndtgpu_pgo *h);
/* installs graph g.  All arrays HOST: pose3 n_nodes x (x, y, yaw), node 0's is the prior's origin; ref_idx / mov_idx n_edges
 * node indices; meas3 n_edges x (x, y, yaw); info9 n_edges x 9 row-major or NULL (100 * I3 for every link).
 * NDTGPU_ERR_INVALID -- checked before the handle is read and the device is looked for -- where an index is out of range, where
 * ref == mov, and where a node is not connected to node 0 (union-find on the host): such a node would make the system
 * singular.  The node-to-edge adjacency (CSR, ascending edge order) is built here.  Synchronous. */
ndtgpu_status ndtgpu_pgo_set_graph(ndtgpu_pgo *h, size_t g, size_t n_nodes, const double *pose3, size_t n_edges,
                                   const uint32_t *ref_idx, const uint32_t *mov_idx, const double *meas3, const double *info9);
/* the same with the links where ndtgpu_register_batch_cov_device left them: pose3, ref_idx, mov_idx HOST; T16_dev (n_edges x 16,
 * column-major), cov36_dev (n_edges x 36) and cov_flags_dev (n_edges) DEVICE and complete when the call is made (after
 * ndtgpu_registrar_sync, or ordered by the caller's own means).  A small kernel (ndt_pgo_links_kernel) turns each T16 into
 * (x, y, robust yaw) and inverts the (x, y, yaw) block of cov36 -- rows / columns 0, 1, 5, its symmetric part -- into the link's
 * information; the covariance 0.02 * I3 stands in where the flags say NDTGPU_COV_SINGULAR, NDTGPU_COV_POSE_UNCHANGED or
 * NDTGPU_COV_NOT_COMPUTED (the reference does the same after "NOTHING HAPPENED", ndt_feature_graph.cpp:283-310) and where the
 * block does not invert (not positive definite, or an inverse that is not finite).  cov36_dev == NULL gives every link
 * 100 * I3 (cov_flags_dev is then not read).  No link value visits the host.  Returns when the kernel has run. */
ndtgpu_status ndtgpu_pgo_set_links_device(ndtgpu_pgo *h, size_t g, size_t n_nodes, const double *pose3, size_t n_edges,
                                          const uint32_t *ref_idx, const uint32_t *mov_idx, const double *T16_dev,
                                          const double *cov36_dev, const int32_t *cov_flags_dev);
/* optimises graphs [first, first + count), each of which has been set, in ONE launch, asynchronous on `stream`; prm NULL: the
 * defaults.  Calls on one handle are ordered (each waits, on the device, for the previous one, whatever stream that one named).
 * A graph that ends with NDTGPU_PGO_NOT_FINITE does not fail the call or touch the other graphs. */
ndtgpu_status ndtgpu_pgo_optimize(ndtgpu_pgo *h, size_t first, size_t count, const ndtgpu_pgo_params *prm, ndtgpu_stream stream);
/* graph g's poses: pose3_out HOST n_nodes x (x, y, yaw); T16_out HOST n_nodes x 16 column-major or NULL; result may be NULL.
 * Waits for the handle. */
ndtgpu_status ndtgpu_pgo_poses(ndtgpu_pgo *h, size_t g, double *pose3_out, double *T16_out, ndtgpu_pgo_result *result);

/* ---- the chip-wide form of the optimiser: ONE large graph spread over the device ---------------------------------------------
 * ndtgpu_pgo_optimize gives a graph to one workgroup, which is right for a bank of small graphs and leaves the rest of the chip
 * idle for the one large graph the offline mapper's loop (ndt_feature_graph_opt.cpp:152-173) optimises once per round.
 * ndtgpu_pgo_optimize_wide optimises graph g of a bank alone with the same algorithm, operation for operation -- linearisation per
 * link, gather and 3x3 block inverse per node, block-Jacobi preconditioned conjugate gradients from zero with the same break
 * rules, the wrapped pose update with the roll-back to the last finite iterate, the same stop rule and exit codes -- so
 * ndtgpu_pgo_poses and ndtgpu_pgo_result mean the same, field for field; linear_iterations counts the inner iterations TAKEN,
 * never the launches enqueued.
 * Launch structure (csrc/ndt_pgo_wide.hip): a lane per link or per node over a grid of ceil(n / 256) workgroups, ONE PLAIN LAUNCH
 * PER PASS on `stream`; the boundary between two launches is the only synchronisation: no grid barrier, no cooperative launch, no
 * workgroup that waits for another, no spin on memory, no atomics, no captured graph.  Per Gauss-Newton update: one launch that
 * gathers and starts the solve; THREE launches per inner iteration (a link pass that forms p = z + beta p of its two end nodes
 * on the fly, a node pass that stores it and gathers A p, a node pass for alpha, x, r and z); then the pose update, the
 * linearisation and the cost assessment.  The run's scalars travel in a control block in device memory, two copies of which a
 * launch reads one and writes the other, so no word is written by a launch in which a workgroup reads it; every launch begins by
 * reading it and does nothing where its phase is over.
 * The host steers the phases: it enqueues check_every inner iterations at a time, then copies the control block to pinned
 * memory and waits for it (also after every cost assessment).  That is why the call is SYNCHRONOUS TOWARDS THE HOST: it returns
 * when the graph is done -- only the host can decide how many more launches to enqueue.  Launches enqueued past a stop do nothing.
 * Summation rule: items are cut into tiles of 256 consecutive items (ndtgpu_pgo_wide_plan), a tile's sum is taken by its
 * workgroup in the order of csrc/ndt_block.h and stored per tile; every workgroup that needs the graph's sum adds the per-tile
 * sums in one fixed order (thread t takes t, t + 256, ... ascending, then the workgroup sum).  A node's incident links are summed
 * in ascending link order by one lane.  The tiling follows the graph's n_nodes and n_edges alone: a graph's poses and result are
 * the same bits for every check_every, whatever the bank's capacity, whatever the other graphs of the bank hold, and from run
 * to run.  They are NOT the bits of ndtgpu_pgo_optimize, which adds in another order (a thread's strided items, 1024 threads):
 * the two forms agree to rounding (tests/test_gpu_pgo_wide.py: both within ten times the model's own floor of the NumPy model).
 * Two more device buffers (the per-tile sums and the control blocks, with a pinned mirror) are allocated by a handle's first
 * wide call and released by ndtgpu_pgo_destroy.
 * Measured on MI355X (tools/pgo_cost.py --wide; the graphs and defaults of the section above; one-workgroup form by device
 * events, wide form by host wall time round the synchronous call, median of the repeats after a warm-up):
 *   nodes / links   updates / inner iterations   one workgroup          wide, check_every 8 / 32 / 128        wide per inner iteration
 *   500 / 1886      5 / 1082                    13.5 ms (12.5 us each)  18.6 / 17.0 / 17.7 ms  (0.80 x)       15.7 us
 *   1500 / 8575     6 / 1965                    93.9 ms (47.8 us each)  40.9 / 37.8 / 36.2 ms  (2.5 x)        19.2 us
 *   5000 / 43 509   5 / 2506                    740 ms  (295 us each)   64.1 / 59.2 / 58.0 ms  (12.5 x)       23.6 us
 * (ratios at the default check_every, 32; every run converged, both forms took the same updates and inner iterations).  The
 * forms cross between 500 and 1500 nodes: BELOW SOME 600 NODES (2.5 k links) ndtgpu_pgo_optimize IS THE ONE TO CALL -- and always
 * for a bank of graphs, which it fills the chip with -- above it the wide form.  At the replay's size the device, not the host,
 * sets the pace: the three launches of an inner iteration run 5.0 + 14.0 + 4.9 us (link, node, step: rocprofv3 --kernel-trace);
 * the node pass gathers some 17 links per lane from 20 workgroups.  Kernels (tools/kernel_resources.py pgo_wide): 18 to 74
 * VGPRs, no spills, no scratch, 128 B of LDS each. */
typedef struct {
    int32_t check_every;             /* inner iterations enqueued between two looks at the control block (ours: 32; >= 1) */
    int32_t pad_;
} ndtgpu_pgo_wide_params;
void ndtgpu_default_pgo_wide_params(ndtgpu_pgo_wide_params *p);
/* pure host: the tile (256), the node and link tiles of a graph of this size and the extra device bytes the wide form needs for
 * it (a handle allocates them for its capacity).  NDTGPU_ERR_INVALID beyond ndtgpu_pgo_create's limits (n_nodes 1 .. 2^24,
 * n_edges <= 2^27).  Any out pointer may be NULL. */
ndtgpu_status ndtgpu_pgo_wide_plan(size_t n_nodes, size_t n_edges, uint32_t *tile, size_t *node_tiles, size_t *edge_tiles,
                                   size_t *extra_bytes);
/* graph g alone, spread over the device; launches on `stream`; RETURNS WHEN THE GRAPH IS DONE (the host steers the phases).
 * prm / wide NULL: the defaults.  The parameter checks of ndtgpu_pgo_optimize and check_every >= 1, made before the handle is
 * read and the device is looked for.  Calls on one handle stay ordered, whichever form and stream they name.  A graph that ends
 * with NDTGPU_PGO_NOT_FINITE does not fail the call. */
ndtgpu_status ndtgpu_pgo_optimize_wide(ndtgpu_pgo *h, size_t g, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_wide_params *wide,
                                       ndtgpu_stream stream);

/* ---- SE(3) pose-graph optimisation of 6-DoF links: a bank of graphs ------------------------------------------------------------
 * Every registration of the library leaves a full pose T16 and a 6x6 covariance cov36 (link.cov_3d, ndt_feature_graph.cpp:296-330,
 * ndt_feature_link.h:27); the reference calls graph.force2D() (ndt_feature_graph_opt.cpp:147) before its only optimiser, and
 * ndtgpu_pgo_* above follows it.  ndtgpu_pgo3_* is the back end of the 3D half: it turns 6-DoF links into node poses that
 * ndtgpu_world_assemble takes as they are.  It is the SE(2) bank's algorithm with 6x6 blocks in place of 3x3.
 * Semantics (restated):
 *   - a node's unknown is its pose T_i = (R_i, t_i); it enters and leaves as T16, column-major.  The rotation of an input is
 *     taken as given: nothing here re-orthonormalises.
 *   - an update is the local retraction T [+] d = (R Exp(phi), t + R rho), d = (rho, phi), phi a rotation vector (Rodrigues).
 *   - a link (ref, mov, Z) has Z = the registrar's T16 = the pose of mov in ref's frame.  Its error is e = (t_E, Log R_E) with
 *     E = T_ref^-1 T_mov Z^-1, associated (T_ref^-1 T_mov) Z^-1.  The error is on the LEFT of Z because the matcher's increment
 *     is T <- TR T with TR = Trans Rx Ry Rz (ndt_matcher_d2d_fusion.h:1035-1042): cov36, ordered (x, y, z, rx, ry, rz), is
 *     therefore, to first order, the covariance of exactly this e.
 *   - Log R = v theta / |v| with v = (R32 - R23, R13 - R31, R21 - R12) / 2 and theta = atan2(|v|, (tr R - 1) / 2); Log R = v
 *     where |v| < 1e-8 and the trace is positive; where |v| < 1e-8 and the trace is negative R is a half turn whose axis is
 *     lost: that is reported (NDTGPU_PGO3_HALF_TURN), not guessed.
 *   - the Jacobians are analytic and exact.  With A = T_ref^-1 T_mov, Z^-1 = (R_z', t_z') and Jr^-1 = Jr^-1(e_phi):
 *       J_ref = [[-I, [t_E]x], [0, -Jr^-1 R_E^T]]      J_mov = [[R_A, -R_A [t_z']x], [0, Jr^-1 R_z'^T]]
 *       Jr^-1(phi) = I + [phi]x / 2 + (1 / theta^2 - (1 + cos theta) / (2 theta sin theta)) [phi]x^2
 *     (the series 1 / 12 + theta^2 / 720 below theta = 0.01; the quotient is evaluated at the half angle, as
 *     cos(theta / 2) / (2 theta sin(theta / 2))).  tests/test_pgo3_model.py holds them against central differences.
 *   - the prior acts on node 0: the same error with T_ref = node 0's pose when the graph was set, T_mov = node 0 and Z = I;
 *     its information is prior_information, default 100 * I6 -- the analogue of ndt_offline_mapper.h:45, :61.
 *   - the cost is sum e^T W e, W a 6x6 information matrix per link (its symmetric part is used); W = NULL is 100 * I6.
 *   - a registered link's W is the Cholesky inverse of the symmetric part of cov36; the covariance 0.02 * I6 (W = 50 * I6)
 *     stands in under NDTGPU_COV_SINGULAR, NDTGPU_COV_POSE_UNCHANGED or NDTGPU_COV_NOT_COMPUTED (ndt_feature_graph.cpp:300-310)
 *     and where the matrix is not positive definite or its inverse is not finite.  A 3-DoF registration's cov36 is singular, so
 *     it lands there too.  The conversion uses +, -, *, / and sqrt only, without contraction: host, device and
 *     tests/pgo3_model.py give the same bits.
 *   - Gauss-Newton with the stop rule, the defaults and the exit codes of ndtgpu_pgo_params / NDTGPU_PGO_*; eps_step is held
 *     against the largest |component| of d, in m or rad.  Each system is solved by conjugate gradients from zero, preconditioned
 *     with the 6x6 diagonal blocks (Cholesky; the identity where a block is not positive definite).  A step that leaves the
 *     finite numbers is rolled back to the last iterate, as in SE(2).  One more exit code, NDTGPU_PGO3_HALF_TURN: the FIRST
 *     linearisation found a factor whose residual rotation is a half turn; the poses are returned as set, iterations 0,
 *     cost_initial NaN.  A half turn met later makes that iterate's cost NaN: the roll-back applies (NDTGPU_PGO_NOT_FINITE).
 * PROVENANCE: the reference has no SE(3) optimiser; the factor is the standard between-factor on SE(3) restated from memory with
 * the side of the error chosen to match cov36, and the optimiser is this library's SE(2) one.
 * DEVIATIONS:
 *   - the matcher's increment is a product of Euler rotations, the error here is a rotation vector: the two agree to FIRST ORDER
 *     only, so cov36 is the covariance of e up to terms of second order in the registration error.
 *   - the stop rule, its defaults and the inner solver are OURS (see the SE(2) section).
 *   - links are taken as given: nothing is added twice (the SE(2) mirror's doubling reproduces ndt_offline_mapper.h:74-93).
 * Device form (csrc/ndt_pgo3.hip, ndt_pgo3_kernel): one workgroup of 512 threads optimises one graph from start to finish, `count`
 * graphs are `count` workgroups of one launch.  Nothing but the workgroup barrier orders its passes: no grid barrier, no queue,
 * no spin on memory, no atomics; every sum has one fixed order, so a graph's poses and result are the same bits whichever
 * batch it runs in, whatever first / count are and whatever the bank's capacity is.  512 threads, not 1024: the
 * linearisation's 3x3 matrices and the gather's 6x6 Cholesky factor do not fit 128 VGPRs a thread without spills (204 of them).
 * Kernels (tools/kernel_resources.py pgo3): ndt_pgo3_kernel 228 VGPRs, no VGPR spill, no scratch, 256 B of LDS (77 scalar
 * registers are kept in vector lanes, not in memory); ndt_pgo3_links_kernel 116 VGPRs, no spill, no scratch.
 * Measured on MI355X, ndtgpu 0.13.0 (tools/pgo3_cost.py: the grid-world graphs of tools/pgo_cost.py lifted to 3D -- heights that
 * undulate by 0.3 m, roll and pitch of +-0.1 rad, start 0.2 m / 0.1 rad off in every component; defaults; device events round
 * the call, median of 5 repeats after a warm-up, 2 at the replay's size; the SE(2) bank on the same nodes and links in the same
 * run):
 *   graphs x nodes / links   updates / inner iterations   SE(3)      per graph   SE(2) same run   SE(3) : SE(2)
 *   1 x 500 / 1886           6 / 2433                     101.8 ms   101.8 ms    13.5 ms          7.5
 *   256 x 500 / 1886         6 / at most 2444             303.2 ms   1.18 ms     24.7 ms          12.3
 *   1 x 5000 / 43 509        6 / 7528                     9.89 s     9.89 s      0.743 s          13.3
 * every graph converged; no inner solve reached max_linear_iterations.  An inner iteration costs 42 us at 500 nodes against the
 * SE(2) kernel's 12.5 us, and the 3D graphs need 2.2 to 3 times as many of them (the 6x6 blocks are worse conditioned than the
 * 3x3 ones).  The NumPy model (dense solve, 16 threads) takes 1.25 s at 500 nodes on the same box.  One workgroup is the wrong
 * shape for the replay's one large graph: that one is for ndtgpu_pgo3_optimize_wide, the chip-wide form below. */
typedef struct ndtgpu_pgo3 ndtgpu_pgo3;
typedef struct {
    int32_t max_iterations;          /* Gauss-Newton updates at most (50) */
    int32_t max_linear_iterations;   /* conjugate-gradient iterations per update at most (2000) */
    double eps_step;                 /* stop when the largest |component| of the update is <= this (1e-8; m and rad) */
    double eps_linear;               /* the inner solve's relative residual |r| / |b| (1e-8) */
    double prior_information[36];    /* the prior's W, row-major, (x, y, z, rx, ry, rz) (100 * I6) */
} ndtgpu_pgo3_params;
void ndtgpu_default_pgo3_params(ndtgpu_pgo3_params *p);
enum {
    NDTGPU_PGO3_HALF_TURN = 4        /* ndtgpu_pgo_result.exit_code, beside NDTGPU_PGO_*: see above */
};
/* room for n_graphs graphs of up to max_nodes nodes and max_edges links each (the limits of ndtgpu_pgo_create) */
ndtgpu_status ndtgpu_pgo3_create(size_t n_graphs, size_t max_nodes, size_t max_edges, ndtgpu_pgo3 **out);
ndtgpu_status ndtgpu_pgo3_destroy(ndtgpu_pgo3 *h);
/* installs graph g.  All arrays HOST: T16_nodes n_nodes x 16 column-major, node 0's is the prior's origin; ref_idx / mov_idx
 * n_edges node indices; Z16 n_edges x 16 column-major; info36 n_edges x 36 row-major or NULL (100 * I6 for every link).
 * The checks of ndtgpu_pgo_set_graph -- index range, ref == mov, every node connected to node 0 -- made before the handle is
 * read and the device is looked for.  Synchronous. */
ndtgpu_status ndtgpu_pgo3_set_graph(ndtgpu_pgo3 *h, size_t g, size_t n_nodes, const double *T16_nodes, size_t n_edges,
                                    const uint32_t *ref_idx, const uint32_t *mov_idx, const double *Z16, const double *info36);
/* the same with the links where ndtgpu_register_batch_cov_device left them: T16_nodes, ref_idx, mov_idx HOST; T16_dev (n_edges x
 * 16), cov36_dev (n_edges x 36) and cov_flags_dev (n_edges) DEVICE and complete when the call is made.  ndt_pgo3_links_kernel
 * converts a link per lane (ndtgpu_pgo3_link_from_registration); cov36_dev == NULL gives every link 100 * I6 (cov_flags_dev is
 * then not read).  No link value visits the host.  Returns when the kernel has run. */
ndtgpu_status ndtgpu_pgo3_set_links_device(ndtgpu_pgo3 *h, size_t g, size_t n_nodes, const double *T16_nodes, size_t n_edges,
                                           const uint32_t *ref_idx, const uint32_t *mov_idx, const double *T16_dev,
                                           const double *cov36_dev, const int32_t *cov_flags_dev);
/* optimises graphs [first, first + count), each of which has been set, in ONE launch, asynchronous on `stream`; prm NULL: the
 * defaults.  Calls on one handle are ordered.  A graph that ends with NDTGPU_PGO_NOT_FINITE or NDTGPU_PGO3_HALF_TURN does not
 * fail the call or touch the other graphs. */
ndtgpu_status ndtgpu_pgo3_optimize(ndtgpu_pgo3 *h, size_t first, size_t count, const ndtgpu_pgo3_params *prm, ndtgpu_stream stream);
/* graph g's poses: T16_out HOST n_nodes x 16 column-major (what ndtgpu_world_assemble takes) or NULL; result may be NULL.  Waits
 * for the handle. */
ndtgpu_status ndtgpu_pgo3_poses(ndtgpu_pgo3 *h, size_t g, double *T16_out, ndtgpu_pgo_result *result);
/* Pure host, no device needed; the code the kernel runs (csrc/ndt_pgo3.h) compiled for the host.
 * e6 = the link's error at (Ti16, Tj16) = (ref, mov); Jref36 / Jmov36 (row-major 6x6, either may be NULL) its derivatives with
 * respect to the retraction of either pose.  NDTGPU_ERR_INVALID at a half turn. */
ndtgpu_status ndtgpu_pgo3_link_error(const double *Ti16, const double *Tj16, const double *Z16, double *e6, double *Jref36, double *Jmov36);
/* T16_out = T16 [+] d6 */
ndtgpu_status ndtgpu_pgo3_retract(const double *T16, const double *d6, double *T16_out);
/* a registered link as the factor takes it: Z16 = T16, W36 (row-major) from cov36 and flags as stated above; cov36 NULL: 100 * I6 */
ndtgpu_status ndtgpu_pgo3_link_from_registration(const double *T16, const double *cov36, int32_t flags, double *Z16, double *W36);

/* ---- the chip-wide form of the SE(3) optimiser: ONE large graph spread over the device -----------------------------------------
 * ndtgpu_pgo3_optimize gives a graph to one workgroup of 512 threads: right for a bank of small graphs, wrong for the one large
 * graph the offline mapper's loop optimises once per round.  ndtgpu_pgo3_optimize_wide optimises graph g of an ndtgpu_pgo3 bank
 * alone with the same algorithm, operation for operation -- the per-link and per-node bodies are the same inlines of
 * csrc/ndt_pgo3.h: linearisation per link with the prior as the link behind the last, gather and 6x6 Cholesky factor per node,
 * preconditioned conjugate gradients from zero with the same break rules, the retraction with the roll-back to the last finite
 * iterate, the same stop rule and exit codes -- so ndtgpu_pgo3_poses and ndtgpu_pgo_result mean the same, field for field;
 * linear_iterations counts the inner iterations TAKEN, never the launches enqueued.  It is ndtgpu_pgo_optimize_wide's structure
 * and shares its control block, tile, combiners and steering loop (csrc/ndt_pgo_wide_core.h), and its parameter struct
 * (ndtgpu_pgo_wide_params, check_every).
 * Launch structure (csrc/ndt_pgo3_wide.hip): a lane per link or per node, workgroups of 256 lanes, ONE PLAIN LAUNCH PER PASS on
 * `stream`; the boundary between two launches is the only synchronisation: no grid barrier, no cooperative launch, no workgroup
 * that waits for another, no spin on memory, no atomics, no captured graph.  The node passes run over n_nodes items, the link
 * passes over n_edges + 1 -- item n_edges is the prior -- so link_tiles = ceil((n_edges + 1) / 256) is never 0 and no pass is
 * skipped for a graph without links; the product pass does nothing for the prior, whose J^T W J p stays in node 0's lane.  Per
 * Gauss-Newton update: ONE launch that gathers, factors and starts the solve (gather and start fit one kernel without a spill, so
 * START is not split); THREE launches per inner iteration (a link pass that forms p = z + beta p of its two end nodes on the fly
 * as one fma, a node pass that stores the same bits of p and gathers A p, a node pass for alpha, x, r and z); then the pose
 * update, the linearisation and the cost assessment.  The run's scalars travel in the double-buffered control block; every
 * launch begins by reading it and does nothing where its phase is over.  The host enqueues check_every inner iterations at a
 * time, then copies the control block to pinned memory and waits for it (also after every cost assessment): the call is
 * SYNCHRONOUS TOWARDS THE HOST and returns when the graph is done.  Launches enqueued past a stop do nothing.
 * Summation rule: items are cut into tiles of 256 consecutive items (ndtgpu_pgo3_wide_plan), a tile's sum is taken by its
 * workgroup in the order of csrc/ndt_block.h and stored per tile -- the cost and, beside it, the tile's count of half turns --;
 * every workgroup that needs the graph's sum adds the per-tile sums in one fixed order (thread t takes t, t + 256, ... ascending,
 * then the workgroup sum).  A node's incident links are summed in ascending link order by one lane.  The tiling follows the
 * graph's n_nodes and n_edges alone: a graph's poses and result are the same bits for every check_every, whatever the bank's
 * capacity, whatever the other graphs of the bank hold or have just run, and from run to run.  They are NOT the bits of
 * ndtgpu_pgo3_optimize, which adds in another order (a thread's strided items, 512 threads) and leaves z + beta * p to the
 * compiler: the two forms agree to rounding (tests/test_gpu_pgo3_wide.py).
 * Exit codes as in ndtgpu_pgo3_optimize: a half turn at the FIRST linearisation gives NDTGPU_PGO3_HALF_TURN -- tested before the
 * finiteness of the cost --, poses as set, iterations 0, cost_initial NaN; a half turn or a cost that is not finite later gives
 * the roll-back and NDTGPU_PGO_NOT_FINITE; NDTGPU_PGO_LINEAR_CAP replaces 0 or 1 where an inner solve was capped.
 * Two more device buffers (the per-tile sums and the control blocks, with a pinned mirror) are allocated by a handle's first
 * wide call, for the handle's capacity, and released by ndtgpu_pgo3_destroy.
 * Kernels (tools/kernel_resources.py pgo3_wide), each of 256 threads with the whole register file to itself: linearise 74 VGPRs,
 * assess 18, start (gather, factor and the solve's start in one) 116, link 70, node 116, step 72, update 72; no VGPR spill, no
 * SGPR spill, no scratch in any of them, 128 B of LDS each -- against the one-workgroup kernel's 228 VGPRs at 512 threads.
 * Measured on MI355X (tools/pgo3_cost.py --wide; the graphs and defaults of the section above; one-workgroup form by device
 * events, wide form by host wall time round the synchronous call, median of the repeats after a warm-up):
 *   nodes / links   updates / inner iterations   one workgroup            wide, check_every 8 / 32 / 128       wide per inner iteration
 *   500 / 1886      6 / 2433                    101.7 ms (41.8 us each)  64.9 / 61.9 / 64.1 ms  (1.6 x)       25.4 us
 *   1500 / 8575     6 / 3992                    921 ms   (231 us each)   134.1 / 127.1 / 126.4 ms  (7.2 x)    31.8 us
 *   5000 / 43 509   6 / 7534 (wide 7450)        9.98 s   (1325 us each)  455 / 446 / 443 ms  (22.4 x)         59.8 us
 * (ratios at the default check_every, 32; every run converged with the same cost_final to the digits printed; the forms took
 * the same updates, and the same inner iterations except at the replay's size).  THE REPLAY'S GRAPH TAKES 0.446 s IN PLACE OF
 * 9.98 s.  Below 500 nodes, same graphs, same run, one workgroup against wide at check_every 32: 60 nodes / 195 links 8.5 against
 * 11.8 ms, 125 / 416 20.3 against 26.5 ms, 200 / 710 31.2 against 35.4 ms, 250 / 906 38.9 against 40.9 ms, 350 / 1298 62.1
 * against 50.8 ms: the forms cross between 250 and 350 nodes -- BELOW SOME 300 NODES (1.1 k links) ndtgpu_pgo3_optimize IS THE
 * ONE TO CALL, and always for a bank of graphs, which it fills the chip with; above it the wide form.  At the replay's size the
 * device, not the host, sets the pace: the three launches of an inner iteration run 8.3 + 42.9 + 6.6 us (link, node, step:
 * rocprofv3 --kernel-trace, a run of its own); the node pass gathers some 17 links of 39 + 6 doubles per lane from 20
 * workgroups.  START (gather, factor, start) runs 342 us, six times in the run; the linearisation 16 us. */
/* pure host: the tile (256), the node and link tiles of a graph of this size -- link_tiles counts the prior, n_edges + 1 items --
 * and the extra device bytes the wide form needs for it (8 per per-tile sum: four per node tile, two per link tile; and the two
 * control blocks; a handle allocates them for its capacity).  NDTGPU_ERR_INVALID beyond ndtgpu_pgo3_create's limits (n_nodes
 * 1 .. 2^24, n_edges <= 2^27).  Any out pointer may be NULL. */
ndtgpu_status ndtgpu_pgo3_wide_plan(size_t n_nodes, size_t n_edges, uint32_t *tile, size_t *node_tiles, size_t *link_tiles,
                                    size_t *extra_bytes);
/* graph g alone, spread over the device; launches on `stream`; RETURNS WHEN THE GRAPH IS DONE (the host steers the phases).
 * prm / wide NULL: the defaults.  The parameter checks of ndtgpu_pgo3_optimize and check_every >= 1, made before the handle is
 * read and the device is looked for; NDTGPU_ERR_INVALID for a graph that has not been set or g out of range.  Calls on one
 * handle stay ordered, whichever form and stream they name.  A graph that ends with NDTGPU_PGO_NOT_FINITE or
 * NDTGPU_PGO3_HALF_TURN does not fail the call. */
ndtgpu_status ndtgpu_pgo3_optimize_wide(ndtgpu_pgo3 *h, size_t g, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_wide_params *wide,
                                        ndtgpu_stream stream);

/* ---- Marginal covariances of the pose-graph banks: the uncertainty of what ndtgpu_pgo_* / ndtgpu_pgo3_* estimated -----------
 * The reference keeps a place for a node's covariance -- NDTFeatureNodeInterface::setCov beside setPose (interfaces.h:16),
 * NDTFeatureNode::cov carried in NDTNodeMsg.cov (ndtgraph_conversion.h:51), drawn by markerMeanCovariance2d (ndt_rviz.h:1261) --
 * but optimizeGraphUsingISAM (ndt_offline_mapper.h:101-104) only ever calls setPose: after optimisation a node's cov is whatever
 * the fuser left there.  ndtgpu_pgo_marginals / ndtgpu_pgo3_marginals fill the place.
 * Semantics (restated; both banks):
 *   - at the poses graph g currently HOLDS -- as set, or after ndtgpu_pgo_optimize / _optimize_wide -- let H = sum J^T W J over
 *     the prior and all links, with exactly the Jacobians, the symmetric part of W and the prior of the optimiser's
 *     linearisation (the sections above).  The cost is sum e^T W e, so the covariance of the estimate is H^-1.
 *   - a query names a graph, a node q and optionally a second node o.  cov is the symmetric part (B + B^T) / 2 of the diagonal
 *     block B = (H^-1)[q, q]; cross, where asked, is the raw block (H^-1)[o, q]: the rows of o, the columns of q.
 *   - SE(2): cov is 3x3 row-major in (x, y, yaw), the coordinates of the additive update p + d: the covariance of (x, y, yaw) IN
 *     THE GRAPH'S FRAME.  SE(3): 6x6 row-major in (rho, phi), the coordinates of the local retraction T [+] d = (R Exp(phi),
 *     t + R rho): the covariance lives IN THE NODE'S OWN TANGENT FRAME, translation part included.
 *   - column k of block column q is the solution of H x = e_(q,k), found by the optimiser's own solve -- from zero, preconditioned
 *     with the inverses of the diagonal blocks, to the relative residual eps_linear, at most max_linear_iterations, the pap > 0
 *     break; the same operations in the same order.  The columns are independent recurrences.
 *   - prior_information, eps_linear and max_linear_iterations come from the ndtgpu_pgo_params / ndtgpu_pgo3_params passed (NULL:
 *     the defaults); the other fields are ignored.  prior_information HAS TO BE THE ONE THE GRAPH WAS OPTIMISED WITH: it is part
 *     of H, and nothing records it with the graph.
 *   - per query a record (ndtgpu_pgo_marginal_result).  exit_code reuses NDTGPU_PGO_*: CONVERGED; LINEAR_CAP: at least one column
 *     stopped at the cap, the values are the iterates so far; NOT_FINITE: the linearisation's cost at the held poses is not finite,
 *     cov and cross are NaN; NDTGPU_PGO3_HALF_TURN: the linearisation met a half turn, the outputs are NaN.  A graph at fault
 *     does not fail the call or touch other graphs' queries.
 *   - ndtgpu_pgo_relative_covariance / ndtgpu_pgo3_relative_covariance: the covariance of the error of a link ref -> mov whose
 *     measurement is the current relative pose, J_ref S_rr J_ref^T + J_ref S_rm J_mov^T + J_mov S_mr J_ref^T + J_mov S_mm J_mov^T
 *     with the link Jacobians of the sections above -- what a covariance-aware loop-closure gate would test.  On a tree it is the
 *     link's W^-1; a loop makes it smaller.
 * PROVENANCE: the reference never asks iSAM for covariances; this is the standard Gauss-Newton covariance of OUR OWN cost.
 * DEVIATIONS:
 *   - not iSAM's marginals (a sparse factorisation's back-substitution): each column is an iterative solve to eps_linear, so a
 *     block is good to about eps_linear times the conditioning the preconditioner leaves, and B is symmetric only to that
 *     (asymmetry reports it).
 *   - with the host mirror's link doubling (ndt_offline_mapper.h:74-93; see above) every doubled link counts twice in H: the
 *     covariances reflect the cost that was optimised, not the links' own covariances.
 *   NOT BUILT: a chip-wide form (many workgroups per column) for the replay's 5000-node graph; a covariance-aware link gate;
 *   covariance markers; moving an SE(3) block into the world frame.
 * Device form (csrc/ndt_pgo.hip, csrc/ndt_pgo3.hip; pgo_solve / pgo3_solve and the inlines of csrc/ndt_pgo.h / ndt_pgo3.h called as
 * they are): three plain launches on one stream -- no atomics, no grid barrier, no cooperative launch, no captured graph, no
 * workgroup that waits for another.  PREPARE: one workgroup per distinct graph the call names linearises it and gathers the
 * preconditioner into the marginals' OWN workspace through a graph view whose written pointers are redirected; the optimiser's
 * scratch, the poses and the graph's ndtgpu_pgo_result are not touched.  SOLVE: one workgroup (1024 threads SE(2), 512 SE(3)) per
 * (query, column) with b, x, r, z, p, Ap, t_e in the workgroup's slot of the workspace, b the unit vector; the slot is the
 * workgroup's position in its launch, nothing is claimed at run time.  FINISH: a lane per query.  A call with more columns than
 * the workspace has slots is cut into consecutive solve launches of at most `slots` workgroups (ndtgpu_pgo_marginal_plan); stream
 * order lets a later launch reuse the slots.  A query's numbers are the same bits whatever the slot count, the number of
 * launches, the other queries of the call, their order and the bank's other graphs are, and from run to run.  The workspace
 * belongs to the handle: allocated by its first marginals call, regrown when a call needs more, released by ndtgpu_pgo_destroy /
 * ndtgpu_pgo3_destroy.  Calls on a handle stay ordered with its optimise calls.
 * Kernels (tools/kernel_resources.py pgo_marginals): SE(2) prepare 110 VGPRs, solve 92, 512 B of LDS; SE(3) prepare 132, solve 133
 * (against ndt_pgo3_kernel's 228: the solve alone is the lighter pass), 256 B of LDS; none spills a VGPR or has scratch.
 * Measured on MI355X, ndtgpu 0.13.0 (tools/pgo_marginals_cost.py: device events round the _device call, median of 7 after a
 * warm-up; the grid-world graphs of tools/pgo_cost.py / pgo3_cost.py, 500 nodes and 1886 links, optimised first; defaults, so every
 * column of a call in ONE solve launch).  SE(2): ALL 500 marginals of one graph, 1500 columns of at most 222 inner iterations
 * (329 k together): 19.1 ms; the last node of each of 256 such graphs, 768 columns: 12.8 ms.  SE(3): all 500 marginals, 3000 columns
 * of at most 412 iterations (1.23 M together): 322 ms; the last node of each of 256 graphs, 1536 columns: 275 ms.  Every query
 * CONVERGED; the blocks are within 2.7e-10 (SE(3): 2.6e-10) of numpy.linalg.inv of the model's dense H, relative to each block's
 * largest entry, and asymmetry is 1.0e-11 (2.9e-11) at most.  numpy.linalg.inv itself takes 40 ms for the 1500 x 1500 H and 151 ms
 * for the 3000 x 3000 one on the same box: for EVERY marginal of ONE graph of this size the dense inverse on the host is as fast
 * (SE(2)) or faster (SE(3), where a workgroup of 512 threads has a compute unit to itself and the 3000 columns take twelve turns);
 * the device form is for a few nodes of many graphs -- 256 dense inverses take 10 s and 39 s --, for graphs whose dense H no
 * longer fits the host's patience, and for results that stay on the device. */
typedef struct {
    uint64_t max_workspace_bytes;    /* the slots of a call take at most this much device memory, one slot at least (OURS: 1 GiB) */
} ndtgpu_pgo_marginal_params;
/* the default above is OURS */
void ndtgpu_default_pgo_marginal_params(ndtgpu_pgo_marginal_params *p);
typedef struct {
    int32_t exit_code;               /* NDTGPU_PGO_CONVERGED, _LINEAR_CAP, _NOT_FINITE or NDTGPU_PGO3_HALF_TURN */
    int32_t linear_iterations;       /* the inner iterations of the query's columns, together */
    int32_t max_column_iterations;   /* ... of the column that took most */
    int32_t capped_columns;          /* columns that stopped at max_linear_iterations */
    double asymmetry;                /* max |B - B^T| of the raw diagonal block */
} ndtgpu_pgo_marginal_result;
/* pure host: the bytes of one slot for a bank of this capacity (dof 3: ndtgpu_pgo, 6: ndtgpu_pgo3), the slots a budget buys --
 * slots >= 1 always, slots * slot_bytes <= max_workspace_bytes unless slots == 1, never more than the call has columns (one where
 * it has none) -- and the solve launches the call takes, ceil(n_queries * dof / slots).  NDTGPU_ERR_INVALID beyond the limits of
 * ndtgpu_pgo_create, for n_queries > 2^27 or for another dof.  Any out pointer may be NULL. */
ndtgpu_status ndtgpu_pgo_marginal_plan(size_t max_nodes, size_t max_edges, size_t n_queries, int32_t dof, uint64_t max_workspace_bytes,
                                       size_t *slot_bytes, size_t *slots, size_t *launches);
/* n_queries >= 1 queries (graph_idx, node_idx, other_idx: HOST, n_queries each; other_idx NULL: no cross blocks, and cross9_out
 * may be NULL).  cov9_out, cross9_out (n_queries x 9) and results_out (n_queries): HOST.  Synchronous.  prm / mprm NULL: the
 * defaults.  NDTGPU_ERR_INVALID -- the outputs' and parameters' checks before the handle is read and the device is looked for --
 * for NULL outputs or index arrays, eps_linear not finite or not positive, max_linear_iterations < 1, a prior that is not finite,
 * a graph index out of range or not set, a node index >= n_nodes. */
ndtgpu_status ndtgpu_pgo_marginals(ndtgpu_pgo *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                   const uint32_t *other_idx, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                   double *cov9_out, double *cross9_out, ndtgpu_pgo_marginal_result *results_out);
/* ... the queries HOST and copied by the call, the outputs DEVICE, asynchronous on `stream` (the call waits for the handle's
 * previous call before it overwrites the queries' pinned copy) */
ndtgpu_status ndtgpu_pgo_marginals_device(ndtgpu_pgo *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                          const uint32_t *other_idx, const ndtgpu_pgo_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                          double *cov9_dev, double *cross9_dev, ndtgpu_pgo_marginal_result *results_dev, ndtgpu_stream stream);
/* the same for a bank of SE(3) graphs, 36 doubles where the entries above have 9 */
ndtgpu_status ndtgpu_pgo3_marginals(ndtgpu_pgo3 *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                    const uint32_t *other_idx, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                    double *cov36_out, double *cross36_out, ndtgpu_pgo_marginal_result *results_out);
ndtgpu_status ndtgpu_pgo3_marginals_device(ndtgpu_pgo3 *h, size_t n_queries, const uint32_t *graph_idx, const uint32_t *node_idx,
                                           const uint32_t *other_idx, const ndtgpu_pgo3_params *prm, const ndtgpu_pgo_marginal_params *mprm,
                                           double *cov36_dev, double *cross36_dev, ndtgpu_pgo_marginal_result *results_dev,
                                           ndtgpu_stream stream);
/* Pure host, no device needed; the Jacobians are those of the kernels' headers compiled for the host.  The covariance of the error
 * of a link ref -> mov at Z = the current relative pose, from the two nodes' cov blocks and cross = the block [mov, ref] (rows of
 * mov: ndtgpu_pgo_marginals with node = ref, other = mov).  pose_ref3 / pose_mov3: (x, y, yaw); Tref16 / Tmov16: column-major 4x4. */
ndtgpu_status ndtgpu_pgo_relative_covariance(const double *pose_ref3, const double *pose_mov3, const double *cov_ref9, const double *cov_mov9,
                                             const double *cross9, double *out9);
ndtgpu_status ndtgpu_pgo3_relative_covariance(const double *Tref16, const double *Tmov16, const double *cov_ref36, const double *cov_mov36,
                                              const double *cross36, double *out36);

/* ---- robust loop-closure weighting of the pose-graph banks: Huber, Cauchy, DCS -------------------------------------------------
 * Links are seeded by feature RANSAC (ndtgpu_featbank_match*), refined by D2D and gated on score, distance and angle
 * (ndtgpu_linkgate_valid: getValidLinks); whatever passes enters ndtgpu_pgo_* / ndtgpu_pgo3_* as a plain quadratic factor, and one
 * perceptual-aliasing link bends the whole map.  ndtgpu_pgo_optimize_robust / ndtgpu_pgo3_optimize_robust optimise with a robust
 * cost by ITERATIVELY RE-WEIGHTED LEAST SQUARES ROUND THE OPTIMISERS AS THEY ARE, and say which links were weighted down.
 * Semantics (restated; both banks):
 *   - W0 is a link's information AS THE GRAPH WAS SET (ndtgpu_pgo_set_graph / _set_links_device); chi2 = e^T W0 e with the link
 *     error e of the sections above at the poses the graph holds.
 *   - the weight w of a link from its chi2 and the scale (k, c or Phi):
 *       Huber(k):    w = 1 where sqrt(chi2) <= k, else k / sqrt(chi2)
 *       Cauchy(c):   w = 1 / (1 + chi2 / c^2)
 *       DCS(Phi):    s = min(1, 2 Phi / (Phi + chi2)), w = s^2
 *     written with +, -, *, / and a correctly rounded square root alone, without contraction: host (ndtgpu_pgo_robust_weight),
 *     device and tests/pgo_robust_model.py give the same bits from the same chi2.
 *   - the link's term of the robust cost: Huber chi2, or 2 k sqrt(chi2) - k^2 where sqrt(chi2) > k; Cauchy c^2 log(1 + chi2 / c^2);
 *     DCS s^2 chi2 + Phi (1 - s)^2.  The robust cost of a graph is the sum of its links' terms: the prior is never re-weighted
 *     and is not part of it (nor of chi2_final).
 *   - links with |mov - ref| < min_index_gap keep w = 1, their information bits and the plain term chi2: at the default gap, 2, that
 *     is the odometry chain.  The prior and the protected chain keep the system non-singular whatever the other weights are.
 *   - a ROUND: at the poses the graph holds every link is weighed and w * W0 written into the bank's information; then the
 *     unchanged ndtgpu_pgo_optimize (ndtgpu_pgo_optimize_wide where `wide` is given; the pgo3 pair) takes updates_per_round
 *     Gauss-Newton updates with the weights frozen.  A graph stops CONVERGED when its optimiser call took at most one update and
 *     that update's max_step <= eps_step; with MAX_ROUNDS -- the slot of NDTGPU_PGO_MAX_ITERATIONS -- after max_rounds rounds; or
 *     with the inner call's NDTGPU_PGO_LINEAR_CAP / NDTGPU_PGO_NOT_FINITE / NDTGPU_PGO3_HALF_TURN passed through.  When a graph
 *     stops its links are weighed once more at the poses it ends with: chi2, weight, inlier, cost_final, chi2_final and outliers
 *     describe those poses, and THE BANK IS LEFT WEIGHTED with exactly these weights, so that ndtgpu_pgo_marginals /
 *     ndtgpu_pgo3_marginals and ndtgpu_world_assemble see the robust problem.  ndtgpu_pgo_robust_restore puts W0 back.
 *   - a chi2 (or weight) that is not finite -- a NaN input, an SE(3) half turn -- ends that graph with NDTGPU_PGO_NOT_FINITE /
 *     NDTGPU_PGO3_HALF_TURN: that weighing is not applied to it, the graph holds W0 again, and the other graphs are unaffected.
 *   - max_rounds = 0 only evaluates: chi2, weights, flags and the record at the held poses; the bank's poses, information and
 *     optimiser records do not change (exit MAX_ROUNDS).  Like every weighing it overwrites the bank's per-link scratch (the
 *     linearisation jac and te = W0 e, written by the optimiser's own per-link body): no entry reads that scratch before it has
 *     linearised again, and nothing else may.
 *   - a robust call always weighs the information as set, never the weighted one a previous robust call left: two robust calls
 *     from the same poses give the same bits as one.  The copy of W0 is taken by the first robust call after a graph is set;
 *     ndtgpu_pgo_set_graph / _set_links_device invalidate it.  A plain ndtgpu_pgo_optimize after a robust call runs on the
 *     weighted information.
 * PROVENANCE: the reference, and iSAM as it calls it (ndt_offline_mapper.h:40-107), have NO robust cost: every factor is a plain
 * quadratic.  Huber's and Cauchy's M-estimators and dynamic covariance scaling (DCS; Agarwal et al., "Robust map optimization using
 * dynamic covariance scaling", ICRA 2013) are restated from memory.
 * DEVIATIONS:
 *   - IRLS FREEZES THE WEIGHTS WITHIN A ROUND: the inner Gauss-Newton updates see a quadratic cost, not the robust cost's own
 *     second derivative; DCS as published scales the error inside the factor at every linearisation, which is the same thing at
 *     updates_per_round = 1.
 *   - all defaults (ndtgpu_pgo_robust_params) and the stop rule are OURS.
 *   NOT BUILT: a device-side stop without the host; optimize_gated (the binding) in 3D; switchable constraints; a covariance-aware
 *   gate.
 * Device form (csrc/ndt_pgo_robust.hip): per round and run of graphs two plain launches in front of the optimiser's.
 * ndt_pgo_robust_weigh_kernel / ndt_pgo3_robust_weigh_kernel: grid (tiles of 256 links) x (graphs), a lane per link, the optimiser's
 * own per-link inline (csrc/ndt_pgo.h, ndt_pgo3.h) through a graph view whose information is the copy of W0; it writes chi2,
 * weight, inlier and w * W0 in the bank's layout, and per-tile sums (robust cost, chi2, links flagged out) taken in the order of
 * csrc/ndt_block.h.  ndt_pgo_robust_finish_kernel / ndt_pgo3_robust_finish_kernel: one workgroup per graph adds the per-tile sums
 * in the order of the wide form's combiner (thread t takes t, t + 256, ..., then the workgroup sum).  No atomics, no grid barrier,
 * no workgroup that waits for another, no spin.  THE HOST STEERS THE ROUNDS, as the wide form's phases: after every round it reads
 * the graphs' records and launches again for the graphs still active, in contiguous runs; a stopped graph gets no further launch
 * that changes it.  Hence the call is SYNCHRONOUS TOWARDS THE HOST, and a graph's poses, weights and record are the same bits in
 * any batch, at any first / count, for any bank capacity and from run to run; with `wide`, for every check_every.
 * Seven more device buffers (the copy of W0, chi2, weight, inlier, the per-tile sums and counts, the graphs' sums) are allocated
 * by a handle's first robust call, for its capacity, and released by ndtgpu_pgo_destroy / ndtgpu_pgo3_destroy.
 * Measured on MI355X: NOT YET MEASURED (tools/pgo_robust_cost.py). */
enum {
    NDTGPU_PGO_ROBUST_HUBER = 1,
    NDTGPU_PGO_ROBUST_CAUCHY = 2,
    NDTGPU_PGO_ROBUST_DCS = 3
};
typedef struct {
    int32_t kind;                    /* NDTGPU_PGO_ROBUST_* (OURS: DCS) */
    int32_t max_rounds;              /* rounds at most; 0: evaluate only (OURS: 50) */
    int32_t updates_per_round;       /* Gauss-Newton updates of a round's optimiser call, >= 1 (OURS: 1) */
    int32_t min_index_gap;           /* links with |mov - ref| below this are never re-weighted, >= 1 (OURS: 2) */
    double scale;                    /* k, c or Phi; finite and > 0 (OURS: 1) */
    double inlier_weight;            /* a link is flagged an inlier where weight >= this; in [0, 1] (OURS: 0.5) */
} ndtgpu_pgo_robust_params;
void ndtgpu_default_pgo_robust_params(ndtgpu_pgo_robust_params *p);
typedef struct {
    int32_t exit_code;               /* NDTGPU_PGO_*, NDTGPU_PGO3_HALF_TURN; NDTGPU_PGO_MAX_ITERATIONS stands for MAX_ROUNDS */
    int32_t rounds;                  /* rounds taken */
    int32_t updates;                 /* Gauss-Newton updates, all rounds together */
    int32_t linear_iterations;       /* conjugate-gradient iterations, all rounds together */
    double cost_initial;             /* the robust cost at the poses as the call found them */
    double cost_final;               /* ... at the poses returned */
    double chi2_final;               /* the plain sum of the links' chi2 at the poses returned */
    int32_t outliers;                /* links with weight < inlier_weight at the poses returned */
    int32_t pad_;
} ndtgpu_pgo_robust_result;
/* pure host: the weight of a link from its chi2, the bits the device gives.  NDTGPU_ERR_INVALID for an unknown kind or a scale
 * that is not finite and positive. */
ndtgpu_status ndtgpu_pgo_robust_weight(int32_t kind, double scale, double chi2, double *weight);
/* graphs [first, first + count), each of which has been set, from the poses they hold; launches on `stream`; RETURNS WHEN EVERY
 * GRAPH HAS STOPPED (the host steers the rounds).  prm / robust NULL: the defaults; prm's max_iterations is not read
 * (updates_per_round takes its place).  wide NULL: the one-workgroup form; otherwise ndtgpu_pgo_optimize_wide, which requires
 * count == 1.  NDTGPU_ERR_INVALID -- checked before the handle is read and the device is looked for -- for an unknown kind, a
 * scale that is not finite and positive, max_rounds < 0, updates_per_round < 1, min_index_gap < 1, inlier_weight outside [0, 1],
 * and the parameter checks of ndtgpu_pgo_optimize / _optimize_wide.  A graph that ends with NDTGPU_PGO_NOT_FINITE does not fail
 * the call. */
ndtgpu_status ndtgpu_pgo_optimize_robust(ndtgpu_pgo *h, size_t first, size_t count, const ndtgpu_pgo_params *prm,
                                         const ndtgpu_pgo_robust_params *robust, const ndtgpu_pgo_wide_params *wide, ndtgpu_stream stream);
ndtgpu_status ndtgpu_pgo3_optimize_robust(ndtgpu_pgo3 *h, size_t first, size_t count, const ndtgpu_pgo3_params *prm,
                                          const ndtgpu_pgo_robust_params *robust, const ndtgpu_pgo_wide_params *wide, ndtgpu_stream stream);
/* what the last robust call left for graph g: chi2, weight (n_edges doubles each) and inlier (n_edges int32) HOST, and its
 * record; any out pointer may be NULL.  NDTGPU_ERR_INVALID where no robust call has weighed the graph since it was set.  Waits
 * for the handle. */
ndtgpu_status ndtgpu_pgo_robust_links(ndtgpu_pgo *h, size_t g, double *chi2, double *weight, int32_t *inlier, ndtgpu_pgo_robust_result *result);
ndtgpu_status ndtgpu_pgo3_robust_links(ndtgpu_pgo3 *h, size_t g, double *chi2, double *weight, int32_t *inlier, ndtgpu_pgo_robust_result *result);
/* ... the DEVICE pointers of the same three arrays (the handle's own: valid until it is destroyed, overwritten by the next robust
 * call on the graph); any out pointer may be NULL */
ndtgpu_status ndtgpu_pgo_robust_links_device(ndtgpu_pgo *h, size_t g, const double **chi2_dev, const double **weight_dev, const int32_t **inlier_dev);
ndtgpu_status ndtgpu_pgo3_robust_links_device(ndtgpu_pgo3 *h, size_t g, const double **chi2_dev, const double **weight_dev,
                                              const int32_t **inlier_dev);
/* A TEST AND INSPECTION AID, not part of the optimisation: it exists so that the bank's information can be compared bit for bit
 * (tests/test_gpu_pgo_robust.py).  Graph g's information as the bank holds it -- as set, or weighted by a robust call -- in the
 * bank's layout, HOST: SE(2) n_edges x 6,
 * the symmetric 3x3 as (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); SE(3) n_edges x 21, the lower triangle of the symmetric 6x6 row by row.
 * Waits for the handle. */
ndtgpu_status ndtgpu_pgo_link_information(ndtgpu_pgo *h, size_t g, double *W6_out);
ndtgpu_status ndtgpu_pgo3_link_information(ndtgpu_pgo3 *h, size_t g, double *W21_out);
/* the information as graph g was set back into the bank, bit for bit; nothing to do where no robust call has touched it.  Synchronous. */
ndtgpu_status ndtgpu_pgo_robust_restore(ndtgpu_pgo *h, size_t g);
ndtgpu_status ndtgpu_pgo3_robust_restore(ndtgpu_pgo3 *h, size_t g);

/* ---- world-map assembly: the node maps of a graph, under its poses, merged into one map -------------------------------------
 * The chain scans -> feature sets -> seeded links -> registered links -> optimised poses ends in node poses; the product the
 * reference's consumers use is ONE map: ndt_feature_mcl_node.cpp:174 localises in a single saved NDT map,
 * ndt_feature2d_fuser.cpp:425-432 publishes graph->getMap() moved by graph->getT(), ndt_feature_graph_opt.cpp:178-185 ends by
 * concatenating every node's getGlobalPointCloud(), and NDTFeatureGraph::fuse() (ndt_feature_graph.h:149-152) is the declared
 * but empty place for combining nodes.  ndtgpu_world_assemble is that step: it fills `count` destination maps
 * [dst_first, dst_first + count) of a destination map set (its own grid, centres and max_cells), world w from the node maps
 * node_idx[node_offsets[w] .. node_offsets[w + 1]) of a source map set, one pose T16 per listed node (node frame -> world
 * frame; what ndtgpu_pgo_poses returns as T16_out).
 * Semantics (restated):
 *   - every Gaussian cell (mu, Sigma, n) of a listed node becomes mu' = R mu + t, Sigma' = R Sigma R^T: pseudoTransformNDT, and
 *     over a whole map NDTMap::pseudoTransformNDTMap -- the call the fuser comments out at ndt_feature2d_fuser.cpp:471 and
 *     publish_graph_message.cpp:588.
 *   - the moved cell is binned by LazyGrid::getIndexForPoint(mu') of the destination grid (per axis
 *     floor((p - c) / res + 0.5) + size / 2.0 truncated to int, in fp64, not contracted: csrc/ndt_math.h lazygrid_index_half).
 *   - a mean outside the destination grid is dropped (n_dropped).  A contribution that is not finite, or whose second moment
 *     would leave the accumulator's room (below), is dropped and counted in n_rejected.
 *   - the contributions of one world cell merge as pooled sample statistics -- what a chain of NDTCell::updateSampleVariance /
 *     addDistributionToCell calls gives in exact arithmetic:  N = sum n_i,  mean = sum n_i mu'_i / N,
 *     (N - 1) C = sum [(n_i - 1) Sigma'_i + n_i (mu'_i - mean)(mu'_i - mean)^T];  then NDTCell::rescaleCovariance once, with
 *     params.eval_factor.
 *   - the finalise step's Gaussian threshold is n_min = 2: every contribution already is a Gaussian.  One node under the identity
 *     pose on an identical grid therefore reproduces itself.
 *   - the destination maps' previous content is replaced.
 * PROVENANCE: perception_oru's NDTCell / NDTMap are restated from memory; no program text is copied.
 * DEVIATIONS:
 *   - OURS: a source cell with n < 2 counts as n = 2 (ndtgpu_mapset_set_cells installs n = 1; a Gaussian stands for at least two
 *     points).
 *   - saturation: params.maxnumpoints (1e5, fuser_hmt.cpp:486; <= 0: never) is applied ONCE at the end, where it only clamps the
 *     stored n -- mean and covariance do not depend on it.  Upstream saturates at every pairwise merge, which makes its result
 *     depend on the order of the merges.
 *   - order independence: a world's cells are the same bits for any order of its nodes in node_idx, in whichever batch it is
 *     assembled, and on repeated calls (the sums are 64-bit integers; the scales are a function of the world's own nodes).
 *   - occupancy: where the destination set has occupancies they are what a plain ndtgpu_mapset_build leaves on such a set --
 *     min(N log(0.6 / 0.4), 255) from the merged N for every touched cell, 0 elsewhere -- and then clamped to
 *     params.occupancy_limit where that is below 255.  Merging the nodes' own log-odds is out of scope.
 *   - the map's n_dropped counter (ndtgpu_mapset_counters) holds n_dropped + n_rejected of the world, saturated.
 * Room of the accumulators (nothing wraps silently).  The scales are ndt_build_shifts of the destination grid for the bound of
 * a cell's N -- the sum of n over ALL listed cells of the world, counted on the device in a first pass
 * (ndt_world_count_kernel); 2^32 or more: NDTGPU_ERR_CAPACITY.  They leave one cell^2 of second moment per point (sixteen on
 * grids with an odd axis, where LazyGrid's truncation lets |u| reach 2): n u_k^2 takes at most 1/4 (4) of it, so a contribution
 * is admitted where
 *        (n - 1) |Sigma'_kl| / res_dst^2  <=  (3/4) n     (12 n with an odd axis)      for all six entries,
 * and rejected otherwise.  A cell built from points of a grid with res_src <= res_dst always passes: its largest eigenvalue is
 * at most its trace <= 3 (res_src / 2)^2 n / (n - 1), and rescaleCovariance only raises the small eigenvalues.  That is why
 * res_dst < res_src is refused.
 * Device form (csrc/ndt_world.hip): sum n_i u_i and sum [(n_i - 1) Sigma'_i / res^2 + n_i u_i u_i^T], u = (mu' - cell origin) /
 * res, are exactly the "sum u" and "sum u u^T" of a virtual point set, so ndt_world_scatter_kernel -- one lane per source cell,
 * grid (chunks of a node's cells, listed node) -- writes the destination map's build scratch in the build's own format (NdtAcc
 * fixed point, every partial rounded once, integer atomics; work table, bitmap and accumulator ids allocated like phase A of
 * the build), and the build's unmodified finalise, rank and placement launches (csrc/ndt_build.hip ndt_launch_finalise) make
 * the Gaussians, the rank map and the counters.  Destination overflow (more world cells than max_cells) is the build's:
 * NdtMapCounters::overflow, reported in the result; the entries that read the map then return NDTGPU_ERR_CAPACITY as after a
 * build.  Plain launches in stream order; no floating-point atomics, no sort, no grid barrier.
 * Measured on MI355X (tools/world_cost.py, builder-run): node maps of the replay's layout (bench.py --config 4: 100 x 100 x 1 m at
 * 0.5 m, one build of a 20 000-point scan each, 246 Gaussian cells on average) into one world of 1360 x 1200 x 2 cells: 64 / 512
 * / 5000 nodes (11 k / 117 k / 1.23 M contributions -> 428 / 2804 / 24 173 world cells) in 0.18 / 0.23 / 0.88 ms per call, host
 * wall time around the synchronous call; 64 worlds of 64 nodes (1.02 M contributions) in one call: 0.85 ms.  The only route
 * without this call -- ndtgpu_mapset_export_cells per node, the NumPy merge of tests/world_model.py, ndtgpu_mapset_set_cells --
 * takes 100 / 96 / 979 ms and 814 ms on the same box (557 / 413 / 1114 and 953 times as long), yields the same cell counts, and
 * loses the point counts. */
typedef struct {
    double maxnumpoints;             /* end-of-chain clamp of the stored n (1e5, fuser_hmt.cpp:486; <= 0: never) */
    double eval_factor;              /* NDTCell::rescaleCovariance (1000) */
    double occupancy_limit;          /* (255) */
    double reserved_[2];
} ndtgpu_world_params;
void ndtgpu_default_world_params(ndtgpu_world_params *p);
typedef struct {
    int32_t  n_nodes;                /* listed nodes of the world */
    int32_t  n_cells;                /* Gaussian cells of the assembled map */
    int64_t  n_contributions;        /* Gaussian cells of the listed nodes */
    int64_t  n_dropped;              /* ... whose moved mean lies outside the destination grid */
    int64_t  n_rejected;             /* ... not finite, or beyond the accumulator's room */
    int64_t  n_points;               /* sum of merged N (before the maxnumpoints clamp) */
    int32_t  overflow;               /* NdtMapCounters::overflow of the destination map */
    int32_t  s1_shift;               /* the accumulators' scales: sum u 2^s1, sum u u^T 2^s2 (cell units) */
    int32_t  s2_shift;
    int32_t  pad_;
} ndtgpu_world_result;
/* node_offsets (count + 1), node_idx and T16 (16 doubles, column-major, per entry of node_idx from node_offsets[0] on) HOST;
 * prm NULL: the defaults; results HOST, `count` records, may be NULL.  NDTGPU_ERR_INVALID before any device work: offsets that
 * are not non-decreasing and dst_set == src_set with a destination map among the listed nodes (both before the device is looked
 * for and before a handle is read), a node index out of range, destination maps out of range (count <= 65535), destination res
 * smaller than source res.  Works on `stream` and returns when the maps and results are complete (synchronous, like
 * ndtgpu_overlap_score_batch).  Temporaries are gone on return; there is no handle: afterwards the destination maps are
 * ordinary maps of their set (ndtgpu_mapset_num_cells / export_cells / export_occupancy, ndtgpu_mcl_create, ndtgpu_match_*,
 * ndtgpu_mapset_pack_*). */
ndtgpu_status ndtgpu_world_assemble(ndtgpu_mapset *dst_set, size_t dst_first, size_t count, ndtgpu_mapset *src_set,
                                    const uint32_t *node_offsets, const uint32_t *node_idx, const double *T16,
                                    const ndtgpu_world_params *prm, ndtgpu_world_result *results, ndtgpu_stream stream);
/* the argument checks of ndtgpu_world_assemble on plain numbers (the sets' map counts and res, same_set: dst_set == src_set):
 * needs no handle and no device */
ndtgpu_status ndtgpu_world_check(size_t dst_n_maps, double dst_res, size_t dst_first, size_t count, size_t src_n_maps,
                                 double src_res, int same_set, const uint32_t *node_offsets, const uint32_t *node_idx);

/* ---- occupancy-grid export: a map rasterised the way lslgeneric::toOccupancyGrid fills a nav_msgs::OccupancyGrid --------------
 * What the reference's mapper publishes on a timer, and what navigation stacks and RViz consume (ndt_feature2d_fuser.cpp:428-433:
 * toOccupancyGrid(graph->getMap(), omap, occ_map_resolution_, world_frame) + moveOccupancyMap(omap, graph->getT()); :450-454 the
 * same for fuser->map).  ndtgpu_mapset_occupancy_grid* rasterises maps [first, first + count) of a set -- node maps, fused maps,
 * or a world of ndtgpu_world_assemble -- into int8 grids, one kernel launch for all of them.
 * Semantics (restated).  A map with centre c, size[] cells per axis of res metres; the pixel size r is occ_resolution:
 *   - size_m[k] = size[k] * res;  width = (int)(size_m[0] / r), height = (int)(size_m[1] / r);
 *     origin = (c.x - size_m[0] / 2, c.y - size_m[1] / 2, 0);  data is row-major, data[j * width + i], i along x, j along y.
 *   - pixel (i, j) is probed at p = (origin.x + (i + 0.5) r, origin.y + (j + 0.5) r, params.z) (params.z 0.0: upstream probes
 *     pcl::PointXYZ(px, py, 0)), in fp64, not contracted; its cell is LazyGrid::getIndexForPoint(p) -- per axis
 *     floor((p - c) / res + 0.5) + size / 2.0 truncated to int (csrc/ndt_math.h lazygrid_index_half) with the map's own centre.  A
 *     point outside the grid gives -1: in z when params.z leaves the grid, and -- LazyGrid's cells are centred on
 *     c + (k - size / 2) res -- in the last half cell of an axis with an even size, which belongs to no cell.
 *   - the value of a pixel whose cell has occupancy occ:  occ == 0 (never observed): -1;  occ < 0 (observed free): 0;
 *     occ > 0 and a Gaussian (mu, Sigma):  l = (p - mu)^T Sigma^-1 (p - mu),  v = 0.5 + 0.5 (exp(-l / 2) + 0.1),
 *     value = v > 1 ? 100 : (int8)(v * 100), truncated: 55 .. 100;  l not finite: -1;
 *     occ > 0 and no Gaussian: params.occupied_no_gaussian (100).
 *   - a set without occupancy arrays (no ndtgpu_mapset_enable_occupancy): a cell with a Gaussian counts as occ > 0, every other
 *     as occ == 0.  A world of ndtgpu_world_assemble on an occupancy-enabled set holds occ > 0 in touched cells and 0 elsewhere.
 *   - ndtgpu_occgrid_move is moveOccupancyMap (ros_utils.h:12-18): origin_pose <- T * origin_pose, a 4 x 4 product on the host.  The
 *     data is not resampled, as in the reference.
 * PROVENANCE: toOccupancyGrid lives in perception_oru (ndt_map/ndt_conversions.h), which is not part of the reference tree; it is
 * restated from memory, like NDTCell / NDTMap in SURVEY.md App. A; no program text is copied.  Uncertain in that recollection: what
 * a cell with occ > 0 and no Gaussian yields (upstream reads the inverse covariance of a cell that has none; a zero matrix gives
 * v = 1.05, hence 100) -- therefore a parameter.
 * DEVIATIONS:
 *   - OURS, pixel count: pixel centres are origin + (i + 0.5) r for exactly width x height pixels.  Upstream advances px += r in a
 *     floating-point loop, so its pixel count can differ from width * height by a row or a column.
 *   - OURS, inverse covariance: Sigma^-1 is recomputed from the stored covariance by the adjugate (csrc/ndt_occgrid.h
 *     ndt_occgrid_inverse), refusing only det <= 0 and a determinant that is not finite (-> -1); upstream keeps V Lambda^-1 V^T from
 *     rescaleCovariance.  Not the |det| > 1e-12 gate of the matcher's (C_i + C_j)^-1: a wall cell at 0.5 m with eigenvalues
 *     (0.02, 2e-5, 2e-5) has det 8e-12, and less spread falls below it.
 *   - a map whose build overflowed max_cells: the synchronous form returns NDTGPU_ERR_CAPACITY like the other readers; the
 *     asynchronous device form cannot report it and writes -1 to every pixel of that map.
 * Device form (csrc/ndt_occgrid.hip ndt_occgrid_kernel): grid (tiles of 256 x 4 pixels, map of the call); one lane owns 4 pixels
 * consecutive in x and writes them as one 32-bit store where the byte address is 4-aligned, with byte stores otherwise (row
 * tails, rows of a width that is no multiple of 4, a map whose first byte k * width * height is unaligned).  Per pixel one rank-map
 * word, and where a Gaussian is present its 80-byte cell, inverse, quadratic form and exp.  No atomics, no barriers: the bytes of
 * a map are the same in any batch and on any call.
 * Measured on MI355X (tools/occgrid_cost.py, builder-run): the replay's world (5000 node maps assembled into 1360 x 1200 x 2 cells
 * of 0.5 m, 24 173 Gaussian cells) at 0.1 m (6800 x 6000 = 40.8 M pixels) / 0.05 m (13600 x 12000 = 163.2 M pixels): device form
 * 0.16 / 0.42 ms (HIP events), host form 13.5 / 49.5 ms (wall: kernel + one copy to pageable memory + the counts); 64 node maps of
 * 100 x 100 m at 0.05 m (256 M pixels) in one call: 0.58 ms and 75 ms.  The output-write rate is 0.25 / 0.38 / 0.44 TB/s, 4 to 7 %
 * of the 6.29 TB/s copy ceiling: the kernel is NOT bound by its writes but by the fp64 index arithmetic of every pixel (one IEEE
 * division each; 99 % of the pixels are empty and cost nothing else).  The route without the call -- ndtgpu_mapset_export_cells + the
 * NumPy rasteriser of tests/occgrid_model.py -- takes 928 ms for the world at 0.1 m and 77 ms for one node map at 0.05 m on the same
 * box (69 and 37 times the host form), with no pixel outside the comparison band different. */
typedef struct {
    double  z;                       /* height the pixels are probed at (0.0) */
    int32_t occupied_no_gaussian;    /* value of a cell with occ > 0 and no Gaussian (100); an int8 */
    int32_t reserved_[5];
} ndtgpu_occgrid_params;
void ndtgpu_default_occgrid_params(ndtgpu_occgrid_params *p);
typedef struct {
    int32_t width, height;
    double  resolution;              /* occ_resolution */
    double  origin[3];               /* of pixel (0, 0)'s lower corner, in the map's frame */
    int64_t n_unknown, n_free, n_occupied;     /* pixels < 0, == 0, > 0: counted on the host from the copied grid */
} ndtgpu_occgrid_info;
/* width, height and origin of the grid of a map with the given geometry: plain numbers, needs no handle and no device (like
 * ndtgpu_world_check).  NDTGPU_ERR_INVALID: res or occ_resolution not positive and finite, an empty axis, width or height 0,
 * 2^30 pixels or more along an axis. */
ndtgpu_status ndtgpu_occgrid_dims(double res, const int32_t cells_per_axis[3], const double centre[3], double occ_resolution,
                                  int32_t *width, int32_t *height, double origin[3]);
/* the handle-dependent argument checks of ndtgpu_mapset_occupancy_grid* on plain numbers (the set's map count, the grid's width and
 * height): needs no handle and no device */
ndtgpu_status ndtgpu_occgrid_check(size_t n_maps, size_t first, size_t count, int32_t width, int32_t height);
/* out: `count` grids of width * height bytes back to back, map first + k at out + k * width * height.  prm NULL: the defaults.
 * NDTGPU_ERR_INVALID before any device work: occ_resolution not finite or <= 0 and a NULL output (both before the device is looked
 * for and before the handle is read), maps out of range, width or height 0, count * width * height beyond 2^40.
 * _device: out_dev DEVICE memory; asynchronous on `stream`.  The other form: out_host and info (`count` records, may be NULL)
 * HOST; works on `stream` and returns when they are complete.  Temporaries are gone on return (ndtgpu_live_resources is
 * unchanged by a call). */
ndtgpu_status ndtgpu_mapset_occupancy_grid_device(ndtgpu_mapset *set, size_t first, size_t count, double occ_resolution,
                                                  const ndtgpu_occgrid_params *prm, int8_t *out_dev, ndtgpu_stream stream);
ndtgpu_status ndtgpu_mapset_occupancy_grid(ndtgpu_mapset *set, size_t first, size_t count, double occ_resolution,
                                           const ndtgpu_occgrid_params *prm, int8_t *out_host, ndtgpu_occgrid_info *info,
                                           ndtgpu_stream stream);
/* moveOccupancyMap: moved16 = T16 * origin_pose16 (4 x 4, column-major; moved16 may be origin_pose16) */
void ndtgpu_occgrid_move(const double T16[16], const double origin_pose16[16], double moved16[16]);

/* ---- link gating: which loop-closure links exist -- candidate pairs and getValidLinks -----------------------------------------
 * The step of the chain scans -> feature sets -> seeded links -> registered links -> optimised poses -> world -> grid that decides
 * which links there are.  Twice in the reference:
 *   - computeAllPossibleLinks (ndt_feature_graph.cpp:395-405) enumerates every pair i < j of the nodes (i ascending, then j) and
 *     calls computeLink for each.  ndtgpu_linkgate_candidates enumerates the same pairs in the same order and keeps those worth
 *     matching: j - i >= min_idx_dist, and the nodes' own poses within max_dist / max_angle of each other
 *     (distanceBetweenAffine3d(T_i, T_j)).  The survivors are written compacted as the arrays ndtgpu_featbank_match_device and
 *     ndtgpu_match_batch_device take unchanged: uint32 ref = i, mov = j, and the initial guess T16 = T_i^-1 T_j.
 *   - getValidLinks (ndt_feature_graph.cpp:527-556) filters the registered links before every optimisation, inside the offline
 *     mapper's loop (ndt_feature_graph_opt.cpp:152-173): gate under the current node poses, optimise, gate again, until the number
 *     of links stops changing.  ndtgpu_linkgate_valid is that filter, ndtgpu_linkgate_gather packs T16 / cov36 / flags / indices of
 *     the links that stay behind the incremental links -- the contiguous arrays ndtgpu_pgo_set_links_device needs -- and only the
 *     keep list (4 bytes per kept link) visits the host, for the index arrays of that call.  With one handle per threshold set this
 *     is also how a ndtgpu_pgo bank gets "the same nodes under several getValidLinks thresholds".
 * Semantics (restated).  Poses are column-major 4 x 4 doubles.
 *   - distanceBetweenAffine3d(p1, p2) (utils.h:42-47):  dist = sqrt(dx^2 + dy^2 + dz^2) of t2 - t1;  r00 = col0(R1) . col0(R2);
 *     ang = fabs(acos(r00)) -- getRobustYawFromAffine3d (utils.h:30-40): the angle of the rotated x axis in the xy plane, its sign
 *     dropped by the fabs.  With clip_cosine r00 is clamped to [-1, 1] first.
 *   - a pair i < j stays when  j - i >= min_idx_dist  &&  dist < max_dist  &&  ang < max_angle  for (T_i, T_j); max_score is not
 *     read.  max_angle = +inf with clip_cosine = 1 switches the angle gate off.
 *   - link k (ref, mov, T, score) stays when  score <= max_score (not tested where score_dev is NULL)  &&
 *     |mov - ref| >= min_idx_dist  &&  dist < max_dist && ang < max_angle  for (T_mov, T_ref * T).  ref > mov is an ordinary link.
 *   - THE NaN RULE, upstream's and the default: acos of a cosine a rounding above 1 is NaN, NaN < max_angle is false, the link is
 *     rejected.  On a consistent graph (links exactly T_ref^-1 T_mov) that is about one link in six.  clip_cosine = 1 is the one
 *     place to switch it off.
 * PROVENANCE: restated from the reference files cited above; the defaults are ndt_feature_graph_opt.cpp:49-52.
 * DEVIATIONS:
 *   - the two of distanceBetweenAffine3d from upstream's p1.inverse() * p2 (both already in distributed.valid_links): the rigid
 *     transpose instead of a general inverse, and no rotation of the difference vector (a rotation keeps its length).  T_ref * T
 *     and T_i^-1 T_j are rigid products as well: the last row is written as 0 0 0 1.
 *   - the operation order is fixed and NOT fused (csrc/ndt_linkgate.h states it; tests/linkgate_model.py follows it), the arc
 *     cosine is the library's own (csrc/ndt_pgo.h ndt_pgo_acos), the same bits on host and device -- within an ulp or two of libm's.
 *   - a NaN score is rejected (score <= max_score is false); upstream's "score > maxScore -> skip" would keep it.
 *   - OURS: a link with an index >= n_nodes is rejected, on the device (upstream reads past its vector); a result larger than the
 *     capacity given is truncated and reported (ndtgpu_linkgate_count), not an error status; max_rounds of the gated loop
 *     (binding.optimize_gated, host/ndt_link_gate_gpu.h optimizeGraphGated): upstream's loop has no cap and can oscillate.
 * Device form (csrc/ndt_linkgate.hip): an ordered selection in three plain launches, with no workgroup waiting on another (no
 * look-back spin, no grid barrier, no atomics): a flag-and-count pass (one count per tile of 1024 consecutive items), a scan of
 * the tile counts by one workgroup, an emit pass that evaluates the gate again and ranks within the tile (csrc/ndt_block.h
 * ndt_block_rank).  Pairs run over a 64-bit linear index; its decoding to (i, j) proposes the row with a square root and settles it
 * in integers.  The output is in input order and the same bits on any run; a link's fate does not depend on its batch.  The gather
 * moves 4-byte words, one lane per word, and reads the count on the device.
 * Calls on one handle are ordered on the device (each waits for the previous one, whatever stream that one named).
 * Measured on MI355X (tools/linkgate_cost.py, HIP events, library 0.9.0): candidates of 5000 nodes (12 497 500 pairs, 119 651 kept, with
 * T16) 0.31 ms, of 500 nodes 0.030 ms -- distributed.all_pairs + the NumPy gate + the initial guesses take 414 ms and 88 ms on the same
 * box; valid of 44 486 links 0.026 ms, with the gathers of T16, cov36 and flags 0.045 ms (distributed.valid_links 9.5 ms + 1.1 ms of
 * fancy indexing); valid of 12 497 500 links 0.49 ms, with the gathers of the 3.83 M links that stay 1.66 ms (3130 ms + 391 ms).
 * Both sides decide the same links in all four cases. */
typedef struct ndtgpu_linkgate ndtgpu_linkgate;
typedef struct {
    double  max_score;               /* a link's score at most (0.1) */
    double  max_dist;                /* metres, strict (1.0) */
    double  max_angle;               /* radians, strict (0.2) */
    int32_t min_idx_dist;            /* node indices apart at least (2) */
    int32_t clip_cosine;             /* 0: upstream's NaN rule; 1: the cosine is clamped to [-1, 1] before acos */
} ndtgpu_linkgate_params;
/* 0.1, 1.0, 0.2, 2 (ndt_feature_graph_opt.cpp:49-52) and clip_cosine = 0 */
void ndtgpu_default_linkgate_params(ndtgpu_linkgate_params *p);
/* the argument checks of the entries below on plain numbers (a handle's max_nodes / max_links; the call's n_nodes, n_links and
 * row_bytes, 0 where the call has none): needs no handle and no device.  NDTGPU_ERR_INVALID: max_nodes 0 or > 65536, max_links
 * > 2^27, row_bytes no multiple of 4 or > 4096;  NDTGPU_ERR_CAPACITY: n_nodes > max_nodes, n_links > max_links. */
ndtgpu_status ndtgpu_linkgate_check(size_t max_nodes, size_t max_links, size_t n_nodes, size_t n_links, size_t row_bytes);
/* room for max_nodes node poses (1 .. 65536), the tile counts of their pairs and of max_links links (<= 2^27), and a keep list of
 * max_links entries */
ndtgpu_status ndtgpu_linkgate_create(size_t max_nodes, size_t max_links, ndtgpu_linkgate **out);
ndtgpu_status ndtgpu_linkgate_destroy(ndtgpu_linkgate *h);
/* the node poses: T16 HOST n_nodes x 16 column-major -- what ndtgpu_pgo_poses returns as T16_out.  Synchronous. */
ndtgpu_status ndtgpu_linkgate_set_nodes(ndtgpu_linkgate *h, size_t n_nodes, const double *T16);
/* the same from DEVICE memory, asynchronous on `stream` */
ndtgpu_status ndtgpu_linkgate_set_nodes_device(ndtgpu_linkgate *h, size_t n_nodes, const double *T16_dev, ndtgpu_stream stream);
/* every pair i < j of the set nodes through the candidate gate; survivors compacted in enumeration order into ref_idx_dev /
 * mov_idx_dev (uint32) and T16_dev (16 doubles each; may be NULL), DEVICE arrays of `capacity` entries.  prm NULL: the defaults.
 * Asynchronous on `stream`. */
ndtgpu_status ndtgpu_linkgate_candidates(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, uint32_t *ref_idx_dev,
                                         uint32_t *mov_idx_dev, double *T16_dev, size_t capacity, ndtgpu_stream stream);
/* getValidLinks of n_links registered links under the set nodes: ref_idx_dev / mov_idx_dev (uint32), T16_dev (n_links x 16) and
 * score_dev (n_links doubles, or NULL: no score test) DEVICE.  The ascending indices of the links that stay go to the handle's
 * keep list and, where keep_dev (DEVICE, `capacity` uint32) is not NULL, to it.  Asynchronous on `stream`. */
ndtgpu_status ndtgpu_linkgate_valid(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, size_t n_links, const uint32_t *ref_idx_dev,
                                    const uint32_t *mov_idx_dev, const double *T16_dev, const double *score_dev, uint32_t *keep_dev,
                                    size_t capacity, ndtgpu_stream stream);
/* the two selections with every array in HOST memory (the host mirror's form, host/ndt_link_gate_gpu.h): synchronous, on the
 * handle's own stream; device temporaries are gone on return (ndtgpu_live_resources is unchanged by a call).  _candidates_host
 * writes min(count, capacity) survivors (capacity 0 with NULL arrays: only the count, read with ndtgpu_linkgate_count);
 * _valid_host leaves the keep list in the handle (ndtgpu_linkgate_count, ndtgpu_linkgate_keep). */
ndtgpu_status ndtgpu_linkgate_candidates_host(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, uint32_t *ref_idx, uint32_t *mov_idx,
                                              double *T16, size_t capacity);
ndtgpu_status ndtgpu_linkgate_valid_host(ndtgpu_linkgate *h, const ndtgpu_linkgate_params *prm, size_t n_links, const uint32_t *ref_idx,
                                         const uint32_t *mov_idx, const double *T16, const double *score);
/* for the keep list of the last ndtgpu_linkgate_valid call: row keep[k] of src_dev becomes row dst_first_row + k of dst_dev, rows
 * of row_bytes bytes (a multiple of 4, at most 4096: T16 128, cov36 288, flags and indices 4, result records), both 4-aligned.
 * The count is read on the device: no host wait.  dst_dev has room for dst_first_row + (the links of that call) rows, or for what
 * the caller knows the count to be; dst_first_row is where the caller has put the incremental links, in front.  Asynchronous on
 * `stream`. */
ndtgpu_status ndtgpu_linkgate_gather(ndtgpu_linkgate *h, const void *src_dev, size_t row_bytes, void *dst_dev, size_t dst_first_row,
                                     ndtgpu_stream stream);
/* how many pairs or links the handle's last candidates / valid call kept; waits for the handle.  A result larger than the call's
 * capacity wrote nothing beyond it: *count is still the true count and *overflow (may be NULL) is 1.  Not an error status. */
ndtgpu_status ndtgpu_linkgate_count(ndtgpu_linkgate *h, size_t *count, int32_t *overflow);
/* entries [first, first + n) of the last valid call's keep list to HOST memory; waits for the handle */
ndtgpu_status ndtgpu_linkgate_keep(ndtgpu_linkgate *h, size_t first, size_t n, uint32_t *keep);

/* single pair convenience == graph.cpp:273 */
ndtgpu_status ndtgpu_match_d2d(ndtgpu_mapset *target_set, size_t target_map, ndtgpu_mapset *source_set,
                               size_t source_map, double T16[16], const ndtgpu_match_params *prm,
                               ndtgpu_match_result *result);

/* ---- profiling hooks ------------------------------------------------------------------ */
/* When enabled, every build launched on `set` and every match whose TARGET set is `set` is
 * bracketed by HIP events recorded on the launch stream (kernel only: table reset and copies are
 * outside the bracket).  ndtgpu_last_kernel_ms waits for the end event and returns the duration
 * of the most recent launch of kernel `which` (0 build, 1 match). */
ndtgpu_status ndtgpu_profiling_enable(ndtgpu_mapset *set, int on);
ndtgpu_status ndtgpu_last_kernel_ms(ndtgpu_mapset *set, int which, float *ms);
/* raw per-map build counters: 8 x uint32 {n_alloc, n_cells, overflow, n_dropped, shader clocks of
 * build phases A (accumulate), B (finalise), C (rank), D (clean)} */
ndtgpu_status ndtgpu_mapset_counters(ndtgpu_mapset *set, size_t map, uint32_t out[8]);
/* kernel names as they appear in rocprofv3 --kernel-trace, for bench.py / profiles/ */
const char *ndtgpu_kernel_name(int which); /* 0 build, 1 match, 2 derivatives */

/* test aid: resources the library currently owns, process-wide */
ndtgpu_status ndtgpu_live_resources(uint64_t counts[4]);
/* device buffers, pinned buffers, events, streams */

/* ---- feature-set RANSAC matching: the seed of every loop-closure link -------------------------------------------------------
 * The offline mapper's first step, computeAllPossibleLinks (ndt_feature_graph.cpp:395-405; ndt_feature_graph_opt.cpp:95 builds the
 * graph it runs on), calls computeLink (ndt_feature_graph.cpp:162-177) for every pair of nodes, and computeLink seeds link.T with
 * matchNodesUsingFeatureMap (ndt_feature_node.h:256) -> matchFeatureMap (ndt_feature_map.h:104-122): flirtlib's
 * RansacFeatureSetMatcher(0.0599, 0.9, 0.1, 0.6, 0.0499, false).matchSets(ref, mov, transform, matches) on BetaGrid descriptors
 * under SymmetricChi2Distance.  The fuser makes the same call for the correspondences of its feature term
 * (ndt_feature_fuser_hmt.cpp:251 with the matcher member of ndt_feature_fuser_hmt.h:213; the flirtlib <-> Eigen conversions are
 * flirtlib_utils.h:32-42), which ndtgpu_match_fusion_feat_batch consumes.  ndtgpu_featbank_* is that call for a batch of
 * (ref, mov) pairs of feature sets kept in device memory, one workgroup per pair, all pairs in one launch.
 * PROVENANCE: flirtlib is not vendored by the reference -- only its call sites and parameters are.  The algorithm below is
 * restated from memory, as perception_oru's is; no program text of either is copied.
 * Semantics (restated).  A feature set holds n points, each a position (x, y, theta) and a descriptor of desc_len doubles
 * (BetaGrid: bin_rho 4 x bin_phi 12 = 48).  For a pair (ref, mov):
 *   1. descriptor distance d(a, b) = 0.5 * sum_k (a_k - b_k)^2 / (a_k + b_k) over the bins with a_k + b_k > 0, summed in
 *      ascending k.
 *   2. candidates: for every mov point i in ascending order the ref point j of smallest distance (strict <, ascending j: the
 *      lowest j wins ties); (i, j) is kept where the distance is < distance_threshold.  n_c of them.  n_c < 2, or
 *      n_c * inlier_probability < 2, or an empty set: NDTGPU_FEATMATCH_TOO_FEW.
 *   3. H = ceil(log(1 - success_probability) / log(1 - inlier_probability^2)) hypotheses (230 at the defaults); hypothesis h
 *      pairs the candidates a = floor(u(seed, 0, h) * n_c) and b = floor(u(seed, 1, h) * (n_c - 1)), plus 1 if b >= a, with u
 *      the counter-based uniform of the Monte Carlo localisation (csrc/ndt_mcl.h ndt_hash_uniform).
 *   4. rigidity: f, g the squared distances between the two mov and between the two ref points; the hypothesis is skipped
 *      where f + g == 0 or (f - g)^2 / (8 (f + g)) > rigidity_threshold.
 *   5. pose from correspondences (compute2DPose), p the mov and q the ref points: centroids subtracted, A = sum dp . dq,
 *      B = sum (dp.x dq.y - dp.y dq.x), h = sqrt(A^2 + B^2), (c, s) = (A / h, B / h) or (1, 0) where h == 0,
 *      t = mean_q - R mean_p.  The pose maps mov into ref: computeLink's link.T.
 *   6. verification (verifyHypothesis) over ALL mov points: the point moved by the hypothesis, its nearest ref point by squared
 *      Euclidean distance (strict <, ascending j); d^2 < acceptance_threshold adds d^2 to the score and (i, j) to the inliers,
 *      otherwise acceptance_threshold is added.  The threshold is compared with the SQUARED distance, as upstream.
 *   7. the best hypothesis has the smallest score, ties to the lowest h.  Every hypothesis skipped:
 *      NDTGPU_FEATMATCH_NO_HYPOTHESIS (upstream: a NaN transform, and matchFeatureMap returns max()).
 *   8. refinement: step 5 over the best hypothesis's inliers, then step 6 with that pose: the reported score, pose and
 *      correspondences (ascending i).
 * DEVIATIONS:
 *   - upstream draws the two samples from a default-seeded boost::mt19937 and redraws the second until it differs from the
 *     first; here the draws are counter-based, so a pair's samples depend on (seed, h, n_c) alone -- not on the pairs matched
 *     before it.
 *   - the rotation is carried as (c, s); theta = atan2(s, c) is only reported.
 *   - only the non-adaptive matcher (the `false` of the constructor call) is offered: params.adaptive != 0 is refused.
 *   - a best hypothesis with an empty inlier set (possible only with thresholds far from the defaults) keeps its own pose in
 *     step 8.
 *   - desc_len <= 128 and max_points <= 1024 (the kernel's LDS tiles).
 * A pair that ends with a status other than NDTGPU_FEATMATCH_OK has score 1e17, the identity pose and no correspondences.
 * Device form (csrc/ndt_featmatch.hip, ndt_featmatch_kernel): one workgroup of 256 threads per pair.  Both sets' positions are
 * staged in LDS; step 2 streams the ref descriptors through an LDS tile with a lane per mov point and compacts the kept
 * candidates in order with a prefix sum; steps 3-7 run one wave per hypothesis, four at a time, the ref positions read from LDS
 * by every lane at once; step 8 is two more sweeps by the whole workgroup.  Every sum has one fixed order that depends on the
 * pair's own sizes only, so a pair's outputs are the same bits whichever batch, position or batch size it runs in.  No
 * environment switches.
 * Measured on MI355X (tools/featmatch_cost.py, builder-run; defaults, 230 hypotheses, 60 % of a pair's points in common): 1024
 * pairs of sets of 64 / 256 / 1024 points: 1.23 / 5.77 / 88.2 ms; the replay's 44 486 gated edges at 128 points: 79.8 ms.  No
 * baseline exists: flirtlib cannot be built here. */
typedef struct ndtgpu_featbank ndtgpu_featbank;
typedef struct {
    double acceptance_threshold;     /* on the squared distance of a moved point to its nearest ref point (0.0599) */
    double success_probability;      /* (0.9) */
    double inlier_probability;       /* (0.1) */
    double distance_threshold;       /* on the descriptor distance of a candidate (0.6) */
    double rigidity_threshold;       /* (0.0499) */
    uint64_t seed;                   /* the key of the sample draws (see DEVIATIONS; 0) */
    int32_t adaptive;                /* must be 0: the adaptive matcher is not offered */
    int32_t pad_;
} ndtgpu_featmatch_params;
/* ndt_feature_map.h:104-122: RansacFeatureSetMatcher(0.0599, 0.9, 0.1, 0.6, 0.0499, false) */
void ndtgpu_default_featmatch_params(ndtgpu_featmatch_params *p);
enum {
    NDTGPU_FEATMATCH_OK = 0,
    NDTGPU_FEATMATCH_TOO_FEW = 1,         /* step 2: too few candidates, or an empty set */
    NDTGPU_FEATMATCH_NO_HYPOTHESIS = 2,   /* step 7: no sample passed the rigidity test */
    NDTGPU_FEATMATCH_BAD_INDEX = 3        /* a set index of the pair is >= n_sets (checked on the device) */
};
typedef struct {
    double score;                    /* step 8's score; 1e17 unless status is OK */
    double x, y, theta;              /* the pose that maps mov into ref; theta = atan2(s, c) */
    double c, s;                     /* its rotation as carried */
    int32_t n_candidates;            /* n_c */
    int32_t n_hypotheses;            /* H */
    int32_t n_tested;                /* hypotheses that passed the rigidity test */
    int32_t best_hypothesis;         /* h of the best one, -1 where there is none */
    int32_t n_inliers;               /* correspondences reported */
    int32_t status;                  /* NDTGPU_FEATMATCH_* */
} ndtgpu_featmatch_result;
/* room for n_sets feature sets of up to max_points points (1 .. 1024) with descriptors of desc_len doubles (1 .. 128); every set
 * starts empty */
ndtgpu_status ndtgpu_featbank_create(size_t n_sets, size_t max_points, size_t desc_len, ndtgpu_featbank **out);
ndtgpu_status ndtgpu_featbank_destroy(ndtgpu_featbank *h);
/* installs set k.  HOST arrays: pos3 n x (x, y, theta), desc n x desc_len row-major.  n <= max_points (NDTGPU_ERR_CAPACITY
 * otherwise); n = 0 empties the set (pos3 / desc may then be NULL).  The arguments are checked before the handle is read and the
 * device is looked for.  Synchronous. */
ndtgpu_status ndtgpu_featbank_set(ndtgpu_featbank *h, size_t k, size_t n, const double *pos3, const double *desc);
/* matches n_pairs pairs (ref_idx[p], mov_idx[p]) of sets, HOST index arrays, in ONE launch, asynchronous on `stream`; prm NULL:
 * the defaults.  The results stay in the handle for ndtgpu_featbank_results.  Calls on one handle are ordered (each waits, on
 * the device, for the previous one, whatever stream that one named). */
ndtgpu_status ndtgpu_featbank_match(ndtgpu_featbank *h, const uint32_t *ref_idx, const uint32_t *mov_idx, size_t n_pairs,
                                    const ndtgpu_featmatch_params *prm, ndtgpu_stream stream);
/* the same on DEVICE arrays: ref_idx_dev / mov_idx_dev n_pairs set indices; results_dev n_pairs records; T16_dev n_pairs x 16
 * doubles, column-major 4x4 built from (c, s, x, y) without trigonometry -- it can be handed to ndtgpu_match_batch_device as
 * the initial guesses unchanged; corr_dev n_pairs x max_points x 2 uint32 (mov_i, ref_j), a pair's entries beyond its n_inliers
 * unspecified.  T16_dev and corr_dev may be NULL. */
ndtgpu_status ndtgpu_featbank_match_device(ndtgpu_featbank *h, const uint32_t *ref_idx_dev, const uint32_t *mov_idx_dev,
                                           size_t n_pairs, const ndtgpu_featmatch_params *prm,
                                           ndtgpu_featmatch_result *results_dev, double *T16_dev, uint32_t *corr_dev,
                                           ndtgpu_stream stream);
/* pairs [first, first + count) of the last ndtgpu_featbank_match: HOST results count records, T16 count x 16, corr
 * count x max_points x 2 (any may be NULL).  Waits for that call. */
ndtgpu_status ndtgpu_featbank_results(ndtgpu_featbank *h, size_t first, size_t count, ndtgpu_featmatch_result *results, double *T16,
                                      uint32_t *corr);

/* ---- laser-scan feature extraction: the interest points and descriptors that the matcher above consumes ---------------------
 * The reference makes features for every scan it fuses: detector_->detect(*reading, pts) and descriptor_->describe(*p, *reading)
 * (ndt_feature2d_fuser.cpp:766-779, publish_graph_message.cpp:1401-1404) with the objects of flirtlib_utils.h:15-42 --
 * SimpleMinMaxPeakFinder(0.34, 0.001), CurvatureDetector(peak, 5, 0.2, 1.4, 2.0) with setUseMaxRange(false) and
 * BetaGridGenerator(0.02, 1.0, 4, 12) -- on a reading built by flirtlib_ros::fromRos (conversions.cpp:69-82): angles
 * angle_min + i * angle_increment, the ranges, the sensor at the origin.  ndtgpu_featbank_extract* is that for a batch of scans
 * in ONE launch, one workgroup per scan; scan b fills set set_idx[b] of the bank, where ndtgpu_featbank_match* finds it with no
 * host round trip: scan -> features -> RANSAC seed -> D2D registration -> gating -> pose-graph optimisation.
 * PROVENANCE: flirtlib is not vendored by the reference -- only its call sites and parameters are.  The algorithm below is
 * restated from memory of what such a detector and descriptor do and is THIS project's specification; no program text of
 * flirtlib or of the reference is copied.
 * Semantics (restated).  A scan is n_beams ranges; beam i looks along angle_min + i * angle_increment, and the sensor is at the
 * origin of the frame the features are reported in.
 *   1. valid points: beam i is valid iff its range is finite and r_min < r < r_max; the valid points p_k = r (cos, sin) in beam
 *      order, m of them.  m < 3: NDTGPU_FEATEXTRACT_TOO_FEW_POINTS and an empty set.
 *   2. chain: d_k = |p_k - p_(k-1)|; a new segment starts at k iff d_k > dmst; the arc length g_0 = 0, g_k = g_(k-1) + d_k.  The
 *      scan is not closed: beam 0 and the last beam are not neighbours.
 *   3. scale space: level s = 0 .. scales - 1 has sigma_s = base_sigma * sigma_step^s.  The window of k is the set of j in k's
 *      segment with |g_j - g_k| <= 3 sigma_s; S_s(k) = sum w_j p_j / sum w_j with w_j = exp(-(g_j - g_k)^2 / (2 sigma_s^2)), both
 *      sums over the window in ascending j; n_s(k) = S_s(k) - p_k and the response R_s(k) = |n_s(k)| / sigma_s.  k is ELIGIBLE at
 *      level s iff g_k - g_first >= 3 sigma_s and g_last - g_k >= 3 sigma_s within its segment (the one-sided windows of
 *      occlusion edges would give responses near 0.8).
 *   4. peaks (SimpleMinMaxPeakFinder::isPeak as recalled): (s, k) is a peak iff k is eligible at s, R_s(k) > min_value,
 *      R_s(k) - R_s(k-1) > min_diff and R_s(k) - R_s(k+1) > min_diff; the neighbours' responses whether eligible or not.
 *   5. one level per point: among the peaks of one k the level of the largest R is kept, ties to the lowest s.
 *   6. separation: a kept peak k is dropped iff another kept peak k' of step 5 in the same segment has |g_k' - g_k| <
 *      min_separation and R' > R, or R' == R and k' < k.  One pass over the step-5 set, not iterated.
 *   7. interest point: position p_k, theta = atan2(n_s(k).y, n_s(k).x) -- it points to the inside of the corner --, level s and
 *      beam i; the points of a scan in ascending beam order.
 *   8. BetaGrid descriptor of (x, y, theta), bin_rho * bin_phi bins indexed a * bin_phi + c.  A location q has the bin of
 *      l = R(-theta)(q - (x, y)), rho = |l|, phi = atan2(l.y, l.x): iff min_rho <= rho < max_rho, a = floor((rho - min_rho) / drho)
 *      with drho = (max_rho - min_rho) / bin_rho, c = min(floor((phi + pi) / (2 pi / bin_phi)), bin_phi - 1).  HITS: every valid
 *      point of the scan that has a bin adds 1 to it.  MISSES: the beam of every valid point q is sampled at
 *      q (1 - u delta / |q|), u = 1, 2, ... while u delta < |q|, delta = drho / 2; a bin holding at least one sample of the beam
 *      gets ONE miss from it, except the bin that q itself hits.  Bin b holds (hit_b + 1) / (hit_b + miss_b + 2), the mean of the
 *      Beta posterior; not normalised.
 * DEVIATIONS:
 *   - flirtlib's CurvatureDetector smooths over geodesic distances in a minimum spanning tree of the scan points with edges up
 *     to dmst; here the tree is the chain of consecutive valid beams, broken at gaps above dmst.
 *   - the response and its normalisation are this project's, and so is what 0.34 means on it: a corner turning more than about
 *     50 degrees, from sqrt(2 / pi) sin(turn / 2) > 0.34 (a noise-free right angle: 0.564 in the continuum, 0.60-0.61 sampled at
 *     1 degree).  It is not calibrated against flirtlib.
 *   - eligibility (step 3) and the separation of step 6 (min_separation) are this project's.
 *   - the misses come from fixed-step samples of the beam, not from flirtlib's traversal of the grid.
 *   - limits: bin_rho * bin_phi <= 64, scales <= 8, n_beams <= 2048.
 * Device form (csrc/ndt_featextract.hip, ndt_featextract_kernel): one workgroup of 256 threads per scan.  Steps 1-2 are ordered
 * compactions and prefix sums over the workgroup, step 3 a lane per point level by level with the window found by walking from k,
 * step 8 a wave per keypoint with a lane per beam, the visited bins as a 64-bit mask and integer LDS atomics.  fp64 throughout;
 * every sum has one fixed order that depends on the scan alone, so a scan's outputs are the same bits in any batch, at any
 * position and for any batch size.  The set indices of one call must differ from each other.  No environment switches.
 * Measured on MI355X (tools/featextract_cost.py, builder-run; defaults, synthetic halls, 1024 scans of 360 / 720 / 1440 beams):
 * the extraction alone 0.22 / 0.46 / 1.41 ms (0.2 / 0.5 / 1.4 us a scan, 6 / 8 / 9 interest points a scan), the extraction and the matching
 * of the 1023 pairs of consecutive scans 0.40 / 0.64 / 1.59 ms.  No baseline exists: flirtlib cannot be built here. */
typedef struct {
    int32_t scales;                  /* levels of the scale space, 1 .. 8 (5) */
    int32_t bin_rho;                 /* rings of the descriptor (4) */
    int32_t bin_phi;                 /* sectors of the descriptor (12); bin_rho * bin_phi <= 64 and == the bank's desc_len */
    int32_t pad_;
    double base_sigma;               /* sigma of level 0, metres of arc length (0.2) */
    double sigma_step;               /* ratio of consecutive levels, > 1 (1.4) */
    double dmst;                     /* a gap between consecutive valid points above this starts a new segment (2.0) */
    double min_value;                /* a peak's response is above this (0.34) */
    double min_diff;                 /* ... and above both neighbours' by more than this (0.001) */
    double min_rho;                  /* the descriptor's inner radius (0.02) */
    double max_rho;                  /* ... and outer radius (1.0) */
    double min_separation;           /* step 6, metres of arc length (0.2; this project's) */
    double r_min;                    /* a valid range is above this (0.5) */
    double r_max;                    /* ... and below this (30.0) */
} ndtgpu_featextract_params;
/* flirtlib_utils.h:15-42; min_separation 0.2; r_min / r_max: the launch files' min and sensor range */
void ndtgpu_default_featextract_params(ndtgpu_featextract_params *p);
enum {
    NDTGPU_FEATEXTRACT_OK = 0,
    NDTGPU_FEATEXTRACT_TOO_FEW_POINTS = 1,   /* step 1: fewer than 3 valid points; the set is emptied */
    NDTGPU_FEATEXTRACT_OVERFLOW = 2,         /* n_found > the bank's max_points: the first max_points in beam order are stored */
    NDTGPU_FEATEXTRACT_BAD_INDEX = 3         /* the scan's set index is >= n_sets (checked on the device); nothing is written */
};
typedef struct {
    int32_t n_valid;                 /* m */
    int32_t n_segments;
    int32_t n_peaks;                 /* peaks (s, k) of step 4, every level counted */
    int32_t n_found;                 /* interest points after step 6 */
    int32_t n_stored;                /* min(n_found, max_points): the set's count */
    int32_t status;                  /* NDTGPU_FEATEXTRACT_* */
} ndtgpu_featextract_result;
/* extracts n_scans scans, HOST ranges n_scans x n_beams (through a pinned staging buffer) and HOST set indices, in ONE launch,
 * asynchronous on `stream`; prm NULL: the defaults.  The bank's desc_len must equal bin_rho * bin_phi (NDTGPU_ERR_INVALID).  The
 * arguments and parameters are checked before the handle is read and the device is looked for.  The records stay in the handle
 * for ndtgpu_featbank_extract_results.  Ordered against the handle's other calls like ndtgpu_featbank_match. */
ndtgpu_status ndtgpu_featbank_extract(ndtgpu_featbank *h, const uint32_t *set_idx, const double *ranges, size_t n_scans, size_t n_beams,
                                      double angle_min, double angle_increment, const ndtgpu_featextract_params *prm,
                                      ndtgpu_stream stream);
/* the same on DEVICE arrays, fully asynchronous: set_idx_dev n_scans set indices, ranges_dev n_scans x n_beams; results_dev
 * n_scans records; beam_dev / level_dev / response_dev n_scans x max_points, a scan's entries beyond its n_stored unspecified
 * (each may be NULL) */
ndtgpu_status ndtgpu_featbank_extract_device(ndtgpu_featbank *h, const uint32_t *set_idx_dev, const double *ranges_dev, size_t n_scans,
                                             size_t n_beams, double angle_min, double angle_increment,
                                             const ndtgpu_featextract_params *prm, ndtgpu_featextract_result *results_dev,
                                             uint32_t *beam_dev, int32_t *level_dev, double *response_dev, ndtgpu_stream stream);
/* scans [first, first + count) of the last ndtgpu_featbank_extract: HOST results count records; beam, level and response
 * count x max_points (any may be NULL).  Waits for that call. */
ndtgpu_status ndtgpu_featbank_extract_results(ndtgpu_featbank *h, size_t first, size_t count, ndtgpu_featextract_result *results,
                                              uint32_t *beam, int32_t *level, double *response);
/* reads set k back, however it was filled (ndtgpu_featbank_set or an extraction): *n its count, HOST pos3 max_points x 3 and desc
 * max_points x desc_len of room (either may be NULL), the first *n rows written, the descriptors row-major.  Waits for the
 * handle's last call. */
ndtgpu_status ndtgpu_featbank_get(ndtgpu_featbank *h, size_t k, size_t *n, double *pos3, double *desc);

/* ---- the fuser bank's feature path: the FLIRT feature term of the registration and the node feature maps ------------------------
 * NDTFeatureFuserHMT::update (ndt_feature_fuser_hmt.cpp:108-512) with Params::useFeat (true in Params()): per scan it matches the
 * scan's interest points against the previous scan's with the RANSAC set matcher (:251), gates the result against the odometry
 * (:279-289), turns the correspondences into fixed-covariance NDT cell pairs (:299-300;
 * convertCorrespondencesToCellvectorsFixedCovWithCorr, conversions.h:52-83), puts them IN FRONT of the 40 odometry cells of
 * matchFusion (:304-357), and afterwards moves the points to the new pose and appends them to the fuser's NDTFeatureMap (:497-502;
 * NDTFeatureMap::update, ndt_feature_map.h:62-68) -- the map that matchNodesUsingFeatureMap (ndt_feature_node.h:254-256) later
 * matches between nodes.  With a feature bank attached the fuser bank does all of it on the caller's stream with no host visit:
 * scan -> ndtgpu_featbank_extract_device -> ndtgpu_fuser_update_batch_feat -> the node's feature map -> ndtgpu_featbank_match*.
 * PROVENANCE: restated from the cited lines of the reference; flirtlib itself is not vendored (see the RANSAC section above).
 * Semantics (restated).  Per fuser slot three sets of the attached ndtgpu_featbank:
 *   cur   the scan's interest points in the sensor frame: named per call, READ ONLY.
 *   prev  ptsPrev: set prev_set_first + slot.
 *   map   featuremap.map: set map_set_first + slot.
 *   1. RANSAC (:251): ndt_featmatch_kernel unchanged on the pair (ref = prev, mov = cur) with prm.match -- ransac_'s constructor
 *      arguments (ndt_feature_fuser_hmt.h:213), which are the defaults.  Skipped when use_feat == 0.
 *   2. feature pose (:252-255): Tfeat = Tfeat_sensor * sensor_pose^-1, Tfeat_sensor the 4x4 built from (c, s, x, y) exactly as
 *      ndtgpu_featbank_match_device's T16.
 *   3. consistency gate (:279-289): the features are INCONSISTENT iff the RANSAC status is not OK or it has no inliers, or
 *      check_consistency is set and, with diff = (Tnow * Tmotion)^-1 * Tfeat, |diff.translation| > max_translation_norm / 10 or
 *      |eulerAngles(0,1,2)(diff)| > max_rotation_norm / 4 (the norms of the post-registration gate).
 *   4. feature cells (:294-325): for correspondence (i, j) in the reported order (ascending i) the source cell has mean
 *      (x_i, y_i, 0) of cur, the target cell mean (x_j, y_j, 0) of prev AS STORED, both covariance diag(feat_cov) ((2e-4, 2e-4,
 *      1e-4), :249); both are pseudo-transformed by sensor_pose, then by Tnow (Tinit = Tnow under globalTransf, the only mode the
 *      bank covers): mean' = T mean, cov' = R cov R^T, the loops of ndtgpu_fuser_prepare.  RESTATED AS WRITTEN, quirk included:
 *      the stored prev points are already in the map frame when the previous call moved them, and both transforms are applied
 *      again all the same.
 *   5. cell order: the FLIRT cells first -- only if use_feat is set, the features are consistent and fusion2d is off (the bank
 *      passes no cells in fusion2d) -- then the 40 odometry cells if use_odom (the last source cell un-rotated, as
 *      ndtgpu_fuser_prepare hands them out).  A slot that ends with no cells is run by the rule ndtgpu_match_fusion_feat_batch
 *      documents for registrations without correspondences; with neither odometry cells nor consistent features this is
 *      upstream's use_odom_or_features = false (:341-347).
 *   6. after the pose update (:497-502): prev <- cur.  With update_feature_map every point is moved by Tnow_new * sensor_pose --
 *      P = the 4x4 of pose2d(x, y, theta), M = T * P, x' = M[12], y' = M[13], theta' = eulerAngles(0,1,2)(M)[2], descriptors
 *      copied (moveInterestPointVec) -- and NDTFeatureMap::update runs: when the slot's call counter is a multiple of map_every
 *      (4) the moved points are appended to map; the counter advances either way.  Without update_feature_map prev <- cur
 *      unmoved and the counter stays.
 *   7. initialize (:78-85): prev <- cur moved by initPose * sensor_pose, then the map update: the counter is 0, so it appends.
 * DEVIATIONS:
 *   - the (c, s) pose: upstream goes through the matcher's theta and a tf quaternion (convertOrientedPoint2DToEigen); here the
 *     rotation is the (c, s) the matcher carries, no trigonometry.
 *   - truncation: the matcher takes 64 correspondences per registration, so at most 64 - 40 * use_odom FLIRT cells are taken, the
 *     FIRST ones; `truncated` reports any cut.  Upstream has no limit.
 *   - prev_in_map_frame = 1 (default 0; an addition) uses a prev point that the previous call MOVED as it is, with the un-rotated
 *     covariance, instead of restating the quirk of step 4.
 *   - the points are moved without the quaternion detour of moveInterestPointVec: theta' comes from the product's rotation block.
 *   - the caller's points are left alone: upstream's `ptsPrev = pts` aliases pointers and so also moves the caller's points;
 *     cur is never written here.
 *   - appending stops at the bank's max_points: the first points that fit are kept, map_overflow is set, nothing is written
 *     outside the set.  ndtgpu_fuser_initialize_batch_feat empties the slot's map set first and resets its counter.
 * Device form (csrc/ndt_fuserfeat.hip).  ndt_fuserfeat_offsets_kernel: one workgroup scans the slots' cell counts in slot order
 * (ndt_block_scan, integers) into the offsets the matcher reads.  ndt_fuserfeat_cells_kernel: one wave per slot, one lane per cell
 * pair (64 lanes = the matcher's 64 correspondences): gate, record, cells.  ndt_fuserfeat_commit_kernel: one workgroup of 256 per
 * slot behind ndt_fuser_post_kernel: positions moved, descriptors copied coalesced, the append, the counts last by one lane.
 * fp64, contraction off, no atomics, no workgroup waits for another; a slot's outputs depend on its own inputs only, so they
 * are the same bits whichever batch the slot runs in.  Launches go on the caller's stream and are ordered against the feature
 * bank's other calls through its fence, in both directions.
 * Measured on MI355X (tools/fuser_feat_cost.py, library 0.10.0; HIP events around each call, median of 8 scan steps after a
 * warm-up; 64 fusers x 100 k points): the plain update 3.30 ms, with cur sets of 24 points 3.79 ms (+0.49 ms), of 256 points
 * 7.05 ms (+3.75 ms: the RANSAC's 64 workgroups run in front of the registration on the same stream). */
typedef struct {
    int32_t use_feat;                /* Params::useFeat (1) */
    int32_t prev_in_map_frame;       /* see DEVIATIONS (0) */
    int32_t map_every;               /* NDTFeatureMap::update appends on every map_every-th call (4) */
    int32_t pad_;
    double feat_cov[3];              /* the diagonal of the feature cells' covariance (2e-4, 2e-4, 1e-4; :249) */
    ndtgpu_featmatch_params match;   /* ransac_ (ndt_feature_fuser_hmt.h:213): the defaults */
} ndtgpu_fuser_feat_params;
void ndtgpu_default_fuser_feat_params(ndtgpu_fuser_feat_params *p);
typedef struct {
    ndtgpu_featmatch_result ransac;  /* step 1 (zeroes when it was not run) */
    double Tfeat[16];                /* step 2 (zeroes when RANSAC was not run) */
    int32_t ransac_run, consistent;
    int32_t n_feat_cells, n_odom_cells;   /* step 5: FLIRT cells taken, odometry cells */
    int32_t truncated;               /* fewer FLIRT cells taken than there are correspondences */
    int32_t n_prev, n_map;           /* points of the slot's prev and map sets after the call */
    int32_t map_appended;            /* points this call appended to map */
    int32_t map_overflow;            /* the append was cut at max_points */
    int32_t pad_;
} ndtgpu_fuser_feat_result;
/* Pure host functions (no device), built on the functions the kernels call (csrc/ndt_fuserfeat.h).
 * ndtgpu_fuser_feat_prepare: steps 2-5 for one slot (:252-334).  ransac: step 1's record (NULL: RANSAC not run); corr:
 * ransac->n_inliers pairs (cur i, prev j); cur_pos3 / prev_pos3: n x (x, y, theta); prev_moved: the previous call moved prev
 * (matters with prev_in_map_frame only).  rec: the record up to `truncated` (the rest zero); cells18: room for 64 records
 * {source mean[3], cov[6] xx xy xz yy yz zz, target mean[3], cov[6]}, the odometry cells included; *n_cells of them written. */
ndtgpu_status ndtgpu_fuser_feat_prepare(const ndtgpu_fuser_params *prm, const ndtgpu_fuser_feat_params *fprm, const double Tnow16[16],
                                        const double Tmotion16[16], const ndtgpu_featmatch_result *ransac, const uint32_t *corr,
                                        const double *cur_pos3, size_t n_cur, const double *prev_pos3, size_t n_prev, int prev_moved,
                                        ndtgpu_fuser_feat_result *rec, double *cells18, uint32_t *n_cells);
/* step 6's move of n points (x, y, theta) by T16 (:500, moveInterestPointVec) */
ndtgpu_status ndtgpu_fuser_feat_move(const double T16[16], const double *pos3_in, size_t n, double *pos3_out);
/* Attaches a feature bank (borrowed: it must outlive the fuser bank or the next attach): slot k's prev set is prev_set_first + k,
 * its map set map_set_first + k.  The two ranges must lie inside the feature bank and must not overlap (NDTGPU_ERR_INVALID).
 * prm NULL: the defaults.  ndtgpu_fuser_update_batch, ndtgpu_fuser_initialize_batch and their _host forms behave exactly as
 * before on a bank with features attached: they leave the feature state (prev, map, the counters) UNTOUCHED. */
ndtgpu_status ndtgpu_fuser_bank_attach_features(ndtgpu_fuser_bank *bank, ndtgpu_featbank *featbank, size_t prev_set_first,
                                                size_t map_set_first, const ndtgpu_fuser_feat_params *prm);
/* ndtgpu_fuser_initialize_batch / ndtgpu_fuser_update_batch with the feature path (:78-85; :245-334, 497-502): the plain entries'
 * arguments plus cur_set_idx, HOST, count indices of the sets that hold the scans' interest points -- filled earlier, for
 * instance by ndtgpu_featbank_extract_device on the same stream.  A cur index inside the prev / map ranges (or outside the
 * feature bank) is refused.  Asynchronous on `stream`, as the plain entries are. */
ndtgpu_status ndtgpu_fuser_initialize_batch_feat(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *initPose16,
                                                 const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                 const uint32_t *cur_set_idx, ndtgpu_stream stream);
ndtgpu_status ndtgpu_fuser_update_batch_feat(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *Tmotion16,
                                             const void *xyz_dev, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                             const uint32_t *cur_set_idx, int update_feature_map, int update_ndt_map,
                                             ndtgpu_stream stream);
/* the same with the clouds in HOST memory, like ndtgpu_fuser_initialize_batch_host / ndtgpu_fuser_update_batch_host: on the
 * bank's own stream (the cur sets were filled by a call that has returned, e.g. ndtgpu_featbank_set; the feature bank's fence
 * orders the rest) */
ndtgpu_status ndtgpu_fuser_initialize_batch_feat_host(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *initPose16,
                                                      const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                      const uint32_t *cur_set_idx);
ndtgpu_status ndtgpu_fuser_update_batch_feat_host(ndtgpu_fuser_bank *bank, size_t first, size_t count, const double *Tmotion16,
                                                  const void *xyz_host, size_t n_points, size_t stride_bytes, size_t map_stride_bytes,
                                                  const uint32_t *cur_set_idx, int update_feature_map, int update_ndt_map);
/* the feature records of the LAST _feat call for the slots it covered (zeroes for the others); waits for the call in flight, as
 * ndtgpu_fuser_poses does */
ndtgpu_status ndtgpu_fuser_feat_results(ndtgpu_fuser_bank *bank, size_t first, size_t count, ndtgpu_fuser_feat_result *out);
/* the cell records the LAST update call handed to the matcher, for slots [first, first + count) of it: offsets count + 1 (from
 * 0), cells18 room for `capacity` records of 18 doubles (NDTGPU_ERR_CAPACITY when they do not fit).  For tests and for callers
 * that drive ndtgpu_match_fusion_feat_batch themselves.  Waits for the call in flight. */
ndtgpu_status ndtgpu_fuser_feat_cells(ndtgpu_fuser_bank *bank, size_t first, size_t count, uint32_t *offsets, double *cells18,
                                      size_t capacity);

/* ---- laser-scan projection: ranges to the clouds that the fuser bank and the registrar take ------------------------------------
 * The first thing every consumer of a scan does in the reference: projector_.projectLaser(*msg_in, cloud), a loop that drops the
 * points outside the range gate, and the z jitter pt.z += varz*((double)rand())/(double)INT_MAX of every point that stays --
 * ndt_feature2d_fuser.cpp:747-765 and :875-888, publish_graph_message.cpp:1356-1381 and :1523-1535, ndt_feature_fuser.cpp:325-336
 * and :378-390, ndt_feature2d_reg_node.cpp:75-86, ndt_feature2d_view.cpp:119-129; the parameters laser_variance_z 0.02,
 * sensor_range 30 and min_laser_range 0.5 from gustav_laser_tf.launch:20-23.  ndtgpu_scanproj_project* is that for a batch of
 * scans: the ranges_dev buffer that ndtgpu_featbank_extract_device reads (n_scans x n_beams doubles) becomes the clouds in the
 * sensor frame that ndtgpu_fuser_update_batch and ndtgpu_register_batch_device read, on the caller's stream with no host visit.
 * One upload of the ranges feeds the feature extraction and the fuser.
 * PROVENANCE: laser_geometry is not vendored by the reference -- only its call sites are.  What projectLaser does is restated from
 * memory: x = r cos, y = r sin, z = 0 in the sensor frame, no time skew, and ranges outside the message's own limits are dropped.
 * No program text of laser_geometry or of the reference is copied.
 * Semantics (restated).  A scan is n_beams ranges; beam i looks along a_i = angle_min + (double)i * angle_increment, in fp64 and not
 * contracted -- the expression of the feature extraction above --, and the sensor is at the origin.
 *   kept     beam i is kept iff its range r is finite and r_min < r < r_max, both comparisons strict.  r_max may be +inf: the lower
 *            gate alone, as at publish_graph_message.cpp:1377, where the fuser's sensor_range cuts later.  With the same r_min /
 *            r_max this is step 1 of the feature extraction: a scan's n_kept equals that call's n_valid.
 *   point    x = (float)(r cos(a_i)), y = (float)(r sin(a_i)), z = (float)(varz u) with u = ndt_hash_uniform(seed, scan_id, i) of
 *            csrc/ndt_mcl.h (synth.hash_uniform), i the BEAM index, not the rank among the kept points.  Every product is fp64
 *            before the one rounding to float, not contracted.  A beam's point is a function of (i, angle_min, angle_increment, r,
 *            seed, scan_id, varz) alone.
 *   cloud    the kept points in ascending beam order in rows 0 .. n_kept - 1 of the scan's block -- the reference's push_back
 *            order: front() and back() are the first and the last kept beam.  Rows n_kept .. n_beams - 1 are (NaN, NaN, NaN), the
 *            padding that ndtgpu_fuser_update_batch documents for scans of unequal length.
 *   records  stride_bytes apart, scans map_stride_bytes apart, as in the fuser and registrar entries.  For stride_bytes >= 16 the
 *            fourth float of EVERY row, pads included, is written as 1.0f (pcl::PointXYZ's pad value).  Every other byte of the
 *            destination is left untouched.
 *   count    n_kept[b], a uint32.
 * DEVIATIONS:
 *   - the gate is on r itself; the reference gates on the float-rounded planar distance of the projected point.
 *   - counter-based draws replace rand(), and u is in [0, 1) (the reference's ratio reaches 1).
 *   - the message's range_min / range_max are folded into r_min / r_max by the caller.
 *   - the cloud is NaN-padded to n_beams rows instead of being shorter.
 *   - one angle_min / angle_increment applies to the whole call.
 *   - the ranges are doubles, as in the feature bank (sensor_msgs/LaserScan carries floats).
 * A known interaction that this entry does not change: with discard_cells the fuser bank reads row n_points - 1 as cloud.back(),
 * and on a padded cloud that row is a NaN pad, not the last kept beam (second finding).
 * Device form (csrc/ndt_scanproject.hip).  The work is tiled over the grid, (scans) x (tiles of T = ndtgpu_scanproj_tile() = 1024
 * beams), in two plain launches: ndt_scanproject_count_kernel leaves every tile's count of kept beams (loads and the gate only) in
 * the handle's scratch; ndt_scanproject_emit_kernel sums the counts of the tiles in front of its own (integers, ndt_block.h), ranks
 * its kept beams (ndt_block_rank) and writes their rows contiguously, then its share of the NaN pads, and the scan's last tile
 * n_kept.  No atomics, no spin on memory, no grid barrier, no environment switches; fp64 with contraction off.  A scan's bytes
 * are the same in any batch, at any position and for any launch geometry.
 * Measured on MI355X (tools/scanproject_cost.py, library 0.11.0; HIP events around the call, median of 9 after a warm-up; synthetic
 * halls, 99 % of the beams kept): 1024 scans of 1440 beams 0.029 ms (0.03 us a scan), 64 scans of 100 000 beams 0.063 ms (1 us a
 * scan), against 62 ms and 61 ms for the path it replaces on the same box (the NumPy projection of the host, 62 / 59 ms, and the
 * upload of the cloud, 0.5 / 1.9 ms).  In front of the fuser bank's plain update on the same stream (64 fusers x 100 000 beams) the
 * update goes from 3.52 ms to 3.56 ms (+0.04 ms, +1.2 %; the steps of either run spread over 3.0 .. 3.9 ms), the same poses.  Kernels
 * (tools/kernel_resources.py scanproject): count 8 VGPRs, emit 46 VGPRs, no spills, no scratch, 32 B of LDS each. */
typedef struct ndtgpu_scanproj ndtgpu_scanproj;
typedef struct {
    double r_min;                    /* a kept range is above this, metres (0.5: min_laser_range) */
    double r_max;                    /* ... and below this; +inf: no upper gate (30.0: sensor_range) */
    double varz;                     /* the z jitter's width, z in [0, varz) (0.02: laser_variance_z) */
    uint64_t seed;                   /* of the z draws (0) */
} ndtgpu_scanproject_params;
/* gustav_laser_tf.launch:20-23 */
void ndtgpu_default_scanproject_params(ndtgpu_scanproject_params *p);
/* T: the beams of a tile */
uint32_t ndtgpu_scanproj_tile(void);
/* Pure host functions (no device), built on what the kernels call (csrc/ndt_scanproject.h).
 * ndtgpu_scanproj_check: the checks of a projection's arguments and parameters (prm NULL: the defaults) -- n_beams 1 .. 2^20,
 * n_scans <= 2^24, angle_min and angle_increment finite, stride_bytes >= 12 and a multiple of 4, map_stride_bytes >=
 * n_beams * stride_bytes and a multiple of 4, r_min finite and >= 0, r_max > r_min (+inf allowed), varz finite and >= 0:
 * NDTGPU_ERR_INVALID with a message that names the argument. */
ndtgpu_status ndtgpu_scanproj_check(size_t n_scans, size_t n_beams, double angle_min, double angle_increment, size_t stride_bytes,
                                    size_t map_stride_bytes, const ndtgpu_scanproject_params *prm);
/* the gate and the point of beam i with range r of scan scan_id: 1 and xyz written iff kept, else 0.  The host's cos and sin: x and
 * y may differ from the device's by one float unit in the last place, the flag and z do not. */
int ndtgpu_scanproj_beam(const ndtgpu_scanproject_params *prm, double angle_min, double angle_increment, uint64_t scan_id, uint32_t i,
                         double r, float xyz[3]);
/* a projector for calls of up to max_scans scans (1 .. 2^24) of up to max_beams beams (1 .. 2^20): it owns the tile counts and,
 * from its first use, the staging of the host form */
ndtgpu_status ndtgpu_scanproj_create(size_t max_scans, size_t max_beams, ndtgpu_scanproj **out);
ndtgpu_status ndtgpu_scanproj_destroy(ndtgpu_scanproj *h);
/* projects n_scans scans, DEVICE ranges_dev n_scans x n_beams, into DEVICE xyz_dev, fully asynchronous on `stream`.  scan_id_dev:
 * n_scans ids (NULL: scan b has id b); n_kept_dev: n_scans counts (may be NULL); prm NULL: the defaults.  The arguments and
 * parameters are checked before the handle is read and the device is looked for; n_scans == 0 is a successful no-op;
 * NDTGPU_ERR_CAPACITY beyond max_scans / max_beams.  Calls on one handle are ordered on the device whatever stream each names (they
 * share the tile counts), like ndtgpu_pgo_optimize. */
ndtgpu_status ndtgpu_scanproj_project_device(ndtgpu_scanproj *h, const double *ranges_dev, const uint64_t *scan_id_dev, size_t n_scans,
                                             size_t n_beams, double angle_min, double angle_increment,
                                             const ndtgpu_scanproject_params *prm, void *xyz_dev, size_t stride_bytes,
                                             size_t map_stride_bytes, uint32_t *n_kept_dev, ndtgpu_stream stream);
/* the same on HOST arrays through the handle's pinned staging, synchronous: xyz and n_kept are written when it returns */
ndtgpu_status ndtgpu_scanproj_project(ndtgpu_scanproj *h, const double *ranges, const uint64_t *scan_id, size_t n_scans, size_t n_beams,
                                      double angle_min, double angle_increment, const ndtgpu_scanproject_params *prm, void *xyz,
                                      size_t stride_bytes, size_t map_stride_bytes, uint32_t *n_kept);

/* ---- extrinsic calibration: the laser's pose on the base, by brute-force search over sensor offsets ------------------------------
 * Every entry that turns a scan into a pose takes a sensor_pose; the reference ships the tool that produces it,
 * ndt_feature/src/laser2d_extrinsic_calibration.cpp (automower_laser2d_calib.launch, cth_laser2d_calib.launch,
 * coop_laser2d_calib.launch): bruteForceOptimization (:176-204) walks a lattice of (x, y, yaw) candidates, errorFunction (:146-152)
 * sums ScanPair::scoreICP (:85-122) over the collected pairs, and the callback (:250-353) collects the pairs.  ndtgpu_calib_search*
 * is that search on the device, over clouds in the layout ndtgpu_scanproj_project_device writes.
 * PROVENANCE: restated from the reference's program text cited above; its kd-tree (PCL / FLANN) is not vendored and is replaced by
 * an exact nearest neighbour, which has one right answer.  No program text of the reference is copied.
 * Semantics (restated).  A pair is (cloud1, pose1, cloud2, pose2), the poses those of the base in a world frame; a candidate is the
 * sensor offset Ts = (x, y, yaw).  The reference moves cloud1 by pose1 Ts and cloud2 by pose2 Ts into the world frame; for every
 * point of cloud2 it takes d2, the squared 3-D distance to its nearest neighbour in cloud1, and adds d2 > th2 ? th2 : d2 with
 * th2 = 0.1 * 0.1; the sum over the points and then over the pairs is the candidate's score.  The winner is the candidate with the
 * smallest score under a strict <, so among equals the first in loop order -- x outer, y middle, yaw inner.  The lattice is
 * for (double x = ix - x_s; x < ix + x_s; x += t_r), repeated addition in doubles, and likewise for y (t_r) and yaw (yaw_r).
 * The form computed here.  |p1 a - p2 b| = |a - M b| with M = Ts^-1 D Ts and D = pose1^-1 pose2; rotations of the plane commute, so
 * M's rotation is D's and only its translation depends on the candidate: t = R(-yaw) (t_D + (R_D - I) t_s).  cloud1 never moves,
 * cloud2 is rotated once per pair, a candidate is a 2-D translation.  The search sees yaw only through R(-yaw) acting on a
 * non-zero bracket, which is why the callback insists on 25 degrees between the scans of a pair.  The order of every operation --
 * fp64, not contracted, on the float32 coordinates widened to double -- is written out in csrc/ndt_calib.h and is part of the
 * contract: tests/calib_model.py restates it and the device's scores equal the model's bit for bit.
 *   rows     rows at or beyond n_kept[scan] are ignored; a row in front of it with a non-finite coordinate is skipped and counted
 *            (n_skipped: per pair, the skipped rows of its cloud1 and of its cloud2); a pair whose cloud1 has no usable row
 *            contributes 0.0, and so does an empty cloud2.
 *   winner   the smallest score, ties to the lowest linear index (ix * ny + iy) * nyaw + iyaw.
 *   flags    NDTGPU_CALIB_NO_RESULT where the winner's score is >= 1e6; NDTGPU_CALIB_BAD_PAIR where a pair of the device form names
 *            a scan >= n_scans (that pair contributes 0.0; the host form refuses such a call).
 *   pairs    ndtgpu_calib_select_pairs: Tmotion = Told^-1 Tgt; a translation above max_translation (1.0 m) resets the anchor with no
 *            pair; |yaw| < min_yaw (25 degrees) keeps waiting; otherwise (anchor, current) is a pair and current the new anchor.
 * DEVIATIONS:
 *   - sensor-frame form: |a - M b| instead of two float clouds in the world frame.  The same value in exact arithmetic; the
 *     rounding is better conditioned (no world coordinates are rounded to float).
 *   - fp64 on the float32 points instead of PCL's float kd-tree and float distances.
 *   - no 1e6 cap: the reference starts from min_score = 1e6 and reports nothing above it; the flag reports the condition instead.
 *   - z offset: clouds from ndtgpu_scanproj_project_device carry the z jitter but not the callback's constant 0.1; only differences
 *     of z enter the distance.  The callback's own gate (r >= range_min && r < range_max && r > 0.3 && r < 20) is the caller's r_min
 *     / r_max of the projection.
 *   - the candidates' cosines and sines come from host tables (ndtgpu_calib_lattice): the device evaluates neither.
 *   - an empty cloud contributes 0 (the reference prints a complaint and queries an empty tree).
 *   - the pair gate uses the robust yaw, acos of the clamped cosine (getRobustYawFromAffine3d's form), not eulerAngles(0,1,2)[2].
 * Limits: 1 .. 2^16 rows per scan, 1 .. 1024 pairs, 1 .. 2^20 scans in the bank, 1 .. 2^24 candidates.  The (pair, candidate) sums
 * live in the handle's scratch, at most 2^22 doubles (32 MiB): a handle made for max_pairs pairs works through the lattice in
 * chunks of floor(2^22 / max_pairs / 256) * 256 candidates (at least 256), two launches per chunk; 16 pairs: 262 144 candidates a chunk.
 * Device form (csrc/ndt_calib.hip): plain launches on the caller's stream, no atomics, no workgroup waits on another.  prepare, a
 * workgroup per pair: usable rows widened, cloud2 rotated, both compacted in row order; score, (candidate tiles of 256) x (pairs)
 * workgroups, a lane per candidate, the cloud rows uniform across the wave; finish, a lane per candidate: the pairs added in
 * order, the volume, the tile's ordered arg-min; winner, one workgroup over the tile winners.  The walk is not pruned.
 * Measured on MI355X (tools/calib_cost.py, library 0.13.0; HIP events around the call, median of 7 after a warm-up; 16 pairs of
 * 720-beam synthetic hall scans, 600 kept points a scan on average): the launch files' lattice, 100 x 100 x 20 = 200 000 candidates or
 * 1.15e12 point pairs, 305.6 ms (304.6 .. 305.9; 3.8e12 point pairs a second); the program's default lattice, 10 x 10 x 80 = 8000
 * candidates, 25.6 ms (512 workgroups: the chip is not full).  The literal form with SciPy's cKDTree on one core of the same box takes
 * 3.07 / 3.02 ms a candidate over 48 sampled candidates; SCALED to the lattices (an extrapolation) that is 613 s and 24 s: ratios of
 * 2000 and 940.  Kernels (tools/kernel_resources.py calib): prepare 32, score 28, finish 13, winner 36 VGPRs, no spills, no scratch,
 * LDS 32 / 0 / 48 / 80 B.  Pruning the walk to the neighbours within reach of the lattice's translations was not built or measured. */
typedef struct ndtgpu_calib ndtgpu_calib;
typedef struct {
    double max_dist;                 /* th: a nearest neighbour farther than this counts as th * th (0.1: scoreICP's error_th) */
} ndtgpu_calib_params;
#define NDTGPU_CALIB_NO_RESULT 1u
#define NDTGPU_CALIB_BAD_PAIR 2u
typedef struct {
    double score;                    /* the winner's */
    uint32_t index;                  /* (ix * ny + iy) * nyaw + iyaw */
    uint32_t flags;                  /* NDTGPU_CALIB_* */
    uint32_t n_skipped;              /* rows in front of n_kept with a non-finite coordinate, summed over the pairs' clouds */
    uint32_t reserved;
} ndtgpu_calib_result;
/* laser2d_extrinsic_calibration.cpp:106 */
void ndtgpu_default_calib_params(ndtgpu_calib_params *p);
/* the candidates of a workgroup */
uint32_t ndtgpu_calib_tile(void);
/* Pure host functions (no device), built on what the kernels call (csrc/ndt_calib.h).
 * ndtgpu_calib_lattice: the three loops of bruteForceOptimization by repeated addition.  counts3 = (nx, ny, nyaw) is always written;
 * xs, ys, yaws, cs = cos(yaws), sn = sin(yaws) are written where not NULL, each with room for `room` doubles (NDTGPU_ERR_CAPACITY
 * where an axis has more nodes than room and an array was given).  NDTGPU_ERR_INVALID for a non-finite argument, a span or step
 * that is not > 0, or more than 2^24 nodes on an axis. */
ndtgpu_status ndtgpu_calib_lattice(double ix, double iy, double iyaw, double x_s, double y_s, double yaw_s, double t_r, double yaw_r,
                                   size_t counts3[3], double *xs, double *ys, double *yaws, double *cs, double *sn, size_t room);
/* D = pose1^-1 pose2 as (dx, dy, cd, sd) of two poses (x, y, c, s) */
ndtgpu_status ndtgpu_calib_pair_motion(const double pose1[4], const double pose2[4], double D[4]);
/* the callback's anchor and gate walk over n poses (x, y, c, s): the first `room` pairs (anchor, current) into pairs2 (may be NULL),
 * their count into n_pairs */
ndtgpu_status ndtgpu_calib_select_pairs(const double *poses4, size_t n, double max_translation, double min_yaw, uint32_t *pairs2,
                                        size_t room, size_t *n_pairs);
/* the checks of a search's arguments and parameters (prm NULL: the defaults): NDTGPU_ERR_INVALID with a message that names the
 * argument */
ndtgpu_status ndtgpu_calib_check(size_t n_scans, size_t n_points, size_t stride_bytes, size_t map_stride_bytes, size_t n_pairs, size_t nx,
                                 size_t ny, size_t nyaw, const ndtgpu_calib_params *prm);
/* a calibrator for searches of up to max_pairs pairs (1 .. 1024) of scans of up to max_points rows (1 .. 2^16) over up to
 * max_candidates candidates (1 .. 2^24): it owns the compacted clouds, the (pair, candidate) sums, the tile winners and, from its
 * first use, the staging */
ndtgpu_status ndtgpu_calib_create(size_t max_pairs, size_t max_points, size_t max_candidates, ndtgpu_calib **out);
ndtgpu_status ndtgpu_calib_destroy(ndtgpu_calib *h);
/* The search.  DEVICE: xyz_dev, a bank of n_scans clouds of n_points rows (stride_bytes / map_stride_bytes as in
 * ndtgpu_scanproj_project_device), n_kept_dev [n_scans], poses_dev [n_scans][4] = (x, y, c, s) of the base, pairs_dev [n_pairs][2] =
 * (scan of cloud1, scan of cloud2), result_dev, volume_dev (NULL, or nx * ny * nyaw doubles: every candidate's score).  HOST: the
 * lattice tables xs [nx], ys [ny], cs / sn [nyaw] of ndtgpu_calib_lattice, copied before the call returns.  prm NULL: the defaults.
 * Asynchronous on `stream`; calls on one handle are ordered on the device whatever stream each names, and a call waits on the host
 * for the previous call's table upload.  The arguments and parameters are checked before the handle is read and the device is
 * looked for; NDTGPU_ERR_CAPACITY beyond what the handle was created for. */
ndtgpu_status ndtgpu_calib_search_device(ndtgpu_calib *h, const void *xyz_dev, size_t n_scans, size_t n_points, size_t stride_bytes,
                                         size_t map_stride_bytes, const uint32_t *n_kept_dev, const double *poses_dev,
                                         const uint32_t *pairs_dev, size_t n_pairs, const double *xs, size_t nx, const double *ys, size_t ny,
                                         const double *cs, const double *sn, size_t nyaw, const ndtgpu_calib_params *prm,
                                         ndtgpu_calib_result *result_dev, double *volume_dev, ndtgpu_stream stream);
/* the same on HOST arrays through the handle's pinned staging, synchronous: result and volume (may be NULL) are written when it
 * returns.  A pair that names a scan >= n_scans is refused (NDTGPU_ERR_INVALID). */
ndtgpu_status ndtgpu_calib_search(ndtgpu_calib *h, const void *xyz, size_t n_scans, size_t n_points, size_t stride_bytes,
                                  size_t map_stride_bytes, const uint32_t *n_kept, const double *poses, const uint32_t *pairs, size_t n_pairs,
                                  const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn, size_t nyaw,
                                  const ndtgpu_calib_params *prm, ndtgpu_calib_result *result, double *volume);

/* ---- localisation monitor: distance field of an occupancy grid, scan-pose badness, pose adjustment, relocalisation pick ------------
 * The chain ends in occupancy grids (ndtgpu_mapset_occupancy_grid_device); this section consumes them and tells a caller whether a
 * robot's pose in such a grid is still right.  The reference ships that piece in flirtlib_ros: ScanPoseEvaluator
 * (flirtlib_ros/src/localization_monitor.cpp:41-120, include/flirtlib_ros/localization_monitor.h:41-63) builds a distance field of
 * the grid; the badness of a (scan, pose) is the median distance from the scan's endpoints to the nearest obstacle; adjustPose
 * (:61-65) is a brute-force lattice search over (x, y, theta) for the smallest badness.  localization_monitor_node.cpp uses it on
 * every scan (scanCB :498-537) to decide "well localised" at badness_threshold_ 0.25 (:214, :324, :529); when not localised,
 * updateUnlocalized (:331-413) matches the scan's features against a bank of reference scans, takes the one with the most matches
 * above min_num_matches (8, :209), composes the pose (common.cpp:56-66) and accepts it only if its badness is below the threshold.
 * startup_loc.cpp:262-329 is the same relocalisation at start-up.
 * PROVENANCE: restated from the reference's program text cited above.  occupancy_grid_utils (distanceField, pointCell,
 * withinBounds) is not vendored by the reference, only its call sites are; its semantics are restated here from those call sites
 * and its public documentation: pointCell is the floor of (point - origin) / resolution per axis, withinBounds is 0 <= cell <
 * (width, height), distanceField is the distance of every cell to the nearest occupied cell, not computed beyond max_dist.  No
 * program text of the reference is copied.
 * Semantics (restated; the order of every fp64 operation -- not contracted -- is written out in csrc/ndt_locmon.h and is part of the
 * contract: tests/locmon_model.py restates it and the device's outputs equal the model's bit for bit).
 *   field    input: n_grids int8 grids of width x height, row-major, back to back, as ndtgpu_mapset_occupancy_grid_device writes
 *            them; resolution; origin[2] per grid.  A pixel is an obstacle iff its value is >= occupied_min.  R = (int)floor(max_dist
 *            / resolution), 1 <= R <= 254.  The field's value at a pixel is k = min(dx^2 + dy^2) over the obstacle pixels of the same
 *            grid with k <= R^2, a uint16; 0xFFFF ("far") where there is none.  Pixels outside the grid are not obstacles.  All
 *            arithmetic is integer.  The handle owns the fields and origins, as the evaluator owns geom_ and distances_.
 *   query    (scan, grid, x, y, c, s): poses are carried as (x, y, cos, sin), as in the calibration entries.  Beam i has the table
 *            entry (cb_i, sb_i) = (cos a_i, sin a_i), a_i = angle_min + (double)i * angle_increment, made on the host once per
 *            scanner geometry (ndtgpu_locmon_set_beams).  Beam i is kept iff its range r is finite and r_min < r < r_max.  For a kept
 *            beam ex = c * cb - s * sb, ey = s * cb + c * sb, px = x + ex * r, py = y + ey * r, fi = floor((px - ox) / resolution),
 *            fj likewise; in bounds iff 0 <= fi < width and 0 <= fj < height, compared as doubles (a NaN is off the map).  The
 *            beam's key is the field's value k, 0x10000 for far, 0x10001 off the map.  The result key is the element at index
 *            n_kept / 2 of the ascending keys: the reference's distances[size / 2], the upper median.
 *   badness  resolution * sqrt((double)k) metres; far: max_dist; off the map: 1e9.
 *   flags    NDTGPU_LOCMON_NO_BEAMS: n_kept == 0 (key off-map, badness 1e9); NDTGPU_LOCMON_BAD_INDEX: scan >= n_scans or grid >=
 *            n_grids (the same); NDTGPU_LOCMON_NO_QUERY: scan == 0xFFFFFFFF, no work is done (the same).
 *   adjust   the three loops of :61-65 are ndtgpu_calib_lattice(x0, y0, theta0, pos_range, pos_range, 3.14, dpos, dtheta, ...): its
 *            xs, ys, cs, sn tables are the candidates.  The smallest key wins, ties to the lowest linear index
 *            (ix * ny + iy) * nyaw + iyaw: the reference's strict < in loop order.  NDTGPU_LOCMON_NO_RESULT where the winner's
 *            badness is >= 1e8 (the reference's ROS_ASSERT(best < 1e8)).
 *   pick     over n_pairs records of ndtgpu_featbank_match_device, pair p = (reference set p, the current scan's set): the pair
 *            with the most n_inliers among those with status OK and n_inliers > min_num_matches, strict >, so the first of equals
 *            wins.  The picked pose is ref_pose o (x, y, c, s of the match) o (post_x, post_y); post is the reference's hard-coded
 *            laser offset (-0.275, 0) of common.cpp:58, a parameter here.  No pair qualifies: the written query's scan is
 *            0xFFFFFFFF and the evaluation that follows on the same stream reports NDTGPU_LOCMON_NO_QUERY.
 * DEVIATIONS:
 *   - occupied_min: an obstacle is a pixel >= occupied_min (55, the smallest value the rasteriser of this library gives an occupied
 *     pixel); upstream seeds on its own OCCUPIED constant (100).
 *   - exact Euclidean transform in squared pixel units; upstream propagates a wavefront from the seeds, which is exact only up to
 *     its neighbourhood's metric.
 *   - the angle-addition form replaces cos(theta0 + a_i) and sin(theta0 + a_i): the device evaluates no trigonometry.
 *   - the range gate: a NaN, an infinite or a gated beam is dropped; the reference pushes every beam, NaN included, into its sort.
 *   - off the map is the key 0x10001 and far the key 0x10000 in place of 1e9 and max_dist among doubles: the same order.
 *   - the badness is a double (the reference returns a float).
 *   - no 1e8 assertion: the flag reports the condition.
 *   - the pick requires n_inliers > min_num_matches for every pair; the reference's second test (best < min_num_matches, :371) can
 *     then never fire and is not restated.
 *   - left out: the scan database, the one-day expiry, the navigation counter, odometry compensation (:415-428).
 * Limits: n_beams 1 .. 8192; R 1 .. 254; width, height 1 .. 2^15; 1 .. 1024 grids, 2^31 pixels a handle; 2^24 scans, queries and
 * candidates; 2^20 pairs.  A search works through the lattice in chunks of floor(2^23 / max_beams / 256) * 256 candidates (at least
 * 256) through the handle's scratch, two launches per chunk.
 * Device form (csrc/ndt_locmon.hip): plain launches on the caller's stream, no atomics, no workgroup waits on another, no
 * environment switches.  Field: two launches over (tiles of 256 pixels) x (grids) -- the row pass writes the nearest obstacle
 * distance along the row, capped at R with 255 for none, one byte per pixel into the handle's scratch; the column pass computes
 * min over |dy| <= R of dy^2 + g^2.  Badness: one workgroup of 256 lanes per query, lanes over beams, the keys in LDS (4 bytes a
 * beam), n_kept by a block count and the n_kept / 2-th key by a 17-round most-significant-bit-first radix select of block counts
 * (csrc/ndt_block.h).  Adjust: the badness kernel over the candidates, a tile arg-min and one workgroup over the tile winners.
 * Pick: one workgroup.  The workgroup-per-query form shipped; a wave-per-query variant was not built.
 * Measured on MI355X (tools/locmon_cost.py, library 0.13.0; HIP events around the call, median of 7 after a warm-up, min .. max): the
 * field of the replay's world at 0.05 m (13600 x 12000 = 163.2 M pixels, 2.4 M obstacle pixels, R = 7) 3.29 ms (3.28 .. 3.33; 50 G
 * pixels a second); evaluate, 1024 queries of 1440 beams, 0.033 ms (0.032 .. 0.039; 0.03 us a query); adjust, pos_range 0.5 by 0.05 and
 * +- 3.14 by 0.02 -- 21 x 21 x 314 = 138 474 candidates by repeated addition, where the issue's arithmetic says 20 x 20 x 315 -- 1.83 ms
 * (1.77 .. 1.90; 0.013 us a candidate); 64 queries in front of the fuser bank's plain update (64 fusers x 1440 beams) on one stream: 2.31
 * ms against 2.32 ms for the update alone (-0.01 ms, inside the spread 2.16 .. 2.42 of either run), the same poses.  On one core of the
 * same box: SciPy's distance_transform_edt on a crop of 3000 x 3000 pixels 256 ms, SCALED to the grid by the pixel count (an
 * extrapolation) 4.6 s, 1400 times the device (the device's field of the crop's interior equals SciPy's); the NumPy evaluator of
 * tests/locmon_model.py 0.138 ms a query (32 queries, the same records as the device), SCALED 141 ms and 5.3 s: 4300 and 2900 times.
 * Kernels (tools/kernel_resources.py locmon): row 11, column 11, badness 32, finish 9, winner 14, pick 16 VGPRs, no spills, no scratch;
 * LDS 0 / 0 / 32 B + 4 B a beam / 32 / 32 / 32 B. */
typedef struct ndtgpu_locmon ndtgpu_locmon;
typedef struct {
    double max_dist;                 /* the field's reach, metres (0.375 = badness_threshold 0.25 * 1.5, :324); read by set_grids* */
    double r_min;                    /* a kept range is above this (0.0); read by evaluate* and adjust* */
    double r_max;                    /* ... and below this; +inf: no upper gate (+inf) */
    double post_x, post_y;           /* the translation behind the match in a picked pose (-0.275, 0: common.cpp:58); read by pick */
    int32_t occupied_min;            /* a pixel >= this is an obstacle (55); read by set_grids* */
    int32_t min_num_matches;         /* a pair qualifies with n_inliers above this (8, :209); read by pick */
} ndtgpu_locmon_params;
#define NDTGPU_LOCMON_NO_BEAMS 1u
#define NDTGPU_LOCMON_BAD_INDEX 2u
#define NDTGPU_LOCMON_NO_QUERY 4u
#define NDTGPU_LOCMON_NO_RESULT 8u
#define NDTGPU_LOCMON_NO_PICK 16u
typedef struct {
    double x, y, c, s;               /* the scanner's pose in the grid's frame */
    uint32_t scan;                   /* row of ranges; 0xFFFFFFFF: no query */
    uint32_t grid;                   /* of the installed grids */
} ndtgpu_locmon_query;
typedef struct {
    double badness;                  /* metres; max_dist for far; 1e9 off the map or where a flag is set */
    uint32_t key;                    /* the median key: dx^2 + dy^2 in pixels, 0x10000 far, 0x10001 off the map */
    uint32_t n_kept;                 /* beams that passed the range gate */
    uint32_t n_offmap;               /* ... whose endpoint is off the map */
    uint32_t flags;                  /* NDTGPU_LOCMON_NO_BEAMS | _BAD_INDEX | _NO_QUERY */
} ndtgpu_locmon_result;
typedef struct {
    double badness;                  /* the winner's */
    uint32_t key;
    uint32_t index;                  /* (ix * ny + iy) * nyaw + iyaw */
    uint32_t flags;                  /* NDTGPU_LOCMON_NO_RESULT */
    uint32_t reserved;
} ndtgpu_locmon_adjust_result;
typedef struct {
    int32_t pair;                    /* the picked pair, -1 where none qualifies */
    int32_t n_inliers;               /* its n_inliers (0) */
    uint32_t flags;                  /* NDTGPU_LOCMON_NO_PICK */
    uint32_t reserved;
} ndtgpu_locmon_pick;
/* localization_monitor_node.cpp:209, :214, :324; common.cpp:58 */
void ndtgpu_default_locmon_params(ndtgpu_locmon_params *p);
/* the lanes of a badness workgroup, the candidates of an arg-min tile, the pixels of a field tile */
uint32_t ndtgpu_locmon_tile(void);
/* Pure host functions (no device), built on what the kernels call (csrc/ndt_locmon.h).
 * ndtgpu_locmon_check: the checks of the arguments of set_grids* (n_grids, width, height, resolution, prm), set_beams (n_beams,
 * angle_min, angle_increment) and evaluate* (n_scans, n_queries) at once; prm NULL: the defaults.  NDTGPU_ERR_INVALID with a message
 * that names the argument. */
ndtgpu_status ndtgpu_locmon_check(size_t n_grids, size_t width, size_t height, double resolution, size_t n_beams, double angle_min,
                                  double angle_increment, size_t n_scans, size_t n_queries, const ndtgpu_locmon_params *prm);
/* R = (int)floor(max_dist / resolution); NDTGPU_ERR_INVALID (and *R = 0) unless both are finite and > 0 and R is 1 .. 254 */
ndtgpu_status ndtgpu_locmon_radius(double max_dist, double resolution, int32_t *R);
/* cb[i] = cos(a_i), sb[i] = sin(a_i), a_i = angle_min + (double)i * angle_increment, i < n_beams: the table set_beams installs */
ndtgpu_status ndtgpu_locmon_beam_table(size_t n_beams, double angle_min, double angle_increment, double *cb, double *sb);
/* the pixel of the endpoint of a beam with table entry (cb, sb) and range r from pose4 = (x, y, c, s) in a grid of width x height at
 * origin2: *in_bounds = 1 and cell2 = (fi, fj), or *in_bounds = 0 (cell2 untouched) */
ndtgpu_status ndtgpu_locmon_pixel(const double pose4[4], double cb, double sb, double r, const double origin2[2], double resolution,
                                  uint32_t width, uint32_t height, int32_t cell2[2], int32_t *in_bounds);
/* the badness of a key */
ndtgpu_status ndtgpu_locmon_metres(uint32_t key, double resolution, double max_dist, double *badness);
/* out4 = ref_pose4 o match4 o (post2 as a translation), poses as (x, y, c, s) */
ndtgpu_status ndtgpu_locmon_compose(const double ref_pose4[4], const double match4[4], const double post2[2], double out4[4]);
/* a monitor for up to max_grids grids (1 .. 1024) of max_pixels pixels in all (1 .. 2^31), scans of up to max_beams beams (1 ..
 * 8192) and searches of up to max_candidates candidates (1 .. 2^24): it owns the fields, the origins, the beam table, the row pass's
 * scratch, the candidates' keys, the tile winners and, from its first use, the staging of the host forms */
ndtgpu_status ndtgpu_locmon_create(size_t max_grids, size_t max_pixels, size_t max_beams, size_t max_candidates, ndtgpu_locmon **out);
ndtgpu_status ndtgpu_locmon_destroy(ndtgpu_locmon *h);
/* installs the beam table of a scanner geometry (made on the host, uploaded on `stream`): every later evaluate*, adjust* reads
 * ranges of n_beams beams a scan.  Waits on the host for the handle's previous call. */
ndtgpu_status ndtgpu_locmon_set_beams(ndtgpu_locmon *h, size_t n_beams, double angle_min, double angle_increment, ndtgpu_stream stream);
/* builds the distance fields of n_grids grids: DEVICE grids_dev, n_grids x height x width int8; HOST origins2, n_grids x 2, copied
 * before the call returns.  prm NULL: the defaults (max_dist, occupied_min are read).  Asynchronous on `stream`.  The arguments are
 * checked before the handle is read and the device is looked for; NDTGPU_ERR_CAPACITY beyond max_grids / max_pixels.  Calls on one
 * handle are ordered on the device whatever stream each names. */
ndtgpu_status ndtgpu_locmon_set_grids_device(ndtgpu_locmon *h, const int8_t *grids_dev, size_t n_grids, size_t width, size_t height,
                                             double resolution, const double *origins2, const ndtgpu_locmon_params *prm,
                                             ndtgpu_stream stream);
/* the same on a HOST array of grids, synchronous */
ndtgpu_status ndtgpu_locmon_set_grids(ndtgpu_locmon *h, const int8_t *grids, size_t n_grids, size_t width, size_t height, double resolution,
                                      const double *origins2, const ndtgpu_locmon_params *prm);
/* copies the field of one installed grid back: HOST field, width x height uint16.  Synchronous. */
ndtgpu_status ndtgpu_locmon_field_get(ndtgpu_locmon *h, size_t grid, uint16_t *field);
/* The badness of n_queries queries.  DEVICE: ranges_dev n_scans x n_beams doubles (the buffer ndtgpu_featbank_extract_device and
 * ndtgpu_scanproj_project_device read), queries_dev, results_dev.  prm NULL: the defaults (r_min, r_max are read).  Asynchronous on
 * `stream`; n_queries == 0 is a successful no-op; NDTGPU_ERR_INVALID where no grids or no beams are installed. */
ndtgpu_status ndtgpu_locmon_evaluate_device(ndtgpu_locmon *h, const double *ranges_dev, size_t n_scans, const ndtgpu_locmon_query *queries_dev,
                                            size_t n_queries, const ndtgpu_locmon_params *prm, ndtgpu_locmon_result *results_dev,
                                            ndtgpu_stream stream);
/* the same on HOST arrays through the handle's pinned staging, synchronous */
ndtgpu_status ndtgpu_locmon_evaluate(ndtgpu_locmon *h, const double *ranges, size_t n_scans, const ndtgpu_locmon_query *queries,
                                     size_t n_queries, const ndtgpu_locmon_params *prm, ndtgpu_locmon_result *results);
/* adjustPose: the candidate of least badness of scan `scan` in grid `grid` over the lattice tables xs [nx], ys [ny], cs / sn [nyaw]
 * (HOST, of ndtgpu_calib_lattice, copied before the call returns).  DEVICE: ranges_dev, result_dev, volume_dev (NULL, or nx * ny *
 * nyaw uint32: every candidate's key).  Asynchronous on `stream`; NDTGPU_ERR_CAPACITY beyond max_candidates. */
ndtgpu_status ndtgpu_locmon_adjust_device(ndtgpu_locmon *h, const double *ranges_dev, size_t n_scans, uint32_t scan, uint32_t grid,
                                          const double *xs, size_t nx, const double *ys, size_t ny, const double *cs, const double *sn,
                                          size_t nyaw, const ndtgpu_locmon_params *prm, ndtgpu_locmon_adjust_result *result_dev,
                                          uint32_t *volume_dev, ndtgpu_stream stream);
/* the same on a HOST array of ranges, synchronous: result and volume (may be NULL) are written when it returns */
ndtgpu_status ndtgpu_locmon_adjust(ndtgpu_locmon *h, const double *ranges, size_t n_scans, uint32_t scan, uint32_t grid, const double *xs,
                                   size_t nx, const double *ys, size_t ny, const double *cs, const double *sn, size_t nyaw,
                                   const ndtgpu_locmon_params *prm, ndtgpu_locmon_adjust_result *result, uint32_t *volume);
/* The pick.  DEVICE: matches_dev n_pairs records of ndtgpu_featbank_match_device, ref_poses_dev n_pairs x 4, query_dev one query
 * (written: the picked pose with `scan` and `grid`, or scan 0xFFFFFFFF), pick_dev one record.  prm NULL: the defaults
 * (min_num_matches, post_x, post_y are read).  n_pairs 0 .. 2^20.  Asynchronous on `stream`: extract -> match -> pick -> evaluate ->
 * verdict stays on the device. */
ndtgpu_status ndtgpu_locmon_pick_device(ndtgpu_locmon *h, const ndtgpu_featmatch_result *matches_dev, const double *ref_poses_dev,
                                        size_t n_pairs, uint32_t scan, uint32_t grid, const ndtgpu_locmon_params *prm,
                                        ndtgpu_locmon_query *query_dev, ndtgpu_locmon_pick *pick_dev, ndtgpu_stream stream);

/* ---- scan simulation: the ranges a laser would measure in an occupancy grid, and the lattice of reference poses ---------------------
 * The localisation monitor's pick (ndtgpu_locmon_pick_device) needs a bank of reference scans with known poses.  The reference makes
 * one from the map alone: generateRefScans (flirtlib_ros/src/place_rec_test.cpp:203-260) walks a lattice of (x, y, theta) over the free
 * cells of the grid (:218-237), calls occupancy_grid_utils::simulateRangeScan(*grid, pose, scanner_params, true) at each pose (:242) and
 * runs the FLIRT detector and descriptor on the simulated scan (:245-254); simulate_scans.cpp:120-142 publishes the scans of virtual
 * lasers through the same call (simulate_scans.cpp:131).  This section is that call and that lattice on the device.  It closes the
 * loop: grid -> simulated reference scans -> ndtgpu_featbank_extract_device -> ndtgpu_featbank_match_device ->
 * ndtgpu_locmon_pick_device -> ndtgpu_locmon_evaluate_device, a robot relocalised in a map this library built, without a scan
 * database and without a visit to the host.
 * PROVENANCE: restated from the reference's call sites cited above.  occupancy_grid_utils (simulateRangeScan) is not vendored by the
 * reference, only its call sites are; its semantics are restated here from those call sites and its public documentation: a ray
 * per beam from the sensor's cell through the grid, the range of the first occupied cell (or unknown cell, where the last argument is
 * true), range_max + 1 where there is none within range_max.  No program text of the reference is copied.
 * Semantics (restated; the order of every fp64 operation -- not contracted -- is written out in csrc/ndt_scansim.h; everything that
 * decides a result is integer: tests/scansim_model.py restates it and the device's outputs equal the model's bit for bit).
 *   grid     int8, width x height, row-major, origin[2], resolution, as ndtgpu_mapset_occupancy_grid_device writes it.  A pixel is an
 *            obstacle iff v >= occupied_min (55), unknown iff v < 0; an unknown pixel counts as an obstacle iff unknown_is_obstacle
 *            (1: every call site passes true).
 *   pose     (x, y, c, s).  Beam i has the table entry (cb_i, sb_i) of ndtgpu_locmon_beam_table, installed by
 *            ndtgpu_scansim_set_beams; its direction is ex = c * cb - s * sb, ey = s * cb + c * sb (the order of ndtgpu_locmon_pixel).
 *   ray      c0 = (floor((x - ox) / res), floor((y - oy) / res)); c1 the same of (x + ex * range_max, y + ey * range_max); (di, dj) =
 *            c1 - c0, n = max(|di|, |dj|).  The cell of step k = 1 .. n advances sign * k on the major axis (x where |di| == |dj|)
 *            and sign * floor((2 * k * dmin + n) / (2 * n)) on the minor one.  The start cell is never tested (upstream's !(c ==
 *            c0)).  A ray with |di| or |dj| above 2^15 or not a number (a direction that is no unit vector) is a miss.
 *   stop     per visited cell, in this order: outside the grid: miss; d2 = di_k^2 + dj_k^2 > R * R: miss, R = (int)floor(range_max /
 *            resolution); an obstacle, or an unknown counted as one: hit, range = resolution * sqrt((double)d2); behind step n: miss.
 *            A miss writes prm.miss (11.0 = range_max + 1, upstream's out-of-range value; above the extraction's r_max, whose gate
 *            drops it).  At most R + 2 steps a beam.
 *   scan     a record {n_hits, flags} per pose.  NDTGPU_SCANSIM_OFFMAP: c0 is outside the grid (compared as doubles; a NaN is off the
 *            map): no walk, every beam a miss.  NDTGPU_SCANSIM_BAD_INDEX: grid index >= n_grids: the same.  NDTGPU_SCANSIM_NO_POSE:
 *            the row is at or beyond count_dev[0]: the same.
 *   lattice  positions ix = 0, skip, ... below width (outer loop), iy likewise (middle loop), headings theta = 0, then += angle_step
 *            while theta < 6.28 (inner loop; cs / sn made on the host by ndtgpu_scansim_headings, the ndtgpu_calib_lattice
 *            convention).  A position is kept iff its pixel == 0 and its centre (ox + ((double)ix + 0.5) * res, oy likewise) lies in
 *            [x0, x1] x [y0, y1].  Kept poses are written compacted, in loop order, as poses_dev[.][4]: the ref_poses_dev layout of
 *            ndtgpu_locmon_pick_device; index_dev[.] is the linear lattice index ((ix / skip) * npy + iy / skip) * nyaw + iyaw, npy =
 *            ceil(height / skip).  count_dev[0] is the number of poses written, at most capacity; count_dev[1] the number that
 *            passed.  skip = (unsigned)(ref_pos_resolution / resolution) (ndtgpu_scansim_skip); 0 is refused.
 * DEVIATIONS:
 *   - ranges run between cell centres: upstream measures from the pose's point; the two agree for generateRefScans, whose poses are
 *     cell centres.
 *   - the reach test is an integer test (d2 > R * R); upstream compares a distance in metres.
 *   - the walk ends on leaving the grid, instead of projecting the ray's endpoint onto the grid first.
 *   - occupied_min replaces upstream's OCCUPIED constant (100): 55 is the smallest value this library's rasteriser gives an occupied
 *     pixel.
 *   - headings by repeated addition of angle_step from 0 (the reference's loop), their cosines and sines from the host.
 *   - flags replace the assertions (a pose off the map aborts upstream).
 *   - left out: the FLIRT detector and descriptor of :245-254 are ndtgpu_featbank_extract_device, behind this on the same stream.
 * Limits: n_beams 1 .. 8192; R 1 .. 4094; width, height 1 .. 2^15; 1 .. 1024 grids; up to 2^24 poses a call, a lattice's capacity and
 * headings; a lattice of at most 2^32 - 1 nodes.
 * Device form (csrc/ndt_scansim.hip): plain launches on the caller's stream, no atomics, no workgroup waits on another, no environment
 * switches.  Cast: one workgroup of 256 lanes per pose, a lane per beam, tiles of 256 beams in turn; all lanes of a wave advance k
 * together, so neighbouring beams load neighbouring bytes in the same iteration and a wave leaves the loop once its last lane has
 * stopped; plain byte loads through L2 (poses in lattice order: neighbouring workgroups walk the same pixels); n_hits by one block
 * count (csrc/ndt_block.h).  A (tiles of beams) x (poses) grid would need a second pass to add a pose's n_hits over its tiles without
 * atomics; the workgroup-per-pose form shipped and that variant was not built, nor was an LDS patch of (2 R + 1)^2 pixels (78 KiB at R =
 * 140 already; R = 200 of the reference's configuration does not fit).  Lattice: the ordered selection of the link gate, three
 * launches: flag-and-count per tile of 256 positions, one workgroup's scan of the tile counts, emit by block rank.
 * Measured on MI355X (tools/scansim_cost.py, library 0.13.0; HIP events around the call, median of 7 after a warm-up, min .. max), in
 * the replay's world at 0.05 m (13600 x 12000 pixels, 2.4 M obstacle pixels; the assembled world carries no free-space evidence, so its
 * unknown pixels are taken as free): 1024 poses x 1440 beams over the full circle, range_max 30 (R = 600), 1.27 ms (1.27 .. 1.30; 1.24 us
 * a pose, 63 % of the beams hit; 218 G cells walked a second, the cells counted by the model on 4 poses and SCALED: an extrapolation).
 * The configuration of place_rec_test -- 181 beams over +- pi / 2, range_max 10 (R = 200), ref_pos_resolution 1 m (skip 20) and 8
 * headings: the lattice, 3 264 000 nodes -> 3 215 968 poses, 0.138 ms (0.134 .. 0.140); their scans 175.8 ms (175.6 .. 175.9; 0.055 us a
 * pose; 12 % of the beams hit, the rest walk the whole reach; 595 G cells a second, SCALED the same way).  The FLIRT extraction of the
 * 11 680 scans within 20 m of the first room on the same stream: 1.75 ms alone (1.73 .. 1.80), 2.27 ms with their simulation in front
 * (2.23 .. 2.32; +0.52 ms; the simulation alone 0.56 ms), 2.1 features a scan.  tests/scansim_model.py on one core of the same box:
 * 44.4 ms a pose at 1440 beams and 4.15 ms at 181 beams (4 poses each, the same bits as the device), SCALED 45.5 s and 13 346 s, 35 700
 * and 75 900 times the device: extrapolations.
 * Kernels (tools/kernel_resources.py scansim): cast 42, flag 12, scan 16, emit 14 VGPRs, no spills, no scratch; LDS 32 B each. */
typedef struct ndtgpu_scansim ndtgpu_scansim;
typedef struct {
    double range_max;                /* the scanner's reach, metres (10.0); R = floor(range_max / resolution) must be 1 .. 4094 */
    double miss;                     /* what a beam without a hit reads (11.0 = range_max + 1) */
    int32_t occupied_min;            /* a pixel >= this is an obstacle (55) */
    int32_t unknown_is_obstacle;     /* 1: a pixel < 0 stops a ray as an obstacle does (1); 0: it is free */
} ndtgpu_scansim_params;
#define NDTGPU_SCANSIM_OFFMAP 1u
#define NDTGPU_SCANSIM_BAD_INDEX 2u
#define NDTGPU_SCANSIM_NO_POSE 4u
typedef struct {
    uint32_t n_hits;                 /* beams that hit */
    uint32_t flags;                  /* NDTGPU_SCANSIM_OFFMAP | _BAD_INDEX | _NO_POSE */
} ndtgpu_scansim_result;
void ndtgpu_default_scansim_params(ndtgpu_scansim_params *p);
/* the lanes of a workgroup: the beams of one pass of a cast, the positions of a lattice tile */
uint32_t ndtgpu_scansim_tile(void);
/* Pure host functions (no device), built on what the kernels call (csrc/ndt_scansim.h).
 * ndtgpu_scansim_check: the checks of set_grids* (n_grids, width, height, resolution), set_beams (n_beams, angle_min,
 * angle_increment) and simulate* (n_poses, prm) at once; prm NULL: the defaults.  NDTGPU_ERR_INVALID with a message that names the
 * argument. */
ndtgpu_status ndtgpu_scansim_check(size_t n_grids, size_t width, size_t height, double resolution, size_t n_beams, double angle_min,
                                   double angle_increment, size_t n_poses, const ndtgpu_scansim_params *prm);
/* R = (int)floor(range_max / resolution); NDTGPU_ERR_INVALID (and *R = 0) unless both are finite and > 0 and R is 1 .. 4094 */
ndtgpu_status ndtgpu_scansim_reach(double range_max, double resolution, int32_t *R);
/* skip = (unsigned)(ref_pos_resolution / resolution); NDTGPU_ERR_INVALID (and *skip = 0) unless it is 1 .. 2^15 */
ndtgpu_status ndtgpu_scansim_skip(double ref_pos_resolution, double resolution, uint32_t *skip);
/* the cell of step k (0 .. max(|di|, |dj|)) of a ray of (di, dj) cells, relative to its start: the closed form above */
ndtgpu_status ndtgpu_scansim_cell(int32_t di, int32_t dj, int32_t k, int32_t cell2[2]);
/* one beam with table entry (cb, sb) from pose4 = (x, y, c, s) on a HOST grid of width x height: *range, *hit (1 or 0) and *flags (0 or
 * NDTGPU_SCANSIM_OFFMAP) */
ndtgpu_status ndtgpu_scansim_beam(const int8_t *grid, size_t width, size_t height, const double origin2[2], double resolution,
                                  const double pose4[4], double cb, double sb, const ndtgpu_scansim_params *prm, double *range, int32_t *hit,
                                  uint32_t *flags);
/* the headings of generateRefScans: *count, and cs[k] = cos(theta_k), sn[k] = sin(theta_k) where not NULL (NDTGPU_ERR_CAPACITY where
 * *count > room) */
ndtgpu_status ndtgpu_scansim_headings(double angle_step, size_t *count, double *cs, double *sn, size_t room);
/* a simulator for up to max_grids grids (1 .. 1024), scans of up to max_beams beams (1 .. 8192) and calls of up to max_poses poses (1 ..
 * 2^24): it owns the origins, the beam table and, from their first use, the grids of the host form, the lattice's tile counts and
 * heading tables and the staging of the host forms */
ndtgpu_status ndtgpu_scansim_create(size_t max_grids, size_t max_beams, size_t max_poses, ndtgpu_scansim **out);
ndtgpu_status ndtgpu_scansim_destroy(ndtgpu_scansim *h);
/* installs the beam table of a scanner geometry (made on the host, uploaded on `stream`).  Waits on the host for the handle's
 * previous call. */
ndtgpu_status ndtgpu_scansim_set_beams(ndtgpu_scansim *h, size_t n_beams, double angle_min, double angle_increment, ndtgpu_stream stream);
/* installs n_grids grids: DEVICE grids_dev, n_grids x height x width int8, BORROWED until the next set_grids* or destroy (as the MCL
 * borrows map sets): the caller keeps the bytes alive and orders its writes to them before the calls that read them; HOST origins2,
 * n_grids x 2, copied before the call returns.  The arguments are checked before the handle is read and the device is looked for.
 * Calls on one handle are ordered on the device whatever stream each names. */
ndtgpu_status ndtgpu_scansim_set_grids_device(ndtgpu_scansim *h, const int8_t *grids_dev, size_t n_grids, size_t width, size_t height,
                                              double resolution, const double *origins2, ndtgpu_stream stream);
/* the same on a HOST array of grids, copied into a buffer the handle owns; synchronous */
ndtgpu_status ndtgpu_scansim_set_grids(ndtgpu_scansim *h, const int8_t *grids, size_t n_grids, size_t width, size_t height, double resolution,
                                       const double *origins2);
/* The lattice of grid `grid`.  HOST cs, sn [nyaw] (copied before the call returns), box4 = (x0, y0, x1, y1) or NULL: no box.  DEVICE:
 * poses_dev capacity x 4 doubles, index_dev capacity uint32 or NULL, count_dev 2 uint32.  Asynchronous on `stream`. */
ndtgpu_status ndtgpu_scansim_lattice_device(ndtgpu_scansim *h, uint32_t grid, uint32_t skip, const double *cs, const double *sn, size_t nyaw,
                                            const double *box4, size_t capacity, double *poses_dev, uint32_t *index_dev, uint32_t *count_dev,
                                            ndtgpu_stream stream);
/* the same into HOST arrays, synchronous: counts2 and the first counts2[0] rows of poses and index (may be NULL) are written */
ndtgpu_status ndtgpu_scansim_lattice(ndtgpu_scansim *h, uint32_t grid, uint32_t skip, const double *cs, const double *sn, size_t nyaw,
                                     const double *box4, size_t capacity, double *poses, uint32_t *index, uint32_t counts2[2]);
/* The scans of n_poses poses.  DEVICE: poses_dev n_poses x 4; grid_idx_dev n_poses uint32 or NULL: grid 0; count_dev NULL: all rows,
 * else rows at or beyond count_dev[0] (what _lattice_device wrote) become all-miss scans flagged NDTGPU_SCANSIM_NO_POSE without a walk:
 * a launch of fixed capacity behind _lattice_device needs no host visit, and the later stages see empty scans, which are never
 * picked; ranges_dev n_poses x n_beams doubles (the buffer ndtgpu_featbank_extract_device, ndtgpu_scanproj_project_device and
 * ndtgpu_locmon_evaluate_device read); results_dev n_poses records or NULL.  prm NULL: the defaults.  Asynchronous on `stream`;
 * NDTGPU_ERR_CAPACITY beyond max_poses; NDTGPU_ERR_INVALID where no grids or no beams are installed. */
ndtgpu_status ndtgpu_scansim_simulate_device(ndtgpu_scansim *h, const double *poses_dev, const uint32_t *grid_idx_dev, size_t n_poses,
                                             const uint32_t *count_dev, const ndtgpu_scansim_params *prm, double *ranges_dev,
                                             ndtgpu_scansim_result *results_dev, ndtgpu_stream stream);
/* the same on HOST arrays through the handle's pinned staging, synchronous; grid_idx and results may be NULL */
ndtgpu_status ndtgpu_scansim_simulate(ndtgpu_scansim *h, const double *poses, const uint32_t *grid_idx, size_t n_poses,
                                      const ndtgpu_scansim_params *prm, double *ranges, ndtgpu_scansim_result *results);

/* ---- marker export: NDT cell axes, graph links and particles as the points of a LINE_LIST ----------------------------------------------
 * The reference's publish timer does two things with a map (ndt_feature2d_fuser.cpp:425-433, 448-454): it rasterises it
 * (toOccupancyGrid: the occupancy-grid export above) and it publishes it as ndt_visualisation::markerNDTCells(...).  markerNDTCells is
 * the most-called function of the reference's application layer: the 2D fuser node (:425, :448), the 3D fuser node
 * (ndt_feature_fuser.cpp:253), the MCL node (ndt_feature_mcl_node.cpp:287), ndt_fusion_test.cpp:31, 232-236 and
 * ndt_feature_pcl_eval.cpp:808-813; markerParticlesNDTMCL3D (mcl node :274) and markerNDTFeatureLinks stand next to it.  Everything
 * upstream of them lives on the device (fused node maps, assembled worlds, optimised poses, gated links, particle banks); this section
 * turns it into marker points there: a 3 x 3 symmetric eigendecomposition per Gaussian cell, a threshold per axis, and 0 .. 3 segments a
 * cell written compacted in a fixed order over all maps of a call, each map under its own pose.
 * PROVENANCE: restated from ndt_rviz.h:1032-1153, 1163-1233, 1277-1297 and ndt_feature_rviz.h:282-313 of the reference and the call
 * sites cited above.  No program text of the reference is copied.
 * Semantics (restated; the order of every fp64 operation -- not contracted -- is written out in csrc/ndt_marker.h, and
 * tests/marker_model.py restates it: the device's outputs equal the model's bit for bit).
 *   marker     a LINE_LIST: a list of points, two per segment, three doubles a point (geometry_msgs/Point is float64); scale.x = 0.02.
 *              A segment is a row of six doubles here: p1, then p2.
 *   cells      (ndt_rviz.h:1090-1153, 1163-1233) for every Gaussian cell of a map, in the order of the map's cell array (slot order), for
 *              j = 0, 1, 2 over the eigenvalues in ascending order: skipped if evals(j) < min_eval (0.0001); else offset = evecs.col(j) *
 *              sqrt(evals(j)), p1 = mean - offset, p2 = mean + offset, emitted as pose * p1, pose * p2 (p1, p2 unchanged with no pose).
 *              Cells without a Gaussian emit nothing: the cell arrays hold Gaussian cells only.  The segments of a call are in (map,
 *              cell, axis) order; src[.] = (map index in the set, cell rank in the map) per segment where asked for.
 *   particles  (ndt_rviz.h:1289-1295) per particle i, in particle order: T.translation() and T * (particle_length, 0, 0) (0.3).
 *   links      (ndt_feature_rviz.h:294-309) per link, in link order: the translations of pose(ref_idx) and pose(mov_idx); where
 *              skip_negative (upstream's skipOdom) is set, links with score < 0 are skipped.
 *   overflow   the link gate's rule: a result larger than `capacity` writes nothing beyond it, the count is still the true count and
 *              overflow is 1; not an error status.
 * DEVIATIONS:
 *   - the eigen-pairs are RECOMPUTED from the stored covariance (NdtCell::cov, already eigen-floored by the build), not kept from
 *     rescaleCovariance: the cell record carries no eigen-pairs.
 *   - the solver is a cyclic Jacobi written out in csrc/ndt_marker.h (upstream: Eigen's SelfAdjointEigenSolver); eigenvalues that tie
 *     keep the order of the Jacobi's diagonal (a stable sort).
 *   - the SIGN of an eigenvector is fixed: its component of largest magnitude is positive, ties go to the lowest index.  Eigen leaves it
 *     unspecified; it decides which endpoint is p1.
 *   - an eigenvalue that is not finite emits nothing and raises NDTGPU_MARKER_NONFINITE in the call's flags (upstream would publish
 *     sqrt(NaN)).
 *   - min_eval (0.0001) and the particle length (0.3) are parameters with those defaults.
 *   - the pose is the upper three rows of a column-major 4 x 4; a point is R p + t, ((R_i0 p0 + R_i1 p1) + R_i2 p2) + t_i as written.
 *   - a KEPT link whose node index is not a node is refused by the host form and, in the device form, emits nothing and raises
 *     NDTGPU_MARKER_BAD_INDEX (upstream indexes out of bounds).  A link that skip_negative skips is never looked at, as upstream: its
 *     indices may be anything.
 *   - left out: colours, namespaces and ids (host constants: host/ndt_rviz_gpu.h), the ellipsoid visuals of the RViz plugin, pose-arrow,
 *     interest-point and correspondence markers, colouring by occupancy.
 * Limits: up to 2^20 maps a call and 5 * 2^20 tiles of 256 cells over them; up to 2^28 links; capacity below 2^32.
 * Device form (csrc/ndt_marker.hip): plain launches on the caller's stream, no atomics, no workgroup waits on another, no cooperative
 * launch, no captured graph, no environment switches.  Cells: count (a lane per cell, tiles of 256 cells x maps, the Jacobi in registers,
 * ndt_block_count), one workgroup's scan of the tile words in (map, tile) order, emit (the eigen-pairs again by the same function,
 * ndt_block_scan of the lanes' counts plus the tile's base, the lane's segments contiguous).  Links: flag-and-count, the same scan,
 * emit by ndt_block_rank.  Particles: one launch that reads the bank's poses in place.  The same bytes in any batch, at any `first`,
 * with any other maps in the call, on any run.
 * Measured on MI355X (tools/marker_cost.py, library 0.13.0, builder-run; HIP events around the asynchronous call, median of 7 after a
 * warm-up, min .. max; `no stores`: the same call with capacity 0, every launch and every Jacobi but nothing written).  The replay's
 * world as one map (24 173 cells, 46 679 segments, with src): 0.032 ms (0.032 .. 0.045; no stores 0.031).  64 node maps under their
 * poses in one call (11 070 cells, 20 790 segments): 0.044 ms (0.040 .. 0.049; no stores 0.042).  5000 node maps in one call
 * (1 231 573 cells, 2 315 505 segments, 130 MB written): 1.81 ms (1.80 .. 1.83; no stores 1.81), 1.1 % of the 6.29 TB/s copy ceiling.
 * Neither the stores nor the per-cell fp64 Jacobi binds: the two small cases are the latency of three launches, and the large one is
 * the dispatch of its 2 x 80 000 workgroups, 15 of 16 of them empty, because tiles are sized by the set's max_cells (4096) and a node
 * map holds about 250 cells; a scan of the tile words that needs two barriers instead of 626 moved it from 1.85 to 1.81 ms only.
 * Against export_cells per map + numpy.linalg.eigh + the loop of ndt_rviz.h in Python on the same box: 95 ms for the world (the loop
 * over 20 000 cells, SCALED: an extrapolation), 78 ms for the 64 maps, 8.6 s for the 5000 (SCALED the same way) -- 2950, 1770 and 4770
 * times the device form, 133, 177 and 337 times the host form (0.72 / 0.44 / 25.6 ms, the copy of the points included); the points
 * agree to 6e-14 m.  The links of 44 486 edges between 5000 nodes (a synthetic list): 0.023 ms (0.021 .. 0.037), with skip_negative
 * 0.022 ms (29 657 kept), against 0.84 ms of NumPy indexing on the host.  A bank of 64 x 5000 particles: 0.022 ms (0.015 .. 0.039), 33 %
 * of the copy ceiling over the bytes read and written, against 100 ms for ndtgpu_mcl_particles + NumPy; the same points.
 * Kernels (tools/kernel_resources.py marker): count 62, scan 18, emit 86, link flag 8, link emit 12, particle 32 VGPRs; no spills, no
 * scratch; 32 B of LDS each (particle: none). */
typedef struct ndtgpu_marker ndtgpu_marker;
typedef struct {
    double min_eval;                 /* an axis whose eigenvalue is below this emits nothing (0.0001); finite, >= 0 */
    double particle_length;          /* the length of a particle's segment along its x axis, metres (0.3) */
    int32_t skip_negative;           /* 1: links with score < 0 are skipped (upstream's skipOdom) (0) */
    int32_t reserved;
} ndtgpu_marker_params;
#define NDTGPU_MARKER_NONFINITE 1u   /* a cell had an eigenvalue that is not finite: that axis emitted nothing */
#define NDTGPU_MARKER_BAD_INDEX 2u   /* a kept link named a node that is none: it emitted nothing */
void ndtgpu_default_marker_params(ndtgpu_marker_params *p);
/* cells, links or particles of one workgroup (256) */
uint32_t ndtgpu_marker_tile(void);
/* Pure host, no device needed: the argument checks of a handle (max_maps_per_call, max_links), a cell call (maps [first, first + count) of
 * n_maps maps of max_cells cells) and a link call (n_nodes, n_links) into `capacity` segments, and of the parameters (NULL: defaults). */
ndtgpu_status ndtgpu_marker_check(size_t max_maps_per_call, size_t max_links, size_t n_maps, size_t first, size_t count, size_t max_cells,
                                  size_t n_nodes, size_t n_links, size_t capacity, const ndtgpu_marker_params *prm);
/* Pure host: the eigen-pairs of cov6 = (xx xy xz yy yz zz) as the kernels compute them: evals3 ascending, V9[3 k + j] component k of the
 * unit eigenvector of evals3[j] */
ndtgpu_status ndtgpu_marker_eig3(const double cov6[6], double evals3[3], double V9[9]);
/* Pure host: the segments of one cell as the kernels compute them.  T16: the map's pose (column-major 4 x 4) or NULL.  seg18: n_seg rows
 * of (p1, p2), the rest zero; evals3 (may be NULL): the ordered eigenvalues; flags: NDTGPU_MARKER_NONFINITE or 0. */
ndtgpu_status ndtgpu_marker_cell(const double mean3[3], const double cov6[6], const double *T16, const ndtgpu_marker_params *prm, double seg18[18],
                                 double evals3[3], uint32_t *n_seg, uint32_t *flags);
/* A handle owns the tile words and the count words of a selection.  max_maps_per_call: 1 .. 2^20; max_links: 0 .. 2^28. */
ndtgpu_status ndtgpu_marker_create(size_t max_maps_per_call, size_t max_links, ndtgpu_marker **out);
ndtgpu_status ndtgpu_marker_destroy(ndtgpu_marker *h);
/* The cell markers of maps [first, first + count) of `set`, asynchronous on `stream`.  T16_dev: count x 16 doubles, the maps' poses
 * (column-major), or NULL; points_dev: capacity x 6 doubles; src_dev: capacity x 2 uint32 or NULL.  The counts stay with the handle
 * (ndtgpu_marker_count).  NDTGPU_ERR_CAPACITY beyond max_maps_per_call. */
ndtgpu_status ndtgpu_mapset_markers_device(ndtgpu_marker *h, ndtgpu_mapset *set, size_t first, size_t count, const double *T16_dev,
                                           const ndtgpu_marker_params *prm, double *points_dev, uint32_t *src_dev, size_t capacity,
                                           ndtgpu_stream stream);
/* the same with HOST poses in and HOST points out through the handle's pinned staging, synchronous: min(n_segments, capacity) rows are
 * written; overflow and flags may be NULL */
ndtgpu_status ndtgpu_mapset_markers(ndtgpu_marker *h, ndtgpu_mapset *set, size_t first, size_t count, const double *T16,
                                    const ndtgpu_marker_params *prm, double *points, uint32_t *src, size_t capacity, size_t *n_segments,
                                    int32_t *overflow, uint32_t *flags);
/* the TRUE number of segments of the handle's last cell or link call, whether it exceeded the capacity, and its flags; waits for the
 * handle.  overflow and flags may be NULL */
ndtgpu_status ndtgpu_marker_count(ndtgpu_marker *h, size_t *n_segments, int32_t *overflow, uint32_t *flags);
/* The link markers of n_links links between n_nodes nodes, asynchronous on `stream`.  T16_nodes_dev: n_nodes x 16 doubles; ref_dev,
 * mov_dev: n_links uint32; score_dev: n_links doubles or NULL; points_dev: capacity x 6 doubles.  NDTGPU_ERR_CAPACITY beyond max_links. */
ndtgpu_status ndtgpu_marker_links_device(ndtgpu_marker *h, const double *T16_nodes_dev, size_t n_nodes, const uint32_t *ref_dev,
                                         const uint32_t *mov_dev, const double *score_dev, size_t n_links, const ndtgpu_marker_params *prm,
                                         double *points_dev, size_t capacity, ndtgpu_stream stream);
/* the same on HOST arrays, synchronous; a node index out of range is NDTGPU_ERR_INVALID */
ndtgpu_status ndtgpu_marker_links(ndtgpu_marker *h, const double *T16_nodes, size_t n_nodes, const uint32_t *ref, const uint32_t *mov,
                                  const double *score, size_t n_links, const ndtgpu_marker_params *prm, double *points, size_t capacity,
                                  size_t *n_segments, int32_t *overflow);
/* The particle markers of filters [first, first + count) of a bank, read in place: count * n_particles rows of points_dev, filters and
 * particles in order; asynchronous on `stream`, behind the bank's last call.  The call records the BANK's fence on `stream`: the bank's
 * next update, readback or destroy waits for the marker kernel, so the particles it reads are not overwritten under it. */
ndtgpu_status ndtgpu_mcl_markers_device(ndtgpu_mcl *mcl, size_t first, size_t count, const ndtgpu_marker_params *prm, double *points_dev,
                                        ndtgpu_stream stream);
/* the same into a HOST array, synchronous */
ndtgpu_status ndtgpu_mcl_markers(ndtgpu_mcl *mcl, size_t first, size_t count, const ndtgpu_marker_params *prm, double *points);

#ifdef __cplusplus
}
#endif
#endif /* NDTGPU_H */
