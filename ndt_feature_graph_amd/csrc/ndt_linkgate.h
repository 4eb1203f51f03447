// ndt_linkgate.h -- what the link-gating kernels (csrc/ndt_linkgate.hip), their C-ABI (csrc/ndtgpu_linkgate.hip) and the host
// mirror's scalar path share: distanceBetweenAffine3d, the gates of a candidate pair and of a registered link, the decoding of a
// pair index and the device view of a gate.  Plain C++ for host and device; tests/linkgate_model.py restates it operation for
// operation.
//
// THE ORDER OF OPERATIONS, part of the contract (the same link is kept or rejected on the host, on the device and in the model):
// every expression below is evaluated as written, left to right, NOT contracted (no fused multiply-add), with IEEE +, -, * and a
// correctly rounded square root (ndt_pgo_sqrt).  The arc cosine is ndt_pgo_acos (csrc/ndt_pgo.h: fdlibm's rational form, the
// same bits everywhere) for |r00| <= 1; |r00| > 1 or a NaN gives NaN where the cosine is not clipped.
//   dx = p2[12] - p1[12], dy = p2[13] - p1[13], dz = p2[14] - p1[14];  dist = sqrt((dx dx + dy dy) + dz dz)
//   r00 = (p1[0] p2[0] + p1[1] p2[1]) + p1[2] p2[2];  clip_cosine: r00 = r00 > 1 ? 1 : (r00 < -1 ? -1 : r00);  ang = |acos(r00)|
//   compose (T_ref T_link), entry (k, c) of the rotation: (R[k,0] L[0,c] + R[k,1] L[1,c]) + R[k,2] L[2,c];
//                           translation k: ((R[k,0] l[0] + R[k,1] l[1]) + R[k,2] l[2]) + t[k]
//   relative (T_i^-1 T_j),  entry (k, c): (Ri[0,k] Rj[0,c] + Ri[1,k] Rj[1,c]) + Ri[2,k] Rj[2,c];
//                           translation k: (Ri[0,k] d[0] + Ri[1,k] d[1]) + Ri[2,k] d[2],  d = t_j - t_i
//
// TWO DEVIATIONS from upstream's distanceBetweenAffine3d (utils.h:42-47: tmp = p1.inverse() * p2, tmp.translation().norm(),
// fabs(getRobustYawFromAffine3d(tmp))), both of which distributed.valid_links already has:
//   - the rigid transpose instead of a general inverse: (R1^T R2)(0, 0) is column 0 of R1 . column 0 of R2;
//   - the difference vector is not rotated: |R1^T (t2 - t1)| = |t2 - t1| for a rotation R1.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/ndtgpu.h"
#include "ndt_pgo.h"

#define NDT_LINKGATE_THREADS 256                  // a workgroup of the flag and emit passes
#define NDT_LINKGATE_WAVES (NDT_LINKGATE_THREADS / 64)
#define NDT_LINKGATE_SUBTILES 4                   // ... works through this many runs of NDT_LINKGATE_THREADS consecutive items
#define NDT_LINKGATE_TILE (NDT_LINKGATE_THREADS * NDT_LINKGATE_SUBTILES)
#define NDT_LINKGATE_SCAN_THREADS 1024            // the one workgroup that scans the tile counts
#define NDT_LINKGATE_MAX_NODES 65536u
#define NDT_LINKGATE_MAX_LINKS (1u << 27)
#define NDT_LINKGATE_MAX_ROW_BYTES 4096u

// the thresholds as the kernels take them
struct NdtLinkGateParamsDev {
    double max_score, max_dist, max_angle;
    int min_idx_dist, clip_cosine;
};

// what the kernels receive of a handle
struct NdtLinkGateView {
    const double *nodes;       // [n_nodes][16] column-major
    uint32_t n_nodes;
    uint32_t *tile;            // per tile: its count after the flag pass, the number kept in the tiles before it after the scan
    uint32_t *total;           // [0] pairs kept by the last candidates call, [1] links kept by the last valid call
    uint32_t *keep;            // [max_links] the last valid call's keep list
};

// distanceBetweenAffine3d(p1, p2) (utils.h:42-47) of two column-major 4x4 poses; see the head of this file
NDT_HD void ndt_linkgate_distance(const double *p1, const double *p2, int clip_cosine, double &dist, double &ang)
{
#pragma clang fp contract(off)
    const double dx = p2[12] - p1[12], dy = p2[13] - p1[13], dz = p2[14] - p1[14];
    dist = ndt_pgo_sqrt((dx * dx + dy * dy) + dz * dz);
    double r00 = (p1[0] * p2[0] + p1[1] * p2[1]) + p1[2] * p2[2];
    if (clip_cosine) r00 = r00 > 1.0 ? 1.0 : (r00 < -1.0 ? -1.0 : r00);        // (a NaN stays a NaN)
    // upstream's acos of a cosine a rounding outside [-1, 1] is NaN, and NaN < max_angle is false
    ang = (r00 >= -1.0 && r00 <= 1.0) ? fabs(ndt_pgo_acos(r00)) : (r00 - r00) / (r00 - r00);
}

// out = T_ref * T_link for rigid poses (the last row is written as 0 0 0 1)
NDT_HD void ndt_linkgate_compose(const double *R, const double *L, double *out)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) out[4 * c + k] = (R[k] * L[4 * c] + R[4 + k] * L[4 * c + 1]) + R[8 + k] * L[4 * c + 2];
    for (int k = 0; k < 3; k++) out[12 + k] = ((R[k] * L[12] + R[4 + k] * L[13]) + R[8 + k] * L[14]) + R[12 + k];
    out[3] = out[7] = out[11] = 0.0;
    out[15] = 1.0;
}

// out = T_i^-1 * T_j by the rigid inverse (R_i^T, -R_i^T t_i)
NDT_HD void ndt_linkgate_relative(const double *Ti, const double *Tj, double *out)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) out[4 * c + k] = (Ti[4 * k] * Tj[4 * c] + Ti[4 * k + 1] * Tj[4 * c + 1]) + Ti[4 * k + 2] * Tj[4 * c + 2];
    const double d[3] = {Tj[12] - Ti[12], Tj[13] - Ti[13], Tj[14] - Ti[14]};
    for (int k = 0; k < 3; k++) out[12 + k] = (Ti[4 * k] * d[0] + Ti[4 * k + 1] * d[1]) + Ti[4 * k + 2] * d[2];
    out[3] = out[7] = out[11] = 0.0;
    out[15] = 1.0;
}

// pairs (i', j') with i' < i among n nodes, in computeAllPossibleLinks' order (i ascending, then j)
NDT_HD uint64_t ndt_linkgate_pairs_before(uint64_t i, uint64_t n) { return i * (2u * n - i - 1u) / 2u; }

// pair index p < n (n - 1) / 2 -> (i, j), i < j.  The square root only proposes the row; the two loops settle it in integers, so
// the result is exact for every p (n <= 65536: (2 n - 1)^2 < 2^34 and 8 p < 2^35 are exact doubles, the proposal is off by at most
// one row).
NDT_HD void ndt_linkgate_decode_pair(uint64_t p, uint32_t n, uint32_t &i, uint32_t &j)
{
    const double b = 2.0 * (double)n - 1.0;
    const double disc = b * b - 8.0 * (double)p;
    double r = 0.5 * (b - ndt_pgo_sqrt(disc > 0.0 ? disc : 0.0));
    if (!(r >= 0.0)) r = 0.0;
    uint64_t row = (uint64_t)r;
    if (row > (uint64_t)n - 2u) row = (uint64_t)n - 2u;
    while (row > 0u && ndt_linkgate_pairs_before(row, n) > p) row--;
    while (row + 2u < (uint64_t)n && ndt_linkgate_pairs_before(row + 1u, n) <= p) row++;
    i = (uint32_t)row;
    j = (uint32_t)(row + 1u + (p - ndt_linkgate_pairs_before(row, n)));
}

// the candidate gate of a pair i < j of the nodes (the index distance, then distanceBetweenAffine3d(T_i, T_j))
NDT_HD bool ndt_linkgate_candidate(const double *nodes, uint32_t i, uint32_t j, const NdtLinkGateParamsDev &prm)
{
    if ((long long)j - (long long)i < (long long)prm.min_idx_dist) return false;
    double dist, ang;
    ndt_linkgate_distance(nodes + 16 * (size_t)i, nodes + 16 * (size_t)j, prm.clip_cosine, dist, ang);
    return dist < prm.max_dist && ang < prm.max_angle;
}

// getValidLinks' test of one registered link (ndt_feature_graph.cpp:527-556); score == NULL: the score is not tested
NDT_HD bool ndt_linkgate_link_valid(const double *nodes, uint32_t n_nodes, uint32_t ref, uint32_t mov, const double *T_link,
                                    const double *score, const NdtLinkGateParamsDev &prm)
{
    if (score && !(*score <= prm.max_score)) return false;
    if (ref >= n_nodes || mov >= n_nodes) return false;
    const long long d = (long long)mov - (long long)ref;
    if ((d < 0 ? -d : d) < (long long)prm.min_idx_dist) return false;
    double pred[16], dist, ang;
    ndt_linkgate_compose(nodes + 16 * (size_t)ref, T_link, pred);
    ndt_linkgate_distance(nodes + 16 * (size_t)mov, pred, prm.clip_cosine, dist, ang);
    return dist < prm.max_dist && ang < prm.max_angle;
}

// host launchers (csrc/ndt_linkgate.hip); every one enqueues on `st` and returns
// all pairs of the view's nodes: total[0] and, up to `capacity`, ref / mov / T16 (T16 may be NULL)
hipError_t ndt_linkgate_launch_candidates(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, uint32_t *ref_dev, uint32_t *mov_dev,
                                          double *T16_dev, size_t capacity, hipStream_t st);
// n_links registered links: total[1], the view's keep list and, up to `capacity`, keep_dev (may be NULL)
hipError_t ndt_linkgate_launch_valid(const NdtLinkGateView &v, const NdtLinkGateParamsDev &prm, size_t n_links, const uint32_t *ref_dev,
                                     const uint32_t *mov_dev, const double *T16_dev, const double *score_dev, uint32_t *keep_dev,
                                     size_t capacity, hipStream_t st);
// rows keep[0 .. total[1]) of src to rows dst_first_row .. of dst, row_words 4-byte words each; max_rows: the links of that valid call
hipError_t ndt_linkgate_launch_gather(const NdtLinkGateView &v, size_t max_rows, const uint32_t *src_dev, size_t row_words, uint32_t *dst_dev,
                                      size_t dst_first_row, hipStream_t st);
