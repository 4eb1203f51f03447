// ndt_pgo_robust.h -- robust loop-closure weighting of the two pose-graph banks (include/ndtgpu.h, "robust loop-closure
// weighting"): the weight functions of Huber, Cauchy and DCS, the device view of a bank's robust buffers and the launchers of
// csrc/ndt_pgo_robust.hip.  The weights are written with +, -, *, / and ndt_pgo_sqrt alone and without contraction: the host,
// the device and tests/pgo_robust_model.py give the same bits from the same chi2.  The cost terms are the device's alone
// (Cauchy's takes a logarithm).
#pragma once
#include "ndt_pgo.h"
#include "ndt_pgo3.h"

#define NDT_PGO_ROBUST_TILE 256                   // links per workgroup of the weigh kernels: part of the summation order

struct NdtPgoRobustParamsDev {
    int kind;                                     // NDTGPU_PGO_ROBUST_*
    int min_index_gap;
    double scale, inlier_weight;
};

// what weigh and finish leave per graph
struct NdtPgoRobustSum {
    double cost;                                  // sum of the links' robust cost terms
    double chi2;                                  // sum of the links' chi2
    int32_t flagged;                              // links with weight < inlier_weight
    int32_t status;                               // NDTGPU_PGO_CONVERGED (finite), NDTGPU_PGO_NOT_FINITE or NDTGPU_PGO3_HALF_TURN
};

// a bank's robust buffers, every per-link array with room for max_edges links per graph (the bank's max_edges, one at least)
struct NdtPgoRobustView {
    double *w0;                                   // [G][K max_edges]   the information as the graph was set, the bank's layout
    double *chi2, *weight;                        // [G][max_edges]
    int32_t *inlier;                              // [G][max_edges]
    double *part;                                 // [G][2 tiles]       per tile: cost, then chi2 (k * tiles + t)
    uint32_t *part_n;                             // [G][3 tiles]       per tile: flagged out, not finite, half turns
    NdtPgoRobustSum *sum;                         // [G]
    unsigned tiles;                               // tiles per graph of the arrays above: ceil(max_edges / 256), one at least
};

// DCS: s = min(1, 2 phi / (phi + chi2))
NDT_HD double ndt_pgo_robust_dcs_s(double phi, double chi2)
{
#pragma clang fp contract(off)
    const double s = (2.0 * phi) / (phi + chi2);
    return s < 1.0 ? s : 1.0;                     // (NaN: 1, and the weight of a NaN chi2 is then decided by the caller's test)
}

// the weight of a link from its chi2 = e^T W0 e; NaN where chi2 is
NDT_HD double ndt_pgo_robust_weight(int kind, double scale, double chi2)
{
#pragma clang fp contract(off)
    if (!(chi2 == chi2)) return chi2;
    if (kind == NDTGPU_PGO_ROBUST_HUBER) {
        const double r = ndt_pgo_sqrt(chi2);
        return r <= scale ? 1.0 : scale / r;
    }
    if (kind == NDTGPU_PGO_ROBUST_CAUCHY) return 1.0 / (1.0 + chi2 / (scale * scale));
    const double s = ndt_pgo_robust_dcs_s(scale, chi2);
    return s * s;
}

// the links closer than the gap in node index (the odometry chain at the default, 2) are never re-weighted
NDT_HD bool ndt_pgo_robust_protected(int32_t ref, int32_t mov, int min_index_gap)
{
    const int64_t d = (int64_t)mov - (int64_t)ref;
    return (d < 0 ? -d : d) < (int64_t)min_index_gap;
}

// launchers (csrc/ndt_pgo_robust.hip): graphs [first, first + count) of the bank, max_links the largest n_edges among them.
// weigh: chi2, weight, inlier and the per-tile partial sums of every link; apply: also info = weight * w0.  finish: the graphs'
// sums and verdicts; a graph whose chi2 is not all finite gets w0 back where apply is set.
hipError_t ndt_pgo_robust_launch(const NdtPgoView &v, const NdtPgoRobustView &r, size_t first, size_t count, size_t max_links,
                                 const NdtPgoRobustParamsDev &prm, bool apply, hipStream_t st);
hipError_t ndt_pgo3_robust_launch(const NdtPgo3View &v, const NdtPgoRobustView &r, size_t first, size_t count, size_t max_links,
                                  const NdtPgoRobustParamsDev &prm, bool apply, hipStream_t st);
