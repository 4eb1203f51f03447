// ndt_pgo.h -- what the SE(2) pose-graph kernels (csrc/ndt_pgo.hip) and their C-ABI (csrc/ndtgpu_pgo.hip) share: the device view
// of a bank of graphs, the angle wrap, and the conversion of a registered link (T16, cov36, flags) into the factor's
// measurement and information.  tests/pgo_model.py restates the conversion operation for operation (its results are compared
// bit for bit), which is why it is written with +, -, *, / and sqrt alone -- the arc cosine included -- and without contraction.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_math.h"

#define NDT_PGO_THREADS 1024                      // one workgroup per graph
#define NDT_PGO_WAVES (NDT_PGO_THREADS / 64)
#define NDT_PGO_NODE_DOUBLES 27                   // per node of scratch: prev, b, x, r, z, p, Ap (3 each) and the 3x3 block inverse (6)

// symmetric 3x3 as 6 numbers: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)

struct NdtPgoParamsDev {
    int max_iterations, max_linear_iterations;
    double eps_step, eps_linear;
    double prior[6];                              // the prior's information, symmetric part
};

// a bank of n_graphs graphs, every array with room for max_nodes / max_edges per graph
struct NdtPgoView {
    size_t max_nodes, max_edges;
    ndtgpu_pgo_result *state;                     // [G]
    double *pose;                                 // [G][3 max_nodes]  (x, y, t)
    double *origin;                               // [G][3]            node 0's pose when the graph was set
    int32_t *ref, *mov;                           // [G][max_edges]
    double *meas;                                 // [G][3 max_edges]
    double *info;                                 // [G][6 max_edges]
    uint32_t *adj_off;                            // [G][max_nodes + 1]  node -> its incident edges, CSR
    uint32_t *adj;                                // [G][2 max_edges]    (edge << 1) | (1 where the node is the edge's mov), ascending
    double *jac;                                  // [G][4 max_edges]    c, s, lx, ly of the linearisation: both Jacobian blocks
    double *te;                                   // [G][3 max_edges]    W e after a linearisation, t_e in the solve
    double *node;                                 // [G][NDT_PGO_NODE_DOUBLES max_nodes]
};

// an angle in (-pi, pi]
NDT_HD double ndt_pgo_wrap(double t)
{
    const double two_pi = 6.283185307179586;
    if (t > -3.141592653589793 && t <= 3.141592653589793) return t;
    return t + two_pi * floor((3.141592653589793 - t) / two_pi);
}

NDT_HD double ndt_pgo_sqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// acos on [-1, 1] by the rational approximation of the freely distributable fdlibm (e_acos.c), which needs correctly rounded
// +, -, *, / and sqrt only: the same bits on the host, on the device and in tests/pgo_model.py
NDT_HD double ndt_pgo_acos(double x)
{
#pragma clang fp contract(off)
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    if (x >= 1.0) return 0.0;
    if (x <= -1.0) return pi + 2.0 * pio2_lo;
    if (!(x == x)) return x;
    const double ax = fabs(x);
    if (ax < 0.5) {
        if (ax <= 6.938893903907228e-18) return pio2_hi + pio2_lo;         // 2^-57
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double s = ndt_pgo_sqrt(z);
        const double r = p / q;
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;
    const double s = ndt_pgo_sqrt(z);
    unsigned long long bits;
    memcpy(&bits, &s, 8);
    bits &= 0xFFFFFFFF00000000ull;                                          // s with its low word cleared
    double df;
    memcpy(&df, &bits, 8);
    const double c = (z - df * df) / (s + df);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    const double w = r * s + c;
    return 2.0 * (df + w);
}

// getRobustYawFromAffine3d (utils.h:30-40) of a column-major 4x4, the cosine brought into [-1, 1] first
NDT_HD double ndt_pgo_robust_yaw(const double *T16)
{
    const double angle = ndt_pgo_acos(T16[0]);
    return (T16[1] > 0.0) ? angle : -angle;
}

// the inverse of the symmetric [[a b c] [b d e] [c e f]] by cofactors; false where the matrix is not positive definite
// (Sylvester's criterion) or the inverse is not finite
NDT_HD bool ndt_pgo_inv_sym3(double a, double b, double c, double d, double e, double f, double *W6)
{
#pragma clang fp contract(off)
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double det = a * c00 + b * c01 + c * c02;
    W6[0] = c00 / det; W6[1] = c01 / det; W6[2] = c02 / det;
    W6[3] = c11 / det; W6[4] = c12 / det; W6[5] = c22 / det;
    bool ok = a > 0.0 && c22 > 0.0 && det > 0.0;
    for (int k = 0; k < 6; k++) ok = ok && (W6[k] - W6[k] == 0.0);
    return ok;
}

// A registered link as the factor takes it: z = (x, y, robust yaw) of T16; W = the inverse of the (x, y, yaw) block of cov36
// (row-major 6x6, rows / columns 0, 1, 5; its symmetric part).  The covariance 0.02 * I stands in where flags has any of
// NDTGPU_COV_SINGULAR / POSE_UNCHANGED / NOT_COMPUTED (ndt_feature_graph.cpp:283-310) and where the block does not invert
// (ndt_pgo_inv_sym3).  cov36 == NULL: W = 100 * I.
NDT_HD void ndt_pgo_link_from_registration(const double *T16, const double *cov36, int flags, double *z3, double *W6)
{
#pragma clang fp contract(off)
    z3[0] = T16[12];
    z3[1] = T16[13];
    z3[2] = ndt_pgo_robust_yaw(T16);
    if (!cov36) {
        W6[0] = W6[3] = W6[5] = 100.0;
        W6[1] = W6[2] = W6[4] = 0.0;
        return;
    }
    const bool flagged = (flags & (NDTGPU_COV_SINGULAR | NDTGPU_COV_POSE_UNCHANGED | NDTGPU_COV_NOT_COMPUTED)) != 0;
    if (!flagged && ndt_pgo_inv_sym3(cov36[0], 0.5 * (cov36[1] + cov36[6]), 0.5 * (cov36[5] + cov36[30]), cov36[7],
                                     0.5 * (cov36[11] + cov36[31]), cov36[35], W6))
        return;
    (void)ndt_pgo_inv_sym3(0.02, 0.0, 0.0, 0.02, 0.0, 0.02, W6);
}

// host launchers (csrc/ndt_pgo.hip)
// graphs [first, first + count) of the bank, one workgroup each
hipError_t ndt_pgo_launch(const NdtPgoView &v, size_t first, size_t count, const NdtPgoParamsDev &prm, hipStream_t st);
// meas / info of graph g from n_edges registered links in device memory
hipError_t ndt_pgo_launch_links(const NdtPgoView &v, size_t g, size_t n_edges, const double *T16_dev, const double *cov36_dev,
                                const int32_t *cov_flags_dev, hipStream_t st);
