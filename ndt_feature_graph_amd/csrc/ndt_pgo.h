// ndt_pgo.h -- what the SE(2) pose-graph kernels (csrc/ndt_pgo.hip: one workgroup per graph; csrc/ndt_pgo_wide.hip: one graph over
// the whole device) and their C-ABI (csrc/ndtgpu_pgo.hip) share: the device view of a bank of graphs, the angle wrap, the
// conversion of a registered link (T16, cov36, flags) into the factor's measurement and information, and the per-link and
// per-node bodies of the optimisation, which both kernel forms call so that they differ in the order of their sums alone.
// tests/pgo_model.py restates the conversion operation for operation (its results are compared bit for bit), which is why it is
// written with +, -, *, / and sqrt alone -- the arc cosine included -- and without contraction.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_math.h"
#include <string.h>                               // memcpy (ndt_pgo_acos, on the host side)

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

// an angle in (-pi, pi].  Without contraction: the device compiler made the last line one fma, the host's is a rounded product and
// a sum, and the two differed in the last place for angles outside the interval (tests/test_pgo_direct.py holds them to the same bits).
NDT_HD double ndt_pgo_wrap(double t)
{
#pragma clang fp contract(off)
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

// ---- what the one-workgroup form (csrc/ndt_pgo.hip) and the chip-wide form (csrc/ndt_pgo_wide.hip) do per link and per node ----

// y = W x, W symmetric as 6 numbers
NDT_D void pgo_symv(const double *W, double x0, double x1, double x2, double &y0, double &y1, double &y2)
{
    y0 = W[0] * x0 + W[1] * x1 + W[2] * x2;
    y1 = W[1] * x0 + W[3] * x1 + W[4] * x2;
    y2 = W[2] * x0 + W[4] * x1 + W[5] * x2;
}

// The factor's error is e = (p_mov ominus p_ref) - z.  With c, s of t_ref and (lx, ly) = p_mov ominus p_ref's translation:
//   J_ref = [[-c, -s, ly], [s, -c, -lx], [0, 0, -1]]      J_mov = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
// J^T w for the side of the edge the node is on
NDT_D void pgo_jt(int side, double c, double s, double lx, double ly, double w0, double w1, double w2, double &g0, double &g1, double &g2)
{
    if (side == 0) {
        g0 = -c * w0 + s * w1;
        g1 = -s * w0 - c * w1;
        g2 = ly * w0 - lx * w1 - w2;
    } else {
        g0 = c * w0 - s * w1;
        g1 = s * w0 + c * w1;
        g2 = w2;
    }
}

// one graph of a bank: its arrays and its part of the scratch
struct PgoGraph {
    unsigned N, E;
    double *pose;
    const double *origin;
    const int32_t *ref, *mov;
    const double *meas, *info;
    const uint32_t *adj_off, *adj;
    double *jac, *te;
    double *prev, *b, *x, *r, *z, *p, *ap, *dinv;
};

// graph g of the bank, with n_nodes nodes and n_edges links
NDT_HD PgoGraph ndt_pgo_graph(const NdtPgoView &v, size_t g, unsigned n_nodes, unsigned n_edges)
{
    PgoGraph G;
    G.N = n_nodes;
    G.E = n_edges;
    G.pose = v.pose + g * 3 * v.max_nodes;
    G.origin = v.origin + g * 3;
    G.ref = v.ref + g * v.max_edges;
    G.mov = v.mov + g * v.max_edges;
    G.meas = v.meas + g * 3 * v.max_edges;
    G.info = v.info + g * 6 * v.max_edges;
    G.adj_off = v.adj_off + g * (v.max_nodes + 1);
    G.adj = v.adj + g * 2 * v.max_edges;
    G.jac = v.jac + g * 4 * v.max_edges;
    G.te = v.te + g * 3 * v.max_edges;
    double *nb = v.node + g * NDT_PGO_NODE_DOUBLES * v.max_nodes;
    G.prev = nb;
    G.b = nb + 3 * v.max_nodes;
    G.x = nb + 6 * v.max_nodes;
    G.r = nb + 9 * v.max_nodes;
    G.z = nb + 12 * v.max_nodes;
    G.p = nb + 15 * v.max_nodes;
    G.ap = nb + 18 * v.max_nodes;
    G.dinv = nb + 21 * v.max_nodes;
    return G;
}

// the prior's error on node 0
NDT_D void pgo_prior_error(const PgoGraph &G, double &e0, double &e1, double &e2)
{
    e0 = G.pose[0] - G.origin[0];
    e1 = G.pose[1] - G.origin[1];
    e2 = ndt_pgo_wrap(G.pose[2] - G.origin[2]);
}

// the prior's term of the cost
NDT_D double pgo_prior_cost(const PgoGraph &G, const NdtPgoParamsDev &prm)
{
    double e0, e1, e2, w0, w1, w2;
    pgo_prior_error(G, e0, e1, e2);
    pgo_symv(prm.prior, e0, e1, e2, w0, w1, w2);
    return e0 * w0 + e1 * w1 + e2 * w2;
}

// link e at the current poses: error, the Jacobian numbers c, s, lx, ly into jac, W e into te; returns e^T W e
NDT_D double pgo_linearise_link(const PgoGraph &G, unsigned e)
{
    const double *pi = G.pose + 3 * (size_t)G.ref[e], *pj = G.pose + 3 * (size_t)G.mov[e];
    double s, c;
    sincos(pi[2], &s, &c);
    const double dx = pj[0] - pi[0], dy = pj[1] - pi[1];
    const double lx = c * dx + s * dy, ly = -s * dx + c * dy;
    const double *zm = G.meas + 3 * (size_t)e;
    const double e0 = lx - zm[0], e1 = ly - zm[1], e2 = ndt_pgo_wrap(ndt_pgo_wrap(pj[2] - pi[2]) - zm[2]);
    double w0, w1, w2;
    pgo_symv(G.info + 6 * (size_t)e, e0, e1, e2, w0, w1, w2);
    double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e;
    j[0] = c; j[1] = s; j[2] = lx; j[3] = ly;
    t[0] = w0; t[1] = w1; t[2] = w2;
    return e0 * w0 + e1 * w1 + e2 * w2;
}

// node i: b = -gradient and the inverse of the 3x3 diagonal block of J^T W J, over the node's incident edges in ascending order
NDT_D void pgo_gather_node(const PgoGraph &G, const NdtPgoParamsDev &prm, unsigned i)
{
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, D[6] = {0, 0, 0, 0, 0, 0};
    for (unsigned k = G.adj_off[i]; k < G.adj_off[i + 1]; k++) {
        const unsigned a = G.adj[k], e = a >> 1;
        const int side = (int)(a & 1u);
        const double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e, *W = G.info + 6 * (size_t)e;
        double h0, h1, h2;
        pgo_jt(side, j[0], j[1], j[2], j[3], t[0], t[1], t[2], h0, h1, h2);
        g0 += h0; g1 += h1; g2 += h2;
        // J^T W J: column q of W J, then J^T of it
        const double c = j[0], s = j[1], lx = j[2], ly = j[3];
        const double Jc[3][3] = {{side ? c : -c, side ? -s : s, 0.0}, {side ? s : -s, side ? c : -c, 0.0},
                                 {side ? 0.0 : ly, side ? 0.0 : -lx, side ? 1.0 : -1.0}};   // Jc[q] = column q of J
        double M[3][3];
        for (int q = 0; q < 3; q++) {
            double u0, u1, u2;
            pgo_symv(W, Jc[q][0], Jc[q][1], Jc[q][2], u0, u1, u2);
            pgo_jt(side, c, s, lx, ly, u0, u1, u2, M[0][q], M[1][q], M[2][q]);
        }
        D[0] += M[0][0]; D[1] += M[0][1]; D[2] += M[0][2]; D[3] += M[1][1]; D[4] += M[1][2]; D[5] += M[2][2];
    }
    if (i == 0) {
        double e0, e1, e2, w0, w1, w2;
        pgo_prior_error(G, e0, e1, e2);
        pgo_symv(prm.prior, e0, e1, e2, w0, w1, w2);
        g0 += w0; g1 += w1; g2 += w2;
        for (int k = 0; k < 6; k++) D[k] += prm.prior[k];
    }
    double *b = G.b + 3 * (size_t)i, *di = G.dinv + 6 * (size_t)i;
    b[0] = -g0; b[1] = -g1; b[2] = -g2;
    if (!ndt_pgo_inv_sym3(D[0], D[1], D[2], D[3], D[4], D[5], di)) {      // (an information matrix that is not positive definite)
        di[0] = di[3] = di[5] = 1.0;
        di[1] = di[2] = di[4] = 0.0;
    }
}

// link e of the matrix-vector product: t_e = W (J_ref p_ref + J_mov p_mov) from the two end nodes' search directions
NDT_D void pgo_link_product(const PgoGraph &G, unsigned e, const double *pi, const double *pj)
{
    const double *j = G.jac + 4 * (size_t)e;
    const double c = j[0], s = j[1], lx = j[2], ly = j[3];
    const double u0 = -c * pi[0] - s * pi[1] + ly * pi[2] + c * pj[0] + s * pj[1];
    const double u1 = s * pi[0] - c * pi[1] - lx * pi[2] - s * pj[0] + c * pj[1];
    const double u2 = pj[2] - pi[2];
    double *t = G.te + 3 * (size_t)e;
    pgo_symv(G.info + 6 * (size_t)e, u0, u1, u2, t[0], t[1], t[2]);
}

// node i of the matrix-vector product: (A p)_i = sum J^T t_e over the node's incident edges in ascending order, the prior's
// block on node 0; p0..p2 is the node's search direction
NDT_D void pgo_node_product(const PgoGraph &G, const NdtPgoParamsDev &prm, unsigned i, double p0, double p1, double p2, double &a0,
                            double &a1, double &a2)
{
    a0 = 0.0; a1 = 0.0; a2 = 0.0;
    for (unsigned q = G.adj_off[i]; q < G.adj_off[i + 1]; q++) {
        const unsigned a = G.adj[q], e = a >> 1;
        const double *j = G.jac + 4 * (size_t)e, *t = G.te + 3 * (size_t)e;
        double h0, h1, h2;
        pgo_jt((int)(a & 1u), j[0], j[1], j[2], j[3], t[0], t[1], t[2], h0, h1, h2);
        a0 += h0; a1 += h1; a2 += h2;
    }
    if (i == 0) {
        double w0, w1, w2;
        pgo_symv(prm.prior, p0, p1, p2, w0, w1, w2);
        a0 += w0; a1 += w1; a2 += w2;
    }
}

// host launchers (csrc/ndt_pgo.hip)
// graphs [first, first + count) of the bank, one workgroup each
hipError_t ndt_pgo_launch(const NdtPgoView &v, size_t first, size_t count, const NdtPgoParamsDev &prm, hipStream_t st);
// meas / info of graph g from n_edges registered links in device memory
hipError_t ndt_pgo_launch_links(const NdtPgoView &v, size_t g, size_t n_edges, const double *T16_dev, const double *cov36_dev,
                                const int32_t *cov_flags_dev, hipStream_t st);
