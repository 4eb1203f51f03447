// ndt_pgo3.h -- what the SE(3) pose-graph kernels (csrc/ndt_pgo3.hip: one workgroup per graph) and their C-ABI
// (csrc/ndtgpu_pgo3.hip) share: the device view of a bank of graphs, Exp / Log / the inverse right Jacobian of SO(3), the link
// error with both Jacobian blocks, the retraction, the conversion of a registered link (T16, cov36, flags) into the factor's
// measurement and information, and the per-link and per-node bodies of the optimisation.  include/ndtgpu.h ("SE(3) pose-graph
// optimisation") states the semantics; tests/pgo3_model.py restates them in NumPy, the conversion operation for operation (its
// results are compared bit for bit), which is why that one is written with +, -, *, / and sqrt alone and without contraction.
//
// Layouts.  A pose is twelve doubles: R column-major (R(r, c) = P[3 c + r]) and t in P[9..12) -- a T16 without its last row.
// A symmetric 6x6 is its lower triangle, 21 doubles, (i, j) with i >= j at i (i + 1) / 2 + j.  The 6-vectors are (rho, phi) =
// (x, y, z, rx, ry, rz), the order of cov36.
// A link's linearisation is 39 doubles (NDT_PGO3_JAC): t_E, R_A, M_B = -R_A [t_z']x, N_C = -Jr^-1 R_E^T, N_D = Jr^-1 R_z'^T,
// the four matrices column-major -- every block of
//   J_ref = [[-I, [t_E]x], [0, N_C]]        J_mov = [[R_A, M_B], [0, N_D]]
// that is not a constant.  The products below use the 3x3 blocks only; no 6x6 Jacobian is ever formed on the device.
#pragma once
#include "../../include/ndtgpu.h"
#include "ndt_math.h"
#include "ndt_pgo.h"

#define NDT_PGO3_THREADS 512                      // one workgroup per graph (csrc/ndt_pgo3.hip says why not 1024)
#define NDT_PGO3_WAVES (NDT_PGO3_THREADS / 64)
#define NDT_PGO3_JAC 39
#define NDT_PGO3_NODE_DOUBLES 69                  // per node of scratch: prev (12), b, x, r, z, p, Ap (6 each), the block's Cholesky factor (21)
#define NDT_PGO3_TINY 1e-8                        // |v| below which Log takes R for the identity or a half turn

struct NdtPgo3ParamsDev {
    int max_iterations, max_linear_iterations;
    double eps_step, eps_linear;
    double prior[21];                             // the prior's information, symmetric part
};

// a bank of n_graphs graphs, every array with room for max_nodes / max_edges per graph
struct NdtPgo3View {
    size_t max_nodes, max_edges;
    ndtgpu_pgo_result *state;                     // [G]
    double *pose;                                 // [G][12 max_nodes]
    double *origin;                               // [G][24]             node 0's pose when the graph was set, then the identity (the prior's Z)
    int32_t *ref, *mov;                           // [G][max_edges]
    double *meas;                                 // [G][12 max_edges]   Z as given (inverted where it is used)
    double *info;                                 // [G][21 max_edges]
    uint32_t *adj_off;                            // [G][max_nodes + 1]  node -> its incident edges, CSR
    uint32_t *adj;                                // [G][2 max_edges]    (edge << 1) | (1 where the node is the edge's mov), ascending
    double *jac;                                  // [G][39 (max_edges + 1)]  the linearisations; a graph's slot n_edges is the prior's
    double *te;                                   // [G][6 (max_edges + 1)]   W e after a linearisation, t_e in the solve
    double *node;                                 // [G][NDT_PGO3_NODE_DOUBLES max_nodes]
};

NDT_HD constexpr int pgo3_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

NDT_HD void pgo3_sincos(double a, double &s, double &c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, &s, &c);
#else
    s = sin(a);
    c = cos(a);
#endif
}

// ---- 3x3, column-major ----
// C = A B
NDT_HD void pgo3_mm(const double *A, const double *B, double *C)
{
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) C[3 * c + r] = A[r] * B[3 * c] + A[3 + r] * B[3 * c + 1] + A[6 + r] * B[3 * c + 2];
}
// C = A^T B
NDT_HD void pgo3_mtm(const double *A, const double *B, double *C)
{
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) C[3 * c + r] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
// C = A B^T
NDT_HD void pgo3_mmt(const double *A, const double *B, double *C)
{
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) C[3 * c + r] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
// y = A x,  y = A^T x
NDT_HD void pgo3_mv(const double *A, const double *x, double *y)
{
    for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}
NDT_HD void pgo3_mtv(const double *A, const double *x, double *y)
{
    for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
// y = a x b
NDT_HD void pgo3_cross(const double *a, const double *b, double *y)
{
    y[0] = a[1] * b[2] - a[2] * b[1];
    y[1] = a[2] * b[0] - a[0] * b[2];
    y[2] = a[0] * b[1] - a[1] * b[0];
}
// M = I + a [p]x + b [p]x^2
NDT_HD void pgo3_rodrigues(const double *p, double a, double b, double *M)
{
    const double xx = p[0] * p[0], yy = p[1] * p[1], zz = p[2] * p[2];
    const double xy = p[0] * p[1], xz = p[0] * p[2], yz = p[1] * p[2];
    M[0] = 1.0 - b * (yy + zz); M[3] = b * xy - a * p[2];   M[6] = b * xz + a * p[1];
    M[1] = b * xy + a * p[2];   M[4] = 1.0 - b * (xx + zz); M[7] = b * yz - a * p[0];
    M[2] = b * xz - a * p[1];   M[5] = b * yz + a * p[0];   M[8] = 1.0 - b * (xx + yy);
}

// Exp of a rotation vector (Rodrigues)
NDT_HD void pgo3_exp(const double *phi, double *R)
{
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double a, b;
    if (t2 < 1e-8) {                              // (theta < 1e-4: the next terms are below 1e-18)
        a = 1.0 - t2 / 6.0;
        b = 0.5 - t2 / 24.0;
    } else {
        const double t = sqrt(t2);
        double s, c;
        pgo3_sincos(t, s, c);
        a = s / t;
        b = (1.0 - c) / t2;
    }
    pgo3_rodrigues(phi, a, b, R);
}

// Log of a rotation: v theta / |v| with v = (R32 - R23, R13 - R31, R21 - R12) / 2 and theta = atan2(|v|, (tr R - 1) / 2); v
// itself where |v| < NDT_PGO3_TINY and the trace is positive.  Where |v| < NDT_PGO3_TINY and the trace is negative the rotation
// is a half turn whose axis v no longer holds: returns false, phi = NaN.  sn = |v| and cs = (tr R - 1) / 2 are the sine and
// cosine of theta, which pgo3_jr_inv takes from here.  Accuracy: v carries the rounding of R's entries, about u = 2^-52, and the
// formula multiplies it by theta / |v| -- phi is good to some u theta / |v|, which is u up to a quarter turn and u / (pi - theta)
// towards a half turn (1e-9 at pi - 1e-7; tests/test_pgo_direct.py measures it).
NDT_HD bool pgo3_log(const double *R, double *phi, double &sn, double &cs)
{
    const double v[3] = {0.5 * (R[5] - R[7]), 0.5 * (R[6] - R[2]), 0.5 * (R[1] - R[3])};
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    sn = n;
    cs = c;
    if (n < NDT_PGO3_TINY) {
        if (c < 0.0) {
            phi[0] = phi[1] = phi[2] = NAN;
            return false;
        }
        phi[0] = v[0]; phi[1] = v[1]; phi[2] = v[2];
        return true;
    }
    const double k = atan2(n, c) / n;
    phi[0] = k * v[0]; phi[1] = k * v[1]; phi[2] = k * v[2];
    return true;
}

// Jr^-1(phi) = I + [phi]x / 2 + k [phi]x^2, k = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), with the sine and cosine
// of theta = |phi| that Log read off the matrix -- no trigonometric call.  (1 + cos) / sin is taken as sin / (1 - cos) where the
// cosine is negative: the same number, cot(theta / 2), without the cancellation in 1 + cos theta near a half turn.  The series
// 1 / 12 + theta^2 / 720 below theta = 0.01 (the next term, theta^4 / 30240, is then below 4e-13 of k).
NDT_HD void pgo3_jr_inv(const double *phi, double sn, double cs, double *J)
{
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double k;
    if (t2 < 1e-4) {
        k = 1.0 / 12.0 + t2 / 720.0;
    } else {
        const double cot_half = cs < 0.0 ? sn / (1.0 - cs) : (1.0 + cs) / sn;
        k = 1.0 / t2 - cot_half / (2.0 * sqrt(t2));
    }
    pgo3_rodrigues(phi, 0.5, k, J);
}

// T [+] d = (R Exp(phi), t + R rho), d = (rho, phi); no re-orthonormalisation.  Q may be P.
NDT_HD void pgo3_retract(const double *P, const double *d, double *Q)
{
    double X[9], RX[9], Rr[3];
    pgo3_exp(d + 3, X);
    pgo3_mm(P, X, RX);
    pgo3_mv(P, d, Rr);
    for (int k = 0; k < 3; k++) Q[9 + k] = P[9 + k] + Rr[k];
    for (int k = 0; k < 9; k++) Q[k] = RX[k];
}

// The factor's error e = (t_E, Log R_E), E = (T_ref^-1 T_mov) Z^-1, and (jac != NULL) its linearisation, each block stored as soon
// as it is known.  false at a half turn (e's rotation part is then NaN and jac is not complete).
NDT_HD bool pgo3_link_error(const double *Pi, const double *Pj, const double *Z, double *e6, double *jac)
{
    double RA[9], d[3], tA[3], tzi[3], Rt[3];
    pgo3_mtm(Pi, Pj, RA);                         // A = T_ref^-1 T_mov
    for (int k = 0; k < 3; k++) d[k] = Pj[9 + k] - Pi[9 + k];
    pgo3_mtv(Pi, d, tA);
    pgo3_mtv(Z, Z + 9, tzi);                      // Z^-1 = (R_z^T, -R_z^T t_z)
    for (int k = 0; k < 3; k++) tzi[k] = -tzi[k];
    pgo3_mv(RA, tzi, Rt);
    for (int k = 0; k < 3; k++) e6[k] = Rt[k] + tA[k];
    if (jac) {
        for (int k = 0; k < 3; k++) jac[k] = e6[k];
        for (int k = 0; k < 9; k++) jac[3 + k] = RA[k];
        for (int c = 0; c < 3; c++) {             // M_B's column c = -R_A (t_z' x e_c) = R_A (e_c x t_z')
            const double unit[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
            double x[3];
            pgo3_cross(unit, tzi, x);
            pgo3_mv(RA, x, jac + 12 + 3 * c);
        }
    }
    double RE[9], sn, cs;
    pgo3_mmt(RA, Z, RE);
    if (!pgo3_log(RE, e6 + 3, sn, cs)) return false;
    if (!jac) return true;
    double Ji[9], M[9];
    pgo3_jr_inv(e6 + 3, sn, cs, Ji);
    pgo3_mmt(Ji, RE, M);
    for (int k = 0; k < 9; k++) jac[21 + k] = -M[k];
    pgo3_mm(Ji, Z, jac + 30);                     // R_z'^T = R_z
    return true;
}

// u = J x for the side of the edge the node is on (0: ref, 1: mov)
NDT_HD void pgo3_j(int side, const double *jac, const double *x, double *u)
{
    if (side == 0) {
        double cx[3];
        pgo3_cross(jac, x + 3, cx);
        for (int k = 0; k < 3; k++) u[k] = cx[k] - x[k];
        pgo3_mv(jac + 21, x + 3, u + 3);
    } else {
        double a[3], b[3];
        pgo3_mv(jac + 3, x, a);
        pgo3_mv(jac + 12, x + 3, b);
        for (int k = 0; k < 3; k++) u[k] = a[k] + b[k];
        pgo3_mv(jac + 30, x + 3, u + 3);
    }
}

// g = J^T w
NDT_HD void pgo3_jt(int side, const double *jac, const double *w, double *g)
{
    if (side == 0) {
        double cx[3], b[3];
        pgo3_cross(jac, w, cx);                   // [t_E]x^T w_t = -t_E x w_t
        pgo3_mtv(jac + 21, w + 3, b);
        for (int k = 0; k < 3; k++) {
            g[k] = -w[k];
            g[3 + k] = b[k] - cx[k];
        }
    } else {
        double a[3], b[3];
        pgo3_mtv(jac + 3, w, g);
        pgo3_mtv(jac + 12, w, a);
        pgo3_mtv(jac + 30, w + 3, b);
        for (int k = 0; k < 3; k++) g[3 + k] = a[k] + b[k];
    }
}

// column q of J (q need not be a constant: no register array is indexed with it)
NDT_HD void pgo3_j_column(int side, const double *jac, int q, double *col)
{
    const bool rot = q >= 3;
    const int c = rot ? q - 3 : q;
    const double unit[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
    for (int k = 0; k < 6; k++) col[k] = 0.0;
    if (side == 0) {
        if (!rot) {
            for (int k = 0; k < 3; k++) col[k] = -unit[k];
        } else {
            pgo3_cross(jac, unit, col);           // [t_E]x's column c = t_E x e_c
            for (int k = 0; k < 3; k++) col[3 + k] = jac[21 + 3 * c + k];
        }
    } else {
        for (int k = 0; k < 3; k++) col[k] = jac[(rot ? 12 : 3) + 3 * c + k];
        if (rot)
            for (int k = 0; k < 3; k++) col[3 + k] = jac[30 + 3 * c + k];
    }
}

// y = W x, W symmetric as 21 numbers
NDT_HD void pgo3_symv(const double *W, const double *x, double *y)
{
    for (int i = 0; i < 6; i++) {
        double s = 0.0;
        for (int j = 0; j < 6; j++) s += W[pgo3_tri(i, j)] * x[j];
        y[i] = s;
    }
}

NDT_HD double pgo3_dot6(const double *a, const double *b)
{
    double s = 0.0;
    for (int k = 0; k < 6; k++) s += a[k] * b[k];
    return s;
}

// the symmetric part of a row-major 6x6, as 21 numbers
NDT_HD void pgo3_sym21(const double *W36, double *W21)
{
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) W21[pgo3_tri(i, j)] = i == j ? W36[7 * i] : 0.5 * (W36[6 * i + j] + W36[6 * j + i]);
}

// the poses of the ABI: a column-major 4x4 to twelve numbers and back
NDT_HD void pgo3_from_T16(const double *T16, double *P)
{
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) P[3 * c + r] = T16[4 * c + r];
    for (int r = 0; r < 3; r++) P[9 + r] = T16[12 + r];
}
NDT_HD void pgo3_to_T16(const double *P, double *T16)
{
    for (int c = 0; c < 4; c++) {
        for (int r = 0; r < 3; r++) T16[4 * c + r] = P[3 * c + r];
        T16[4 * c + 3] = c == 3 ? 1.0 : 0.0;
    }
}

// W = S^-1 for the symmetric part S of the row-major C36, by Cholesky: S = L L^T, Y = L^-1, W = Y^T Y (row-major, both
// triangles).  false where S is not positive definite (a pivot that is not > 0) or an entry of W is not finite.
NDT_HD bool ndt_pgo3_inv_sym6(const double *C36, double *W36)
{
#pragma clang fp contract(off)
    double L[6][6], Y[6][6];
    bool ok = true;
    for (int j = 0; j < 6; j++) {
        double d = C36[7 * j];
        for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k];
        ok = ok && (d > 0.0);
        const double l = ndt_pgo_sqrt(d > 0.0 ? d : 1.0);
        L[j][j] = l;
        for (int i = j + 1; i < 6; i++) {
            double s = 0.5 * (C36[6 * i + j] + C36[6 * j + i]);
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
            L[i][j] = s / l;
        }
    }
    for (int j = 0; j < 6; j++) {                 // column j of Y = L^-1: forward substitution on the unit vector
        Y[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < 6; i++) {
            double s = 0.0;
            for (int k = j; k < i; k++) s = s - L[i][k] * Y[k][j];
            Y[i][j] = s / L[i][i];
        }
    }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int k = i; k < 6; k++) s = s + Y[k][i] * Y[k][j];
            W36[6 * i + j] = W36[6 * j + i] = s;
            ok = ok && (s - s == 0.0);
        }
    return ok;
}

// A registered link as the factor takes it: Z16 = T16; W = the inverse of cov36's symmetric part (row-major 6x6, ordered
// x, y, z, rx, ry, rz).  W = 50 * I6 -- the covariance 0.02 * I6 -- where flags has any of NDTGPU_COV_SINGULAR / POSE_UNCHANGED /
// NOT_COMPUTED (ndt_feature_graph.cpp:300-310) and where the matrix does not invert (ndt_pgo3_inv_sym6; a 3-DoF registration's
// cov36 is singular and lands here).  cov36 == NULL: W = 100 * I6.
NDT_HD void ndt_pgo3_link_from_registration(const double *T16, const double *cov36, int flags, double *Z16, double *W36)
{
    for (int k = 0; k < 16; k++) Z16[k] = T16[k];
    const bool flagged = (flags & (NDTGPU_COV_SINGULAR | NDTGPU_COV_POSE_UNCHANGED | NDTGPU_COV_NOT_COMPUTED)) != 0;
    if (cov36 && !flagged && ndt_pgo3_inv_sym6(cov36, W36)) return;
    for (int k = 0; k < 36; k++) W36[k] = 0.0;
    for (int k = 0; k < 6; k++) W36[7 * k] = cov36 ? 50.0 : 100.0;
}

// ---- what the kernel does per link and per node ----

// one graph of a bank: its arrays and its part of the scratch
struct Pgo3Graph {
    unsigned N, E;
    double *pose;
    const double *origin;
    const int32_t *ref, *mov;
    const double *meas, *info;
    const uint32_t *adj_off, *adj;
    double *jac, *te;
    double *prev, *b, *x, *r, *z, *p, *ap, *chol;
};

// graph g of the bank, with n_nodes nodes and n_edges links
NDT_HD Pgo3Graph ndt_pgo3_graph(const NdtPgo3View &v, size_t g, unsigned n_nodes, unsigned n_edges)
{
    Pgo3Graph G;
    G.N = n_nodes;
    G.E = n_edges;
    G.pose = v.pose + g * 12 * v.max_nodes;
    G.origin = v.origin + g * 24;
    G.ref = v.ref + g * v.max_edges;
    G.mov = v.mov + g * v.max_edges;
    G.meas = v.meas + g * 12 * v.max_edges;
    G.info = v.info + g * 21 * v.max_edges;
    G.adj_off = v.adj_off + g * (v.max_nodes + 1);
    G.adj = v.adj + g * 2 * v.max_edges;
    G.jac = v.jac + g * NDT_PGO3_JAC * (v.max_edges + 1);
    G.te = v.te + g * 6 * (v.max_edges + 1);
    double *nb = v.node + g * NDT_PGO3_NODE_DOUBLES * v.max_nodes;
    G.prev = nb;
    G.b = nb + 12 * v.max_nodes;
    G.x = nb + 18 * v.max_nodes;
    G.r = nb + 24 * v.max_nodes;
    G.z = nb + 30 * v.max_nodes;
    G.p = nb + 36 * v.max_nodes;
    G.ap = nb + 42 * v.max_nodes;
    G.chol = nb + 48 * v.max_nodes;
    return G;
}

// Link e at the current poses -- e == G.E: the prior, a link from the origin to node 0 with Z = I -- : the linearisation into
// jac, W e into te; returns e^T W e, and sets `half` where the residual rotation is a half turn (the cost is then NaN).
NDT_D double pgo3_linearise_link(const Pgo3Graph &G, const NdtPgo3ParamsDev &prm, unsigned e, bool &half)
{
    const bool prior = e == G.E;
    const double *Pi = prior ? G.origin : G.pose + 12 * (size_t)G.ref[e], *Pj = prior ? G.pose : G.pose + 12 * (size_t)G.mov[e];
    const double *Z = prior ? G.origin + 12 : G.meas + 12 * (size_t)e, *W = prior ? prm.prior : G.info + 21 * (size_t)e;
    double err[6], w[6];
    if (!pgo3_link_error(Pi, Pj, Z, err, G.jac + NDT_PGO3_JAC * (size_t)e)) half = true;
    pgo3_symv(W, err, w);
    double *t = G.te + 6 * (size_t)e;
    for (int k = 0; k < 6; k++) t[k] = w[k];
    return pgo3_dot6(err, w);
}

// node i: b = -gradient and the Cholesky factor of the 6x6 diagonal block of J^T W J (15 entries below the diagonal, then the 6
// inverse diagonal entries; the identity where the block is not positive definite), over the node's incident edges in ascending
// order, the prior's behind them on node 0.  The block is summed where its factor will lie, in the node's scratch, a column at
// a time: this pass runs once per update, and its registers would otherwise set the kernel's.
NDT_D void pgo3_gather_node(const Pgo3Graph &G, const NdtPgo3ParamsDev &prm, unsigned i)
{
    double g[6] = {0, 0, 0, 0, 0, 0};
    double *D = G.chol + 21 * (size_t)i;
    for (int k = 0; k < 21; k++) D[k] = 0.0;
    const unsigned k0 = G.adj_off[i], k1 = G.adj_off[i + 1];
    for (unsigned k = k0; k < k1 + (i == 0 ? 1u : 0u); k++) {
        const bool prior = k == k1;
        const unsigned a = prior ? ((G.E << 1) | 1u) : G.adj[k], e = a >> 1;
        const int side = (int)(a & 1u);
        const double *jac = G.jac + NDT_PGO3_JAC * (size_t)e, *W = prior ? prm.prior : G.info + 21 * (size_t)e;
        double h[6];
        pgo3_jt(side, jac, G.te + 6 * (size_t)e, h);
        for (int d = 0; d < 6; d++) g[d] += h[d];
#pragma unroll 1
        for (int q = 0; q < 6; q++) {             // column q of J^T W J, its rows q .. 5
            double col[6], u[6], m[6];
            pgo3_j_column(side, jac, q, col);
            pgo3_symv(W, col, u);
            pgo3_jt(side, jac, u, m);
            for (int r = 0; r < 6; r++)
                if (r >= q) D[r * (r + 1) / 2 + q] += m[r];
        }
    }
    double A[6][6], l[6][6], dinv[6];
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) A[r][c] = D[pgo3_tri(r, c)];
    const bool pd = chol_is_pd<6>(A, l, dinv);
    double *b = G.b + 6 * (size_t)i;
    for (int d = 0; d < 6; d++) b[d] = -g[d];
    int o = 0;
    for (int r = 1; r < 6; r++)
        for (int c = 0; c < r; c++) D[o++] = pd ? l[r][c] : 0.0;
    for (int d = 0; d < 6; d++) D[15 + d] = pd ? dinv[d] : 1.0;
}

// z = M^-1 r with node i's factor
NDT_D void pgo3_precondition(const Pgo3Graph &G, unsigned i, const double (&r)[6], double (&z)[6])
{
    const double *ch = G.chol + 21 * (size_t)i;
    double l[6][6], dinv[6];
    int o = 0;
    for (int a = 1; a < 6; a++)
        for (int c = 0; c < a; c++) l[a][c] = ch[o++];
    for (int d = 0; d < 6; d++) dinv[d] = ch[15 + d];
    chol_solve<6>(l, dinv, r, z);
}

// link e of the matrix-vector product: t_e = W (J_ref p_ref + J_mov p_mov) from the two end nodes' search directions
NDT_D void pgo3_link_product(const Pgo3Graph &G, unsigned e)
{
    const double *jac = G.jac + NDT_PGO3_JAC * (size_t)e;
    double u[6], v[6], t[6];
    pgo3_j(0, jac, G.p + 6 * (size_t)G.ref[e], u);
    pgo3_j(1, jac, G.p + 6 * (size_t)G.mov[e], v);
    for (int k = 0; k < 6; k++) u[k] += v[k];
    pgo3_symv(G.info + 21 * (size_t)e, u, t);
    double *te = G.te + 6 * (size_t)e;
    for (int k = 0; k < 6; k++) te[k] = t[k];
}

// node i of the matrix-vector product: (A p)_i = sum J^T t_e over the node's incident edges in ascending order, then the prior's
// J^T W J p on node 0; p is the node's search direction
NDT_D void pgo3_node_product(const Pgo3Graph &G, const NdtPgo3ParamsDev &prm, unsigned i, const double (&p)[6], double (&ap)[6])
{
    for (int d = 0; d < 6; d++) ap[d] = 0.0;
    for (unsigned q = G.adj_off[i]; q < G.adj_off[i + 1]; q++) {
        const unsigned a = G.adj[q], e = a >> 1;
        double h[6];
        pgo3_jt((int)(a & 1u), G.jac + NDT_PGO3_JAC * (size_t)e, G.te + 6 * (size_t)e, h);
        for (int d = 0; d < 6; d++) ap[d] += h[d];
    }
    if (i == 0) {
        const double *jac = G.jac + NDT_PGO3_JAC * (size_t)G.E;
        double u[6], w[6], h[6];
        pgo3_j(1, jac, p, u);
        pgo3_symv(prm.prior, u, w);
        pgo3_jt(1, jac, w, h);
        for (int d = 0; d < 6; d++) ap[d] += h[d];
    }
}

// host launchers (csrc/ndt_pgo3.hip)
// graphs [first, first + count) of the bank, one workgroup each
hipError_t ndt_pgo3_launch(const NdtPgo3View &v, size_t first, size_t count, const NdtPgo3ParamsDev &prm, hipStream_t st);
// meas / info of graph g from n_edges registered links in device memory
hipError_t ndt_pgo3_launch_links(const NdtPgo3View &v, size_t g, size_t n_edges, const double *T16_dev, const double *cov36_dev,
                                 const int32_t *cov_flags_dev, hipStream_t st);
