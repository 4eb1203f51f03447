// ndt_pairterm.h -- the D2D pair term of the matcher (csrc/ndt_match.hip): one (source cell, target cell) term of the score, its
// gradient and its Hessian, with the exponential and the reciprocal it is built on.  Device only; depends on ndt_common.h and
// ndt_math.h alone, so that tests/native/pairterm_checks.hip can run every function here by itself.
#pragma once
#include "ndt_common.h"
#include "ndt_math.h"

// A constant that is (re)made in scalar registers where it is used: the pair term is inlined into loops whose vector
// registers are all taken, and a loop-invariant constant hoisted into a vector register there is spilled to scratch
// memory and reloaded, with a full memory wait, at every use.
NDT_D double sgpr_const(double c)
{
    asm volatile("" : "+s"(c));
    return c;
}

// exp(x) for x <= 0 (the exponent of a Gaussian): 2^k exp(r), k = rint(x log2 e), r = x - k ln 2 in two parts
// (|r| <= 0.3466), exp(r) by its Taylor polynomial of degree 13 (truncation 4e-18), about one ulp like the library's;
// 0 below the double range, NaN for NaN.
NDT_D double exp_nonpos(double x)
{
    const double kf = rint(x * sgpr_const(1.4426950408889634));
    double r = fma(kf, sgpr_const(-6.93147180369123816490e-01), x);
    r = fma(kf, sgpr_const(-1.90821492927058770002e-10), r);
    double p = sgpr_const(1.60590438368216133e-10);               // 1/13!
    p = fma(p, r, sgpr_const(2.08767569878681002e-09));   // 1/12!
    p = fma(p, r, sgpr_const(2.50521083854417202e-08));   // 1/11!
    p = fma(p, r, sgpr_const(2.75573192239858883e-07));   // 1/10!
    p = fma(p, r, sgpr_const(2.75573192239858925e-06));   // 1/9!
    p = fma(p, r, sgpr_const(2.48015873015873016e-05));   // 1/8!
    p = fma(p, r, sgpr_const(1.98412698412698413e-04));   // 1/7!
    p = fma(p, r, sgpr_const(1.38888888888888894e-03));   // 1/6!
    p = fma(p, r, sgpr_const(8.33333333333333322e-03));   // 1/5!
    p = fma(p, r, sgpr_const(4.16666666666666644e-02));   // 1/4!
    p = fma(p, r, sgpr_const(1.66666666666666657e-01));   // 1/3!
    p = fma(p, r, sgpr_const(5.00000000000000000e-01));   // 1/2!
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    // (Estrin's scheme -- the same polynomial in 16 instructions of depth 5 -- was measured in round 5: 643 against 647 k
    //  registrations/s on the bench; the chain through the exponential is not what the gradient term waits for)
    const double v = ldexp(p, (int)fmax(kf, -1100.0));
    return x < -745.2 ? 0.0 : v;
}

// 1 / x for a finite x of ordinary magnitude (|det(CSum)| > 1e-12): hardware reciprocal + two Newton steps -- five
// instructions against the eleven of the IEEE division sequence, last-bit accurate away from the denormal range.
NDT_D double rcp_nr(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// One (source cell, target cell) term of NDTMatcherD2D::derivativesNDT + updateGradientHessianLocal
// (SURVEY.md App. A.4).  m, C: source mean / covariance already in the target frame.
// acc: [0] score, [1..6] gradient, [7..27] upper triangle of the Hessian (row-major).
// With x = m - mu, B = (C + Cj)^-1, q = (B x, (m - C B x) x B x) [so that x^T B (dx/dp_a) ... = 2 q_a], s = -d1 exp(-d2/2 x^T B x):
//   score += s,   gradient_a += 2 f q_a,   Hessian_ab += 2 f (h_ab - d2 q_a q_b),   f = -(d2 / 2) s,
// h = half the second-order bracket of the reference formula (the factor 2 of every term is applied once, in 2 f).
// a (e_K x v) and a . (e_K x v) without the component of e_K x v that is zero by construction: written with the vectors
// {0, -v.z, v.y} etc. every such product is an instruction (x * 0 cannot be folded: it is NaN for an infinite x), 42 of the
// 385 of a pair term with its Hessian.  The terms that are left come in the order they had: for finite operands the same
// bits (a leading +-0 does not change the sum that follows it).
template <int K>
NDT_D d3 mul_ecross(const sym3 &a, d3 v)
{
    if constexpr (K == 0) return {a.xy * (-v.z) + a.xz * v.y, a.yy * (-v.z) + a.yz * v.y, a.yz * (-v.z) + a.zz * v.y};
    else if constexpr (K == 1) return {a.xx * v.z + a.xz * (-v.x), a.xy * v.z + a.yz * (-v.x), a.xz * v.z + a.zz * (-v.x)};
    else return {a.xx * (-v.y) + a.xy * v.x, a.xy * (-v.y) + a.yy * v.x, a.xz * (-v.y) + a.yz * v.x};
}
template <int K>
NDT_D double dot_ecross(d3 a, d3 v)
{
    if constexpr (K == 0) return a.y * (-v.z) + a.z * v.y;
    else if constexpr (K == 1) return a.x * v.z + a.z * (-v.x);
    else return a.x * (-v.y) + a.y * v.x;
}

// PLANAR: the term of NDTMatcherD2D_2D ({x, y, yaw}, dof_mask 0x23): of the gradient the entries 0, 1, 5, of the Hessian the six
// entries among them -- the expressions of the full term for those entries (the same bits), nothing else (the other sums stay 0;
// newton_mask decouples their dofs anyway).  One rotational vector d_2 instead of three: ~135 instead of 276 instructions per
// 64 terms with the Hessian.  Only where nobody reads the inactive entries: not under the Tikhonov term (H^T H mixes them in).
template <bool WITH_H, bool PLANAR = false>
NDT_D void pair_term(d3 m, sym3 C, d3 mu, sym3 Cj, double lfd1, double lfd2, double *acc)
{
    const d3 x = m - mu;
    const sym3 S = C + Cj;
    // CSum.computeInverseAndDetWithCheck: adjugate / determinant, |det| > 1e-12
    sym3 A;
    A.xx = S.yy * S.zz - S.yz * S.yz;
    A.xy = S.yz * S.xz - S.xy * S.zz;
    A.xz = S.xy * S.yz - S.yy * S.xz;
    const double det = S.xx * A.xx + S.xy * A.xy + S.xz * A.xz;
    if (!(fabs(det) > NDT_DET_EPS)) return;
    A.yy = S.xx * S.zz - S.xz * S.xz;
    A.yz = S.xy * S.xz - S.xx * S.yz;
    A.zz = S.xx * S.yy - S.xy * S.xy;
    const double id = rcp_nr(det);
    const d3 xB = id * mul(A, x);                    // B x
    const double l = dot(x, xB);
    if (!(l * 0.0 == 0.0)) return;                   // if(l*0 != 0) continue;
#ifdef NDT_EXP_NO_EXP
    const double sh = -lfd1 * (1.0 - lfd2 * l * 0.5);
#else
    const double sh = -lfd1 * exp_nonpos(-lfd2 * l * 0.5);
#endif
    const double f2 = -lfd2 * sh;                    // 2 f
    const d3 w = mul(C, xB);
    if constexpr (PLANAR) {
        const d3 mw = m - w;
        const double q5 = mw.x * xB.y - mw.y * xB.x;         // (cross(m - w, B x)).z
        acc[0] += sh;
        acc[1] += f2 * xB.x; acc[2] += f2 * xB.y; acc[6] += f2 * q5;
        if (!WITH_H) return;
        const sym3 B = {A.xx * id, A.xy * id, A.xz * id, A.yy * id, A.yz * id, A.zz * id};
        const d3 c2 = mul_ecross<2>(C, xB);
        const d3 r2 = d3{-w.y - c2.x, w.x - c2.y, 0.0 - c2.z};
        const d3 d2 = d3{c2.x - mw.y, c2.y + mw.x, c2.z};
        const d3 Bd2 = mul(B, d2);
        const double xBH22 = -(xB.x * m.x + xB.y * m.y);
        const double qk0 = lfd2 * xB.x, qk1 = lfd2 * xB.y, qk5 = lfd2 * q5;
        const double h55 = dot(d2, Bd2) + xBH22 + dot_ecross<2>(r2, xB);
        acc[7] += f2 * (B.xx - qk0 * xB.x);      // (0, 0)
        acc[8] += f2 * (B.xy - qk0 * xB.y);      // (0, 1)
        acc[12] += f2 * (Bd2.x - qk0 * q5);      // (0, 5)
        acc[13] += f2 * (B.yy - qk1 * xB.y);     // (1, 1)
        acc[17] += f2 * (Bd2.y - qk1 * q5);      // (1, 5)
        acc[27] += f2 * (h55 - qk5 * q5);        // (5, 5)
        return;
    }
    const d3 qr = cross(m - w, xB);                  // x^T B j_k - x^T B Z_k B x / 2,  j_k = e_k x m
    const double q[6] = {xB.x, xB.y, xB.z, qr.x, qr.y, qr.z};
    acc[0] += sh;
#pragma unroll
    for (int a = 0; a < 6; a++) acc[1 + a] += f2 * q[a];
    if (!WITH_H) return;

    const sym3 B = {A.xx * id, A.xy * id, A.xz * id, A.yy * id, A.yz * id, A.zz * id};
    // j_k = e_k x m, p_k = e_k x (B x), e_k x w: never formed (see mul_ecross).
    // With r_k = Z_k (B x) = e_k x w - C (e_k x B x) and d_k = j_k - r_k, B symmetric:
    //   j_i^T B j_k - (B r_i)^T j_k - (B r_k)^T j_i + (B r_i)^T r_k = d_i^T B d_k      (rotation x rotation block)
    //   B j_k - B r_k = B d_k                                                          (translation x rotation block)
    // -- three matrix-vector products B d_k instead of six (B j_k, B r_k) and one dot per entry instead of four (round 5:
    // 345 -> 276 vector instructions per 64 terms; the sums associate differently: rounding-level changes of the Hessian).
    d3 r[3], d[3], Bd[3];
    {
        const d3 c0 = mul_ecross<0>(C, xB), c1 = mul_ecross<1>(C, xB), c2 = mul_ecross<2>(C, xB);
        const d3 mw = m - w;
        r[0] = d3{0.0 - c0.x, -w.z - c0.y, w.y - c0.z};
        r[1] = d3{w.z - c1.x, 0.0 - c1.y, -w.x - c1.z};
        r[2] = d3{-w.y - c2.x, w.x - c2.y, 0.0 - c2.z};
        d[0] = d3{c0.x, c0.y - mw.z, c0.z + mw.y};                // e_k x (m - w) + C (e_k x B x)
        d[1] = d3{c1.x + mw.z, c1.y, c1.z - mw.x};
        d[2] = d3{c2.x - mw.y, c2.y + mw.x, c2.z};
    }
#pragma unroll
    for (int k = 0; k < 3; k++) Bd[k] = mul(B, d[k]);
    const double Bm[3][3] = {{B.xx, B.xy, B.xz}, {B.xy, B.yy, B.yz}, {B.xz, B.yz, B.zz}};
    const double Bdv[3][3] = {{Bd[0].x, Bd[0].y, Bd[0].z}, {Bd[1].x, Bd[1].y, Bd[1].z}, {Bd[2].x, Bd[2].y, Bd[2].z}};
    // x^T B H_ik, H_ik = e_i x (e_k x m), i <= k
    const double xBH[3][3] = {{-(xB.y * m.y + xB.z * m.z), xB.y * m.x, xB.z * m.x},
                              {0.0, -(xB.x * m.x + xB.z * m.z), xB.z * m.y},
                              {0.0, 0.0, -(xB.x * m.x + xB.y * m.y)}};
    double qk[6];
#pragma unroll
    for (int a = 0; a < 6; a++) qk[a] = lfd2 * q[a];
    int o = 7;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = a; b < 6; b++) {
            double h;
            if (b < 3) {
                h = Bm[a][b];
            } else if (a < 3) {
                h = Bdv[b - 3][a];
            } else {
                const int i = a - 3, k = b - 3;
                // d_i^T B d_k + x^T B H_ik + p_i . r_k,  p_i = e_i x (B x)
                const double pr = i == 0 ? dot_ecross<0>(r[k], xB) : i == 1 ? dot_ecross<1>(r[k], xB) : dot_ecross<2>(r[k], xB);
                h = dot(d[i], Bd[k]) + xBH[i][k] + pr;
            }
            acc[o++] += f2 * (h - qk[a] * q[b]);
        }
    }
}
