"""References for the matcher's pair term (csrc/ndt_pairterm.h) that rest on a definition, not on a restatement of the kernel.

The term is the score of one (source cell, target cell) pair with its first and second derivatives at p = 0,

    s(p) = -d1 exp(-d2/2 x^T (R C R^T + Cj)^-1 x),   x = R m + t - mu,   t = p[0:3],   R = Rx(p3) Ry(p4) Rz(p5)

(the score tests/golden/make_golden.py defines).  A case is 20 doubles: m (3), C (xx xy xz yy yz zz), mu (3), Cj (6), d1, d2;
a result is 28 numbers in the layout of the kernel's accumulators: score, gradient (6), upper triangle of the Hessian (21).

  exact(case)         the derivatives of s by central differences in mpmath (400 bits, h = 1e-30): nobody's formula.
  formula(case, ctx)  the term as the papers write it -- j_k, Z_k, H_ik, ZH_ik and the six-term second-order bracket, nothing
                      regrouped -- generic over Python/NumPy doubles (DOUBLE) and mpmath (MP).  In mpmath it equals exact()
                      to 1e-25 (tests/test_pairterm_model.py) and is the reference from there on; in doubles its error
                      against that reference is the FLOOR of a family of cases: what any plain evaluation of the formula in
                      doubles loses there.  The bound of the device test is a multiple of it.
  exp_model(x)        exp_nonpos of the header, operation by operation, every one of them correctly rounded (the fma exact in
                      fractions.Fraction): the bits the device has to produce.
  families()          the seeded case families: generic, flat (map cells of a planar scan), skewed (ill-conditioned in a random
                      direction), far (from the origin), tails, degenerate.  All of them stay clear of the kernel's guard
                      |det(C + Cj)| > 1e-12, which skips a pair of small cells as the reference does.
"""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

MP_BITS = 400
FD_STEP_EXP = -30                    # h = 10^-30
PARTS = ((0, 1), (1, 7), (7, 28))    # score, gradient, Hessian in a 28-vector
DENORM = 2.0 ** -1074


def workprec():
    """Everything that touches mpmath numbers of this module runs under this precision (mpf operations round to the
    precision of the context they run in, not to that of their operands)."""
    return mpmath.workprec(MP_BITS)


class DOUBLE:
    num = staticmethod(float)
    exp = staticmethod(math.exp)


class MP:
    num = staticmethod(lambda v: mpmath.mpf(float(v)))        # (doubles convert exactly)
    exp = staticmethod(mpmath.exp)


# ---- 3x3 algebra on lists, for any number type ------------------------------------------------------------------------------
def _sym(ctx, s):
    xx, xy, xz, yy, yz, zz = [ctx.num(v) for v in s]
    return [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _add(*Ms):
    out = Ms[0]
    for M in Ms[1:]:
        out = [[out[i][j] + M[i][j] for j in range(3)] for i in range(3)]
    return out


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _inv(S):
    """adjugate / determinant"""
    c = [[S[(i + 1) % 3][(j + 1) % 3] * S[(i + 2) % 3][(j + 2) % 3] - S[(i + 1) % 3][(j + 2) % 3] * S[(i + 2) % 3][(j + 1) % 3]
          for j in range(3)] for i in range(3)]
    det = S[0][0] * c[0][0] + S[0][1] * c[0][1] + S[0][2] * c[0][2]
    return [[c[j][i] / det for j in range(3)] for i in range(3)]


def _ecross(ctx, k):
    """[e_k]x: the derivative of the rotation about axis k at angle 0"""
    z, o = ctx.num(0.0), ctx.num(1.0)
    return [[[z, z, z], [z, z, -o], [z, o, z]], [[z, z, o], [z, z, z], [-o, z, z]], [[z, -o, z], [o, z, z], [z, z, z]]][k]


# ---- the formula ------------------------------------------------------------------------------------------------------------
def formula(case, ctx, source=None):
    """score, gradient and Hessian of one pair at p = 0 as a list of 28 numbers of ctx.
    With l = x^T B x, B = (C + Cj)^-1:   ds/da = -d2/2 s l_a,   d2s/da db = -d2/2 s (l_ab - d2/2 l_a l_b),
      l_a  = 2 x^T B j_a - x^T B Z_a B x
      l_ab = 2 j_a^T B j_b - 2 x^T B Z_a B j_b - 2 x^T B Z_b B j_a + 2 x^T B H_ab + 2 x^T B Z_a B Z_b B x - x^T B ZH_ab B x
    j_a = dx/dp_a (e_a for the translations, e_k x m for the rotations), Z_a = d(R C R^T)/dp_a (rotations only),
    H_ab = d2x/dp_a dp_b and ZH_ab = d2(R C R^T)/dp_a dp_b (both rotations only; for i <= k the factor of axis i stands left
    of the factor of axis k in R = Rx Ry Rz, so d2R/dp_i dp_k = [e_i]x [e_k]x)."""
    m, C, j, Z, Hx, ZH = source_terms(case, ctx) if source is None else source
    mu = [ctx.num(v) for v in case[9:12]]
    Cj = _sym(ctx, case[12:18])
    d1, d2 = ctx.num(case[18]), ctx.num(case[19])
    zero, half, two = ctx.num(0.0), ctx.num(0.5), ctx.num(2.0)
    zero3 = [zero, zero, zero]
    # the pair
    x = [m[i] - mu[i] for i in range(3)]
    B = _inv(_add(C, Cj))
    Bx = _mv(B, x)
    l = _dot(x, Bx)
    s = -d1 * ctx.exp(-d2 * half * l)
    u = [zero3 if Z[a] is None else _mv(Z[a], Bx) for a in range(6)]          # Z_a B x
    Bj = [_mv(B, j[a]) for a in range(6)]
    Bu = [zero3 if Z[a] is None else _mv(B, u[a]) for a in range(6)]
    la = [two * _dot(Bx, j[a]) - _dot(Bx, u[a]) for a in range(6)]
    out = [s] + [-d2 * half * s * la[a] for a in range(6)]
    for a in range(6):
        for b in range(a, 6):
            lab = two * _dot(j[a], Bj[b]) - two * _dot(u[a], Bj[b]) - two * _dot(u[b], Bj[a]) + two * _dot(u[a], Bu[b])
            if Hx[a][b] is not None:
                lab = lab + two * _dot(Bx, Hx[a][b]) - _dot(Bx, _mv(ZH[a][b], Bx))
            out.append(-d2 * half * s * (lab - d2 * half * la[a] * la[b]))
    return out


def source_terms(case, ctx):
    """what depends on the source cell (case[0:9]) alone: m, C, j_a, Z_a, H_ab, ZH_ab.  formula() takes it as `source` where
    one source cell meets many target cells."""
    m = [ctx.num(v) for v in case[0:3]]
    C = _sym(ctx, case[3:9])
    E = [_ecross(ctx, k) for k in range(3)]
    j = [[ctx.num(1.0 if i == a else 0.0) for i in range(3)] for a in range(3)] + [_mv(E[k], m) for k in range(3)]
    Z = [None] * 3 + [_add(_mm(E[k], C), _mm(C, _tr(E[k]))) for k in range(3)]
    Hx = [[None] * 6 for _ in range(6)]
    ZH = [[None] * 6 for _ in range(6)]
    for i in range(3):
        for k in range(i, 3):
            EE = _mm(E[i], E[k])
            Hx[3 + i][3 + k] = _mv(EE, m)
            ZH[3 + i][3 + k] = _add(_mm(EE, C), _mm(_mm(E[i], C), _tr(E[k])), _mm(_mm(E[k], C), _tr(E[i])), _mm(C, _tr(EE)))
    return m, C, j, Z, Hx, ZH


# ---- the definition ---------------------------------------------------------------------------------------------------------
def _score(case_mp, p):
    m, C, mu, Cj, d1, d2 = case_mp
    s3, c3, s4, c4, s5, c5 = mpmath.sin(p[3]), mpmath.cos(p[3]), mpmath.sin(p[4]), mpmath.cos(p[4]), mpmath.sin(p[5]), mpmath.cos(p[5])
    Rx = [[1, 0, 0], [0, c3, -s3], [0, s3, c3]]
    Ry = [[c4, 0, s4], [0, 1, 0], [-s4, 0, c4]]
    Rz = [[c5, -s5, 0], [s5, c5, 0], [0, 0, 1]]
    R = _mm(_mm(Rx, Ry), Rz)
    Rm = _mv(R, m)
    x = [Rm[i] + p[i] - mu[i] for i in range(3)]
    B = _inv(_add(_mm(_mm(R, C), _tr(R)), Cj))
    return -d1 * mpmath.exp(-d2 / 2 * _dot(x, _mv(B, x)))


def exact(case):
    """score, gradient and Hessian as central differences of the score itself (call under workprec())."""
    assert mpmath.mp.prec >= 300
    h = mpmath.mpf(10) ** FD_STEP_EXP
    cm = ([MP.num(v) for v in case[0:3]], _sym(MP, case[3:9]), [MP.num(v) for v in case[9:12]], _sym(MP, case[12:18]),
          MP.num(case[18]), MP.num(case[19]))

    def at(*steps):
        p = [mpmath.mpf(0)] * 6
        for a, sg in steps:
            p[a] = p[a] + sg * h
        return _score(cm, p)
    s0 = at()
    sp = [at((a, +1)) for a in range(6)]
    sm = [at((a, -1)) for a in range(6)]
    out = [s0] + [(sp[a] - sm[a]) / (2 * h) for a in range(6)]
    for a in range(6):
        for b in range(a, 6):
            if a == b:
                out.append((sp[a] - 2 * s0 + sm[a]) / (h * h))
            else:
                out.append((at((a, 1), (b, 1)) - at((a, 1), (b, -1)) - at((a, -1), (b, 1)) + at((a, -1), (b, -1))) / (4 * h * h))
    return out


def part_errors(got, ref):
    """errors of the score, the gradient and the Hessian of `got` (28 numbers of any kind) against `ref` (28 mpf), each
    relative to the largest reference entry of that quantity; 0 where both are all zero, inf where only the reference is.
    Call under workprec()."""
    out = []
    for lo, hi in PARTS:
        diff = max(abs(MP.num(g) - r) if not isinstance(g, mpmath.mpf) else abs(g - r) for g, r in zip(got[lo:hi], ref[lo:hi]))
        scale = max(abs(r) for r in ref[lo:hi])
        out.append(0.0 if diff == 0 else math.inf if scale == 0 else float(diff / scale))
    return out


# ---- case families ----------------------------------------------------------------------------------------------------------
def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def _sym6(M):
    M = 0.5 * (M + M.T)
    return [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]


def _full(s6):
    return np.array([[s6[0], s6[1], s6[2]], [s6[1], s6[3], s6[4]], [s6[2], s6[4], s6[5]]])


def _generic_cov(rng, floor_lo, floor_hi):
    lam_max = (10.0 ** rng.uniform(-2.0, 0.0)) ** 2              # scales 1e-2 .. 1 m
    floor = 10.0 ** rng.uniform(floor_lo, floor_hi)              # the smallest eigenvalue sits on the finaliser's floor
    lam = lam_max * np.array([1.0, 10.0 ** rng.uniform(np.log10(floor), 0.0), floor])
    Q = _rotation(rng)
    return _sym6(Q @ np.diag(lam) @ Q.T)


def _exponent(C6, Cj6, x, d2):
    return 0.5 * d2 * float(x @ np.linalg.solve(_full(C6) + _full(Cj6), x))


def _case(C6, Cj6, mu, x, d1=1.0, d2=0.05):
    mu = np.asarray(mu, dtype=np.float64)
    return np.array(list(mu + x) + list(C6) + list(mu) + list(Cj6) + [d1, d2])


def _clamped(rng, C6, Cj6, x, d2, most):
    """x shortened, where it has to be, until the exponent d2 l / 2 is at most `most`: a term that is not a tail"""
    e = _exponent(C6, Cj6, x, d2)
    return x * np.sqrt(most / e) * rng.uniform(0.3, 1.0) if e > most else x


DET_MIN = 1e-11      # the families stay clear of the kernel's guard |det(C + Cj)| > 1e-12 (the guard has cases of its own)
COND_MAX = 1e3       # cond(C + Cj) of the families of randomly oriented cells; beyond it: the families `flat` and `skewed`


def _generic(rng, mu_radius=20.0, floor=(-6.0, -2.0), d1=1.0, d2=0.05):
    while True:
        C6, Cj6 = _generic_cov(rng, *floor), _generic_cov(rng, *floor)
        if kernel_det(C6, Cj6) > DET_MIN and np.linalg.cond(_full(C6) + _full(Cj6)) <= COND_MAX:
            break
    v = rng.normal(size=3)
    x = v / np.linalg.norm(v) * 10.0 ** rng.uniform(-3.0, np.log10(2.0))          # |x| 1e-3 .. 2 m
    return C6, Cj6, rng.uniform(-mu_radius, mu_radius, 3), _clamped(rng, C6, Cj6, x, d2, 20.0)


def _flat_cov(rng, yaw, thin):
    a2 = rng.uniform(0.15, 0.5) ** 2
    lam = a2 / np.array([1.0, 10.0 ** rng.uniform(1.0, 3.0), thin * rng.uniform(0.8, 1.25)])
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return _sym6(R @ np.diag(lam) @ R.T), lam


@functools.lru_cache(maxsize=None)
def families():
    """name -> [n, 20] array of cases, about 600 in all."""
    rng = np.random.default_rng(20240611)
    fam = {}
    fam["generic"] = np.array([_case(*_generic(rng)) for _ in range(200)])
    # flat-map cells: a wall seen in a planar scan -- long along the wall, thin across it and in z; the two cells nearly parallel
    rows = []
    while len(rows) < 150:
        yaw = rng.uniform(-np.pi, np.pi)
        thin = 10.0 ** rng.uniform(3.0, np.log10(5e6))               # how much thinner in z than along the wall
        C6, lam = _flat_cov(rng, yaw, thin)
        Cj6, _ = _flat_cov(rng, yaw + rng.normal(0.0, 0.02), thin)
        if not kernel_det(C6, Cj6) > DET_MIN:
            continue
        x = (rng.uniform(-0.5, 0.5) * np.array([np.cos(yaw), np.sin(yaw), 0.0])
             + rng.normal(0.0, 2.0 * np.sqrt(lam[1])) * np.array([-np.sin(yaw), np.cos(yaw), 0.0])
             + np.array([0.0, 0.0, rng.normal(0.0, np.sqrt(lam[2]))]))
        mu = np.array([rng.uniform(-50.0, 50.0), rng.uniform(-50.0, 50.0), rng.normal(0.0, 0.01)])
        rows.append(_case(C6, Cj6, mu, _clamped(rng, C6, Cj6, x, 0.05, 20.0)))
    fam["flat"] = np.array(rows)
    # two cells thin along nearly the same direction, anywhere in space: C + Cj is ill-conditioned and not aligned with any axis
    # (a plain evaluation in doubles loses far more here -- cancellation in the cofactors -- so the family has a floor of its own)
    rows = []
    while len(rows) < 60:
        lam = (10.0 ** rng.uniform(-1.0, 0.0)) ** 2 * np.array([1.0, 10.0 ** rng.uniform(-2.0, 0.0), 10.0 ** rng.uniform(-5.5, -3.0)])
        Q = _rotation(rng)
        w = rng.normal(0.0, 0.01, 3)
        dQ = np.eye(3) + np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        Q2, _ = np.linalg.qr(Q @ dQ)
        C6, Cj6 = _sym6(Q @ np.diag(lam) @ Q.T), _sym6(Q2 @ np.diag(lam * rng.uniform(0.5, 2.0, 3)) @ Q2.T)
        if not (kernel_det(C6, Cj6) > DET_MIN and np.linalg.cond(_full(C6) + _full(Cj6)) > COND_MAX):
            continue
        v = rng.normal(size=3)
        x = v / np.linalg.norm(v) * 10.0 ** rng.uniform(-3.0, np.log10(2.0))
        rows.append(_case(C6, Cj6, rng.uniform(-20.0, 20.0, 3), _clamped(rng, C6, Cj6, x, 0.05, 20.0)))
    fam["skewed"] = np.array(rows)
    # far from the origin: |mu| up to 5000 m
    rows = []
    for _ in range(100):
        C6, Cj6, _, x = _generic(rng, floor=(-4.0, -2.0))
        v = rng.normal(size=3)
        rows.append(_case(C6, Cj6, v / np.linalg.norm(v) * rng.uniform(100.0, 5000.0), x))
    fam["far"] = np.array(rows)
    # tails: x several sigma out, the exponent d2 l / 2 between 30 and 650 (the score stays a normal double)
    rows = []
    for _ in range(100):
        C6, Cj6, mu, x = _generic(rng, floor=(-3.0, -2.0))
        want = 10.0 ** rng.uniform(np.log10(30.0), np.log10(650.0))
        rows.append(_case(C6, Cj6, mu, x * np.sqrt(want / _exponent(C6, Cj6, x, 0.05))))
    fam["tails"] = np.array(rows)
    # degenerate but legal: x = 0 exactly, C = Cj, other d1 / d2 -- alone and together
    rows = []
    while len(rows) < 51:
        k = len(rows)
        d1, d2 = (rng.uniform(0.2, 5.0), 10.0 ** rng.uniform(-2.0, 0.0)) if k % 3 == 2 or k >= 42 else (1.0, 0.05)
        C6, Cj6, mu, x = _generic(rng, floor=(-4.0, -2.0), d1=d1, d2=d2)
        if k % 3 == 0 or k >= 45:
            x = np.zeros(3)
        if k % 3 == 1 or k >= 42:
            Cj6 = list(C6)
            if not kernel_det(C6, Cj6) > DET_MIN:
                continue
            x = _clamped(rng, C6, Cj6, x, d2, 20.0)
        rows.append(_case(C6, Cj6, mu, x, d1, d2))
    fam["degenerate"] = np.array(rows)
    return fam


@functools.lru_cache(maxsize=None)
def references():
    """name -> per case the 28 mpf of formula(case, MP): the reference of every comparison with doubles."""
    with workprec():
        return {name: [formula(c, MP) for c in cases] for name, cases in families().items()}


@functools.lru_cache(maxsize=None)
def _double_errors():
    refs = references()
    with workprec():
        return {name: [max(part_errors(formula(c, DOUBLE), r)) for c, r in zip(cases, refs[name])]
                for name, cases in families().items()}


def floors():
    """name -> the largest error (part_errors) of formula(case, DOUBLE) over the family's cases and the three quantities."""
    return {name: max(e) for name, e in _double_errors().items()}


def median_floors():
    """name -> the median over the family's cases of the same error: the floor is set by a family's worst-conditioned case,
    the median by its ordinary ones."""
    return {name: float(np.median(e)) for name, e in _double_errors().items()}


# ---- the exponential --------------------------------------------------------------------------------------------------------
_LOG2E = 1.4426950408889634
_LN2_HI = 6.93147180369123816490e-01
_LN2_LO = 1.90821492927058770002e-10
_TAYLOR = [1.60590438368216133e-10, 2.08767569878681002e-09, 2.50521083854417202e-08, 2.75573192239858883e-07,
           2.75573192239858925e-06, 2.48015873015873016e-05, 1.98412698412698413e-04, 1.38888888888888894e-03,
           8.33333333333333322e-03, 4.16666666666666644e-02, 1.66666666666666657e-01, 5.00000000000000000e-01, 1.0, 1.0]


def _fma(a, b, c):
    """a * b + c rounded once (finite operands; int / int division in Python is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exp_model(x):
    """exp_nonpos(x) of csrc/ndt_pairterm.h for x <= 0, -inf or NaN: the same operations in the same order."""
    x = float(x)
    if math.isnan(x):
        return math.nan
    if x == -math.inf:
        return 0.0                                   # (the polynomial is NaN there; x < -745.2 selects the 0)
    kf = float(np.rint(np.float64(x) * np.float64(_LOG2E)))
    r = _fma(kf, -_LN2_HI, x)
    r = _fma(kf, -_LN2_LO, r)
    p = _TAYLOR[0]
    for c in _TAYLOR[1:]:
        p = _fma(p, r, c)
    v = math.ldexp(p, int(max(kf, -1100.0)))
    return 0.0 if x < -745.2 else v


def exp_ulp_error(got, x):
    """|got - exp(x)| in units of the spacing of doubles at exp(x) (2^-1074 in the denormal range); call under workprec()."""
    want = mpmath.exp(mpmath.mpf(float(x)))
    _, e = mpmath.frexp(want)                        # want = f * 2^e, 0.5 <= f < 1
    return float(abs(mpmath.mpf(float(got)) - want) / mpmath.ldexp(mpmath.mpf(1), max(int(e) - 53, -1074)))


EXP_SPECIALS = ((-0.0, 1.0), (-745.2, 0.0), (-745.3, 0.0), (-math.inf, 0.0), (math.nan, math.nan))


@functools.lru_cache(maxsize=None)
def exp_points():
    """the finite points the exponential is checked at (the specials apart): (main range, denormal range)."""
    rng = np.random.default_rng(77)
    ln2 = mpmath.ln2
    edges = []
    with workprec():
        for half in range(0, 2 * 1022):              # k ln 2 and (k +- 1/2) ln 2, k < 1022: the point and its two neighbours
            e = -float(half * ln2 / 2)
            edges += [np.nextafter(e, 0.0), e, np.nextafter(e, -np.inf)]
    main = np.concatenate([rng.uniform(-708.0, 0.0, 6000), -10.0 ** rng.uniform(-18.0, 0.0, 2000), np.array(edges)])
    return main, rng.uniform(-745.2, -708.4, 3000)


# ---- the reciprocal ---------------------------------------------------------------------------------------------------------
def rcp_exact(x):
    """1 / x correctly rounded"""
    f = Fraction(float(x))
    return float(Fraction(f.denominator, f.numerator))


def kernel_det(C6, Cj6):
    """det(C + Cj) by the kernel's own expression, in doubles without contraction"""
    S = [np.float64(a) + np.float64(b) for a, b in zip(C6, Cj6)]
    xx, xy, xz, yy, yz, zz = S
    Axx = yy * zz - yz * yz
    Axy = yz * xz - xy * zz
    Axz = xy * yz - yy * xz
    return float(xx * Axx + xy * Axy + xz * Axz)
