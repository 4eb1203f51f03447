"""csrc/ndt_pgo3.h and csrc/ndt_pgo.h checked directly, as host code and on the device: the small functions under both pose-graph
optimisers and their chip-wide forms.

tests/native/pgo_checks.hip includes the SE(3) header alone and runs ONE function per case, in a loop on the host or from a
one-thread-per-case kernel on the device; the per-link and per-node bodies (device functions) run on a whole 8-node graph in one
workgroup.  Every check below is written once, as a function of a run(mode, table) callable, and used twice: unmarked with the host
target, under @pytest.mark.gpu with the device target (one GPU process per test).  The references are the mathematical functions
the headers document, evaluated on the exact double inputs -- mpmath at 400 bits for anything with a transcendental,
fractions.Fraction for pure products and sums -- and take no branch and no series: R^-1 is R^T, Log R is v atan2(|v|, c) / |v|,
Jr^-1 has k = 1 / theta^2 - cot(theta / 2) / (2 theta).  tests/pgo3_model.py and tests/pgo_model.py give fixtures and the bit-for-bit
restatements only.

Below u = 2^-52; S is the sum of the magnitudes of the exact terms of the output in question; scale = max(1, |t|_inf of the poses
involved); amp = theta / |v| (1 where |v| < 1e-8), the factor by which Log's v-formula amplifies rounding.  No bound was set from the
code under test: each is a forward bound of the short chains involved, or the project's 64 cond_2 u (tests/test_solver_direct.py).

Measured maxima, each in the unit of its bound.  The `device` column was measured on an MI355X, the `host` column on the x86 build
of the same source; the graph checks have no host target.
                                                                bound    host     device
  exp         entries / u                                         8      1.225    2.830
  retract     rotation / u                                       16      1.562    2.082
  retract     translation / (u max(1, |t|, |rho|))               16      0.722    0.525
  link_error  t_E / (u scale)                                    16      1.957    1.799
  link_error  phi / (u amp)                                      16      0.726    0.825
  link_error  R_A / u                                            16      0.810    0.596
  link_error  M_B / (u scale)                                    16      1.782    1.196
  link_error  N_C, N_D / (u amp max(1, theta)^2)                 16      2.460    2.681
  log         Log R against mpmath's of the same matrix / (u amp) 16     0.592    0.981
  log         Log(round(Exp w)) - w / (u amp)                    16      0.665    0.958
  jop         j, jt, symv / (u S)                                 8      0.862, 1.147, 0.868    0.812, 1.147, 0.906
  wrap        |r - (t + 2 pi_d k)| / (u max(|t|, pi))             1      0.474    0.474 (0.000 before the fix below)
  graph3      t_E, R_A, M_B, N_C / N_D in the units above        16       -       1.213, 0.443, 1.221, 3.139
  graph3      te = W e and e^T W e / their carried bounds         1       -       0.054, 0.035
  graph3      b / (u S)                                          32       -       0.717
  graph3      |L L^T - D| / (32 u S + 8 u |L||L^T|)               1       -       0.037
  graph3      precondition / (cond_2 u)                          64       -       0.080
  graph3      ap / (u S)                                         32       -       0.896
  graph2      c, s / u                                            4       -       0.251
  graph2      lx, ly / (u max(1, |dx|, |dy|))                     8       -       0.547
  graph2      te and cost / their carried bounds                  1       -       0.029, 0.023
  graph2      the prior's cost, b, ap / (u S)                    32       -       0.378, 1.050, 0.934
  graph2      dinv / (cond_2 u)                                  64       -       0.355
The carried bounds: e is not returned by the link bodies, so te = W e is held to sum_j |W_ij| (bound of e_j) plus the rounding of the
product itself (8 u S for SE(3), 32 u S for SE(2)), and e^T W e to the same carried one step further.
Exact (bit or numerical equality, no unit): exp(0), retract(P, 0), j_column, sym21, the T16 round trip, pgo3_tri; inv_sym6, inv_sym3,
acos and both link conversions on the device against the host and the Python restatements; wrap on the device against the host.

Log's accuracy near a half turn: the round trip Log(round(Exp w)) loses 1.1e-13 at pi - 1e-3, 1.3e-11 at pi - 1e-5 and 1.1e-9 at
pi - 1e-7 (host and device alike), about 1.5 u / (pi - theta): the v-formula's amplification u theta / |v|, well within 16 u amp.  It
is a property of the formula and is left as it is; the comment above pgo3_log now states it.

Found by wrap on the device (it passed on the host): ndt_pgo_wrap's t + two_pi * floor(...) was one fma on the device and a rounded
product and a sum on the host, so the two disagreed in the last place for angles outside (-pi, pi] -- the device and the host (and
tests/pgo_model.py's wrap) did not compute the same function.  ndt_pgo_wrap is now compiled without contraction; the 917 values stay
as the regression.

The SE(2) conversion has no covariance list elsewhere in the suite to share (tests/test_pgo_model.py::test_link_conversion_restatement
holds the model's conversion to a handful of hand-made cases); _cov2_list below is built like the SE(3) test's.
"""
import functools
import math
import os
import subprocess
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

import pgo3_model as M
import pgo_model as M2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pgo_checks.hip")
U = 2.0 ** -52
TINY = 1e-8
MP = mpmath.mp.clone()
MP.prec = 400
WIDTH_IN = {"exp": 3, "retract": 18, "log": 9, "linkerr": 36, "jop": 69, "sym21": 36, "tri": 2, "t16": 16, "invsym6": 36, "link3": 54,
            "wrap": 1, "acos": 1, "invsym3": 6, "link2": 54, "graph3": 1, "graph2": 1}
GRAPH_MODES = ("graph3", "graph2")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = str(tmp_path_factory.mktemp("pgo") / "pgo_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", SRC, "-o", out])
    return out


def _runner(exe, target):
    cmd = [exe] if target == "host" else ["timeout", "-k", "10", "60", exe]

    def run(mode, table):
        table = np.ascontiguousarray(table, dtype=np.float64)
        if mode in GRAPH_MODES:
            assert table.ndim == 1
        else:
            assert table.ndim == 2 and table.shape[1] == WIDTH_IN[mode]
        n = table.shape[0]
        out = subprocess.run(cmd + [mode, target], input=np.uint32(n).tobytes() + table.tobytes(), capture_output=True)
        assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace"))
        res = np.frombuffer(out.stdout, dtype=np.float64)
        return res if mode in GRAPH_MODES else res.reshape(n, -1)
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """the same bits, a NaN standing for any NaN (an invalid operation's NaN has the sign bit set on x86 and clear on the device)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


# ---- mpmath, 3x3 as lists of rows ------------------------------------------------------------------------------------------------
def _mpf(x):
    return MP.mpf(float(x))


def _eye():
    return [[MP.mpf(int(r == c)) for c in range(3)] for r in range(3)]


def _mm(A, B):
    return [[sum(A[r][k] * B[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def _tr(A):
    return [[A[c][r] for c in range(3)] for r in range(3)]


def _mv(A, x):
    return [sum(A[r][k] * x[k] for k in range(3)) for r in range(3)]


def _hat(v):
    return [[0 * v[0], -v[2], v[1]], [v[2], 0 * v[0], -v[0]], [-v[1], v[0], 0 * v[0]]]


def _rodrigues(p, a, b):
    K = _hat(p)
    K2 = _mm(K, K)
    I = _eye()
    return [[I[r][c] + a * K[r][c] + b * K2[r][c] for c in range(3)] for r in range(3)]


def _exp_mp(phi):
    p = [_mpf(v) for v in phi]
    t = MP.sqrt(sum(v * v for v in p))
    if t == 0:
        return _eye()
    return _rodrigues(p, MP.sin(t) / t, (1 - MP.cos(t)) / (t * t))


def _log_parts(R):
    """v, |v|, c, theta of a 3x3 (rows of mpf): what Log reads off the matrix"""
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    n = MP.sqrt(sum(x * x for x in v))
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    return v, n, c, MP.atan2(n, c)


def _pose12(T):
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[:3, :3].T.reshape(9), T[:3, 3]])


def _mp_pose(P):
    return [[_mpf(P[3 * c + r]) for c in range(3)] for r in range(3)], [_mpf(P[9 + r]) for r in range(3)]


def _cm(A):
    """a 3x3 (rows) column-major, as the headers store it"""
    return [A[r][c] for c in range(3) for r in range(3)]


def _units(got, ref, unit):
    """max |got - ref| / unit with got doubles and ref mpf.  A value that is not finite is refused here: max() would drop a NaN, and
    an output nobody stored (the harness prefills with NaN) or a NaN from a device function would pass as an error of 0."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(ref),) and np.all(np.isfinite(got)), got
    return float(max(abs(_mpf(g) - r) for g, r in zip(got, ref)) / unit) if len(ref) else 0.0


def _axis(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


# ---- 1: exp, retract --------------------------------------------------------------------------------------------------------------
EXP_THETAS = [0.0, 1e-300, 1e-12, 9.999e-5, 1.0001e-4, 1e-3, 0.3, 1.5, math.pi - 1e-6, math.pi]


@functools.lru_cache(maxsize=None)
def _exp_cases():
    rng = np.random.default_rng(31)
    rows = np.array([_axis(rng) * t for t in EXP_THETAS for _ in range(8)])
    return rows, [_cm(_exp_mp(r)) for r in rows]


def check_exp(run, label):
    rows, ref = _exp_cases()
    t2 = np.sum(rows * rows, -1)
    assert np.any((t2 < 1e-8) & (t2 > 9.99e-9)) and np.any((t2 >= 1e-8) & (t2 < 1.001e-8))       # both sides of the series' threshold
    out = run("exp", np.concatenate([rows, np.zeros((1, 3))]))
    assert np.array_equal(out[-1], np.eye(3).reshape(9))
    for k in range(8):                                                     # theta = 0 in every "direction" is the identity too
        assert np.array_equal(out[k], np.eye(3).reshape(9))
    worst = max(_units(o, r, U) for o, r in zip(out, ref))
    print("exp on %s: worst entry error %.3f u (bound 8)" % (label, worst))
    assert worst <= 8.0


def test_exp_host(exe):
    check_exp(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_exp_gpu(exe):
    check_exp(_runner(exe, "gpu"), "device")


@functools.lru_cache(maxsize=None)
def _retract_cases():
    rng = np.random.default_rng(32)
    rows, ref = [], []
    for t in EXP_THETAS:
        for _ in range(6):
            P = _pose12(M._rand_T(rng, 10.0))
            d = np.concatenate([rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-3, 1), _axis(rng) * t])
            R, tr = _mp_pose(P)
            Q = _mm(R, _exp_mp(d[3:]))
            Rr = _mv(R, [_mpf(v) for v in d[:3]])
            rows.append(np.concatenate([P, d]))
            ref.append((_cm(Q), [tr[k] + Rr[k] for k in range(3)], max(1.0, np.max(np.abs(P[9:])), np.max(np.abs(d[:3])))))
    return np.array(rows), ref


def check_retract(run, label):
    rows, ref = _retract_cases()
    still = rows[::7].copy()
    still[:, 12:] = 0.0                                                    # retract(P, 0) is P
    out = run("retract", np.concatenate([rows, still]))
    assert np.array_equal(_bits(out[len(rows):]), _bits(still[:, :12]))
    wr = max(_units(o[:9], r[0], U) for o, r in zip(out, ref))
    wt = max(_units(o[9:], r[1], U * r[2]) for o, r in zip(out, ref))
    print("retract on %s: worst rotation error %.3f u (bound 16), worst translation error %.3f u max(1, |t|, |rho|) (bound 16)" % (label, wr, wt))
    assert wr <= 16.0 and wt <= 16.0


def test_retract_host(exe):
    check_retract(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_retract_gpu(exe):
    check_retract(_runner(exe, "gpu"), "device")


# ---- 2: log, jr_inv, link_error ---------------------------------------------------------------------------------------------------
# (0.09 is not one of the angles the checks were specified with: it is here because a series region of Jr^-1 widened from 0.01 to 0.1
#  costs 3e-11 just below 0.1 and nothing measurable at 0.0101)
ANGLES = [0.0, 1e-9, 2e-8, 1e-4, 0.0099, 0.0101, 0.09, 0.3, 1.5, 2.5, 3.0, math.pi - 1e-3, math.pi - 1e-5, math.pi - 1e-7]


def _link_ref(Pi, Pj, Z):
    """the link error and the 39 Jacobian numbers of three poses (12 doubles each), in mpmath; the rotation part None at a half turn"""
    Ri, ti = _mp_pose(Pi)
    Rj, tj = _mp_pose(Pj)
    Rz, tz = _mp_pose(Z)
    RA = _mm(_tr(Ri), Rj)
    tA = _mv(_tr(Ri), [tj[k] - ti[k] for k in range(3)])
    tzi = [-x for x in _mv(_tr(Rz), tz)]
    tE = [a + b for a, b in zip(_mv(RA, tzi), tA)]
    MB = [[-x for x in row] for row in _mm(RA, _hat(tzi))]
    RE = _mm(RA, _tr(Rz))
    v, n, c, theta = _log_parts(RE)
    scale = max(1.0, float(np.max(np.abs(Pi[9:]))), float(np.max(np.abs(Pj[9:]))), float(np.max(np.abs(Z[9:]))))
    r = dict(tE=tE, RA=_cm(RA), MB=_cm(MB), scale=scale, n=float(n), c=float(c), theta=float(theta), half=bool(n < TINY and c < 0))
    if r["half"]:
        return r
    if n == 0:
        phi, k = v, MP.mpf(1) / 12
    else:
        phi = [x * theta / n for x in v]
        k = 1 / theta ** 2 - MP.cot(theta / 2) / (2 * theta)
    Ji = _rodrigues(phi, MP.mpf(1) / 2, k)
    r.update(phi=phi, NC=_cm([[-x for x in row] for row in _mm(Ji, _tr(RE))]), ND=_cm(_mm(Ji, Rz)),
             amp=float(theta / n) if n >= TINY else 1.0)
    return r


def _link_units(o, r, worst):
    """one row of `linkerr` (ok, e, jac) against its reference: updates the five worst values"""
    e, jac = o[1:7], o[7:46]
    worst["tE"] = max(worst["tE"], _units(e[:3], r["tE"], U * r["scale"]), _units(jac[:3], r["tE"], U * r["scale"]))
    worst["RA"] = max(worst["RA"], _units(jac[3:12], r["RA"], U))
    worst["MB"] = max(worst["MB"], _units(jac[12:21], r["MB"], U * r["scale"]))
    if r["half"]:
        # false, the rotation part NaN, t_E / R_A / M_B complete (_units above took no NaN) and nothing stored behind them
        assert o[0] == 0.0 and np.all(np.isnan(e[3:])) and np.all(np.isnan(jac[21:]))
        return
    assert o[0] == 1.0
    worst["phi"] = max(worst["phi"], _units(e[3:], r["phi"], U * r["amp"]))
    a = U * r["amp"] * max(1.0, r["theta"]) ** 2
    worst["N"] = max(worst["N"], _units(jac[21:30], r["NC"], a), _units(jac[30:39], r["ND"], a))


@functools.lru_cache(maxsize=None)
def _link_cases():
    rng = np.random.default_rng(33)
    poses = [M.residual_fixture(rng, a, t_max=10.0) for a in ANGLES for _ in range(25)]
    poses.append(M.residual_fixture(rng, math.pi - 2e-8, t_max=10.0))      # not yet a half turn for Log
    poses.append(M.residual_fixture(rng, math.pi - 5e-9, t_max=10.0))      # a half turn
    Ti, Tj = M.euler_T(1, 2, 3, 0.1, 0.2, 0.3), M.euler_T(-1, 0.5, 2, -0.3, 0.1, 1.0)
    poses.append((Ti, Tj, M.inv_T(M.make_T(np.diag([-1.0, 1.0, -1.0]), [0.0, 0.2, 0.0])) @ (M.inv_T(Ti) @ Tj)))
    rows = np.array([np.concatenate([_pose12(T) for T in p]) for p in poses])
    return rows, [_link_ref(r[:12], r[12:24], r[24:]) for r in rows]


def check_linkerr(run, label):
    rows, ref = _link_cases()
    assert [r["half"] for r in ref[-3:]] == [False, True, True] and not any(r["half"] for r in ref[:-3])
    assert ref[-3]["n"] < 3e-8 and ref[-3]["c"] < 0
    th = np.array([r["theta"] for r in ref[:-3]])
    assert np.any((th < 0.01) & (th > 0.0098)) and np.any((th >= 0.01) & (th < 0.0102))          # both sides of Jr^-1's series threshold
    assert np.any([r["n"] < TINY for r in ref[:-3]]) and np.any([TINY <= r["n"] < 1e-7 for r in ref[:-3]])
    out = run("linkerr", rows)
    worst = dict(tE=0.0, phi=0.0, RA=0.0, MB=0.0, N=0.0)
    for o, r in zip(out, ref):
        _link_units(o, r, worst)
    print("link_error on %s, worst errors: t_E %.3f u scale, phi %.3f u amp, R_A %.3f u, M_B %.3f u scale, N_C / N_D %.3f u amp max(1, theta)^2 "
          "(bound 16 each; %d cases)" % (label, worst["tE"], worst["phi"], worst["RA"], worst["MB"], worst["N"], len(ref)))
    assert max(worst.values()) <= 16.0, worst


def test_linkerr_host(exe):
    check_linkerr(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_linkerr_gpu(exe):
    check_linkerr(_runner(exe, "gpu"), "device")


@functools.lru_cache(maxsize=None)
def _log_cases():
    rng = np.random.default_rng(34)
    w = np.array([_axis(rng) * a for a in ANGLES for _ in range(8)])
    rows = np.array([[float(x) for x in _cm(_exp_mp(v))] for v in w])      # round(Exp(w))
    ref = []
    for R in rows:
        v, n, c, theta = _log_parts([[_mpf(R[3 * cc + r]) for cc in range(3)] for r in range(3)])
        ref.append(([x * theta / n for x in v] if n != 0 else v, float(theta / n) if n >= TINY else 1.0, float(n), float(c)))
    return w, rows, ref


def check_log(run, label):
    w, rows, ref = _log_cases()
    half = np.array([-1.0, 0, 0, 0, 1.0, 0, 0, 0, -1.0])                   # a half turn about y
    out = run("log", np.concatenate([rows, half[None]]))
    assert out[-1, 0] == 0.0 and np.all(np.isnan(out[-1, 1:4])) and out[-1, 4] == 0.0 and out[-1, 5] == -1.0
    wm = wr = 0.0
    near = {}
    for k, (o, x, (phi, amp, n, c)) in enumerate(zip(out, w, ref)):
        assert o[0] == 1.0 and np.all(np.isfinite(o[1:6]))
        assert abs(o[4] - n) <= 4 * U * max(n, U) and abs(o[5] - c) <= 4 * U            # sn and cs as jr_inv takes them
        wm = max(wm, _units(o[1:4], phi, U * amp))
        err = float(np.max(np.abs(o[1:4] - x)))
        wr = max(wr, err / (U * amp))
        t = ANGLES[k // 8]
        if t > 3.1:
            near[t] = max(near.get(t, 0.0), err)
    print("log on %s: worst error against mpmath's Log of the same matrix %.3f u amp, of Log(round(Exp w)) against w %.3f u amp (bound 16 each)"
          % (label, wm, wr))
    print("log on %s: worst |Log(round(Exp w)) - w| by pi - theta: %s" % (label, ", ".join("%.0e: %.2e" % (math.pi - t, e) for t, e in sorted(near.items()))))
    assert wm <= 16.0 and wr <= 16.0


def test_log_host(exe):
    check_log(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_log_gpu(exe):
    check_log(_runner(exe, "gpu"), "device")


# ---- exact algebra ----------------------------------------------------------------------------------------------------------------
def _tri(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def _fr(a):
    return [F(float(v)) for v in a]


def _J3(jac, side):
    """J_ref (side 0) or J_mov (side 1) as a 6x6 of Fraction from the 39 doubles of a linearisation, by the header's layout comment"""
    j = _fr(jac)
    Z = F(0)
    blk = lambda o: [[j[o + 3 * c + r] for c in range(3)] for r in range(3)]
    J = [[Z] * 6 for _ in range(6)]
    if side == 0:
        t = j[:3]
        TL, TR, BR = [[-F(int(r == c)) for c in range(3)] for r in range(3)], [[Z, -t[2], t[1]], [t[2], Z, -t[0]], [-t[1], t[0], Z]], blk(21)
    else:
        TL, TR, BR = blk(3), blk(12), blk(30)
    for r in range(3):
        for c in range(3):
            J[r][c], J[r][3 + c], J[3 + r][3 + c] = TL[r][c], TR[r][c], BR[r][c]
    return J


def _W6x6(w21):
    w = _fr(w21)
    return [[w[_tri(i, j)] for j in range(6)] for i in range(6)]


def _T(A):
    return [list(r) for r in zip(*A)]


def _abs(A):
    return [[abs(v) for v in r] for r in A]


def _mul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _matvec(A, x):
    """(A x, the sum of the magnitudes of its terms)"""
    return [sum(a * b for a, b in zip(r, x)) for r in A], [sum(abs(a * b) for a, b in zip(r, x)) for r in A]


def _add(A, B):
    return [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def _fsolve(A, B):
    """A^-1 B by Gauss-Jordan elimination over the rationals (A, B: lists of rows of Fraction)"""
    n = len(A)
    Mx = [list(ra) + list(rb) for ra, rb in zip(A, B)]
    for c in range(n):
        p = next(r for r in range(c, n) if Mx[r][c] != 0)
        Mx[c], Mx[p] = Mx[p], Mx[c]
        d = Mx[c][c]
        Mx[c] = [v / d for v in Mx[c]]
        for r in range(n):
            if r != c and Mx[r][c] != 0:
                f = Mx[r][c]
                Mx[r] = [a - f * b for a, b in zip(Mx[r], Mx[c])]
    return [row[n:] for row in Mx]


def _funits(got, ref, S, scale=1.0):
    """max |got - ref| / (u S) entry by entry (got doubles; ref, S Fractions); an entry with S == 0 must be exact"""
    worst = 0.0
    for g, r, s in zip(got, ref, S):
        d = abs(F(float(g)) - r)
        if s == 0:
            assert d == 0, (g, r)
        else:
            worst = max(worst, float(d / s) / (U * scale))
    return worst


def _spd21(rng, scale):
    A = rng.normal(size=(6, 6))
    W = (A @ A.T + 0.5 * np.eye(6)) * scale
    return np.array([W[i, j] for i in range(6) for j in range(i + 1)])


# ---- 3: j, jt, j_column, symv, sym21, tri, T16 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jac_rows(exe):
    """linearisations as check 2 produces them (the host target's), one per residual angle and three more, with no NaN in them"""
    rows, ref = _link_cases()
    pick = [k for k in list(range(0, 25 * len(ANGLES), 25)) + [7, 185, 240] if not ref[k]["half"]]
    out = _runner(exe, "host")("linkerr", rows[pick])
    assert np.all(out[:, 0] == 1.0) and np.all(np.isfinite(out))
    return out[:, 7:46]


def check_jop(run, label, jac_rows):
    rng = np.random.default_rng(35)
    rows, want = [], []
    for jac in jac_rows:
        x = rng.normal(size=6) * 10.0 ** rng.uniform(-2, 2, size=6)
        W = _spd21(rng, 10.0 ** rng.uniform(-2, 4))
        J = [_J3(jac, 0), _J3(jac, 1)]
        for side in (0, 1):
            rows.append(np.concatenate([[0, side, 0], jac, x, W]))
            want.append(("j",) + _matvec(J[side], _fr(x)))
            rows.append(np.concatenate([[1, side, 0], jac, x, W]))
            want.append(("jt",) + _matvec(_T(J[side]), _fr(x)))
            for q in range(6):
                rows.append(np.concatenate([[2, side, q], jac, x, W]))
                want.append(("col", [J[side][r][q] for r in range(6)], None))
        rows.append(np.concatenate([[3, 0, 0], jac, x, W]))
        want.append(("symv",) + _matvec(_W6x6(W), _fr(x)))
    out = run("jop", np.array(rows))
    worst = dict(j=0.0, jt=0.0, symv=0.0)
    for o, (kind, ref, S) in zip(out, want):
        if kind == "col":
            assert all(F(float(g)) == r for g, r in zip(o, ref)), (o, ref)              # copies, negations, products with 0 or 1
        else:
            worst[kind] = max(worst[kind], _funits(o, ref, S))
    print("jop on %s, worst error / (u S): j %.3f  jt %.3f  symv %.3f (bound 8 each; %d cases)" % (label, worst["j"], worst["jt"], worst["symv"], len(want)))
    assert max(worst.values()) <= 8.0, worst


def test_jop_host(exe, jac_rows):
    check_jop(_runner(exe, "host"), "host", jac_rows)


@pytest.mark.gpu
def test_jop_gpu(exe, jac_rows):
    check_jop(_runner(exe, "gpu"), "device", jac_rows)


def check_sym21(run):
    rng = np.random.default_rng(36)
    # entries on a grid of 2^-20 below 2^10: every sum and half is a double, so the result is exact or wrong
    grid = np.round(rng.uniform(-1e3, 1e3, size=(20, 36)) * 2.0 ** 20) / 2.0 ** 20
    free = rng.normal(size=(20, 36)) * 10.0 ** rng.uniform(-3, 3, size=(20, 36))
    out = run("sym21", np.concatenate([grid, free]))
    for W, o in zip(grid, out):
        Wf = [[F(float(v)) for v in r] for r in W.reshape(6, 6)]
        for i in range(6):
            for j in range(i + 1):
                assert F(float(o[_tri(i, j)])) == (Wf[i][j] + Wf[j][i]) / 2
    for W, o in zip(free, out[20:]):                                       # (any doubles: the one rounding of the sum)
        S = 0.5 * (W.reshape(6, 6) + W.reshape(6, 6).T)
        assert np.array_equal(_bits(o), _bits([S[i, j] for i in range(6) for j in range(i + 1)]))


def test_sym21_host(exe):
    check_sym21(_runner(exe, "host"))


@pytest.mark.gpu
def test_sym21_gpu(exe):
    check_sym21(_runner(exe, "gpu"))


def check_tri(run):
    ij = np.array([[i, j] for i in range(6) for j in range(6)], dtype=np.float64)
    out = run("tri", ij)
    assert [int(v) for v in out[:, 0]] == [_tri(int(i), int(j)) for i, j in ij]
    assert sorted({int(v) for v in out[:, 0]}) == list(range(21))


def test_tri_host(exe):
    check_tri(_runner(exe, "host"))


@pytest.mark.gpu
def test_tri_gpu(exe):
    check_tri(_runner(exe, "gpu"))


def check_t16(run):
    rng = np.random.default_rng(37)
    T = rng.normal(size=(10, 16)) * 10.0 ** rng.uniform(-3, 3, size=(10, 16))            # (the last row is NOT 0 0 0 1 going in)
    out = run("t16", T)
    for t, o in zip(T, out):
        C = t.reshape(4, 4)                                                # C[c] = column c
        assert np.array_equal(_bits(o[:12]), _bits(np.concatenate([C[0, :3], C[1, :3], C[2, :3], C[3, :3]])))
        back = C.copy()
        back[:, 3] = 0.0, 0.0, 0.0, 1.0
        assert np.array_equal(_bits(o[12:]), _bits(back.reshape(16)))


def test_t16_host(exe):
    check_t16(_runner(exe, "host"))


@pytest.mark.gpu
def test_t16_gpu(exe):
    check_t16(_runner(exe, "gpu"))


# ---- 4: inv_sym6 and the SE(3) link conversion, bit for bit -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cov_list():
    """the covariance list of tests/test_pgo3_abi.py::test_link_from_registration_bit_for_bit: (cov or None, flags)"""
    rng = np.random.default_rng(23)
    M.residual_fixture(rng, 1.0)                                           # (that test draws its pose first)
    covs = []
    for k in range(40):                                                    # SPD, badly scaled, not quite symmetric
        A = rng.normal(size=(6, 6)) * np.array([1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3])[:, None]
        covs.append((A @ A.T + 1e-7 * np.eye(6) + 1e-9 * rng.normal(size=(6, 6)), 0))
    covs.append((None, 0))
    cov = np.diag([1e-4, 2e-4, 3e-4, 1e-5, 2e-5, 3e-5])
    covs += [(cov, f) for f in (M.COV_SINGULAR, M.COV_POSE_UNCHANGED, M.COV_NOT_COMPUTED, 7, 8)]
    planar = np.zeros((6, 6))
    planar[np.ix_([0, 1, 5], [0, 1, 5])] = np.diag([1e-4, 1e-4, 1e-5])
    nan = cov.copy()
    nan[2, 3] = np.nan
    covs += [(c, 0) for c in (np.zeros((6, 6)), np.diag([1, 1, -1, 1, 1, 1.0]), planar, nan, 1e-320 * np.eye(6))]
    return covs


def _conv_rows(T16s):
    covs = _cov_list()
    rows = np.zeros((len(covs), 54))
    for k, (cov, flags) in enumerate(covs):
        rows[k, :16] = T16s[k % len(T16s)]
        rows[k, 16:18] = cov is not None, flags
        if cov is not None:
            rows[k, 18:] = cov.reshape(36)
    return covs, rows


def check_invsym6(run, host_out=None):
    covs = [c for c, f in _cov_list() if c is not None and f == 0]
    out = run("invsym6", np.array([c.reshape(36) for c in covs]))
    n_ok = 0
    for c, o in zip(covs, out):
        W, ok = M.inv_sym6(c)
        assert bool(o[0]) == ok
        n_ok += ok
        if ok:
            assert np.array_equal(_bits(o[1:]), _bits(np.array(W).reshape(36)))
        else:
            assert _same(o[1:], np.array(W).reshape(36))
    assert n_ok == 40 and len(covs) == 45
    if host_out is not None:
        assert _same(out, host_out)
    return out


def test_invsym6_host(exe):
    check_invsym6(_runner(exe, "host"))


@pytest.mark.gpu
def test_invsym6_gpu(exe):
    check_invsym6(_runner(exe, "gpu"), check_invsym6(_runner(exe, "host")))


def check_link3(run, host_out=None):
    rng = np.random.default_rng(38)
    covs, rows = _conv_rows([M._rand_T(rng, 10.0).T.reshape(16) for _ in range(5)])
    out = run("link3", rows)
    for (cov, flags), r, o in zip(covs, rows, out):
        _, W = M.link_from_registration(r[:16].reshape(4, 4), cov, flags)
        assert np.array_equal(_bits(o[:16]), _bits(r[:16]))
        assert np.array_equal(_bits(o[16:]), _bits(np.asarray(W, dtype=np.float64).reshape(36))), (flags, cov)
    kinds = {tuple(np.diag(o[16:].reshape(6, 6))[:1]) for o in out[40:]}
    assert kinds >= {(100.0,), (50.0,)}
    if host_out is not None:
        assert np.array_equal(_bits(out), _bits(host_out))
    return out


def test_link3_host(exe):
    check_link3(_runner(exe, "host"))


@pytest.mark.gpu
def test_link3_gpu(exe):
    check_link3(_runner(exe, "gpu"), check_link3(_runner(exe, "host")))


# ---- 6: wrap ----------------------------------------------------------------------------------------------------------------------
PI_D, TWO_PI_D = 3.141592653589793, 6.283185307179586


@functools.lru_cache(maxsize=None)
def _wrap_inputs():
    rng = np.random.default_rng(39)
    t = [PI_D, -PI_D, 0.0, -0.0, 3 * PI_D, -3 * PI_D, 1e3, -1e3, 1.0, -2.5]
    for x in (PI_D, -PI_D):
        t += [np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]
    for k in range(1, 101):
        for s in (1.0, -1.0):
            x = s * TWO_PI_D * k
            t += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]
    t += list(rng.uniform(-1e3, 1e3, 200)) + list(rng.uniform(-4, 4, 100))
    return np.array(t + [np.nan, np.inf, -np.inf], dtype=np.float64)


def check_wrap(run, label, host_out=None):
    t = _wrap_inputs()
    out = run("wrap", t[:, None])[:, 0]
    assert np.all(np.isnan(out[-3:]))                                      # (the optimiser's NOT_FINITE exit rests on it)
    worst = 0.0
    n_in = 0
    for x, r in zip(t[:-3], out[:-3]):
        if -PI_D < x <= PI_D:
            assert _bits(r) == _bits(x), (x, r)                            # untouched, the sign of zero included
            n_in += 1
            continue
        assert -PI_D <= r <= PI_D, (x, r)
        k = round((F(float(r)) - F(float(x))) / F(TWO_PI_D))
        worst = max(worst, float(abs(F(float(r)) - (F(float(x)) + F(TWO_PI_D) * k))) / (U * max(abs(x), math.pi)))
    print("wrap on %s: worst |r - (t + 2 pi_d k)| = %.3f u max(|t|, pi) (bound 1; %d values, %d of them in (-pi_d, pi_d])" % (label, worst, len(t), n_in))
    assert worst <= 1.0 and n_in >= 50
    if host_out is not None:
        assert _same(out, host_out)
    return out


def test_wrap_host(exe):
    check_wrap(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_wrap_gpu(exe):
    check_wrap(_runner(exe, "gpu"), "device", check_wrap(_runner(exe, "host"), "host"))


# ---- 7: acos, inv_sym3 and the SE(2) link conversion, bit for bit -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _acos_inputs():
    rng = np.random.default_rng(40)
    x = list(np.linspace(-1.0, 1.0, 1801)) + list(rng.uniform(-1, 1, 150))
    for p in (0.5, -0.5, 2.0 ** -57, -2.0 ** -57, 1.0, -1.0, 0.0):
        x += [p, np.nextafter(p, np.inf), np.nextafter(p, -np.inf)]
    x += [-0.0, 1.5, -1.5, 2.0, -1e300, 1e-300, np.inf, -np.inf, np.nan]
    return np.array(x, dtype=np.float64)


def check_acos(run, host_out=None):
    x = _acos_inputs()
    assert 1900 <= len(x) <= 2100
    out = run("acos", x[:, None])[:, 0]
    want = np.array([M2.acos_fd(v) for v in x])
    assert np.isnan(out[-1]) and np.isnan(want[-1])
    assert np.array_equal(_bits(out[:-1]), _bits(want[:-1]))
    if host_out is not None:
        assert np.array_equal(_bits(out), _bits(host_out))                 # (the NaN is the argument itself on both)
    return out


def test_acos_host(exe):
    check_acos(_runner(exe, "host"))


@pytest.mark.gpu
def test_acos_gpu(exe):
    check_acos(_runner(exe, "gpu"), check_acos(_runner(exe, "host")))


@functools.lru_cache(maxsize=None)
def _cov2_list():
    """(cov or None, flags) for the SE(2) conversion, which reads rows / columns x, y, yaw: blocks of the registrar's kind (SPD, badly
    scaled, not quite symmetric), NULL, the flag values, and blocks that do not invert -- zero, indefinite, a non-positive first
    entry, singular, NaN, and one whose inverse overflows"""
    rng = np.random.default_rng(41)
    covs = []
    for k in range(40):
        A = rng.normal(size=(6, 6)) * np.array([1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 10.0 ** rng.uniform(-5, -2)])[:, None]
        covs.append((A @ A.T + 1e-9 * np.eye(6) + 1e-10 * rng.normal(size=(6, 6)), 0))
    covs.append((None, 0))
    cov = np.diag([1e-4, 2e-4, 3e-4, 1e-5, 2e-5, 3e-5])
    cov[0, 1] = cov[1, 0] = 4e-5
    covs += [(cov, f) for f in (M2.COV_SINGULAR, M2.COV_POSE_UNCHANGED, M2.COV_NOT_COMPUTED, 7, 8)]
    nan = cov.copy()
    nan[0, 5] = np.nan
    sing = cov.copy()
    sing[1, :], sing[:, 1] = 2.0 * sing[0, :], 2.0 * sing[:, 0]
    sing[1, 1] = 4.0 * sing[0, 0]
    covs += [(c, 0) for c in (np.zeros((6, 6)), np.diag([1, -1, 1, 1, 1, 1.0]), np.diag([-1, 1, 1, 1, 1, 1.0]), sing, nan, 1e-320 * np.eye(6),
                              np.diag([1, 1, 1, 1, 1, -1.0]))]
    return covs


def _cov2_rows():
    rng = np.random.default_rng(42)
    covs = _cov2_list()
    rows = np.zeros((len(covs), 54))
    for k, (cov, flags) in enumerate(covs):
        yaw = rng.uniform(-math.pi, math.pi)
        T = M.euler_T(rng.uniform(-10, 10), rng.uniform(-10, 10), 0.0, 0.0, 0.0, yaw)
        rows[k, :16] = T.T.reshape(16)
        rows[k, 16:18] = cov is not None, flags
        if cov is not None:
            rows[k, 18:] = cov.reshape(36)
    # the cosine a rounding outside [-1, 1], exactly +-1, and a sine that is zero or negative zero
    rows[0, 0], rows[1, 0], rows[2, 0], rows[3, 0] = np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 1.0, -1.0
    rows[2, 1], rows[3, 1] = 0.0, -0.0
    return covs, rows


def _sym3_args(C):
    C = [float(v) for v in np.asarray(C, dtype=np.float64).reshape(36)]
    return [C[0], 0.5 * (C[1] + C[6]), 0.5 * (C[5] + C[30]), C[7], 0.5 * (C[11] + C[31]), C[35]]


def check_invsym3(run, host_out=None):
    args = np.array([_sym3_args(c) for c, f in _cov2_list() if c is not None and f == 0])
    out = run("invsym3", args)
    n_ok = 0
    for a, o in zip(args, out):
        with np.errstate(all="ignore"):
            W6, ok = M2.inv_sym3(*[float(v) for v in a])
        assert bool(o[0]) == bool(ok), a
        n_ok += bool(ok)
        assert _same(o[1:], W6), (a, o[1:], W6)
    assert n_ok == 40 and len(args) == 47
    if host_out is not None:
        assert _same(out, host_out)
    return out


def test_invsym3_host(exe):
    check_invsym3(_runner(exe, "host"))


@pytest.mark.gpu
def test_invsym3_gpu(exe):
    check_invsym3(_runner(exe, "gpu"), check_invsym3(_runner(exe, "host")))


def check_link2(run, host_out=None):
    covs, rows = _cov2_rows()
    out = run("link2", rows)
    fallback = 0
    for (cov, flags), r, o in zip(covs, rows, out):
        with np.errstate(all="ignore"):
            z, W = M2.link_from_registration(r[:16], None if cov is None else cov.reshape(36), flags)
        assert np.array_equal(_bits(o[:3]), _bits(z)), (r[:2], o[:3], z)
        assert np.array_equal(_bits(o[3:]), _bits([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]])), (flags, cov)
        fallback += abs(o[3] - 50.0) < 1e-9
    assert fallback == 4 + 7                                               # the three flags and 7; the seven that do not invert
    if host_out is not None:
        assert np.array_equal(_bits(out), _bits(host_out))
    return out


def test_link2_host(exe):
    check_link2(_runner(exe, "host"))


@pytest.mark.gpu
def test_link2_gpu(exe):
    check_link2(_runner(exe, "gpu"), check_link2(_runner(exe, "host")))


# ---- the graph of checks 5 and 8 --------------------------------------------------------------------------------------------------
# 8 nodes, 14 links.  Node 0 carries the prior and is ref (links 0, 6) and mov (link 5); node 3 has six links of both sides; links 1
# and 10 are the same pair; node 6 is a leaf; node 7's only link (13) has zero information, so its block is not positive definite.
N_NODES, MAX_NODES, MAX_EDGES = 8, 11, 17
REF = [0, 1, 2, 3, 4, 5, 0, 3, 5, 3, 1, 2, 4, 3]
MOV = [1, 2, 3, 4, 5, 0, 3, 1, 3, 5, 2, 5, 6, 7]
ZERO_INFO_LINK, ZERO_INFO_NODE = 13, 7
N_EDGES = len(REF)


def _adjacency():
    """CSR by the header's description: per node its incident links as (edge << 1) | (1 where the node is the link's mov), ascending"""
    off, adj = [0], []
    for i in range(N_NODES):
        adj += sorted([(e << 1) | 0 for e in range(N_EDGES) if REF[e] == i] + [(e << 1) | 1 for e in range(N_EDGES) if MOV[e] == i])
        off.append(len(adj))
    assert off[-1] == 2 * N_EDGES and off[4] - off[3] >= 5 and off[7] - off[6] == 1 and off[8] - off[7] == 1
    return off, adj


def test_graph_tables_are_checked_before_any_launch(exe):
    """a malformed graph table is refused by the host side (exit 65) -- on a machine without a device too, where a table that passed
    would fail at the device count instead"""
    g = _graph3_case()
    good = g["table"]
    base = 4 + 12 * N_NODES + 24
    adj_off0 = base + 2 * N_EDGES + 12 * N_EDGES + 21 * N_EDGES + 21
    adj0 = adj_off0 + N_NODES + 1
    # (`gpu` is the only target the graph modes have; the table is refused before a device is looked for, and the time limit of
    #  every GPU process is kept all the same)
    cmd = ["timeout", "-k", "10", "60", exe]
    bad = {"N": (0, 0.0), "E": (1, 5000.0), "max_nodes": (2, N_NODES - 1.0), "max_edges": (3, N_EDGES - 1.0), "ref": (base + 2, float(N_NODES)),
           "ref negative": (base + 3, -1.0), "mov": (base + N_EDGES + 1, 8.5), "mov NaN": (base + N_EDGES, np.nan),
           "adj_off start": (adj_off0, 1.0), "adj_off order": (adj_off0 + 3, 1.0), "adj_off end": (adj_off0 + N_NODES, 2.0 * N_EDGES + 1),
           "adj range": (adj0 + 5, 2.0 * N_EDGES), "adj other node": (adj0, float((12 << 1) | 1))}
    for name, (k, v) in bad.items():
        t = good.copy()
        t[k] = v
        out = subprocess.run(cmd + ["graph3", "gpu"], input=np.uint32(len(t)).tobytes() + t.tobytes(), capture_output=True)
        assert out.returncode == 65 and b"nothing was launched" in out.stderr, (name, out.returncode, out.stderr)
    for t in (good[:-1], np.concatenate([good, [0.0]])):                   # the length does not fit the counts
        out = subprocess.run(cmd + ["graph3", "gpu"], input=np.uint32(len(t)).tobytes() + t.tobytes(), capture_output=True)
        assert out.returncode == 65, out.stderr
    t = _graph2_case()["table"].copy()
    t[4 + 3 * N_NODES + 3 + 1] = 99.0
    out = subprocess.run(cmd + ["graph2", "gpu"], input=np.uint32(len(t)).tobytes() + t.tobytes(), capture_output=True)
    assert out.returncode == 65 and b"nothing was launched" in out.stderr
    out = subprocess.run([exe, "graph3", "host"], input=np.uint32(len(good)).tobytes() + good.tobytes(), capture_output=True)
    assert out.returncode == 64 and b"no host target" in out.stderr


# ---- 5: the SE(3) bodies on a graph (device only) -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph3_case():
    rng = np.random.default_rng(43)
    T = [M._rand_T(rng, 10.0) for _ in range(N_NODES)]
    origin = M.retract(T[0], np.array([0.05, -0.1, 0.08, 0.2, -0.15, 0.1]))
    Z, info = [], []
    for e in range(N_EDGES):
        angle = 1e-9 if e in (4, 11) else rng.uniform(0.25, 0.35)
        E = M.make_T(M.exp_so3(_axis(rng) * angle), rng.uniform(-0.5, 0.5, size=3))
        Z.append(M.inv_T(E) @ (M.inv_T(T[REF[e]]) @ T[MOV[e]]))
        info.append(np.zeros(21) if e == ZERO_INFO_LINK else _spd21(rng, 10.0 ** rng.uniform(-2, 4)))
    Z[10], info[10] = Z[1].copy(), info[1] * 3.0                           # the duplicate pair: the same measurement, more weight
    prior = _spd21(rng, 40.0)
    pose = np.array([_pose12(t) for t in T])
    org = np.concatenate([_pose12(origin), _pose12(np.eye(4))])
    meas = np.array([_pose12(z) for z in Z])
    off, adj = _adjacency()
    r = rng.normal(size=(N_NODES, 6)) * 10.0 ** rng.uniform(-2, 2, size=(N_NODES, 6))
    p = rng.normal(size=(N_NODES, 6)) * 10.0 ** rng.uniform(-1, 1, size=(N_NODES, 6))
    table = np.concatenate([[N_NODES, N_EDGES, MAX_NODES, MAX_EDGES], pose.reshape(-1), org, REF, MOV, meas.reshape(-1), np.array(info).reshape(-1),
                            prior, off, adj, r.reshape(-1), p.reshape(-1)]).astype(np.float64)
    links = [(pose[REF[e]], pose[MOV[e]], meas[e], info[e]) for e in range(N_EDGES)] + [(org[:12], pose[0], org[12:], prior)]
    return dict(table=table, links=links, ref=[_link_ref(a, b, z) for a, b, z, _ in links], off=off, adj=adj, r=r, p=p, prior=prior, info=info)


def _split(out, widths):
    parts, o = [], 0
    for w in widths:
        parts.append(out[o:o + w])
        o += w
    assert o == len(out)
    return parts


def check_graph3(run, label):
    g = _graph3_case()
    N, E = N_NODES, N_EDGES
    out = run("graph3", g["table"])
    cost, half, jac, te, b, chol, z, te2, ap = _split(out, [E + 1, E + 1, 39 * (E + 1), 6 * (E + 1), 6 * N, 21 * N, 6 * N, 6 * E, 6 * N])
    jac, te, b, chol, z, ap = jac.reshape(E + 1, 39), te.reshape(E + 1, 6), b.reshape(N, 6), chol.reshape(N, 21), z.reshape(N, 6), ap.reshape(N, 6)
    assert np.all(half == 0.0) and np.all(np.isfinite(out))
    # jac, te = W e and e^T W e against mpmath (the prior's slot E included): the bounds of check 2 carried through W, plus 8 u S
    worst = dict(tE=0.0, phi=0.0, RA=0.0, MB=0.0, N=0.0)
    w_te = w_cost = 0.0
    small = 0
    for e, ((_, _, _, w21), r) in enumerate(zip(g["links"], g["ref"])):
        small += r["theta"] < 1e-8
        e_ref = r["tE"] + r["phi"]
        # (link_error's e is not returned: jac[0..3) is its t_E, and te carries all six components)
        _link_units(np.concatenate([[1.0], [float(x) for x in e_ref], jac[e]]), r, worst)
        be = [16 * U * r["scale"]] * 3 + [16 * U * r["amp"]] * 3
        W = [[_mpf(w21[_tri(i, j)]) for j in range(6)] for i in range(6)]
        te_ref = [sum(W[i][j] * e_ref[j] for j in range(6)) for i in range(6)]
        tb = [sum(abs(W[i][j]) * be[j] + 8 * U * abs(W[i][j] * e_ref[j]) for j in range(6)) for i in range(6)]
        for i in range(6):
            d = abs(_mpf(te[e][i]) - te_ref[i])
            assert (d == 0) if tb[i] == 0 else True
            w_te = max(w_te, float(d / tb[i]) if tb[i] != 0 else 0.0)
        c_ref = sum(a * t for a, t in zip(e_ref, te_ref))
        cb = sum(abs(e_ref[i]) * tb[i] + abs(te_ref[i]) * be[i] + 8 * U * abs(e_ref[i] * te_ref[i]) for i in range(6))
        d = abs(_mpf(cost[e]) - c_ref)
        w_cost = max(w_cost, float(d / cb) if cb != 0 else float(d))
    assert small == 2
    print("graph3 on %s, linearisation: t_E %.3f  R_A %.3f  M_B %.3f  N_C / N_D %.3f (bound 16, units of check 2); te %.3f and e^T W e %.3f of their bounds"
          % (label, worst["tE"], worst["RA"], worst["MB"], worst["N"], w_te, w_cost))
    assert max(worst.values()) <= 16.0 and w_te <= 1.0 and w_cost <= 1.0, (worst, w_te, w_cost)
    assert cost[ZERO_INFO_LINK] == 0.0 and np.all(te[ZERO_INFO_LINK] == 0.0)
    # everything else from the device's own jac and te, read as exact doubles
    J = [(_J3(jac[e], 0), _J3(jac[e], 1)) for e in range(E + 1)]
    W = [_W6x6(w) for w in g["info"]] + [_W6x6(g["prior"])]
    inc = [[(a >> 1, a & 1) for a in g["adj"][g["off"][i]:g["off"][i + 1]]] + ([(E, 1)] if i == 0 else []) for i in range(N)]   # the prior last
    P = [_fr(v) for v in g["p"]]
    w_b = w_llt = w_pre = w_ap = 0.0
    for i in range(N):
        grad, Sg = [F(0)] * 6, [F(0)] * 6
        D, SD = [[F(0)] * 6 for _ in range(6)], [[F(0)] * 6 for _ in range(6)]
        for e, s in inc[i]:
            v, sv = _matvec(_T(J[e][s]), _fr(te[e]))
            grad, Sg = [a + c for a, c in zip(grad, v)], [a + c for a, c in zip(Sg, sv)]
            D = _add(D, _mul(_mul(_T(J[e][s]), W[e]), J[e][s]))
            SD = _add(SD, _mul(_mul(_abs(_T(J[e][s])), _abs(W[e])), _abs(J[e][s])))
        if i == ZERO_INFO_NODE:
            assert np.all(b[i] == 0.0) and np.array_equal(chol[i], np.array([0.0] * 15 + [1.0] * 6))
            assert all(v == 0 for r in D for v in r)
            L = [[F(int(r == c)) for c in range(6)] for r in range(6)]
        else:
            w_b = max(w_b, _funits(b[i], [-v for v in grad], Sg))
            L = [[F(0)] * 6 for _ in range(6)]
            o = 0
            for r in range(1, 6):
                for c in range(r):
                    L[r][c] = F(float(chol[i][o]))
                    o += 1
            for d in range(6):
                assert chol[i][15 + d] > 0.0
                L[d][d] = 1 / F(float(chol[i][15 + d]))
        LLt, aLLt = _mul(L, _T(L)), _mul(_abs(L), _abs(_T(L)))
        for r in range(6):
            for c in range(r + 1):
                bound = 32 * F(U) * SD[r][c] + 8 * F(U) * aLLt[r][c]
                if i != ZERO_INFO_NODE:
                    w_llt = max(w_llt, float(abs(LLt[r][c] - D[r][c]) / bound))
        zref = [v[0] for v in _fsolve(LLt, [[F(float(v))] for v in g["r"][i]])]
        cond = float(np.linalg.cond(np.array([[float(v) for v in r] for r in LLt])))
        w_pre = max(w_pre, float(max(abs(F(float(a)) - c) for a, c in zip(z[i], zref)) / max(abs(c) for c in zref)) / (cond * U))
        if i == ZERO_INFO_NODE:
            assert np.array_equal(z[i], g["r"][i])
        # (A p)_i = sum J^T W (J_ref p_ref + J_mov p_mov) over the node's links, the prior's J^T W J p on node 0
        hp, Sh = [F(0)] * 6, [F(0)] * 6
        for e, s in inc[i]:
            ends = [(1, 0)] if e == E else [(0, REF[e]), (1, MOV[e])]
            for s2, node in ends:
                v, _ = _matvec(_mul(_mul(_T(J[e][s]), W[e]), J[e][s2]), P[node])
                _, sv = _matvec(_mul(_mul(_abs(_T(J[e][s])), _abs(W[e])), _abs(J[e][s2])), [abs(x) for x in P[node]])
                hp, Sh = [a + c for a, c in zip(hp, v)], [a + c for a, c in zip(Sh, sv)]
        w_ap = max(w_ap, _funits(ap[i], hp, Sh))
    print("graph3 on %s: b %.3f u S (bound 32), L L^T - D %.3f of 32 u S + 8 u |L||L^T|, precondition %.3f cond_2 u (bound 64), ap %.3f u S (bound 32)"
          % (label, w_b, w_llt, w_pre, w_ap))
    assert w_b <= 32.0 and w_llt <= 1.0 and w_pre <= 64.0 and w_ap <= 32.0
    # the link products themselves: t_e = W (J_ref p_ref + J_mov p_mov)
    for e in range(E):
        u0, s0 = _matvec(J[e][0], P[REF[e]])
        u1, s1 = _matvec(J[e][1], P[MOV[e]])
        v, _ = _matvec(W[e], [a + c for a, c in zip(u0, u1)])
        _, sv = _matvec(_abs(W[e]), [a + c for a, c in zip(s0, s1)])
        assert _funits(te2[6 * e:6 * e + 6], v, sv) <= 32.0


@pytest.mark.gpu
def test_graph3_gpu(exe):
    check_graph3(_runner(exe, "gpu"), "device")


# ---- 8: the SE(2) bodies on the same graph (device only) ----------------------------------------------------------------------------
def _W3x3(w6):
    w = _fr(w6)
    return [[w[0], w[1], w[2]], [w[1], w[3], w[4]], [w[2], w[4], w[5]]]


def _J2(j, side):
    c, s, lx, ly = _fr(j)
    Z, I = F(0), F(1)
    return [[-c, -s, ly], [s, -c, -lx], [Z, Z, -I]] if side == 0 else [[c, s, Z], [-s, c, Z], [Z, Z, I]]


def _spd6(rng, scale):
    A = rng.normal(size=(3, 3))
    W = (A @ A.T + 0.5 * np.eye(3)) * scale
    return np.array([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]])


@functools.lru_cache(maxsize=None)
def _graph2_case():
    rng = np.random.default_rng(44)
    yaw = [3.0, -3.0, 2.5, -2.8, 0.3, -1.0, 3.1, -3.1]
    pose = np.array([[rng.uniform(-10, 10), rng.uniform(-10, 10), y] for y in yaw])
    origin = pose[0] + [0.05, -0.1, 0.02]
    resid = rng.uniform(0.2, 0.35, size=(N_EDGES, 3)) * rng.choice([-1.0, 1.0], size=(N_EDGES, 3))
    resid[3, 2], resid[12, 2] = -0.3, -0.3                                 # links whose ominus - z leaves (-pi, pi]: z wraps, and so must e
    meas = M2.ominus(pose[MOV], pose[REF]) - resid
    meas[:, 2] = M2.wrap(meas[:, 2])
    info = [np.zeros(6) if e == ZERO_INFO_LINK else _spd6(rng, 10.0 ** rng.uniform(-2, 4)) for e in range(N_EDGES)]
    meas[10], info[10] = meas[1], info[1] * 3.0
    prior = _spd6(rng, 40.0)
    off, adj = _adjacency()
    p = rng.normal(size=(N_NODES, 3)) * 10.0 ** rng.uniform(-1, 1, size=(N_NODES, 3))
    table = np.concatenate([[N_NODES, N_EDGES, MAX_NODES, MAX_EDGES], pose.reshape(-1), origin, REF, MOV, meas.reshape(-1), np.array(info).reshape(-1),
                            prior, off, adj, p.reshape(-1)]).astype(np.float64)
    return dict(table=table, pose=pose, origin=origin, meas=meas, info=info, prior=prior, off=off, adj=adj, p=p)


def check_graph2(run, label):
    g = _graph2_case()
    N, E = N_NODES, N_EDGES
    pose, meas = g["pose"], g["meas"]
    d_yaw = pose[MOV, 2] - pose[REF, 2]
    outside = (d_yaw <= -math.pi) | (d_yaw > math.pi)
    second = np.abs(M2.wrap(d_yaw) - meas[:, 2]) > math.pi                 # the outer wrap has work to do as well
    assert outside.sum() >= 3 and (~outside).sum() >= 3 and second.sum() >= 1
    out = run("graph2", g["table"])
    cost, jac, te, b, dinv, te2, ap = _split(out, [E + 1, 4 * E, 3 * E, 3 * N, 6 * N, 3 * E, 3 * N])
    jac, te, te2, b, dinv, ap = jac.reshape(E, 4), te.reshape(E, 3), te2.reshape(E, 3), b.reshape(N, 3), dinv.reshape(N, 6), ap.reshape(N, 3)
    assert np.all(np.isfinite(out))
    two_pi = 2 * MP.pi
    w_cs = w_l = w_te = w_cost = 0.0
    for e in range(E):
        pi_, pj, zm = pose[REF[e]], pose[MOV[e]], meas[e]
        c, s = MP.cos(_mpf(pi_[2])), MP.sin(_mpf(pi_[2]))
        dx, dy = _mpf(pj[0]) - _mpf(pi_[0]), _mpf(pj[1]) - _mpf(pi_[1])
        lx, ly = c * dx + s * dy, -s * dx + c * dy
        m = max(1.0, abs(float(dx)), abs(float(dy)))
        w_cs = max(w_cs, _units(jac[e][:2], [c, s], U))
        w_l = max(w_l, _units(jac[e][2:], [lx, ly], U * m))
        e2 = _mpf(pj[2]) - _mpf(pi_[2]) - _mpf(zm[2])
        e2 -= two_pi * MP.nint(e2 / two_pi)
        assert abs(e2) <= math.pi - 1e-6 and abs(abs(_mpf(pj[2]) - _mpf(pi_[2]) - _mpf(zm[2])) - MP.pi) >= 1e-6
        e_ref = [lx - _mpf(zm[0]), ly - _mpf(zm[1]), e2]
        W = [[_mpf(v) for v in r] for r in _W3x3(g["info"][e])]
        te_ref = [sum(W[i][j] * e_ref[j] for j in range(3)) for i in range(3)]
        tb = [sum(abs(W[i][j]) * 8 * U * m + 32 * U * abs(W[i][j] * e_ref[j]) for j in range(3)) for i in range(3)]
        for i in range(3):
            d = abs(_mpf(te[e][i]) - te_ref[i])
            assert tb[i] != 0 or d == 0
            w_te = max(w_te, float(d / tb[i]) if tb[i] != 0 else 0.0)
        cb = sum(abs(e_ref[i]) * tb[i] + abs(te_ref[i]) * 8 * U * m + 32 * U * abs(e_ref[i] * te_ref[i]) for i in range(3))
        d = abs(_mpf(cost[e]) - sum(a * t for a, t in zip(e_ref, te_ref)))
        assert cb != 0 or d == 0
        w_cost = max(w_cost, float(d / cb) if cb != 0 else 0.0)
    # the prior: e = pose_0 - origin (no wrap here: the yaws are 0.02 apart), its cost and its part of b and ap exactly
    e0 = [F(float(a)) - F(float(c)) for a, c in zip(pose[0], g["origin"])]
    W0 = _W3x3(g["prior"])
    we0, swe0 = _matvec(W0, e0)
    c0 = sum(a * t for a, t in zip(e0, we0))
    s0 = sum(abs(a) * t for a, t in zip(e0, swe0))
    w_cost0 = float(abs(F(float(cost[E])) - c0) / s0) / U
    print("graph2 on %s, linearisation: c, s %.3f u (bound 4); lx, ly %.3f u max(1, |dx|, |dy|) (bound 8); te %.3f and cost %.3f of their bounds; "
          "the prior's cost %.3f u S (bound 32)" % (label, w_cs, w_l, w_te, w_cost, w_cost0))
    assert w_cs <= 4.0 and w_l <= 8.0 and w_te <= 1.0 and w_cost <= 1.0 and w_cost0 <= 32.0
    J = [(_J2(jac[e], 0), _J2(jac[e], 1)) for e in range(E)]
    W = [_W3x3(w) for w in g["info"]]
    inc = [[(a >> 1, a & 1) for a in g["adj"][g["off"][i]:g["off"][i + 1]]] for i in range(N)]
    P = [_fr(v) for v in g["p"]]
    w_b = w_dinv = w_ap = 0.0
    for i in range(N):
        grad, Sg = [F(0)] * 3, [F(0)] * 3
        D = [[F(0)] * 3 for _ in range(3)]
        hp, Sh = [F(0)] * 3, [F(0)] * 3
        for e, s in inc[i]:
            v, sv = _matvec(_T(J[e][s]), _fr(te[e]))
            grad, Sg = [a + c for a, c in zip(grad, v)], [a + c for a, c in zip(Sg, sv)]
            D = _add(D, _mul(_mul(_T(J[e][s]), W[e]), J[e][s]))
            for s2, node in ((0, REF[e]), (1, MOV[e])):
                v, _ = _matvec(_mul(_mul(_T(J[e][s]), W[e]), J[e][s2]), P[node])
                _, sv = _matvec(_mul(_mul(_abs(_T(J[e][s])), _abs(W[e])), _abs(J[e][s2])), [abs(x) for x in P[node]])
                hp, Sh = [a + c for a, c in zip(hp, v)], [a + c for a, c in zip(Sh, sv)]
        if i == 0:
            grad, Sg = [a + c for a, c in zip(grad, we0)], [a + c for a, c in zip(Sg, swe0)]
            D = _add(D, W0)
            v, sv = _matvec(W0, P[0])
            hp, Sh = [a + c for a, c in zip(hp, v)], [a + c for a, c in zip(Sh, sv)]
        w_ap = max(w_ap, _funits(ap[i], hp, Sh))
        if i == ZERO_INFO_NODE:
            assert np.all(b[i] == 0.0) and np.array_equal(dinv[i], np.array([1.0, 0, 0, 1.0, 0, 1.0]))
            assert all(v == 0 for r in D for v in r)
            continue
        w_b = max(w_b, _funits(b[i], [-v for v in grad], Sg))
        X = _fsolve(D, [[F(int(r == c)) for c in range(3)] for r in range(3)])
        ref6 = [X[0][0], X[0][1], X[0][2], X[1][1], X[1][2], X[2][2]]
        cond = float(np.linalg.cond(np.array([[float(v) for v in r] for r in D])))
        w_dinv = max(w_dinv, float(max(abs(F(float(a)) - c) for a, c in zip(dinv[i], ref6)) / max(abs(c) for c in ref6)) / (cond * U))
    print("graph2 on %s: b %.3f u S (bound 32), dinv %.3f cond_2 u (bound 64), ap %.3f u S (bound 32)" % (label, w_b, w_dinv, w_ap))
    assert w_b <= 32.0 and w_dinv <= 64.0 and w_ap <= 32.0
    for e in range(E):                                                     # the link products themselves
        u0, s0_ = _matvec(J[e][0], P[REF[e]])
        u1, s1_ = _matvec(J[e][1], P[MOV[e]])
        v, _ = _matvec(W[e], [a + c for a, c in zip(u0, u1)])
        _, sv = _matvec(_abs(W[e]), [a + c for a, c in zip(s0_, s1_)])
        assert _funits(te2[e], v, sv) <= 32.0


@pytest.mark.gpu
def test_graph2_gpu(exe):
    check_graph2(_runner(exe, "gpu"), "device")
