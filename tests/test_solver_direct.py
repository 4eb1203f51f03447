"""csrc/ndt_solver.h and the 6x6 solves of csrc/ndt_math.h checked directly, as host code and on the device.

tests/native/solver_checks.hip includes the solver header alone and runs ONE function per case, in a loop on the host or from
a one-thread-per-case kernel on the device.  Every check below is written once, as a function of a run(mode, table)
callable, and used twice: unmarked with the host target, under @pytest.mark.gpu with the device target.  References:

  cstep       the 60 rows of golden["mt_cstep"] (1e-13 * max(1, |want|), the tolerance make_golden.py uses against scipy's
              dcstep; bit equality on the host) and the rejected inputs of the oracle's mt_cstep.
  linesearch  oracle.binding.mt_linesearch with a Python phi that records every (stp, f, dg); the product is fed the
              recorded pairs, so it evaluates no phi and cannot drift.  The seven LS_FUNCS of tests/golden/make_golden.py plus
              functions for the exits the goldens never reach: `down` (info 5, stp == stpmax), `spike` (info 4,
              stp == stpmin), `kink` (info 2, the bracket shrinks below xtol), and `ftol_edge`, whose first trial misses the
              sufficient decrease by the last digit of ftol = 0.11111 -- each kept only with the info intended, and the
              test fails if one is not kept.
              The maxfev exit (info 3) is NOT reached: an unbracketed search grows the step five-fold per trial and is at
              stpmax = 4 after three trials (info 5 or a bracket), and a bracket that is not down to 66 % of its width of
              two trials ago is bisected, so it is under xtol = 1 % of its upper end long before the 40th evaluation; no
              plain phi gets there, and none was contorted to.  Likewise the program's own cut-off at 41 trials only ever
              fires on a recording that is too short (one such case checks that it is reported).
  trialpose   the pose apply_step moves to against the pose of the accepted trial: equal bits (what final_from_trial rests
              on), and both against numpy's composition.
  solve       the exact solution by Gauss-Jordan elimination in fractions.Fraction (doubles convert exactly).  Error of x
              by Cholesky (newton_factor), x by the packed LDL^T (newton_ldlt) and cov = H^-1 (0.0009 J^T J) H^-1, each
              relative to the largest entry of the reference, in units of cond_2(H) * 2^-52; bound 64 (the textbook bound
              for n = 6, Higham's gamma_{3n+1}, is about 40 of these units; a wrong pivot or a dropped term is an error of
              order 1).  cov takes cond_2(H) ONCE: the measured values did not need it twice.
  newton      the system assembled in Fraction from the inputs (soft constraint, Tikhonov, inactive dofs, regulariser with
              numpy's eigenvalues) and solved exactly; bound (64 * 2^-52 + 1e-13 in the non-pd branch) * cond_2(M).

Measured maxima of the solve and Newton checks, in units of cond_2 * 2^-52 (379 solve cases, 168 Newton cases; the
device is an MI355X; bound 64, and 64 + 1e-13 / 2^-52 = 514 for the regularised Newton systems):
                                     host     device
  chol_solve                         0.719    0.769
  packed LDL^T                       0.845    0.845
  cov_from_sums                      1.585    1.128
  newton increment, H pd             1.412    2.431
  newton increment, regularised      1.232    1.602
Worst |x0 - closed form| of the Tikhonov cases (absolute bound 1e-13): 2.2e-15 on the host, 3.1e-15 on the device.

Found by trialpose on the device (it passed on the host): apply_step's translation came out as fma(step, incr, R t) where
the trial's was R t + round(step * incr) -- the device compiler contracted the product into rigid_mul's add in one stage
and not in the other, so the pose a search moved to was NOT the pose of its accepted trial (up to an ulp apart in each
translation component).  Both stages now scale the increment in scaled_increment (no contraction); the 200 cases stay as
the regression.
"""
import functools
import importlib.util
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "solver_checks.hip")
MAX_TRIALS = 41
EPS = 2.0 ** -52
NEXT_NONE, NEXT_APPLY_STEP, NEXT_REQUEST_TRIAL = 0, 1, 2
WIDTH_IN = {"cstep": 12, "linesearch": 3 + 2 * MAX_TRIALS, "trialpose": 19, "solve": 63, "newton": 98}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = str(tmp_path_factory.mktemp("solver") / "solver_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", SRC, "-o", out])
    return out


def _runner(exe, target):
    cmd = [exe] if target == "host" else ["timeout", "-k", "10", "60", exe]

    def run(mode, table):
        table = np.ascontiguousarray(table, dtype=np.float64)
        assert table.ndim == 2 and table.shape[1] == WIDTH_IN[mode]
        n = table.shape[0]
        out = subprocess.run(cmd + [mode, target], input=np.uint32(n).tobytes() + table.tobytes(), capture_output=True)
        assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace"))
        return np.frombuffer(out.stdout, dtype=np.float64).reshape(n, -1)
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- cstep ----------------------------------------------------------------------------------------------------------------------
# (rejected by mt_cstep: dx * (stp - stx) >= 0, and stmax < stmin -- info 0, nothing touched)
CSTEP_REJECTED = [[0.0, 1.0, +0.5, 2.0, 1.0, 0.1, 1.0, 0.9, -0.1, 0.0, 0.0, 4.0],
                  [0.0, 1.0, -0.5, 2.0, 1.0, 0.1, 1.0, 0.9, -0.1, 0.0, 4.0, 0.0]]


def check_cstep(run, golden, bitwise):
    rows = golden["mt_cstep"]
    out = run("cstep", np.concatenate([rows[:, :12], np.array(CSTEP_REJECTED)]))
    got, rej = out[:len(rows)], out[len(rows):]
    assert np.array_equal(got[:, 0], rows[:, 12])                          # info
    assert np.array_equal(got[:, 8], rows[:, 20])                          # brackt
    assert set(rows[:, 12]) == {1.0, 2.0, 3.0, 4.0}                        # (every case of the step selection is among them)
    want = rows[:, 13:20]
    assert np.all(np.abs(got[:, 1:8] - want) <= 1e-13 * np.maximum(1.0, np.abs(want)))
    if bitwise:
        assert np.array_equal(_bits(got[:, 1:8]), _bits(want))
    for r, row in zip(rej, CSTEP_REJECTED):
        info, vals, br = O.mt_cstep(*row[:9], bool(row[9]), row[10], row[11])
        assert info == 0 and r[0] == 0
        assert np.array_equal(r[1:8], np.array(vals)) and np.array_equal(r[1:8], np.array(row[:7])) and r[8] == float(br)


def test_cstep_host(exe, golden):
    check_cstep(_runner(exe, "host"), golden, bitwise=True)


@pytest.mark.gpu
def test_cstep_gpu(exe, golden):
    check_cstep(_runner(exe, "gpu"), golden, bitwise=False)


# ---- linesearch -----------------------------------------------------------------------------------------------------------------
# name: (phi, dphi, the oracle's info this function is here for)
LS_EXTRA = {
    # decreases for ever: every trial gives sufficient decrease and too steep a slope, the step grows to stpmax
    "down": (lambda t: -t, lambda t: -1.0, 5),
    # slope -1 at 0, minimum at 5e-5, rising from there on: no trial down to stpmin = 0.001 gives sufficient decrease
    "spike": (lambda t: t * t / 1e-4 - t, lambda t: 2 * t / 1e-4 - 1.0, 4),
    # a kink at 0.5, slope -1 before and +3 after: the curvature condition never holds, the bracket closes on the kink
    "kink": (lambda t: -t if t < 0.5 else 3.0 * (t - 0.5) - 0.5, lambda t: -1.0 if t < 0.5 else 3.0, 2),
    # phi(1) = -0.111105 lies between finit + 0.11111 dginit and finit + 0.1111 dginit, with a flat enough slope there: the
    # first trial just misses the sufficient decrease (ftol = 0.11111 to its last digit) and the search goes on
    "ftol_edge": (lambda t: 0.888895 * t * t - t, lambda t: 1.77779 * t - 1.0, 1),
}


@functools.lru_cache(maxsize=None)
def _ls_records():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    funcs = {name: (f, df, None) for name, (f, df) in mg.LS_FUNCS.items()}
    funcs.update(LS_EXTRA)
    recs = {}
    for name, (f, df, intended) in funcs.items():
        log = []

        def phi(t, f=f, df=df, log=log):
            v = (float(f(t)), float(df(t)))
            log.append((float(t),) + v)
            return v
        stp, nfev, info = O.mt_linesearch(phi, float(f(0.0)), float(df(0.0)))
        assert len(log) == nfev <= 40
        if intended is not None and info != intended:
            continue                                                       # (kept only with the info it is here for)
        recs[name] = dict(finit=float(f(0.0)), dginit=float(df(0.0)), log=log, stp=stp, nfev=nfev, info=info, golden=intended is None)
    return recs


def _ls_row(finit, dginit, pairs):
    row = np.zeros(3 + 2 * MAX_TRIALS)
    row[:3] = finit, dginit, len(pairs)
    for k, (f, dg) in enumerate(pairs):
        row[3 + 2 * k], row[4 + 2 * k] = f, dg
    return row


def check_linesearch(run, golden):
    recs = _ls_records()
    for name, (_, _, intended) in LS_EXTRA.items():                        # (none of them was dropped)
        assert name in recs and recs[name]["info"] == intended, name
    assert recs["ftol_edge"]["nfev"] > 1
    names = list(recs)
    rows = [_ls_row(r["finit"], r["dginit"], [(f, dg) for _, f, dg in r["log"]]) for r in recs.values()]
    # the increment points uphill (dginit > 0): mt_start_local negates it, the search is the one along -e0 -- mt1 mirrored
    m = recs["mt1"]
    rows.append(_ls_row(m["finit"], -m["dginit"], [(f, -dg) for _, f, dg in m["log"]]))
    # dginit == 0: still no descent direction after the negation, the recovery step without a trial
    rows.append(_ls_row(1.0, 0.0, []))
    # a recording that ends one pair early: the program stops there and says so
    rows.append(_ls_row(m["finit"], m["dginit"], [(f, dg) for _, f, dg in m["log"][:-1]]))
    out = run("linesearch", np.stack(rows))
    tail = out[:, MAX_TRIALS:]

    def same_search(o, r):
        steps, (step_size, nfev, from_trial, spec_ok, reuse, used, cut, first, has_h) = o[:MAX_TRIALS], o[MAX_TRIALS:]
        assert first == NEXT_REQUEST_TRIAL and cut == 0
        assert used == nfev == r["nfev"]                                   # the same number of trials
        for k, (stp, _, _) in enumerate(r["log"]):
            assert abs(steps[k] - stp) <= 1e-12 * max(1.0, abs(stp)), (k, steps[k], stp)
        assert np.all(steps[r["nfev"]:] == 0.0)
        want = r["stp"] if r["info"] == 1 else 0.1
        assert r["info"] == 1 or r["stp"] == 0.1
        assert abs(step_size - want) <= 1e-12 * max(1.0, abs(want))
        assert from_trial == (r["info"] == 1)
        assert spec_ok == (r["info"] == 1 and r["nfev"] == 1)
        # the sums are consumed again exactly when the accepted trial was evaluated with its Hessian (which trials are is
        # tuning, NDT_SPEC_FROM; only the first is fixed here: spec_ok starts at 0, so it never is)
        assert reuse == (r["info"] == 1 and has_h == 1)
        assert r["nfev"] > 1 or has_h == 0

    for name, o in zip(names, out):
        r = recs[name]
        same_search(o, r)
        if r["golden"]:
            want = golden["mt_ls_" + name]
            assert o[MAX_TRIALS + 1] == want[1] and r["info"] == want[2], name
            assert abs(o[MAX_TRIALS] - want[0]) <= 1e-12 * max(1.0, abs(want[0])), name
    assert tail[names.index("mt2"), 0] == 0.1 and tail[names.index("mt2"), 1] == 6
    assert abs(tail[names.index("steep"), 0] - 0.076144121984716) < 1e-12 and tail[names.index("steep"), 1] == 3
    same_search(out[len(names)], m)
    o = out[len(names) + 1]
    assert o[MAX_TRIALS + 7] == NEXT_APPLY_STEP and o[MAX_TRIALS] == 0.1 and o[MAX_TRIALS + 5] == 0 and np.all(o[:MAX_TRIALS] == 0.0)
    o = out[len(names) + 2]
    assert o[MAX_TRIALS + 6] == 2 and o[MAX_TRIALS + 5] == m["nfev"] - 1
    assert abs(o[m["nfev"] - 1] - m["log"][-1][0]) <= 1e-12 * max(1.0, m["log"][-1][0])


def test_linesearch_host(exe, golden):
    check_linesearch(_runner(exe, "host"), golden)


@pytest.mark.gpu
def test_linesearch_gpu(exe, golden):
    check_linesearch(_runner(exe, "gpu"), golden)


# ---- trialpose ------------------------------------------------------------------------------------------------------------------
def _rot(p):
    cx, sx, cy, sy, cz, sz = np.cos(p[0]), np.sin(p[0]), np.cos(p[1]), np.sin(p[1]), np.cos(p[2]), np.sin(p[2])
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]))


@functools.lru_cache(maxsize=None)
def _trialpose_cases():
    g = np.random.default_rng(11)
    n = 200
    rows = np.zeros((n, 19))
    for k in range(n):
        rows[k, :9] = _rot(g.uniform(-np.pi, np.pi, 3)).reshape(-1)
        rows[k, 9:12] = g.uniform(-20, 20, 3)
        rows[k, 12:15] = g.uniform(-1, 1, 3)
        ang = g.uniform(0.01, 0.5, 3) * g.choice([-1.0, 1.0], 3)          # non-zero rotation components
        rows[k, 15:18] = ang
        rows[k, 18] = 10.0 ** g.uniform(-3, np.log10(4.0))
    rows[:4, 18] = 0.001, 4.0, 1.0, 0.5
    rows[4, 15:18] = 0.5, -0.5, 0.5                                        # the largest angles at the largest step
    rows[4, 18] = 4.0
    return rows


def check_trialpose(run):
    rows = _trialpose_cases()
    out = run("trialpose", rows)
    assert np.all(out[:, 24] == 1.0)                                       # every trial was accepted (info 1) ...
    assert np.array_equal(_bits(out[:, 25]), _bits(rows[:, 18]))           # ... at the step it was made with
    # the claim final_from_trial rests on: the pose apply_step moves to IS the trial's pose
    assert np.array_equal(_bits(out[:, :12]), _bits(out[:, 12:24]))
    for r, o in zip(rows, out):                                            # and it is the right pose
        p = r[18] * r[12:18]
        R = _rot(p[3:]) @ r[:9].reshape(3, 3)
        t = _rot(p[3:]) @ r[9:12] + p[:3]
        assert np.max(np.abs(o[:9].reshape(3, 3) - R)) < 1e-14 and np.max(np.abs(o[9:12] - t)) < 1e-13


def test_trialpose_host(exe):
    check_trialpose(_runner(exe, "host"))


@pytest.mark.gpu
def test_trialpose_gpu(exe):
    check_trialpose(_runner(exe, "gpu"))


# ---- exact algebra --------------------------------------------------------------------------------------------------------------
def _fmat(a):
    return [[F(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _fsolve(A, B):
    """A^-1 B by Gauss-Jordan elimination over the rationals (A, B: lists of rows of Fraction); None when A is singular."""
    n = len(A)
    M = [list(ra) + list(rb) for ra, rb in zip(A, B)]
    for c in range(n):
        p = next((r for r in range(c, n) if M[r][c] != 0), None)
        if p is None:
            return None
        M[c], M[p] = M[p], M[c]
        d = M[c][c]
        M[c] = [v / d for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def _fmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _rel_err(got, ref):
    """max |got - ref| / max |ref|, exactly, then rounded once (got: floats, ref: Fractions, flat)."""
    scale = max(abs(r) for r in ref)
    return float(max(abs(F(float(g)) - r) for g, r in zip(got, ref)) / scale)


# ---- solve ----------------------------------------------------------------------------------------------------------------------
def _sym(A):
    return 0.5 * (A + A.T)


def _pivot_trace(A):
    """(step, pivot) pairs of an LDL^T with diagonal pivoting (largest |diagonal| of the rest, the first on ties)."""
    a = np.array(A, dtype=np.float64)
    trace = []
    for k in range(5):
        piv = k + int(np.argmax(np.abs(np.diag(a)[k:])))
        trace.append((k, piv))
        a[[k, piv]] = a[[piv, k]]
        a[:, [k, piv]] = a[:, [piv, k]]
        if a[k, k] != 0.0:
            a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:]) / a[k, k]
    return trace


@functools.lru_cache(maxsize=None)
def _solve_cases():
    g = np.random.default_rng(7)
    mats = []

    def spectrum(ev):
        Q, _ = np.linalg.qr(g.normal(size=(6, 6)))
        return _sym(Q @ np.diag(ev) @ Q.T)
    for k in range(150):                                   # SPD, cond 1 .. 1e12 over scales 1e-3 .. 1e6
        cond = 10.0 ** (12.0 * k / 149.0)
        ev = np.concatenate([[1.0, cond], cond ** g.uniform(0, 1, 4)]) / cond
        mats.append(spectrum(ev) * 10.0 ** g.uniform(-3, 6))
    S = np.diag([1, 1, 1e-3, 30, 30, 300.0])
    for _ in range(40):                                    # Hessian-like scalings (test_native_math._cases): indefinite ...
        A = g.normal(size=(6, 6))
        mats.append(_sym(S @ (A + A.T) @ S) * 10.0 ** g.uniform(0, 4))
    for _ in range(40):                                    # ... and positive definite
        A = g.normal(size=(6, 6))
        mats.append(_sym(S @ (A @ A.T + 0.1 * np.eye(6)) @ S) * 10.0 ** g.uniform(0, 4))
    for _ in range(80):                                    # indefinite, lambda_min <= -1e-6 lambda_max
        ev = 10.0 ** g.uniform(-6, 0, 6) * g.choice([-1.0, 1.0], 6)
        ev[0], ev[1] = 1.0, -10.0 ** g.uniform(-6, 0)
        mats.append(spectrum(ev) * 10.0 ** g.uniform(-3, 6))
    for k in range(60):                                    # a prescribed pivot order (every swap_k<K> branch), indefinite
        order = g.permutation(6) if k else np.arange(6)[::-1]
        d = np.empty(6)
        d[order] = [32.0, 16.0, 8.0, 4.0, 2.0, 1.0]
        A = g.normal(size=(6, 6)) * 0.05
        mats.append(_sym(A) + np.diag(d * g.choice([-1.0, 1.0], 6)))
    for _ in range(10):                                    # the largest diagonal entry last, positive definite
        A = g.normal(size=(6, 6)) * 0.05
        mats.append(_sym(A) + np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 60.0]))
    for _ in range(10):                                    # tied diagonals
        A = g.normal(size=(6, 6)) * 0.3
        A = _sym(A)
        np.fill_diagonal(A, 2.0 * g.choice([-1.0, 1.0], 6))
        mats.append(A)
    ev = [np.linalg.eigvalsh(A) for A in mats]
    # the sign of lambda_min is not rounding noise
    mats = [A for A, e in zip(mats, ev) if abs(e[0]) >= 1e-12 * np.max(np.abs(e))]
    assert len(mats) >= 350
    n = len(mats)
    rows = np.zeros((n, 63))
    ref = []
    for k, A in enumerate(mats):
        b = g.normal(size=6) * 10.0 ** g.uniform(-2, 2)
        B = g.normal(size=(8, 6))
        JJ = B.T @ B
        rows[k, :36] = A.reshape(-1)
        rows[k, 36:42] = b
        rows[k, 42:] = JJ[np.triu_indices(6)]
        Hf = _fmat(A)
        X = _fsolve(Hf, [[F(int(i == j)) for j in range(6)] + [F(float(b[i]))] for i in range(6)])
        Hinv = [r[:6] for r in X]
        JK = [[F(0.03 * 0.03) * F(float(JJ[min(i, j), max(i, j)])) for j in range(6)] for i in range(6)]
        cov = _fmul(_fmul(Hinv, JK), Hinv)
        e = np.linalg.eigvalsh(A)
        ref.append(dict(x=[r[6] for r in X], cov=[v for r in cov for v in r], pd=bool(e[0] > 0), cond=float(np.linalg.cond(A))))
    return rows, ref, mats


def check_solve(run, label):
    rows, ref, mats = _solve_cases()
    # every exchange of the packed LDL^T is among the cases that reach it, and there are ties to break
    seen = {kp for A in mats for kp in _pivot_trace(A)}
    assert seen >= {(k, c) for k in range(5) for c in range(k, 6)}
    # singular: an exact zero pivot (row and column 2 are zero), and its right-hand side
    Z = np.diag([4.0, 3.0, 0.0, -2.0, 1.0, 5.0])
    Z[0, 1] = Z[1, 0] = 0.5
    Z[3, 5] = Z[5, 3] = -0.25
    zrow = np.zeros(63)
    zrow[:36] = Z.reshape(-1)
    zrow[36:42] = 1.0, -2.0, 3.0, 0.5, -1.5, 2.5
    zrow[42:] = rows[0, 42:]
    out = run("solve", np.concatenate([rows, zrow[None]]))
    got, zout = out[:-1], out[-1]
    worst = dict(chol=0.0, ldlt=0.0, cov=0.0)
    n_pd = 0
    for k, (o, r) in enumerate(zip(got, ref)):
        assert bool(o[0]) == r["pd"], (k, o[0], r["pd"])
        unit = r["cond"] * EPS
        if r["pd"]:
            n_pd += 1
            worst["chol"] = max(worst["chol"], _rel_err(o[1:7], r["x"]) / unit)
        else:
            assert np.all(o[1:7] == 0.0)
        worst["ldlt"] = max(worst["ldlt"], _rel_err(o[7:13], r["x"]) / unit)
        assert o[13] == 0.0
        worst["cov"] = max(worst["cov"], _rel_err(o[14:50], r["cov"]) / unit)
    print("solve on %s, worst error / (cond_2 * 2^-52): chol_solve %.3f  packed LDL^T %.3f  cov_from_sums %.3f  (%d cases, %d pd)"
          % (label, worst["chol"], worst["ldlt"], worst["cov"], len(ref), n_pd))
    assert 150 <= n_pd <= len(ref) - 150
    assert worst["chol"] <= 64.0 and worst["ldlt"] <= 64.0 and worst["cov"] <= 64.0, worst
    # the zero pivot: not positive definite, a zero component like Eigen's LDLT::solve (and the oracle's), no covariance
    assert zout[0] == 0.0
    want = O.ldlt_solve(Z, zrow[36:42])
    assert want[2] == 0.0 and zout[7 + 2] == 0.0
    assert np.all(np.abs(zout[7:13] - want) <= 64 * EPS * np.max(np.abs(want)))
    assert zout[13] == 1.0 and np.all(zout[14:50] == 0.0)


def test_solve_host(exe):
    check_solve(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_solve_gpu(exe):
    check_solve(_runner(exe, "gpu"), "device")


# ---- newton ---------------------------------------------------------------------------------------------------------------------
def _rigid12(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(-1), np.asarray(t, dtype=np.float64)])


IDENT12 = _rigid12(np.eye(3), np.zeros(3))


def _newton_row(score, grad, H, mask=0x3f, delta=1e-6, step_control=0, flags=0, Q=None, pose_local=None, T=IDENT12, Tinit=IDENT12):
    row = np.zeros(98)
    row[0] = score
    row[1:7] = grad
    row[7:28] = np.asarray(H)[np.triu_indices(6)]
    row[28:32] = mask, delta, step_control, flags
    row[32:68] = np.zeros(36) if Q is None else np.asarray(Q).reshape(-1)
    row[68:74] = np.zeros(6) if pose_local is None else pose_local
    row[74:86] = T
    row[86:98] = Tinit
    return row


def _newton_ref(row, x0):
    """The Newton system of one case, exactly: score, gnorm, active dofs, -M^-1 g on them, cond_2(M), pd, M's diagonal."""
    s = [F(float(v)) for v in row[:28]]
    mask, flags = int(row[28]), int(row[31])
    H = [[None] * 6 for _ in range(6)]
    o = 7
    for a in range(6):
        for b in range(a, 6):
            H[a][b] = H[b][a] = s[o]
            o += 1
    g = s[1:7]
    score = s[0]
    Q = _fmat(row[32:68].reshape(6, 6))
    pl = [F(float(v)) for v in row[68:74]]
    xf = [F(float(v)) for v in x0]
    if flags & 1:                                          # soft constraint: H + Q + Q^T, g + (Q + Q^T) pose_local
        for a in range(6):
            for b in range(6):
                H[a][b] += Q[a][b] + Q[b][a]
            g[a] += sum((Q[a][j] + Q[j][a]) * pl[j] for j in range(6))
        score += sum(pl[i] * Q[i][j] * pl[j] for i in range(6) for j in range(6))
    if flags & 2:                                          # Tikhonov: H^T H + Q, H^T g + Q x0
        g = [sum(H[k][a] * g[k] for k in range(6)) + sum(Q[a][k] * xf[k] for k in range(6)) for a in range(6)]
        H = [[sum(H[k][a] * H[k][b] for k in range(6)) + Q[a][b] for b in range(6)] for a in range(6)]
        score += sum(xf[i] * Q[i][j] * xf[j] for i in range(6) for j in range(6))
    act = [a for a in range(6) if (mask >> a) & 1]
    ga = [g[a] for a in act]
    Ha = [[H[a][b] for b in act] for a in act]
    gnorm = float(np.sqrt(float(sum(v * v for v in ga))))
    Hfl = np.array([[float(v) for v in r] for r in Ha])
    ev = np.linalg.eigvalsh(_sym(Hfl))
    pd = bool(ev[0] > 0)
    reg = 0.0
    if not pd:
        reg = gnorm if gnorm + ev[0] > 0 else 0.001 * ev[-1] - ev[0]
        # both decisions are clear of rounding
        assert -ev[0] >= 1e-6 * ev[-1] and abs(gnorm + ev[0]) >= 1e-6 * ev[-1]
    M = [[Ha[i][j] + (F(reg) if i == j else 0) for j in range(len(act))] for i in range(len(act))]
    x = _fsolve(M, [[-v] for v in ga])
    Mfl = np.array([[float(v) for v in r] for r in M])
    return dict(score=score, gnorm=gnorm, act=act, x=[r[0] for r in x], cond=float(np.linalg.cond(Mfl)), pd=pd,
                diag=[float(M[i][i]) for i in range(len(act))], lam=float(np.max(np.abs(ev))), reg_gnorm=(not pd) and reg == gnorm)


@functools.lru_cache(maxsize=None)
def _newton_cases():
    g = np.random.default_rng(19)
    cases = []                                             # (kind, row, x0)

    def spd(cond, scale):
        Q, _ = np.linalg.qr(g.normal(size=(6, 6)))
        ev = np.concatenate([[1.0, cond], cond ** g.uniform(0, 1, 4)]) / cond
        return _sym(Q @ np.diag(ev) @ Q.T) * scale

    def prior():                                           # Tcov^-1: not symmetric, positive, diagonally dominant
        return np.diag(g.uniform(1.0, 10.0, 6)) + 0.05 * g.normal(size=(6, 6))
    zero = np.zeros(6)
    for k in range(40):                                    # the plain 6-dof iteration, no step control
        H = spd(10.0 ** g.uniform(0, 8), 10.0 ** g.uniform(0, 4))
        cases.append(("plain", _newton_row(-g.uniform(10, 500), g.normal(size=6) * 10.0 ** g.uniform(-1, 2), H), zero))
    for k in range(10):                                    # ... with it: the search starts along the same increment
        H = spd(10.0 ** g.uniform(0, 6), 10.0 ** g.uniform(0, 4))
        cases.append(("search", _newton_row(-g.uniform(10, 500), g.normal(size=6) * 10.0, H, step_control=1), zero))
    for k in range(20):                                    # x, y, yaw
        H = spd(10.0 ** g.uniform(0, 6), 10.0 ** g.uniform(0, 4))
        cases.append(("planar", _newton_row(-g.uniform(10, 500), g.normal(size=6) * 10.0, H, mask=0x23), zero))
    for k in range(20):                                    # soft constraint
        H = spd(10.0 ** g.uniform(0, 6), 10.0 ** g.uniform(0, 2))
        cases.append(("prior", _newton_row(-g.uniform(10, 500), g.normal(size=6) * 10.0, H, flags=1, Q=prior(),
                                           pose_local=g.normal(size=6) * 0.3), zero))
    # Tikhonov.  x0 = (tx, ty, 0, 0, 0, yaw) of T Tinit^-1 with T = D Tinit for a planar offset D, so x0 is D's.  The yaw is
    # the acos of a matrix entry c (condition 1 / |sin yaw|): with c off by a few 2^-53 the bound of 1e-13 on x0 is within
    # reach for |sin yaw| >= 0.05 under a general Tinit, and for yaw = 0 and yaw near +-pi only where the product T Tinit^-1
    # is exact or nearly so -- a Tinit of quarter turns and short dyadic translations.
    quarter = _rigid12([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]], [2.0, -3.5, 0.25])
    offsets = [(0.25, -0.5, 0.0, quarter), (0.0, 0.0, 0.0, IDENT12), (-1.5, 0.75, np.pi - 0.01, quarter), (0.5, 2.0, -(np.pi - 0.01), IDENT12),
               (1.0, -1.0, np.pi - 0.01, IDENT12)]
    for k in range(20):
        yaw = g.uniform(0.05, 3.0) * g.choice([-1.0, 1.0])
        Ti = _rigid12(_rot(g.uniform(-0.3, 0.3, 3) + [0, 0, g.uniform(-3, 3)]), g.uniform(-10, 10, 3))
        offsets.append((g.uniform(-2, 2), g.uniform(-2, 2), yaw, Ti))
    for dx, dy, yaw, Ti in offsets:
        D = _rot([0.0, 0.0, yaw])
        if yaw == 0.0:
            D = np.eye(3)
        T = _rigid12(D @ Ti[:9].reshape(3, 3), D @ Ti[9:] + [dx, dy, 0.0])
        H = spd(10.0 ** g.uniform(0, 3), 10.0 ** g.uniform(0, 2))
        Q = prior()
        cases.append(("tikhonov", _newton_row(-g.uniform(10, 500), g.normal(size=6) * 10.0, H, flags=2, Q=_sym(Q), T=T, Tinit=Ti),
                      np.array([dx, dy, 0.0, 0.0, 0.0, yaw])))
    for k in range(48):                                    # H not positive definite: both branches of the regulariser
        mask = 0x23 if k >= 32 else 0x3f
        act = [a for a in range(6) if (mask >> a) & 1]
        n = len(act)
        ev = 10.0 ** g.uniform(-3, 0, n)
        ev[0], ev[1] = 1.0, -10.0 ** g.uniform(-3, -0.5)   # lambda_max and lambda_min of the active block
        if k % 4 == 0:
            ev[2] = 0.5 * ev[1]                            # a second negative eigenvalue
        Qm, _ = np.linalg.qr(g.normal(size=(n, n)))
        scale = 10.0 ** g.uniform(0, 4)
        H = _sym(g.normal(size=(6, 6))) * scale            # (what the inactive dofs hold is masked away)
        H[np.ix_(act, act)] = _sym(Qm @ np.diag(ev) @ Qm.T) * scale
        grad = g.normal(size=6)
        grad *= (2.0 if k % 2 else 0.5) * -ev[1] * scale / np.linalg.norm(grad[act])   # gnorm + lambda_min > 0, or not
        cases.append(("nonpd", _newton_row(-g.uniform(10, 500), grad, H, mask=mask), zero))
    for k in range(4):                                     # a gradient below delta_score: converged ...
        H = spd(100.0, 50.0)
        grad = g.normal(size=6)
        grad *= (0.5e-6 if k < 3 else 0.999e-6) / np.linalg.norm(grad)
        kw = dict(flags=1, Q=np.zeros((6, 6)), pose_local=zero) if k == 2 else {}
        cases.append(("converged", _newton_row(-123.5, grad, H, step_control=k % 2, **kw), zero))
    grad = g.normal(size=6)                                # ... and one just above it: not converged
    cases.append(("plain", _newton_row(-123.5, grad * 1.001e-6 / np.linalg.norm(grad), spd(100.0, 50.0)), zero))
    refs = [_newton_ref(row, x0) for _, row, x0 in cases]
    return cases, refs


def check_newton(run, label):
    cases, refs = _newton_cases()
    kinds = [c[0] for c in cases]
    assert sum(k == "nonpd" for k in kinds) >= 30
    assert {(r["reg_gnorm"], len(r["act"])) for k, r in zip(kinds, refs) if k == "nonpd"} == {(True, 6), (False, 6), (True, 3), (False, 3)}
    out = run("newton", np.stack([c[1] for c in cases]))
    worst = {True: 0.0, False: 0.0}                                        # by pd, in units of cond_2(M) * 2^-52
    worst_x0 = 0.0
    for k, ((kind, row, x0), r, o) in enumerate(zip(cases, refs, out)):
        nxt, exit_code, done, score, is_pd, gnorm = o[:6]
        incr, diag, gx0, step_size, dx = o[6:12], o[12:18], o[18:24], o[24], o[25:31]
        sref = float(r["score"])
        assert abs(score - sref) <= 1e-13 * abs(sref), (kind, k, score, sref)             # with its Mahalanobis / Tikhonov term
        worst_x0 = max(worst_x0, float(np.max(np.abs(gx0 - x0))))
        assert np.all(np.abs(gx0 - x0) <= 1e-13), (kind, k, gx0, x0)
        assert abs(gnorm - r["gnorm"]) <= 8 * EPS * r["gnorm"], (kind, k)
        if kind == "converged":
            assert r["gnorm"] <= row[29]
            assert (nxt, exit_code, done) == (NEXT_NONE, 1, 1), (kind, k)
            assert np.all(incr == 0.0)
            continue
        assert r["gnorm"] > row[29]
        assert bool(is_pd) == r["pd"] and r["pd"] == (kind != "nonpd"), (kind, k)
        assert (exit_code, done) == (0, 0), (kind, k)
        if row[30] == 0:                                                   # no step control: the full step
            assert nxt == NEXT_APPLY_STEP and step_size == 1.0, (kind, k)
        else:
            assert nxt == NEXT_REQUEST_TRIAL, (kind, k)
        # the increment the line search gets is -M^-1 g (M is positive definite: it points downhill, nothing negates it)
        assert np.array_equal(incr, np.where([(int(row[28]) >> a) & 1 for a in range(6)], -dx, 0.0)), (kind, k)
        inactive = [a for a in range(6) if a not in r["act"]]
        assert np.array_equal(_bits(incr[inactive]), _bits(np.zeros(len(inactive)))), (kind, k)   # exactly 0.0
        tol = (64 * EPS + (0.0 if r["pd"] else 1e-13)) * r["cond"]
        err = _rel_err(incr[r["act"]], r["x"])
        worst[r["pd"]] = max(worst[r["pd"]], err / (r["cond"] * EPS))
        assert err <= tol, (kind, k, err, tol)
        if not r["pd"]:                                                    # the regulariser went onto the diagonal
            assert np.all(np.abs(diag[r["act"]] - r["diag"]) <= 1e-13 * r["lam"] + 8 * EPS * np.abs(r["diag"])), (kind, k)
    print("newton on %s, worst increment error / (cond_2(M) * 2^-52): %.3f positive definite (bound 64), %.3f regularised (bound %.0f)  (%d cases)"
          % (label, worst[True], worst[False], 64 + 1e-13 / EPS, len(cases)))
    print("newton on %s, worst |x0 - closed form|: %.3e (bound 1e-13)" % (label, worst_x0))


def test_newton_host(exe):
    check_newton(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_newton_gpu(exe):
    check_newton(_runner(exe, "gpu"), "device")
