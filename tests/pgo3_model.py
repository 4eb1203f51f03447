"""NumPy restatement of the SE(3) pose-graph optimiser (include/ndtgpu.h, ndtgpu_pgo3_*): the prior and the 6-DoF link errors
e = (t_E, Log R_E), E = T_ref^-1 T_mov Z^-1, their analytic Jacobians, the retraction T [+] d = (R Exp(phi), t + R rho),
Gauss-Newton with the library's stop rule, each linear system solved densely (numpy.linalg.solve: the reference of the GPU tests)
or by a restatement of the device's block-Jacobi preconditioned conjugate gradients (the floor of the GPU tests' tolerance).  Also
the graph generators the CPU and the GPU tests share, and ndt_pgo3_link_from_registration (csrc/ndt_pgo3.h) restated operation for
operation in Python floats, whose results the library's are compared with bit for bit.

Poses are 4x4 matrices; 6-vectors are (rho, phi) = (x, y, z, rx, ry, rz), the order of cov36.

The tolerance of "compare with the model" (tests/test_gpu_pgo3.py).  tests/test_pgo3_model.py::test_floor runs the model on every
graph the GPU tests compare with it three ways -- dense; with the restated conjugate gradients at the default eps_linear; dense
with E associated the other way, T_ref^-1 (T_mov Z^-1) -- and takes the largest entrywise difference of the 4x4 poses (PCG3_FLOOR)
and the largest relative difference of cost_final (COST3_FLOOR).  Measured there: poses 1.02e-14 (weighted, whose largest
coordinate is 22 m: three units in its last place; 6.2e-15 on grid3d, 1.4e-15 or less on the rings), cost 5.4e-15 (weighted).  The
GPU tests allow ten times each; the factor covers the device's summation order and its sincos / atan2.  No number here comes from a device."""
import math

import numpy as np

CONVERGED, MAX_ITERATIONS, LINEAR_CAP, NOT_FINITE, HALF_TURN = 0, 1, 2, 3, 4
DEFAULTS = dict(max_iterations=50, max_linear_iterations=2000, eps_step=1e-8, eps_linear=1e-8)
COV_SINGULAR, COV_POSE_UNCHANGED, COV_NOT_COMPUTED = 1, 2, 4
TINY = 1e-8

PCG3_FLOOR = 1.1e-14
TOL = 10 * PCG3_FLOOR
COST3_FLOOR = 5.5e-15
COST_RTOL = 10 * COST3_FLOOR


# ---- SO(3) and SE(3), vectorised over leading axes -----------------------------------------------------------------------------

def hat(v):
    v = np.asarray(v, dtype=np.float64)
    o = np.zeros_like(v[..., 0])
    return np.stack([np.stack([o, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], o, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], o], -1)], -2)


def exp_so3(phi):
    """Rodrigues"""
    phi = np.asarray(phi, dtype=np.float64)
    t2 = np.sum(phi * phi, -1)
    small = t2 < 1e-8
    t = np.sqrt(np.where(small, 1.0, t2))
    a = np.where(small, 1.0 - t2 / 6.0, np.sin(t) / t)
    b = np.where(small, 0.5 - t2 / 24.0, (1.0 - np.cos(t)) / np.where(small, 1.0, t2))
    K = hat(phi)
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def log_so3(R):
    """-> (phi, half): v theta / |v|; v where |v| is tiny and the trace positive; half (phi NaN) where tiny and the trace negative"""
    R = np.asarray(R, dtype=np.float64)
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    n = np.sqrt(np.sum(v * v, -1))
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    tiny = n < TINY
    half = tiny & (c < 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(tiny, 1.0, np.arctan2(n, c) / np.where(tiny, 1.0, n))
    phi = k[..., None] * v
    phi = np.where(half[..., None], np.nan, phi)
    return phi, half


def jr_inv(phi):
    """the inverse right Jacobian of SO(3): I + [phi]x / 2 + (1 / theta^2 - (1 + cos theta) / (2 theta sin theta)) [phi]x^2"""
    phi = np.asarray(phi, dtype=np.float64)
    t2 = np.sum(phi * phi, -1)
    small = t2 < 1e-4
    t = np.sqrt(np.where(small, 1.0, t2))
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(small, 1.0 / 12.0 + t2 / 720.0, 1.0 / t ** 2 - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t)))
    K = hat(phi)
    return np.eye(3) + 0.5 * K + k[..., None, None] * (K @ K)


def make_T(R, t):
    T = np.zeros(np.asarray(R).shape[:-2] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = t
    T[..., 3, 3] = 1.0
    return T


def inv_T(T):
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    return make_T(Rt, -np.einsum("...ab,...b->...a", Rt, T[..., :3, 3]))


def retract(T, d):
    """T [+] d = (R Exp(phi), t + R rho); no re-orthonormalisation"""
    T, d = np.asarray(T, dtype=np.float64), np.asarray(d, dtype=np.float64)
    R = T[..., :3, :3]
    return make_T(R @ exp_so3(d[..., 3:]), T[..., :3, 3] + np.einsum("...ab,...b->...a", R, d[..., :3]))


def euler_T(x, y, z, roll, pitch, yaw):
    """Trans(x, y, z) Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    return make_T(Rz @ Ry @ Rx, [x, y, z])


def link_error(Ti, Tj, Z, assoc="left", jacobians=False):
    """e [.., 6] of the link (ref = Ti, mov = Tj, Z); assoc: "left" (T_ref^-1 T_mov) Z^-1 as the device, "right" T_ref^-1 (T_mov Z^-1).
    -> (e, half) or (e, half, J_ref, J_mov)"""
    Ti, Tj, Z = (np.asarray(a, dtype=np.float64) for a in (Ti, Tj, Z))
    Zi = inv_T(Z)
    A = inv_T(Ti) @ Tj
    E = A @ Zi if assoc == "left" else inv_T(Ti) @ (Tj @ Zi)
    phi, half = log_so3(E[..., :3, :3])
    e = np.concatenate([E[..., :3, 3], phi], -1)
    if not jacobians:
        return e, half
    RA, RE, Rzi, tzi = A[..., :3, :3], E[..., :3, :3], Zi[..., :3, :3], Zi[..., :3, 3]
    Ji = jr_inv(phi)
    Jr = np.zeros(e.shape[:-1] + (6, 6))
    Jm = np.zeros_like(Jr)
    Jr[..., :3, :3] = -np.eye(3)
    Jr[..., :3, 3:] = hat(E[..., :3, 3])
    Jr[..., 3:, 3:] = -Ji @ np.swapaxes(RE, -1, -2)
    Jm[..., :3, :3] = RA
    Jm[..., :3, 3:] = -RA @ hat(tzi)
    Jm[..., 3:, 3:] = Ji @ np.swapaxes(Rzi, -1, -2)
    return e, half, Jr, Jm


def _sym(W):
    W = np.asarray(W, dtype=np.float64)
    return 0.5 * (W + np.swapaxes(W, -1, -2))


class Graph:
    """poses [n, 4, 4] (start; node 0's is the prior's origin), links ref -> mov with meas [m, 4, 4] and info [m, 6, 6] or None"""

    def __init__(self, poses, ref, mov, meas, info=None, truth=None):
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        self.ref = np.asarray(ref, dtype=np.int64).reshape(-1)
        self.mov = np.asarray(mov, dtype=np.int64).reshape(-1)
        self.meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 4, 4)
        self.info = None if info is None else np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6, 6)
        self.truth = truth

    @property
    def n_nodes(self):
        return self.poses.shape[0]

    @property
    def n_edges(self):
        return self.ref.shape[0]

    def W(self):
        return np.tile(100.0 * np.eye(6), (self.n_edges, 1, 1)) if self.info is None else _sym(self.info)


class _System:
    """the linearisation at T: cost, half, b = -gradient, and what a matrix-vector product needs"""

    def __init__(self, G, T, W, W0, assoc="left"):
        self.G, self.W, self.W0 = G, W, W0
        e, half, self.Jr, self.Jm = link_error(T[G.ref], T[G.mov], G.meas, assoc, jacobians=True)
        e0, half0, _, self.J0 = link_error(G.poses[0], T[0], np.eye(4), assoc, jacobians=True)
        self.half = bool(np.any(half) or half0)
        we = np.einsum("mab,mb->ma", W, e)
        self.cost = float(e0 @ W0 @ e0 + np.sum(e * we))
        g = np.zeros((T.shape[0], 6))
        np.add.at(g, G.ref, np.einsum("mba,mb->ma", self.Jr, we))
        np.add.at(g, G.mov, np.einsum("mba,mb->ma", self.Jm, we))
        g[0] += self.J0.T @ (W0 @ e0)
        self.b = -g
        self.H0 = self.J0.T @ W0 @ self.J0

    def blocks(self):
        WJr, WJm = self.W @ self.Jr, self.W @ self.Jm
        T = lambda A: np.swapaxes(A, -1, -2)
        return T(self.Jr) @ WJr, T(self.Jr) @ WJm, T(self.Jm) @ WJm

    def dense(self):
        n = self.b.shape[0]
        rr, rm, mm = self.blocks()
        H = np.zeros((n, n, 6, 6))
        np.add.at(H, (self.G.ref, self.G.ref), rr)
        np.add.at(H, (self.G.ref, self.G.mov), rm)
        np.add.at(H, (self.G.mov, self.G.ref), np.swapaxes(rm, -1, -2))
        np.add.at(H, (self.G.mov, self.G.mov), mm)
        H[0, 0] += self.H0
        return H.transpose(0, 2, 1, 3).reshape(6 * n, 6 * n)

    def diag_inverse(self):
        """the inverses of the 6x6 diagonal blocks, the identity where a block is not positive definite"""
        rr, _, mm = self.blocks()
        D = np.zeros((self.b.shape[0], 6, 6))
        np.add.at(D, self.G.ref, rr)
        np.add.at(D, self.G.mov, mm)
        D[0] += self.H0
        out = np.empty_like(D)
        for i in range(D.shape[0]):
            try:
                L = np.linalg.cholesky(D[i])
                Y = np.linalg.inv(L)
                out[i] = Y.T @ Y
            except np.linalg.LinAlgError:
                out[i] = np.eye(6)
        return out

    def matvec(self, p):
        u = np.einsum("mab,mb->ma", self.Jr, p[self.G.ref]) + np.einsum("mab,mb->ma", self.Jm, p[self.G.mov])
        t = np.einsum("mab,mb->ma", self.W, u)
        out = np.zeros_like(p)
        np.add.at(out, self.G.ref, np.einsum("mba,mb->ma", self.Jr, t))
        np.add.at(out, self.G.mov, np.einsum("mba,mb->ma", self.Jm, t))
        out[0] += self.H0 @ p[0]
        return out

    def pcg(self, eps_linear, max_linear_iterations):
        """the device's solve: from zero, preconditioned by the 6x6 diagonal blocks -> (x, iterations, capped)"""
        Dinv = self.diag_inverse()
        x = np.zeros_like(self.b)
        r = self.b.copy()
        z = np.einsum("nab,nb->na", Dinv, r)
        p = z.copy()
        rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
        tol2 = eps_linear * eps_linear * rr
        k = 0
        while rr > tol2:
            if k >= max_linear_iterations:
                return x, k, True
            ap = self.matvec(p)
            pap = float(np.sum(p * ap))
            if not pap > 0.0:
                break
            alpha = rz / pap
            x += alpha * p
            r -= alpha * ap
            z = np.einsum("nab,nb->na", Dinv, r)
            rz_new, rr = float(np.sum(r * z)), float(np.sum(r * r))
            p = z + (rz_new / rz) * p
            rz = rz_new
            k += 1
        return x, k, False


def optimize(G, solver="dense", assoc="left", prior_information=None, **params):
    """Gauss-Newton with the library's stop rule -> (poses [n, 4, 4], result dict with ndtgpu_pgo_result's fields)"""
    prm = dict(DEFAULTS)
    for k, v in params.items():
        if k not in prm:
            raise TypeError("unknown parameter %r" % k)
        prm[k] = v
    W0 = _sym(100.0 * np.eye(6) if prior_information is None else np.asarray(prior_information, dtype=np.float64).reshape(6, 6))
    W = G.W()
    T = G.poses.copy()
    res = dict(exit_code=CONVERGED, iterations=0, linear_iterations=0, max_step=0.0, n_nodes=G.n_nodes, n_edges=G.n_edges)
    with np.errstate(invalid="ignore"):
        S = _System(G, T, W, W0, assoc)
    res["cost_initial"] = res["cost_final"] = S.cost
    if S.half:
        res["exit_code"] = HALF_TURN
        return T, res
    if not np.isfinite(S.cost):
        res["exit_code"] = NOT_FINITE
        return T, res
    capped = False
    while True:
        if res["iterations"] >= prm["max_iterations"]:
            res["exit_code"] = MAX_ITERATIONS
            break
        if solver == "dense":
            x = np.linalg.solve(S.dense(), S.b.reshape(-1)).reshape(-1, 6)
        else:
            x, k, c = S.pcg(prm["eps_linear"], prm["max_linear_iterations"])
            res["linear_iterations"] += k
            capped = capped or c
        Q = retract(T, x)
        res["max_step"] = float(np.max(np.abs(x)))
        res["iterations"] += 1
        Sn = _System(G, Q, W, W0, assoc)
        if not np.isfinite(Sn.cost):
            res["exit_code"] = NOT_FINITE
            break
        T, S = Q, Sn
        res["cost_final"] = S.cost
        if res["max_step"] <= prm["eps_step"]:
            break
    if res["exit_code"] != NOT_FINITE and capped:
        res["exit_code"] = LINEAR_CAP
    return T, res


# ---- graphs -------------------------------------------------------------------------------------------------------------------

def _perturbed(truth, rng, d_t=0.2, d_r=0.1):
    """the start: every node but node 0 up to d_t m and d_r rad off in every component"""
    start = truth.copy()
    n = truth.shape[0] - 1
    d = np.concatenate([rng.uniform(-d_t, d_t, size=(n, 3)), rng.uniform(-d_r, d_r, size=(n, 3))], -1)
    start[1:] = retract(truth[1:], d)
    return start


def _measure(truth, ref, mov, rng=None, s_t=0.0, s_r=0.0):
    ref, mov = np.asarray(ref), np.asarray(mov)
    Z = inv_T(truth[ref]) @ truth[mov]
    if rng is not None:
        m = Z.shape[0]
        Z = retract(Z, np.concatenate([rng.normal(0.0, s_t, size=(m, 3)), rng.normal(0.0, s_r, size=(m, 3))], -1))
    return Z


def _rand_T(rng, t_max=10.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return make_T(exp_so3(axis * rng.uniform(0.0, 3.0)), rng.uniform(-t_max, t_max, size=3))


def residual_fixture(rng, angle, t_max=10.0):
    """(Ti, Tj, Z) with |t| <= t_max whose residual rotation Log R_E has the angle given"""
    Ti, Tj = _rand_T(rng, t_max), _rand_T(rng, t_max)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    E = make_T(exp_so3(axis * angle), rng.uniform(-1.0, 1.0, size=3))
    return Ti, Tj, inv_T(E) @ (inv_T(Ti) @ Tj)


def two_nodes():
    """one link: the closed form is T_1 = T_0 Z, cost 0"""
    origin = euler_T(0.7, -0.4, 1.1, 0.3, -0.2, 2.9)
    Z = euler_T(1.5, 0.3, -0.6, -0.4, 0.25, 0.6)
    start1 = retract(origin @ Z, np.array([0.2, -0.15, 0.1, 0.08, -0.1, 0.05]))
    return Graph(np.stack([origin, start1]), [0], [1], [Z]), origin @ Z


def chain(n=5):
    """a chain without a loop closure, set at its solution: it stays at cost 0"""
    truth = np.stack([euler_T(0.9 * i, 0.1 * i * i, 0.2 * i, 0.05 * i, -0.04 * i, 0.2 * i) for i in range(n)])
    ref, mov = np.arange(n - 1), np.arange(1, n)
    return Graph(truth, ref, mov, _measure(truth, ref, mov), truth=truth)


def helix_ring(n=8, seed=3):
    """a ring of n nodes that climbs 0.25 m a node and closes with one long link, whose measurement is off by (0.3, -0.2, 0.1) m and
    (0.1, -0.05, 0.15) rad: the residual is not zero"""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([euler_T(3.0 * math.cos(a[i]), 3.0 * math.sin(a[i]), 0.25 * i, -0.05 * i, 0.1, a[i] + np.pi / 2) for i in range(n)])
    ref, mov = np.arange(n), (np.arange(n) + 1) % n
    Z = _measure(truth, ref, mov)
    Z[-1] = retract(Z[-1], np.array([0.3, -0.2, 0.1, 0.1, -0.05, 0.15]))
    return Graph(_perturbed(truth, rng), ref, mov, Z, truth=truth)


def helix(n=40, turns=2, seed=4):
    """a helix of `turns` turns with odometry links and a loop closure from every node to the one a turn above, noisy"""
    rng = np.random.default_rng(seed)
    per = n // turns
    a = 2.0 * np.pi * np.arange(n) / per
    truth = np.stack([euler_T(4.0 * math.cos(a[i]), 4.0 * math.sin(a[i]), 0.1 * i, 0.1 * math.sin(a[i]), -0.08, a[i] + np.pi / 2) for i in range(n)])
    ref = np.concatenate([np.arange(n - 1), np.arange(n - per)])
    mov = np.concatenate([np.arange(1, n), np.arange(per, n)])
    return Graph(_perturbed(truth, rng), ref, mov, _measure(truth, ref, mov, rng, 0.02, 0.01), truth=truth)


def grid3d(levels=3, rows=14, cols=14, cell=0.5, seed=5):
    """the SE(2) grid world lifted to `levels` z-levels 1 m apart with roll and pitch of +-0.1: one lawn-mower trajectory through every
    level (588 nodes: more than the workgroup's 512 threads) with odometry links, loop closures to the row below, some diagonal ones
    and closures to the level below at every other cell (1524 links), noisy measurements"""
    rng = np.random.default_rng(seed)
    truth, idx = [], {}
    for l in range(levels):
        rs = range(rows) if l % 2 == 0 else range(rows - 1, -1, -1)
        for r in rs:
            fwd = (r + l * rows) % 2 == 0
            for c in (range(cols) if fwd else range(cols - 1, -1, -1)):
                idx[(l, r, c)] = len(truth)
                k = len(truth)
                truth.append(euler_T(cell * c, cell * r, 1.0 * l, 0.1 if k % 2 else -0.1, -0.1 if (k // 2) % 2 else 0.1, 0.0 if fwd else np.pi))
    truth = np.array(truth)
    n = truth.shape[0]
    ref, mov = list(range(n - 1)), list(range(1, n))
    for l in range(levels):
        for r in range(rows - 1):
            for c in range(cols):
                ref.append(idx[(l, r, c)]); mov.append(idx[(l, r + 1, c)])
                if c % 3 == 0 and c + 1 < cols:
                    ref.append(idx[(l, r + 1, c + 1)]); mov.append(idx[(l, r, c)])
        if l:
            for r in range(rows):
                for c in range(r % 2, cols, 2):
                    ref.append(idx[(l - 1, r, c)]); mov.append(idx[(l, r, c)])
    return Graph(_perturbed(truth, rng), ref, mov, _measure(truth, ref, mov, rng, 0.01, 0.005), truth=truth)


def random_graph(n, seed, per_link_info=False):
    """a wandering chain of n nodes with about n / 2 random loop closures, noisy; per_link_info: a random SPD W per link"""
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 4, 4))
    truth[0] = np.eye(4)
    for i in range(1, n):
        truth[i] = truth[i - 1] @ euler_T(rng.uniform(0.5, 1.0), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2),
                                          rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5))
    ref, mov = list(range(n - 1)), list(range(1, n))
    for _ in range(n // 2 if n > 2 else 0):
        a, b = rng.choice(n, size=2, replace=False)
        ref.append(int(a)); mov.append(int(b))
    Z = _measure(truth, ref, mov, rng, 0.02, 0.01)
    info = None
    if per_link_info:
        A = rng.normal(size=(len(ref), 6, 6))
        info = A @ np.swapaxes(A, -1, -2) * 15.0 + 20.0 * np.eye(6)
    return Graph(_perturbed(truth, rng), ref, mov, Z, info, truth=truth)


def batch_graphs(count=64, lo=2, hi=300, seed=11):
    """`count` graphs of different sizes lo .. hi (both included)"""
    rng = np.random.default_rng(seed)
    sizes = [lo, hi] + [int(s) for s in rng.integers(lo, hi + 1, size=count - 2)]
    return [random_graph(s, 1000 + k) for k, s in enumerate(sizes)]


def planar_graph(n=12, seed=6):
    """z = 0, yaw-only rotations, information block-diagonal between (x, y, rz) and (z, rx, ry): the optimum is planar"""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([euler_T(4.0 * math.cos(a[i]), 3.0 * math.sin(a[i]), 0.0, 0.0, 0.0, a[i] + 2.0) for i in range(n)])
    ref = np.concatenate([np.arange(n), [1, 3]])
    mov = np.concatenate([(np.arange(n) + 1) % n, [7, 10]])
    m = ref.shape[0]
    noise = np.zeros((m, 6))
    noise[:, [0, 1, 5]] = rng.normal(0.0, [0.03, 0.03, 0.02], size=(m, 3))
    Z = retract(inv_T(truth[ref]) @ truth[mov], noise)
    d = np.zeros((n - 1, 6))
    d[:, [0, 1, 5]] = rng.uniform(-1.0, 1.0, size=(n - 1, 3)) * [0.2, 0.2, 0.1]
    start = truth.copy()
    start[1:] = retract(truth[1:], d)
    info = np.zeros((m, 6, 6))
    P, Q = [0, 1, 5], [2, 3, 4]
    for e in range(m):
        A, B = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
        info[e][np.ix_(P, P)] = A @ A.T * 20.0 + 30.0 * np.eye(3)
        info[e][np.ix_(Q, Q)] = B @ B.T * 20.0 + 30.0 * np.eye(3)
    return Graph(start, ref, mov, Z, info, truth=truth)


def weighting_graphs():
    """the graphs of GPU test 4: the helix ring with its closing link given twice, and with that link at twice the information"""
    G = helix_ring()
    W = np.tile(100.0 * np.eye(6), (G.n_edges, 1, 1))
    twice = Graph(G.poses, np.append(G.ref, G.ref[-1]), np.append(G.mov, G.mov[-1]), np.concatenate([G.meas, G.meas[-1:]]))
    W2 = W.copy()
    W2[-1] *= 2.0
    return twice, Graph(G.poses, G.ref, G.mov, G.meas, W2), Graph(G.poses, G.ref, G.mov, G.meas, W)


def model_graphs():
    """every graph the GPU tests compare with the model, by name"""
    return {"helix_ring": helix_ring(), "grid3d": grid3d(), "doubled": weighting_graphs()[1], "weighted": random_graph(40, 10, per_link_info=True)}


# ---- ndt_pgo3_link_from_registration, in Python floats (IEEE double, one rounding per operation) -------------------------------

def inv_sym6(C):
    """ndt_pgo3_inv_sym6 -> (W [6][6] as lists, ok): Cholesky of the symmetric part, Y = L^-1, W = Y^T Y"""
    C = [float(v) for v in np.asarray(C, dtype=np.float64).reshape(36)]
    L = [[0.0] * 6 for _ in range(6)]
    Y = [[0.0] * 6 for _ in range(6)]
    W = [[0.0] * 6 for _ in range(6)]
    ok = True
    for j in range(6):
        d = C[7 * j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        ok = ok and d > 0.0
        l = math.sqrt(d if d > 0.0 else 1.0)
        L[j][j] = l
        for i in range(j + 1, 6):
            s = 0.5 * (C[6 * i + j] + C[6 * j + i])
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / l
    for j in range(6):
        Y[j][j] = 1.0 / L[j][j]
        for i in range(j + 1, 6):
            s = 0.0
            for k in range(j, i):
                s = s - L[i][k] * Y[k][j]
            Y[i][j] = s / L[i][i]
    for i in range(6):
        for j in range(i + 1):
            s = 0.0
            for k in range(i, 6):
                s = s + Y[k][i] * Y[k][j]
            W[i][j] = W[j][i] = s
            ok = ok and math.isfinite(s)
    return W, ok


def link_from_registration(T, cov36=None, flags=0):
    """-> (Z [4, 4], W [6, 6]) of one registered link: T 4x4, cov36 row-major 6x6"""
    Z = np.array(T, dtype=np.float64).reshape(4, 4).copy()
    if cov36 is None:
        return Z, 100.0 * np.eye(6)
    if not flags & (COV_SINGULAR | COV_POSE_UNCHANGED | COV_NOT_COMPUTED):
        W, ok = inv_sym6(cov36)
        if ok:
            return Z, np.array(W)
    return Z, 50.0 * np.eye(6)
