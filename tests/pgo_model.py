"""NumPy restatement of the SE(2) pose-graph optimiser (include/ndtgpu.h, ndtgpu_pgo_*): the prior and link errors of
optimizeGraphUsingISAM (ndt_offline_mapper.h:40-107), Gauss-Newton with the library's stop rule, each linear system solved
densely (numpy.linalg.solve: the reference of the GPU tests) or by a restatement of the device's block-Jacobi preconditioned
conjugate gradients (the floor of the GPU tests' tolerance).  Also the graph generators the CPU and the GPU tests share, and
ndt_pgo_link_from_registration (csrc/ndt_pgo.h) restated operation for operation in Python floats, whose results the device's
are compared with bit for bit."""
import math
import struct

import numpy as np

CONVERGED, MAX_ITERATIONS, LINEAR_CAP, NOT_FINITE = 0, 1, 2, 3
DEFAULTS = dict(max_iterations=50, max_linear_iterations=2000, eps_step=1e-8, eps_linear=1e-8)
COV_SINGULAR, COV_POSE_UNCHANGED, COV_NOT_COMPUTED = 1, 2, 4

# The tolerance of "compare with the model" (tests/test_gpu_pgo.py).  PCG_FLOOR is the largest pose difference between the model
# with the dense solve and the model with the restated conjugate gradients at the default eps_linear, over the graphs of GPU
# tests 2 to 4, as tests/test_pgo_model.py::test_pcg_floor measures it: 3.55e-15 (m or rad) on the grid world -- two units in the
# last place of its largest coordinate, 16 m -- and 9.0e-16 on the rings.  Both runs stop at the same iterate: the last update is
# some 1e-9 long and the conjugate gradients are 1e-8 of that away from the dense solve, so rounding is all that is left.
# COST_FLOOR is the largest relative difference of cost_final between the same runs (8.9e-15, on ring_wrap).  The GPU tests allow
# ten times each floor; the factor covers the device's other summation order.  No number here comes from a device's output.
PCG_FLOOR = 3.6e-15
TOL = 10 * PCG_FLOOR
COST_FLOOR = 9e-15
COST_RTOL = 10 * COST_FLOOR


def wrap(t):
    """an angle (array) in (-pi, pi]"""
    t = np.asarray(t, dtype=np.float64)
    return t + 2.0 * np.pi * np.floor((np.pi - t) / (2.0 * np.pi))


def ominus(pj, pi):
    """p_mov ominus p_ref: the pose of mov in ref's frame"""
    c, s = np.cos(pi[..., 2]), np.sin(pi[..., 2])
    dx, dy = pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1]
    return np.stack([c * dx + s * dy, -s * dx + c * dy, wrap(pj[..., 2] - pi[..., 2])], axis=-1)


def oplus(pi, d):
    """p_ref oplus d: the pose whose ominus with p_ref is d"""
    c, s = np.cos(pi[..., 2]), np.sin(pi[..., 2])
    return np.stack([pi[..., 0] + c * d[..., 0] - s * d[..., 1], pi[..., 1] + s * d[..., 0] + c * d[..., 1],
                     wrap(pi[..., 2] + d[..., 2])], axis=-1)


def link_error(pi, pj, z):
    d = ominus(pj, pi) - z
    d[..., 2] = wrap(d[..., 2])
    return d


def link_jacobians(pi, pj):
    """(J_ref, J_mov) [m, 3, 3] of link_error, analytic"""
    c, s = np.cos(pi[..., 2]), np.sin(pi[..., 2])
    dx, dy = pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1]
    lx, ly = c * dx + s * dy, -s * dx + c * dy
    o, l = np.zeros_like(c), np.ones_like(c)
    Jr = np.stack([np.stack([-c, -s, ly], -1), np.stack([s, -c, -lx], -1), np.stack([o, o, -l], -1)], -2)
    Jm = np.stack([np.stack([c, s, o], -1), np.stack([-s, c, o], -1), np.stack([o, o, l], -1)], -2)
    return Jr, Jm


def _sym(W):
    W = np.asarray(W, dtype=np.float64)
    return 0.5 * (W + np.swapaxes(W, -1, -2))


class Graph:
    """poses [n, 3] (start; node 0's is the prior's origin), links ref -> mov with meas [m, 3] and info [m, 3, 3] or None"""

    def __init__(self, poses, ref, mov, meas, info=None, truth=None):
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        self.ref = np.asarray(ref, dtype=np.int64).reshape(-1)
        self.mov = np.asarray(mov, dtype=np.int64).reshape(-1)
        self.meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        self.info = None if info is None else np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 3, 3)
        self.truth = truth

    @property
    def n_nodes(self):
        return self.poses.shape[0]

    @property
    def n_edges(self):
        return self.ref.shape[0]

    def W(self):
        return np.tile(100.0 * np.eye(3), (self.n_edges, 1, 1)) if self.info is None else _sym(self.info)


class _System:
    """the linearisation at p: cost, b = -gradient, and what a matrix-vector product needs"""

    def __init__(self, G, p, W, W0):
        self.G, self.W, self.W0 = G, W, W0
        pi, pj = p[G.ref], p[G.mov]
        e = link_error(pi, pj, G.meas)
        self.Jr, self.Jm = link_jacobians(pi, pj)
        e0 = p[0] - G.poses[0]
        e0[2] = wrap(e0[2])
        we = np.einsum("mab,mb->ma", W, e)
        self.cost = float(e0 @ W0 @ e0 + np.sum(e * we))
        g = np.zeros_like(p)
        np.add.at(g, G.ref, np.einsum("mba,mb->ma", self.Jr, we))
        np.add.at(g, G.mov, np.einsum("mba,mb->ma", self.Jm, we))
        g[0] += W0 @ e0
        self.b = -g

    def blocks(self):
        WJr, WJm = self.W @ self.Jr, self.W @ self.Jm
        T = lambda A: np.swapaxes(A, -1, -2)
        return T(self.Jr) @ WJr, T(self.Jr) @ WJm, T(self.Jm) @ WJm

    def dense(self):
        n = self.b.shape[0]
        rr, rm, mm = self.blocks()
        H = np.zeros((n, n, 3, 3))
        np.add.at(H, (self.G.ref, self.G.ref), rr)
        np.add.at(H, (self.G.ref, self.G.mov), rm)
        np.add.at(H, (self.G.mov, self.G.ref), np.swapaxes(rm, -1, -2))
        np.add.at(H, (self.G.mov, self.G.mov), mm)
        H[0, 0] += self.W0
        return H.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)

    def diag_inverse(self):
        rr, _, mm = self.blocks()
        D = np.zeros((self.b.shape[0], 3, 3))
        np.add.at(D, self.G.ref, rr)
        np.add.at(D, self.G.mov, mm)
        D[0] += self.W0
        return np.linalg.inv(D)

    def matvec(self, p):
        u = np.einsum("mab,mb->ma", self.Jr, p[self.G.ref]) + np.einsum("mab,mb->ma", self.Jm, p[self.G.mov])
        t = np.einsum("mab,mb->ma", self.W, u)
        out = np.zeros_like(p)
        np.add.at(out, self.G.ref, np.einsum("mba,mb->ma", self.Jr, t))
        np.add.at(out, self.G.mov, np.einsum("mba,mb->ma", self.Jm, t))
        out[0] += self.W0 @ p[0]
        return out

    def pcg(self, eps_linear, max_linear_iterations):
        """the device's solve: from zero, preconditioned by the inverses of the 3x3 diagonal blocks -> (x, iterations, capped)"""
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


def optimize(G, solver="dense", prior_information=None, **params):
    """Gauss-Newton with the library's stop rule -> (poses [n, 3], result dict with ndtgpu_pgo_result's fields)"""
    prm = dict(DEFAULTS)
    for k, v in params.items():
        if k not in prm:
            raise TypeError("unknown parameter %r" % k)
        prm[k] = v
    W0 = _sym(100.0 * np.eye(3) if prior_information is None else np.asarray(prior_information, dtype=np.float64).reshape(3, 3))
    W = G.W()
    p = G.poses.copy()
    res = dict(exit_code=CONVERGED, iterations=0, linear_iterations=0, max_step=0.0, n_nodes=G.n_nodes, n_edges=G.n_edges)
    S = _System(G, p, W, W0)
    res["cost_initial"] = res["cost_final"] = S.cost
    if not np.isfinite(S.cost):
        res["exit_code"] = NOT_FINITE
        return p, res
    capped = False
    while True:
        if res["iterations"] >= prm["max_iterations"]:
            res["exit_code"] = MAX_ITERATIONS
            break
        if solver == "dense":
            x = np.linalg.solve(S.dense(), S.b.reshape(-1)).reshape(-1, 3)
        else:
            x, k, c = S.pcg(prm["eps_linear"], prm["max_linear_iterations"])
            res["linear_iterations"] += k
            capped = capped or c
        q = p + x
        q[:, 2] = wrap(q[:, 2])
        res["max_step"] = float(np.max(np.abs(x)))
        res["iterations"] += 1
        Sn = _System(G, q, W, W0)
        if not np.isfinite(Sn.cost):
            res["exit_code"] = NOT_FINITE
            break
        p, S = q, Sn
        res["cost_final"] = S.cost
        if res["max_step"] <= prm["eps_step"]:
            break
    if res["exit_code"] != NOT_FINITE and capped:
        res["exit_code"] = LINEAR_CAP
    return p, res


# ---- graphs -------------------------------------------------------------------------------------------------------------------

def _perturbed(truth, rng, d_xy=0.2, d_t=0.1):
    """the start: every node but node 0 up to d_xy m and d_t rad off"""
    start = truth.copy()
    start[1:, :2] += rng.uniform(-d_xy, d_xy, size=(truth.shape[0] - 1, 2))
    start[1:, 2] = wrap(start[1:, 2] + rng.uniform(-d_t, d_t, size=truth.shape[0] - 1))
    return start


def _measure(truth, ref, mov, rng=None, s_xy=0.0, s_t=0.0):
    z = ominus(truth[np.asarray(mov)], truth[np.asarray(ref)])
    if rng is not None:
        z[:, :2] += rng.normal(0.0, s_xy, size=(z.shape[0], 2))
        z[:, 2] = wrap(z[:, 2] + rng.normal(0.0, s_t, size=z.shape[0]))
    return z


def two_nodes():
    """one link: the closed form is p_1 = origin oplus z, cost 0"""
    origin = np.array([0.7, -0.4, 2.9])
    z = np.array([1.5, 0.3, 0.6])
    return Graph(np.stack([origin, origin + [1.2, 0.5, 0.3]]), [0], [1], [z]), oplus(origin, z)


def chain(n=5):
    """a chain without a loop closure, set at its solution: it stays at cost 0"""
    truth = np.stack([[0.9 * i, 0.1 * i * i, 0.2 * i] for i in range(n)])
    ref, mov = np.arange(n - 1), np.arange(1, n)
    return Graph(truth, ref, mov, _measure(truth, ref, mov), truth=truth)


def ring_inconsistent(n=8, seed=3):
    """a ring of n nodes whose closing link is off by (0.3 m, -0.2 m, 0.15 rad): the residual is not zero"""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([3.0 * np.cos(a), 3.0 * np.sin(a), wrap(a + np.pi / 2)], -1)
    ref, mov = np.arange(n), (np.arange(n) + 1) % n
    z = _measure(truth, ref, mov)
    z[-1] += [0.3, -0.2, 0.15]
    return Graph(_perturbed(truth, rng), ref, mov, z, truth=truth)


def ring_wrap(n=12, seed=4):
    """a ring whose yaws run once round the circle, node n / 2 at pi - 0.03: yaws, errors and updates cross +-pi.  The links to
    and from that node and one chord are measured across the cut, and the node starts on the other side of it."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([4.0 * np.cos(a), 4.0 * np.sin(a), wrap(a - 0.03)], -1)
    ref = np.concatenate([np.arange(n), [n // 2 - 1, 1]])
    mov = np.concatenate([(np.arange(n) + 1) % n, [n // 2 + 2, n - 2]])
    z = _measure(truth, ref, mov, rng, 0.02, 0.01)
    start = _perturbed(truth, rng)
    start[n // 2, 2] = wrap(truth[n // 2, 2] + 0.08)
    return Graph(start, ref, mov, z, truth=truth)


def grid_world(rows=33, cols=34, cell=0.5, seed=5):
    """a lawn-mower trajectory over a rows x cols grid of `cell` m (1122 nodes and 2561 links: more of each than a workgroup has
    threads) with odometry links, loop closures to the row below and some diagonal ones, noisy measurements.  The cell is 0.5 m, not
    more: the prior alone holds the graph's rotation about node 0, with a stiffness of 100 / sum r_i^2, so the optimum's
    sensitivity to rounding grows with the square of the extent while the floor (units in the last place of a coordinate) grows
    with the extent."""
    rng = np.random.default_rng(seed)
    truth, idx = [], {}
    for r in range(rows):
        cs = range(cols) if r % 2 == 0 else range(cols - 1, -1, -1)
        for c in cs:
            idx[(r, c)] = len(truth)
            truth.append([cell * c, cell * r, 0.0 if r % 2 == 0 else np.pi])
    truth = np.array(truth)
    ends = (truth[:, 0] == cell * (cols - 1)) & (truth[:, 2] == 0.0) | (truth[:, 0] == 0.0) & (truth[:, 2] != 0.0)
    truth[ends, 2] = np.pi / 2                                      # the turns face the next row
    n = truth.shape[0]
    ref, mov = list(range(n - 1)), list(range(1, n))
    for r in range(rows - 1):
        for c in range(cols):
            ref.append(idx[(r, c)]); mov.append(idx[(r + 1, c)])
            if c % 3 == 0 and c + 1 < cols:
                ref.append(idx[(r + 1, c + 1)]); mov.append(idx[(r, c)])
    z = _measure(truth, ref, mov, rng, 0.01, 0.005)
    return Graph(_perturbed(truth, rng), ref, mov, z, truth=truth)


def random_graph(n, seed, per_link_info=False):
    """a wandering chain of n nodes with about n / 2 random loop closures, noisy; per_link_info: a random SPD W per link"""
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 3))
    for i in range(1, n):
        truth[i] = oplus(truth[i - 1], np.array([rng.uniform(0.5, 1.0), rng.uniform(-0.1, 0.1), rng.uniform(-0.5, 0.5)]))
    ref, mov = list(range(n - 1)), list(range(1, n))
    for _ in range(n // 2 if n > 2 else 0):
        a, b = rng.choice(n, size=2, replace=False)
        ref.append(int(a)); mov.append(int(b))
    z = _measure(truth, ref, mov, rng, 0.02, 0.01)
    info = None
    if per_link_info:
        A = rng.normal(size=(len(ref), 3, 3))
        info = A @ np.swapaxes(A, -1, -2) * 30.0 + 20.0 * np.eye(3)
    return Graph(_perturbed(truth, rng), ref, mov, z, info, truth=truth)


def batch_graphs(count=64, lo=2, hi=300, seed=11):
    """`count` graphs of different sizes lo .. hi (both included)"""
    rng = np.random.default_rng(seed)
    sizes = [lo, hi] + [int(s) for s in rng.integers(lo, hi + 1, size=count - 2)]
    return [random_graph(s, 1000 + k) for k, s in enumerate(sizes)]


def model_graphs():
    """the graphs of GPU tests 2 to 4, by name"""
    return {"ring_inconsistent": ring_inconsistent(), "ring_wrap": ring_wrap(), "grid_world": grid_world()}


# ---- ndt_pgo_link_from_registration, in Python floats (IEEE double, one rounding per operation) -------------------------------

def acos_fd(x):
    """ndt_pgo_acos: fdlibm's rational approximation with +, -, *, / and sqrt alone"""
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
    pS0, pS1, pS2 = 1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01
    pS3, pS4, pS5 = -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05
    qS1, qS2, qS3, qS4 = -2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02
    x = float(x)
    if x >= 1.0:
        return 0.0
    if x <= -1.0:
        return pi + 2.0 * pio2_lo
    if x != x:
        return x
    P = lambda z: z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))))
    Q = lambda z: 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)))
    ax = abs(x)
    if ax < 0.5:
        if ax <= 6.938893903907228e-18:
            return pio2_hi + pio2_lo
        z = x * x
        r = P(z) / Q(z)
        return pio2_hi - (x - (pio2_lo - x * r))
    if x < 0.0:
        z = (1.0 + x) * 0.5
        p, q = P(z), Q(z)
        s = math.sqrt(z)
        r = p / q
        w = r * s - pio2_lo
        return pi - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", s))[0] & 0xFFFFFFFF00000000))[0]
    c = (z - df * df) / (s + df)
    r = P(z) / Q(z)
    w = r * s + c
    return 2.0 * (df + w)


def inv_sym3(a, b, c, d, e, f):
    """ndt_pgo_inv_sym3 -> (W6, ok)"""
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    with np.errstate(all="ignore"):
        W6 = [float(np.float64(v) / np.float64(det)) for v in (c00, c01, c02, c11, c12, c22)]
    ok = a > 0.0 and c22 > 0.0 and det > 0.0 and all(math.isfinite(v) for v in W6)
    return W6, ok


def link_from_registration(T16, cov36=None, flags=0):
    """-> (z [3], W [3, 3]) of one registered link: T16 column-major, cov36 row-major 6x6"""
    T16 = [float(v) for v in T16]
    angle = acos_fd(T16[0])
    z = np.array([T16[12], T16[13], angle if T16[1] > 0.0 else -angle])
    if cov36 is None:
        return z, 100.0 * np.eye(3)
    C = [float(v) for v in np.asarray(cov36, dtype=np.float64).reshape(36)]
    W6, ok = None, False
    if not flags & (COV_SINGULAR | COV_POSE_UNCHANGED | COV_NOT_COMPUTED):
        W6, ok = inv_sym3(C[0], 0.5 * (C[1] + C[6]), 0.5 * (C[5] + C[30]), C[7], 0.5 * (C[11] + C[31]), C[35])
    if not ok:
        W6, _ = inv_sym3(0.02, 0.0, 0.0, 0.02, 0.0, 0.02)
    return z, np.array([[W6[0], W6[1], W6[2]], [W6[1], W6[3], W6[4]], [W6[2], W6[4], W6[5]]])
