"""NumPy model of the marginal covariances of the two pose-graph banks (include/ndtgpu.h: ndtgpu_pgo_marginals,
ndtgpu_pgo3_marginals, ndtgpu_pgo_relative_covariance, ndtgpu_pgo3_relative_covariance), on top of tests/pgo_model.py and
tests/pgo3_model.py, which it imports and leaves as they are.

H is the model's own linearisation (_System.dense()).  The yardstick of every test is numpy.linalg.inv(H); the device's way to a
column -- the optimiser's conjugate gradients on a unit vector -- is written out here as _System.pcg is (column_solve).

FLOORS: the tolerance of the GPU tests comes from this model alone (the rule of tests/test_gpu_pgo.py).  The floor of a graph is the
larger of (a) the model's column solves against the dense inverse and (b) the model's column solves against themselves on the
same graph with nodes and links relabelled by a seeded permutation (node 0 stays: the prior is its), so that every sum runs in
another order, which is the only way the device differs from the model.  Both are the largest entry difference of a queried block
(cov's raw block B and cross), relative to that block's largest entry, at the default parameters.  (b) is taken at the model's
optimised poses; (a) there and at three seeded copies of them with every number moved by at most one unit in its last place
(nudged), the largest of the four.  The GPU tests build their dense inverse at the DEVICE's poses, which are such a copy, and on
the small graphs, where the conjugate gradients end on the step that is exact in exact arithmetic, (a) is numpy.linalg.inv's own
error: some cond(H) * 2^-53, whose realisation moves by an order of magnitude with the last place of the poses (ring_wrap,
cond(H) 2.4e4: 4.9e-15 to 7.95e-14 over eleven such copies, 8.6e-15 at the optimum itself, while two column solves differ by
2.6e-15).  One sample of it is no floor.
tests/test_pgo_marginals_model.py::test_floors re-measures them and holds the constants below within a factor 2; the GPU tests
allow ten times the floor, the factor covering the device's summation order.  No number here comes from a device.
Measured (a / b):
  SE(2)  two_nodes 7.95e-16 / 0 (one node and one link to relabel), chain 8.29e-15 / 8.86e-16, ring_inconsistent 1.85e-14 / 1.56e-15,
         ring_wrap 7.95e-14 / 2.58e-15, weighted 3.07e-10 / 7.06e-14, random300 1.38e-10 / 3.75e-13, grid_world 1.19e-9 / 1.23e-10
  SE(3)  two_nodes 1.58e-15 / 0, chain 9.29e-13 / 5.26e-13, helix_ring 3.01e-14 / 2.08e-15, weighted 2.97e-10 / 8.16e-11,
         random300 2.89e-10 / 1.20e-10, grid3d 6.80e-10 / 3.68e-11
On the larger graphs (a) is what the stop rule's eps_linear = 1e-8 leaves.  The columns took 4 to 445 inner iterations (SE(3): 2
to 598), none near the cap of 2000."""
import functools
import math

import numpy as np

import pgo3_model as M3
import pgo_model as M2

DEFAULTS = dict(eps_linear=1e-8, max_linear_iterations=2000)
JITTER_SEEDS = (1, 2, 3)

FLOOR2 = {"two_nodes": 8.0e-16, "chain": 8.3e-15, "ring_inconsistent": 1.9e-14, "ring_wrap": 8.0e-14, "weighted": 3.1e-10,
          "random300": 1.4e-10, "grid_world": 1.2e-9}
FLOOR3 = {"two_nodes": 1.6e-15, "chain": 9.3e-13, "helix_ring": 3.0e-14, "weighted": 3.0e-10, "random300": 2.9e-10, "grid3d": 6.8e-10}


# ---- the graphs and queries the CPU and the GPU tests share ---------------------------------------------------------------------

def _every_node(G):
    q = np.arange(G.n_nodes)
    return q, (q + 1) % G.n_nodes


def _some(G, nodes):
    q = np.asarray(nodes)
    return q, (q + 1) % G.n_nodes


@functools.lru_cache(maxsize=None)
def graphs(dof):
    """{name: (graph, query nodes, other nodes)} of the bank with this dof: every node with other = the next node on the small
    graphs, a few nodes on the large ones"""
    if dof == 3:
        gw, r300 = M2.grid_world(), M2.random_graph(300, 8, per_link_info=True)
        small = {"two_nodes": M2.two_nodes()[0], "chain": M2.chain(5), "ring_inconsistent": M2.ring_inconsistent(8),
                 "ring_wrap": M2.ring_wrap(12), "weighted": M2.random_graph(40, 10, per_link_info=True)}
        out = {k: (G,) + _every_node(G) for k, G in small.items()}
        out["grid_world"] = (gw,) + _some(gw, [0, 1, 560, 1121])
        out["random300"] = (r300,) + _some(r300, [0, 1, 150, 299])
        return out
    g3, r300 = M3.grid3d(), M3.random_graph(300, 8, per_link_info=True)
    small = {"two_nodes": M3.two_nodes()[0], "chain": M3.chain(5), "helix_ring": M3.helix_ring(8),
             "weighted": M3.random_graph(40, 10, per_link_info=True)}
    out = {k: (G,) + _every_node(G) for k, G in small.items()}
    out["grid3d"] = (g3,) + _some(g3, [0, 587])
    out["random300"] = (r300,) + _some(r300, [0, 1, 150, 299])
    return out


def floors(dof):
    return FLOOR2 if dof == 3 else FLOOR3


# ---- the system, its dense inverse and the column solve -----------------------------------------------------------------------

def system(G, poses=None, prior_information=None):
    """the model's linearisation of G at `poses` (None: as set), prior None: 100 I"""
    if G.poses.ndim == 2:
        W0 = M2._sym(100.0 * np.eye(3) if prior_information is None else np.asarray(prior_information, dtype=np.float64).reshape(3, 3))
        return M2._System(G, np.array(G.poses if poses is None else poses, dtype=np.float64), G.W(), W0)
    W0 = M3._sym(100.0 * np.eye(6) if prior_information is None else np.asarray(prior_information, dtype=np.float64).reshape(6, 6))
    return M3._System(G, np.array(G.poses if poses is None else poses, dtype=np.float64), G.W(), W0)


def dense_inverse(S):
    """H^-1 as blocks [n, n, dof, dof]"""
    n, d = S.b.shape
    return np.linalg.inv(S.dense()).reshape(n, d, n, d).transpose(0, 2, 1, 3)


def column_solve(S, q, k, eps_linear=1e-8, max_linear_iterations=2000):
    """H x = e_(q,k) by the device's solve, written out as _System.pcg is: from zero, preconditioned with the inverses of the
    diagonal blocks -> (x [n, dof], iterations, capped)"""
    Dinv = S.diag_inverse()
    b = np.zeros_like(S.b)
    b[q, k] = 1.0
    x = np.zeros_like(b)
    r = b.copy()
    z = np.einsum("nab,nb->na", Dinv, r)
    p = z.copy()
    rz, rr = float(np.sum(r * z)), float(np.sum(r * r))
    tol2 = eps_linear * eps_linear * rr
    it = 0
    while rr > tol2:
        if it >= max_linear_iterations:
            return x, it, True
        ap = S.matvec(p)
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
        it += 1
    return x, it, False


def marginal(S, q, o=None, **params):
    """one query by column solves -> (B = raw (H^-1)[q, q], cross = raw (H^-1)[o, q] or None, iterations per column, capped columns)"""
    prm = dict(DEFAULTS, **params)
    d = S.b.shape[1]
    B, X, its, capped = np.zeros((d, d)), (None if o is None else np.zeros((d, d))), [], 0
    for k in range(d):
        x, it, c = column_solve(S, q, k, prm["eps_linear"], prm["max_linear_iterations"])
        B[:, k] = x[q]
        if o is not None:
            X[:, k] = x[o]
        its.append(it)
        capped += int(c)
    return B, X, its, capped


def cov_of(B):
    return 0.5 * (B + B.T)


def relabelled(G, seed):
    """G with nodes 1.. and links renamed by a seeded permutation -> (graph, new index of every old node)"""
    rng = np.random.default_rng(seed)
    new = np.concatenate([[0], 1 + rng.permutation(G.n_nodes - 1)])
    old = np.argsort(new)
    e = rng.permutation(G.n_edges)
    cls = M2.Graph if G.poses.ndim == 2 else M3.Graph
    return cls(G.poses[old], new[G.ref][e], new[G.mov][e], G.meas[e], None if G.info is None else G.info[e]), new


@functools.lru_cache(maxsize=None)
def optimised(dof, name):
    """the model's dense optimum of a graph of graphs(dof), computed once"""
    G = graphs(dof)[name][0]
    return (M2 if dof == 3 else M3).optimize(G)[0]


def block_diff(a, b):
    """the largest entry difference, relative to b's largest entry"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def nudged(P, seed):
    """P with every stored number moved by -1, 0 or +1 unit in its last place (a seeded draw): poses as good as P"""
    rng = np.random.default_rng(seed)
    Q = P + np.spacing(P) * rng.integers(-1, 2, size=P.shape)
    if P.ndim == 3:
        Q[:, 3, :] = P[:, 3, :]
    return Q


def measure_floor(dof, name, seed=17, nudges=JITTER_SEEDS):
    """(a, b, iterations seen) of the module's docstring for one graph"""
    G, qs, os_ = graphs(dof)[name]
    P = optimised(dof, name)
    S = system(G, P)
    Hi = dense_inverse(S)
    G2, new = relabelled(G, seed)
    S2 = system(G2, P[np.argsort(new)])
    a = b = 0.0
    its = []
    for q, o in zip(qs, os_):
        B, X, it, capped = marginal(S, int(q), int(o))
        B2, X2, _, _ = marginal(S2, int(new[q]), int(new[o]))
        assert capped == 0
        its += it
        a = max(a, block_diff(B, Hi[q, q]), block_diff(X, Hi[o, q]))
        b = max(b, block_diff(B2, B), block_diff(X2, X))
    for s in nudges:                                     # (a) again at poses a rounding away
        Sn = system(G, nudged(P, s))
        Hn = dense_inverse(Sn)
        for q, o in zip(qs, os_):
            B, X, _, _ = marginal(Sn, int(q), int(o))
            a = max(a, block_diff(B, Hn[q, q]), block_diff(X, Hn[o, q]))
    return a, b, its


# ---- the covariance of a link's error from the marginals of its two nodes -----------------------------------------------------

def _jsjt(J, Srr, Smm, Smr):
    """J S J^T, S = [[S_rr, S_mr^T], [S_mr, S_mm]], in Python floats in the order of ndt_pgo_jsjt (csrc/ndt_pgo_marginals.h): every
    sum from 0.0 in ascending index order"""
    n = len(J)
    S = [[0.0] * (2 * n) for _ in range(2 * n)]
    for r in range(n):
        for c in range(n):
            S[r][c] = float(Srr[r][c])
            S[n + r][n + c] = float(Smm[r][c])
            S[n + r][c] = float(Smr[r][c])
            S[c][n + r] = float(Smr[r][c])
    Mx = [[0.0] * (2 * n) for _ in range(n)]
    for i in range(n):
        for j in range(2 * n):
            s = 0.0
            for k in range(2 * n):
                s = s + J[i][k] * S[k][j]
            Mx[i][j] = s
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            s = 0.0
            for k in range(2 * n):
                s = s + Mx[i][k] * J[j][k]
            out[i, j] = s
    return out


def relative_covariance(pose_ref, pose_mov, cov_ref, cov_mov, cross):
    """SE(2), operation for operation as ndt_pgo_relative_covariance: cross = the block [mov, ref]"""
    pr, pm = [float(v) for v in pose_ref], [float(v) for v in pose_mov]
    c, s = math.cos(pr[2]), math.sin(pr[2])
    dx, dy = pm[0] - pr[0], pm[1] - pr[1]
    lx, ly = c * dx + s * dy, -s * dx + c * dy
    J = [[-c, -s, ly, c, s, 0.0], [s, -c, -lx, -s, c, 0.0], [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]]
    return _jsjt(J, np.asarray(cov_ref), np.asarray(cov_mov), np.asarray(cross))


def relative_covariance3(T_ref, T_mov, cov_ref, cov_mov, cross):
    """SE(3): the link Jacobians of pgo3_model.link_error at Z = T_ref^-1 T_mov"""
    Z = M3.inv_T(T_ref) @ T_mov
    _, _, Jr, Jm = M3.link_error(T_ref, T_mov, Z, jacobians=True)
    J = np.concatenate([Jr, Jm], axis=1)
    S = np.block([[np.asarray(cov_ref), np.asarray(cross).T], [np.asarray(cross), np.asarray(cov_mov)]])
    return J @ S @ J.T
