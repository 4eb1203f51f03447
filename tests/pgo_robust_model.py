"""NumPy restatement of the robust loop-closure weighting of the two pose-graph banks (include/ndtgpu.h, ndtgpu_pgo_optimize_robust /
ndtgpu_pgo3_optimize_robust): the weights of Huber, Cauchy and DCS restated operation for operation in Python floats (the device's
are compared with them bit for bit), their cost terms, and the iteratively re-weighted least squares on top of tests/pgo_model.py
and tests/pgo3_model.py -- their linearisation (_System), dense solve and restated conjugate gradients as they are, imported and
not edited.  Also the outlier graphs the CPU and the GPU tests share.

The rounds are the library's: weigh every link at the held poses with the information as set, W = w * W0; updates_per_round
Gauss-Newton updates with the models' stop rule; CONVERGED when that call took at most one update within eps_step, MAX_ROUNDS
after max_rounds, the inner LINEAR_CAP / NOT_FINITE / HALF_TURN passed through; one more weighing at the poses a graph ends with.
The models' optimize() starts from G.poses and takes the prior's origin from the same array, so a later round cannot be started
through it: _gauss_newton below is that function's loop from given poses, the origin staying G.poses[0].

Floors (tests/test_pgo_robust_model.py::test_floor, CPU only, no number from a device): the largest pose difference and the
largest relative difference of the final robust cost between the dense IRLS and the IRLS with the restated conjugate gradients,
over the outlier graphs of the GPU tests (floor_cases) and the three kinds.  Measured there: SE(2) poses 1.78e-15 (grid world 17 x 16,
whose largest coordinate is 8 m: two units in its last place; 1.33e-15 on the 9 x 10 one), cost 2.2e-16 (one unit in the last
place); SE(3) poses 2.2e-15 (Huber), cost 7.1e-16 (DCS).  Both runs take the same rounds and stop at the same iterate: the last
update is below 1e-8 and the conjugate gradients are 1e-8 of that away from the dense solve, so rounding is all that is left.  The
GPU tests allow ten times each floor, the project's factor for the device's other summation order."""
import math

import numpy as np

import pgo3_model
import pgo_model

HUBER, CAUCHY, DCS = 1, 2, 3
KINDS = {"huber": HUBER, "cauchy": CAUCHY, "dcs": DCS}
CONVERGED, MAX_ROUNDS, LINEAR_CAP, NOT_FINITE, HALF_TURN = 0, 1, 2, 3, 4
ROBUST_DEFAULTS = dict(kind=DCS, max_rounds=50, updates_per_round=1, min_index_gap=2, scale=1.0, inlier_weight=0.5)

ROBUST_FLOOR = 1.8e-15          # SE(2): poses (m or rad)
ROBUST_COST_FLOOR = 2.3e-16     # SE(2): relative robust cost
ROBUST3_FLOOR = 2.3e-15         # SE(3): entries of the 4x4 poses
ROBUST3_COST_FLOOR = 7.2e-16    # SE(3): relative robust cost
TOL, COST_RTOL = 10 * ROBUST_FLOOR, 10 * ROBUST_COST_FLOOR
TOL3, COST3_RTOL = 10 * ROBUST3_FLOOR, 10 * ROBUST3_COST_FLOOR


# ---- the weights, in Python floats (IEEE double, one rounding per operation): csrc/ndt_pgo_robust.h -----------------------------

def dcs_s(phi, chi2):
    """ndt_pgo_robust_dcs_s: min(1, 2 phi / (phi + chi2))"""
    d = phi + chi2
    s = (2.0 * phi) / d if d != 0.0 else math.copysign(math.inf, 2.0 * phi) * math.copysign(1.0, d)
    return s if s < 1.0 else 1.0


def weight(kind, scale, chi2):
    """ndt_pgo_robust_weight of one chi2"""
    kind, scale, chi2 = KINDS.get(kind, kind), float(scale), float(chi2)
    if chi2 != chi2:
        return chi2
    if kind == HUBER:
        if chi2 < 0.0:
            return math.nan
        r = math.sqrt(chi2)
        return 1.0 if r <= scale else scale / r
    if kind == CAUCHY:
        return 1.0 / (1.0 + chi2 / (scale * scale))
    s = dcs_s(scale, chi2)
    return s * s


def weights(kind, scale, chi2):
    """weight() over an array"""
    return np.array([weight(kind, scale, c) for c in np.asarray(chi2, dtype=np.float64).ravel()]).reshape(np.shape(chi2))


def rho(kind, scale, chi2):
    """the link's term of the robust cost"""
    kind, scale, chi2 = KINDS.get(kind, kind), float(scale), float(chi2)
    if kind == HUBER:
        r = math.sqrt(chi2)
        return chi2 if r <= scale else 2.0 * scale * r - scale * scale
    if kind == CAUCHY:
        return scale * scale * math.log(1.0 + chi2 / (scale * scale))
    s = dcs_s(scale, chi2)
    return s * s * chi2 + scale * (1.0 - s) * (1.0 - s)


def protected(G, min_index_gap=2):
    """the links that are never re-weighted"""
    return np.abs(G.mov - G.ref) < min_index_gap


# ---- the rounds ------------------------------------------------------------------------------------------------------------------

def _is2(mod):
    return mod is pgo_model


def link_chi2(mod, G, P, W0):
    """(chi2 [m] = e^T W0 e at the poses P, any half turn)"""
    if _is2(mod):
        e, half = mod.link_error(P[G.ref], P[G.mov], G.meas), False
    else:
        with np.errstate(invalid="ignore"):
            e, h = mod.link_error(P[G.ref], P[G.mov], G.meas)
        half = bool(np.any(h))
    return np.einsum("ma,mab,mb->m", e, W0, e), half


def weigh(mod, G, P, W0, kind, scale, min_index_gap, inlier_weight):
    """one weighing -> dict(chi2, weight, inlier, cost, chi2_sum, outliers, status)"""
    chi2, half = link_chi2(mod, G, P, W0)
    prot = protected(G, min_index_gap)
    w = np.where(prot, 1.0, weights(kind, scale, chi2))
    terms = [c if p else (rho(kind, scale, c) if np.isfinite(c) and c >= 0.0 else math.nan) for c, p in zip(chi2, prot)]
    inlier = w >= inlier_weight
    finite = bool(np.all(np.isfinite(chi2)) and np.all(np.isfinite(w)))
    return dict(chi2=chi2, weight=w, inlier=inlier, cost=float(np.sum(terms)), chi2_sum=float(np.sum(chi2)), outliers=int(np.sum(~inlier)),
                status=HALF_TURN if half else (CONVERGED if finite else NOT_FINITE))


def _gauss_newton(mod, G, P, W, W0, prm, solver):
    """the loop of mod.optimize from the poses P with the information W; the prior's origin stays G.poses[0]"""
    two = _is2(mod)
    res = dict(exit_code=mod.CONVERGED, iterations=0, linear_iterations=0, max_step=0.0)
    with np.errstate(invalid="ignore"):
        S = mod._System(G, P, W, W0)
    if not two and S.half:
        res["exit_code"] = mod.HALF_TURN
        return P, res
    if not np.isfinite(S.cost):
        res["exit_code"] = mod.NOT_FINITE
        return P, res
    capped = False
    while True:
        if res["iterations"] >= prm["max_iterations"]:
            res["exit_code"] = mod.MAX_ITERATIONS
            break
        if solver == "dense":
            x = np.linalg.solve(S.dense(), S.b.reshape(-1)).reshape(S.b.shape)
        else:
            x, k, c = S.pcg(prm["eps_linear"], prm["max_linear_iterations"])
            res["linear_iterations"] += k
            capped = capped or c
        if two:
            Q = P + x
            Q[:, 2] = mod.wrap(Q[:, 2])
        else:
            Q = mod.retract(P, x)
        res["max_step"] = float(np.max(np.abs(x)))
        res["iterations"] += 1
        Sn = mod._System(G, Q, W, W0)
        if not np.isfinite(Sn.cost):
            res["exit_code"] = mod.NOT_FINITE
            break
        P, S = Q, Sn
        if res["max_step"] <= prm["eps_step"]:
            break
    if res["exit_code"] != mod.NOT_FINITE and capped:
        res["exit_code"] = mod.LINEAR_CAP
    return P, res


def irls(mod, G, solver="dense", prior_information=None, robust=None, **params):
    """the robust optimisation of graph G of model `mod` (pgo_model or pgo3_model) -> (poses, out) with out = the last weighing's
    dict, the weighted information W, and result = ndtgpu_pgo_robust_result's fields"""
    rp = dict(ROBUST_DEFAULTS)
    rp.update(robust or {})
    rp["kind"] = KINDS.get(rp["kind"], rp["kind"])
    prm = dict(mod.DEFAULTS)
    prm.update(params)
    prm["max_iterations"] = rp["updates_per_round"]
    d = 3 if _is2(mod) else 6
    Wp = mod._sym(100.0 * np.eye(d) if prior_information is None else np.asarray(prior_information, dtype=np.float64).reshape(d, d))
    W0 = G.W()
    P = G.poses.copy()
    args = (rp["kind"], rp["scale"], rp["min_index_gap"], rp["inlier_weight"])
    out = weigh(mod, G, P, W0, *args)
    res = dict(exit_code=MAX_ROUNDS, rounds=0, updates=0, linear_iterations=0, cost_initial=out["cost"])
    go = out["status"] == CONVERGED and rp["max_rounds"] > 0
    if out["status"] != CONVERGED:
        res["exit_code"] = out["status"]
    while go:
        W = out["weight"][:, None, None] * W0
        P, r = _gauss_newton(mod, G, P, W, Wp, prm, solver)
        res["rounds"] += 1
        res["updates"] += r["iterations"]
        res["linear_iterations"] += r["linear_iterations"]
        stop = True
        if r["exit_code"] in (LINEAR_CAP, NOT_FINITE, HALF_TURN):
            res["exit_code"] = r["exit_code"]
        elif r["iterations"] <= 1 and r["max_step"] <= prm["eps_step"]:
            res["exit_code"] = CONVERGED
        elif res["rounds"] >= rp["max_rounds"]:
            res["exit_code"] = MAX_ROUNDS
        else:
            stop = False
        out = weigh(mod, G, P, W0, *args)
        if out["status"] != CONVERGED:
            if not stop or res["exit_code"] in (CONVERGED, MAX_ROUNDS):
                res["exit_code"] = out["status"]
            stop = True
        go = not stop
    res.update(cost_final=out["cost"], chi2_final=out["chi2_sum"], outliers=out["outliers"])
    out = dict(out, result=res, W=out["weight"][:, None, None] * W0)
    return P, out


# ---- the outlier graphs ------------------------------------------------------------------------------------------------------------

def _false_pairs(positions, n_false, rng, min_gap=2, min_dist=2.0):
    pairs = []
    n = positions.shape[0]
    while len(pairs) < n_false:
        a, b = (int(v) for v in rng.integers(0, n, size=2))
        if abs(a - b) < min_gap or np.linalg.norm(positions[a] - positions[b]) < min_dist:
            continue
        pairs.append((a, b))
    return pairs


def outlier_graph(rows=9, cols=10, n_false=6, seed=77):
    """pgo_model.grid_world(rows, cols) and the same graph with n_false false closures behind its links: pairs of nodes at least 2
    apart in index and 2 m apart in truth, measured uniformly in +-0.5 m / +-0.5 m / +-0.3 rad -> (clean, dirty, false mask)"""
    G = pgo_model.grid_world(rows, cols)
    rng = np.random.default_rng(seed)
    pairs = _false_pairs(G.truth[:, :2], n_false, rng)
    z = rng.uniform(-1.0, 1.0, size=(n_false, 3)) * [0.5, 0.5, 0.3]
    ref = np.concatenate([G.ref, [a for a, _ in pairs]])
    mov = np.concatenate([G.mov, [b for _, b in pairs]])
    dirty = pgo_model.Graph(G.poses, ref, mov, np.concatenate([G.meas, z]), truth=G.truth)
    return G, dirty, np.arange(dirty.n_edges) >= G.n_edges


def outlier_graph3(levels=2, rows=6, cols=7, n_false=6, seed=78):
    """the same for pgo3_model.grid3d(levels, rows, cols): the false closures measure +-0.5 m in x, y, z and +-0.3 rad in roll,
    pitch and yaw"""
    G = pgo3_model.grid3d(levels, rows, cols)
    rng = np.random.default_rng(seed)
    pairs = _false_pairs(G.truth[:, :3, 3], n_false, rng)
    u = rng.uniform(-1.0, 1.0, size=(n_false, 6)) * [0.5, 0.5, 0.5, 0.3, 0.3, 0.3]
    Z = np.stack([pgo3_model.euler_T(*row) for row in u])
    ref = np.concatenate([G.ref, [a for a, _ in pairs]])
    mov = np.concatenate([G.mov, [b for _, b in pairs]])
    dirty = pgo3_model.Graph(G.poses, ref, mov, np.concatenate([G.meas, Z]), truth=G.truth)
    return G, dirty, np.arange(dirty.n_edges) >= G.n_edges


def distance(mod, P, Q):
    """the largest distance between corresponding node positions (m)"""
    if _is2(mod):
        return float(np.max(np.linalg.norm(P[:, :2] - Q[:, :2], axis=1)))
    return float(np.max(np.linalg.norm(P[:, :3, 3] - Q[:, :3, 3], axis=1)))


def floor_cases():
    """(name, model, generator arguments, kinds) of the outlier graphs the GPU tests compare with the model"""
    return [("grid9x10", pgo_model, outlier_graph, (9, 10, 6), ("dcs", "cauchy", "huber")),
            ("grid17x16", pgo_model, outlier_graph, (17, 16, 12), ("dcs", "cauchy", "huber")),
            ("grid3d", pgo3_model, outlier_graph3, (2, 6, 7, 6), ("dcs", "cauchy", "huber"))]


def edge_graph(mod, n_edges):
    """a graph of model `mod` with exactly n_edges links, a random SPD information each: one link is two_nodes(); otherwise
    random_graph's chain of n nodes with as many of its loop closures as make n_edges (n - 1 <= n_edges <= n - 1 + n // 2)"""
    if n_edges == 1:
        G = mod.two_nodes()[0]
        d = 3 if _is2(mod) else 6
        A = np.random.default_rng(1).normal(size=(1, d, d))
        return mod.Graph(G.poses, G.ref, G.mov, G.meas, A @ np.swapaxes(A, -1, -2) * 20.0 + 20.0 * np.eye(d))
    n = (2 * n_edges + 4) // 3
    G = mod.random_graph(n, 100 + n_edges, per_link_info=True)
    assert n - 1 <= n_edges <= G.n_edges
    return mod.Graph(G.poses, G.ref[:n_edges], G.mov[:n_edges], G.meas[:n_edges], G.info[:n_edges], truth=G.truth)
