"""The NumPy model of the SE(3) pose-graph optimiser (tests/pgo3_model.py) held against what does not depend on it: central
differences for its Jacobians, the closed form of the smallest graph, SciPy's least squares on the same residuals, and -- the
floor of the GPU tests' tolerance -- itself with another linear solver and with the error associated the other way.

Measured here (CPU, NumPy double):
  Jacobians against central differences (h = 1e-6), worst |difference| / max(1, |J|): 3.4e-9, 2.5e-9, 2.5e-9, 2.1e-9 at residual
    rotations of 1e-9, 1e-4, 0.3 and 2.5 rad (allowed 1e-6; the differences' own rounding, 1e-16 |t| / h with |t| <= 10 m)
  model against scipy.optimize.least_squares (3-point Jacobian, xtol = ftol = gtol = 1e-15): helix_ring 8.0e-11, helix 3.4e-10
    (allowed 1e-7: SciPy's own stopping)
  floor: poses 1.02e-14 (weighted), cost 5.4e-15 (weighted) -> pgo3_model.PCG3_FLOOR = 1.1e-14, COST3_FLOOR = 5.5e-15"""
import numpy as np
import pytest

import pgo3_model as M


@pytest.mark.parametrize("angle", [1e-9, 1e-4, 0.3, 2.5])
def test_jacobians_against_central_differences(angle):
    """1: both branches of Jr^-1 (series below 0.01 rad) and of Log (|v| below 1e-8)"""
    rng = np.random.default_rng(int(angle * 1e9) % 1000 + 1)
    h, worst = 1e-6, 0.0
    for _ in range(20):
        Ti, Tj, Z = M.residual_fixture(rng, angle)
        e, half, Jr, Jm = M.link_error(Ti, Tj, Z, jacobians=True)
        assert not half and abs(np.linalg.norm(e[3:]) - angle) <= 1e-12 + 1e-9 * angle
        for J, which in ((Jr, 0), (Jm, 1)):
            num = np.zeros((6, 6))
            for q in range(6):
                d = np.zeros(6)
                d[q] = h
                ep = M.link_error(M.retract(Ti, d) if which == 0 else Ti, M.retract(Tj, d) if which == 1 else Tj, Z)[0]
                em = M.link_error(M.retract(Ti, -d) if which == 0 else Ti, M.retract(Tj, -d) if which == 1 else Tj, Z)[0]
                num[:, q] = (ep - em) / (2.0 * h)
            worst = max(worst, float(np.max(np.abs(num - J))) / max(1.0, float(np.max(np.abs(J)))))
    print("residual rotation %g rad: worst |central difference - analytic| / max(1, |J|) = %.3g (allowed 1e-6)" % (angle, worst))
    assert worst <= 1e-6


def test_log_exp_and_the_half_turn():
    rng = np.random.default_rng(2)
    for angle in (0.0, 1e-12, 1e-9, 5e-9, 2e-8, 1e-4, 1.0, 3.0, np.pi - 1e-6):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        phi, half = M.log_so3(M.exp_so3(axis * angle))
        assert not half and np.max(np.abs(phi - axis * angle)) <= 1e-9 * max(angle, 1e-9) + 1e-15, angle
    phi, half = M.log_so3(np.diag([1.0, -1.0, -1.0]))
    assert half and np.all(np.isnan(phi))
    # Jr^-1 inverts the right Jacobian: Log(Exp(phi) Exp(d)) = phi + Jr^-1 d to first order
    phi, d = np.array([0.4, -0.7, 0.2]), 1e-6 * np.array([0.3, 0.5, -0.8])
    lhs = M.log_so3(M.exp_so3(phi) @ M.exp_so3(d))[0]
    assert np.max(np.abs(lhs - phi - M.jr_inv(phi) @ d)) <= 1e-11


def test_closed_form():
    """2: two nodes and one link reach T_1 = T_0 Z"""
    G, want = M.two_nodes()
    for solver in ("dense", "pcg"):
        T, r = M.optimize(G, solver=solver)
        assert r["exit_code"] == M.CONVERGED and r["cost_final"] <= 1e-24 < r["cost_initial"]
        assert np.array_equal(T[0], G.poses[0])
        assert np.max(np.abs(T[1] - want)) <= 16 * np.spacing(np.max(np.abs(want)))


def _scipy_solution(G):
    from scipy.optimize import least_squares
    L = np.linalg.cholesky(G.W())                     # W = L L^T: r = L^T e has r.r = e^T W e
    L0 = np.linalg.cholesky(100.0 * np.eye(6))

    def residuals(x):
        T = M.retract(G.poses, x.reshape(-1, 6))
        e = M.link_error(T[G.ref], T[G.mov], G.meas)[0]
        e0 = M.link_error(G.poses[0], T[0], np.eye(4))[0]
        return np.concatenate([L0.T @ e0, np.einsum("mba,mb->ma", L, e).reshape(-1)])

    sol = least_squares(residuals, np.zeros(6 * G.n_nodes), jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, method="trf")
    return M.retract(G.poses, sol.x.reshape(-1, 6)), float(np.sum(sol.fun ** 2))


@pytest.mark.parametrize("name", ["helix_ring", "helix"])
def test_model_against_scipy(name):
    """3: the model's optimum is SciPy's, to SciPy's own stopping"""
    G = {"helix_ring": M.helix_ring, "helix": M.helix}[name]()
    T, r = M.optimize(G)
    Ts, cost = _scipy_solution(G)
    d = float(np.max(np.abs(T - Ts)))
    print("%s: model against SciPy: largest pose difference %.3g (allowed 1e-7), %d updates, cost %.9g (SciPy %.9g)"
          % (name, d, r["iterations"], r["cost_final"], cost))
    assert r["exit_code"] == M.CONVERGED and r["cost_final"] > 1e-3
    assert d <= 1e-7
    assert abs(cost - r["cost_final"]) <= 1e-9 * r["cost_final"]


def test_floor():
    """4: the floor of the GPU tests' tolerance: dense, conjugate gradients at the default eps_linear, dense with E associated the
    other way, on every graph the GPU tests compare with the model"""
    worst_pose, worst_cost = 0.0, 0.0
    for name, G in M.model_graphs().items():
        runs = [M.optimize(G), M.optimize(G, solver="pcg"), M.optimize(G, assoc="right")]
        its = [r["iterations"] for _, r in runs]
        assert all(r["exit_code"] == M.CONVERGED for _, r in runs) and len(set(its)) == 1, (name, its)
        last = runs[0][1]["max_step"]
        assert not (0.5e-8 <= last <= 2e-8), (name, last)      # (the stop is not a coin toss between the three runs)
        dp = max(float(np.max(np.abs(runs[0][0] - T))) for T, _ in runs[1:])
        dc = max(abs(runs[0][1]["cost_final"] - r["cost_final"]) / runs[0][1]["cost_final"] for _, r in runs[1:])
        print("%s: %d nodes, %d links, %d updates (%d inner iterations), last step %.3g, floor: poses %.3g, cost %.3g, largest coordinate %.3g"
              % (name, G.n_nodes, G.n_edges, its[0], runs[1][1]["linear_iterations"], last, dp, dc, float(np.max(np.abs(runs[0][0])))))
        worst_pose, worst_cost = max(worst_pose, dp), max(worst_cost, dc)
    print("floor: poses %.3g (PCG3_FLOOR %.3g), cost %.3g (COST3_FLOOR %.3g)" % (worst_pose, M.PCG3_FLOOR, worst_cost, M.COST3_FLOOR))
    assert worst_pose <= M.PCG3_FLOOR and worst_cost <= M.COST3_FLOOR
    assert M.PCG3_FLOOR <= 2.0 * worst_pose and M.COST3_FLOOR <= 2.0 * worst_cost      # (the constants are the measurement, not a cushion)


def test_exit_codes_of_the_model():
    G = M.helix_ring()
    assert M.optimize(G, max_iterations=1)[1]["exit_code"] == M.MAX_ITERATIONS
    assert M.optimize(M.grid3d(), solver="pcg", max_linear_iterations=3, max_iterations=2)[1]["exit_code"] == M.LINEAR_CAP
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1, 3] = np.nan
    T, r = M.optimize(bad)
    assert r["exit_code"] == M.NOT_FINITE and r["iterations"] == 0 and np.array_equal(T, G.poses)
    half = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    half.meas[2] = M.inv_T(M.make_T(np.diag([1.0, -1.0, -1.0]), [0.1, 0.0, 0.0])) @ (M.inv_T(G.poses[G.ref[2]]) @ G.poses[G.mov[2]])
    T, r = M.optimize(half)
    assert r["exit_code"] == M.HALF_TURN and r["iterations"] == 0 and np.array_equal(T, G.poses)


def test_planar_graph_stays_planar():
    G = M.planar_graph()
    T, r = M.optimize(G)
    assert r["exit_code"] == M.CONVERGED and r["cost_final"] > 1e-3
    assert np.max(np.abs(T[:, 2, 3])) <= 1e-12 and np.max(np.abs(T[:, 2, :3] - [0, 0, 1])) <= 1e-12
