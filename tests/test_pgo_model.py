"""The NumPy model of the pose-graph optimiser (tests/pgo_model.py) checked on its own, on the CPU: analytic Jacobians against
central differences, the two-node closed form, convergence from the stated start on every graph the GPU tests use (a GPU
failure is never the generator's fault), and the floor of the GPU tests' tolerance: dense solve against restated conjugate
gradients."""
import math

import numpy as np
import pytest

import pgo_model as M


@pytest.fixture(scope="module")
def dense_runs():
    return {name: M.optimize(G) for name, G in M.model_graphs().items()}


def test_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(0)
    pi = rng.uniform(-3, 3, size=(50, 3))
    pj = rng.uniform(-3, 3, size=(50, 3))
    z = M.ominus(pj, pi) + rng.normal(0, 0.05, size=(50, 3))      # (errors small enough that the wrap is smooth around them)
    Jr, Jm = M.link_jacobians(pi, pj)
    h = 1e-6
    for a in range(3):
        d = np.zeros(3)
        d[a] = h
        fr = (M.link_error(pi + d, pj, z) - M.link_error(pi - d, pj, z)) / (2 * h)
        fm = (M.link_error(pi, pj + d, z) - M.link_error(pi, pj - d, z)) / (2 * h)
        assert np.max(np.abs(fr - Jr[:, :, a])) < 1e-8
        assert np.max(np.abs(fm - Jm[:, :, a])) < 1e-8


def test_two_nodes_reach_the_closed_form():
    G, want = M.two_nodes()
    for solver in ("dense", "pcg"):
        p, r = M.optimize(G, solver=solver)
        assert r["exit_code"] == M.CONVERGED
        assert np.max(np.abs(p[1] - want)) < 1e-12 and np.all(p[0] == G.poses[0])
        assert r["cost_final"] < 1e-20 < r["cost_initial"]


def test_chain_without_loop_closure_stays_at_cost_zero():
    G = M.chain()
    p, r = M.optimize(G)
    assert r["exit_code"] == M.CONVERGED and r["cost_final"] < 1e-24 and np.max(np.abs(p - G.truth)) < 1e-13


def test_model_converges_on_the_graphs_of_the_gpu_tests(dense_runs):
    for name, (p, r) in dense_runs.items():
        assert r["exit_code"] == M.CONVERGED and r["iterations"] <= 10, (name, r)
        assert r["cost_final"] < r["cost_initial"] and r["cost_final"] > 1e-3, (name, r)      # (a residual that is not zero)
    ring = M.ring_wrap()
    assert ring.truth[6, 2] > 3.1 and ring.poses[6, 2] < -3.0                  # (a node that starts across the cut)
    big = M.grid_world()
    assert big.n_nodes > 1024 and big.n_edges > 2 * 1024
    for G in M.batch_graphs() + [M.random_graph(40, 7, per_link_info=True)]:
        p, r = M.optimize(G)
        assert r["exit_code"] == M.CONVERGED and r["iterations"] <= 15, (G.n_nodes, r)
    sizes = [G.n_nodes for G in M.batch_graphs()]
    assert len(sizes) == 64 and min(sizes) == 2 and max(sizes) == 300 and len(set(sizes)) > 40


def test_pcg_floor(dense_runs):
    """the floor of the GPU tests' tolerance (pgo_model.PCG_FLOOR, COST_FLOOR): the constants are the measured values, up to
    the factor 2 that another BLAS' rounding may move numbers this close to the last place"""
    floor, cost_floor = 0.0, 0.0
    for name, G in M.model_graphs().items():
        pd, rd = dense_runs[name]
        pp, rp = M.optimize(G, solver="pcg")
        assert rp["exit_code"] == M.CONVERGED and rp["iterations"] == rd["iterations"] and rp["linear_iterations"] > 0
        d = pd - pp
        d[:, 2] = M.wrap(d[:, 2])
        floor = max(floor, float(np.max(np.abs(d))))
        cost_floor = max(cost_floor, abs(rd["cost_final"] - rp["cost_final"]) / rd["cost_final"])
        print("%s: %d nodes, %d links, %d updates, %d inner iterations, largest pose difference %.3g, cost %.3g relative"
              % (name, G.n_nodes, G.n_edges, rp["iterations"], rp["linear_iterations"], float(np.max(np.abs(d))),
                 abs(rd["cost_final"] - rp["cost_final"]) / rd["cost_final"]))
    assert M.PCG_FLOOR / 2 <= floor <= 2 * M.PCG_FLOOR, floor
    assert cost_floor <= 2 * M.COST_FLOOR, cost_floor
    assert M.TOL == 10 * M.PCG_FLOOR and M.COST_RTOL == 10 * M.COST_FLOOR


def test_iteration_cap_and_non_finite_input():
    G = M.ring_inconsistent()
    p1, r1 = M.optimize(G, max_iterations=1)
    assert r1["exit_code"] == M.MAX_ITERATIONS and r1["iterations"] == 1 and r1["max_step"] > 1e-3
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1] = np.nan
    p, r = M.optimize(bad)
    assert r["exit_code"] == M.NOT_FINITE and r["iterations"] == 0 and np.array_equal(p, G.poses)


def test_link_conversion_restatement():
    rng = np.random.default_rng(2)
    for x in np.concatenate([rng.uniform(-1, 1, 20000), [1.0, -1.0, 0.0, 0.5, -0.5, 1e-20, 0.9999999999]]):
        a, b = M.acos_fd(x), math.acos(x)
        assert abs(a - b) <= np.spacing(max(b, 1e-300)), x                 # (within one unit in the last place of libm's)
    T = np.eye(4)
    T[:2, :2] = [[math.cos(-2.5), -math.sin(-2.5)], [math.sin(-2.5), math.cos(-2.5)]]
    T[:2, 3] = [1.25, -0.5]
    cov = np.diag([0.01, 0.02, 1.0, 1.0, 1.0, 0.005])
    cov[0, 1] = cov[1, 0] = 0.004
    z, W = M.link_from_registration(T.T.reshape(16), cov.reshape(36), 0)
    assert abs(z[2] + 2.5) < 1e-15 and z[0] == 1.25 and z[1] == -0.5
    blk = cov[np.ix_([0, 1, 5], [0, 1, 5])]
    assert np.max(np.abs(W @ blk - np.eye(3))) < 1e-12
    for flags in (M.COV_SINGULAR, M.COV_POSE_UNCHANGED, M.COV_NOT_COMPUTED):
        _, Wf = M.link_from_registration(T.T.reshape(16), cov.reshape(36), flags)
        assert np.max(np.abs(Wf - 50.0 * np.eye(3))) < 1e-12
    _, Ws = M.link_from_registration(T.T.reshape(16), np.zeros(36), 0)      # a block that does not invert
    assert np.max(np.abs(Ws - 50.0 * np.eye(3))) < 1e-12
    _, Wn = M.link_from_registration(T.T.reshape(16), None, 0)
    assert np.array_equal(Wn, 100.0 * np.eye(3))
