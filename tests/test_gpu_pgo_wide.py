"""ndtgpu_pgo_optimize_wide: the chip-wide form of the pose-graph optimiser on the device (-m gpu) against the NumPy model
(tests/pgo_model.py, dense solve), against the one-workgroup form, and against itself bit for bit.

Tolerance of "compare with the model": as in tests/test_gpu_pgo.py, ten times the floor of the graph -- the largest pose
difference, and the relative difference of cost_final, between the model's dense run and its run with the restated conjugate
gradients.  The three graphs of pgo_model.model_graphs() keep pgo_model.TOL / COST_RTOL; the graphs on the tile's edges and the
hub graph have floors of their own (tests/pgo_wide_graphs.py, measured on the CPU by tests/test_pgo_wide_model.py).  The two
device forms are compared at twice a graph's tolerance: each sits within one tolerance of the model.  Where two wide runs are
compared the bits must match."""
import numpy as np
import pytest

import pgo_model as M
import pgo_wide_graphs as WG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def graphs():
    g = dict(M.model_graphs())
    g.update(WG.wide_graphs())
    return g


@pytest.fixture(scope="module")
def reference(graphs):
    """the model's dense run of every graph, computed once"""
    return {name: M.optimize(G) for name, G in graphs.items()}


@pytest.fixture(scope="module")
def alone(N, graphs):
    """every graph's wide run alone in a bank created for exactly its size, at the default check_every, computed once"""
    return {name: wide(N, G) for name, G in graphs.items()}


def wide(N, G, check_every=None, **params):
    bank = N.PGO(1, G.n_nodes, max(G.n_edges, 1))
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize_wide(0, check_every=check_every, **params)
    out = bank.poses(0)
    bank.close()
    return out


def pose_diff(a, b):
    d = np.asarray(a) - np.asarray(b)
    d[:, 2] = M.wrap(d[:, 2])
    return float(np.max(np.abs(d)))


def test_smallest_graphs(N):
    """1: one node without a link; two nodes and one link reach the closed form; a chain set at its solution stays at cost 0"""
    one = M.Graph([[0.7, -0.4, 2.9]], [], [], np.zeros((0, 3)))
    p, r = wide(N, one)
    assert r["exit_code"] == M.CONVERGED and (r["n_nodes"], r["n_edges"]) == (1, 0) and np.array_equal(p, one.poses)
    assert r["cost_initial"] == 0.0 and r["cost_final"] == 0.0 and r["max_step"] == 0.0 and r["linear_iterations"] == 0
    two, want = M.two_nodes()
    p2, r2 = wide(N, two)
    assert r2["exit_code"] == M.CONVERGED and (r2["n_nodes"], r2["n_edges"]) == (2, 1)
    assert np.array_equal(p2[0], two.poses[0])
    assert np.max(np.abs(p2[1] - want)) <= 16 * np.spacing(4.0)         # (either way to the closed form is a few roundings of numbers below 4)
    assert r2["cost_final"] <= 1e-24 < r2["cost_initial"]
    chain = M.chain(5)
    pc, rc = wide(N, chain)
    assert rc["exit_code"] == M.CONVERGED and rc["cost_initial"] <= 1e-24 and rc["cost_final"] <= 1e-24
    assert np.max(np.abs(pc - chain.truth)) <= 16 * np.spacing(4.0) and rc["max_step"] <= 1e-8


@pytest.mark.parametrize("name", ["ring_inconsistent", "ring_wrap", "grid_world", "random_255", "random_256", "random_257", "hub",
                                  "weighted_40"])
def test_against_the_model(graphs, reference, alone, name):
    """2: exit code, the last step, cost_initial, and poses and cost within the graph's tolerance"""
    G, (pm, rm), (p, r) = graphs[name], reference[name], alone[name]
    tol, cost_rtol = WG.tolerance(name)
    d, dc = pose_diff(p, pm), abs(r["cost_final"] - rm["cost_final"]) / rm["cost_final"]
    print("%s: %d nodes (%d tiles), %d links (%d tiles), %d updates (model %d), %d inner iterations, exit %d, cost %.9g (model %.9g, "
          "relative difference %.3g, allowed %.3g), largest pose difference %.3g (allowed %.3g)"
          % (name, G.n_nodes, WG.tiles(G.n_nodes), G.n_edges, WG.tiles(G.n_edges), r["iterations"], rm["iterations"], r["linear_iterations"],
             r["exit_code"], r["cost_final"], rm["cost_final"], dc, cost_rtol, d, tol))
    assert r["exit_code"] == M.CONVERGED and (r["n_nodes"], r["n_edges"]) == (G.n_nodes, G.n_edges)
    assert r["max_step"] <= 1e-8 and r["iterations"] >= 1 and r["linear_iterations"] >= r["iterations"]
    assert abs(r["cost_initial"] - rm["cost_initial"]) <= 1e-12 * rm["cost_initial"]
    assert np.all(p[:, 2] > -np.pi) and np.all(p[:, 2] <= np.pi)
    assert d <= tol
    assert dc <= cost_rtol


@pytest.mark.parametrize("name", ["grid_world", "hub"])
def test_against_the_one_workgroup_form(N, graphs, alone, name):
    """3: both forms sit within one tolerance of the model, so within two of each other; the iteration counts need not match"""
    G = graphs[name]
    bank = N.PGO(1, G.n_nodes, G.n_edges)
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize()
    p1, r1 = bank.poses(0)
    bank.close()
    p, r = alone[name]
    tol, cost_rtol = WG.tolerance(name)
    d, dc = pose_diff(p, p1), abs(r["cost_final"] - r1["cost_final"]) / r1["cost_final"]
    print("%s: wide %d updates / %d inner iterations, one workgroup %d / %d, largest pose difference %.3g (allowed %.3g), cost %.3g relative"
          % (name, r["iterations"], r["linear_iterations"], r1["iterations"], r1["linear_iterations"], d, 2 * tol, dc))
    assert r["exit_code"] == r1["exit_code"] == M.CONVERGED and r["cost_initial"] > 0
    assert d <= 2 * tol and dc <= 2 * cost_rtol


@pytest.mark.parametrize("name", ["grid_world", "random_257"])
def test_same_bits(N, graphs, alone, name):
    """4: the bits do not depend on check_every, the run, the bank's capacity, the slot or what the neighbours have just done"""
    G = graphs[name]
    p0, r0 = alone[name]
    for every in (1, 7, None):
        p, r = wide(N, G, check_every=every)
        assert np.array_equal(p, p0) and r == r0, (every, r, r0)
    bank = N.PGO(5, 3000, 9000)
    other = graphs["random_255"]
    for with_neighbours in (False, True):
        bank.set_graph(3, G.poses, G.ref, G.mov, G.meas, G.info)
        if with_neighbours:
            for k in (2, 4):
                bank.set_graph(k, other.poses, other.ref, other.mov, other.meas, other.info)
            bank.optimize(first=2, count=1)
            bank.optimize(first=4, count=1)
        bank.optimize_wide(3, check_every=7 if with_neighbours else None)
        p, r = bank.poses(3)
        assert np.array_equal(p, p0) and r == r0, (with_neighbours, r, r0)
    bank.close()


def test_exit_codes(N, graphs, alone):
    """5: the caps, a cap below check_every (the launches enqueued past it do nothing), a NaN measurement"""
    G = graphs["ring_inconsistent"]
    pm, rm = M.optimize(G, max_iterations=1)
    p, r = wide(N, G, max_iterations=1)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 1 and r["max_step"] > 1e-3
    S = M._System(G, G.poses, G.W(), 100.0 * np.eye(3))                  # (the bound of tests/test_gpu_pgo.py::test_exit_codes)
    bound = float(np.linalg.cond(S.dense())) * 1e-8 * rm["max_step"]
    assert pose_diff(p, pm) <= bound and abs(r["max_step"] - rm["max_step"]) <= bound
    p, r = wide(N, G, max_iterations=0)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 0 and r["linear_iterations"] == 0 and np.array_equal(p, G.poses)
    assert r["cost_final"] == r["cost_initial"] > 0
    big = graphs["grid_world"]
    p, r = wide(N, big, max_linear_iterations=3, max_iterations=4)       # (the default check_every is larger than the cap)
    assert N.pgo_wide_params().check_every > 3
    assert r["exit_code"] == M.LINEAR_CAP and r["iterations"] == 4 and r["linear_iterations"] == 12
    assert r["cost_final"] < r["cost_initial"]
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1] = np.nan
    good = graphs["ring_wrap"]
    bank = N.PGO(2, 12, 14)
    bank.set_graph(0, bad.poses, bad.ref, bad.mov, bad.meas)
    bank.set_graph(1, good.poses, good.ref, good.mov, good.meas)
    bank.optimize_wide(0)
    bank.optimize_wide(1)
    (pb, rb), (pg, rg) = bank.poses(0), bank.poses(1)
    bank.close()
    assert rb["exit_code"] == M.NOT_FINITE and rb["iterations"] == 0 and np.array_equal(pb, G.poses)
    assert not np.isfinite(rb["cost_initial"])
    assert np.array_equal(pg, alone["ring_wrap"][0]) and rg == alone["ring_wrap"][1] and rg["exit_code"] == M.CONVERGED


def test_the_gated_loop_and_the_handle_resources(N):
    """6: optimize_gated(wide=True) on the 30-node loop of the link gate's tests keeps the same links in every round as
    wide=False and ends at the same poses within twice the tolerance of the last round's graph (its floor measured here by the
    model, on the CPU); the wide form's buffers go with the handle"""
    import torch
    import linkgate_fixtures as F
    from ndt_feature_graph_amd.binding import live_resources
    g = F.loop_graph()
    n, k, m = len(g["start"]), len(g["incr_ref"]), len(g["ref"])
    cm = lambda T: np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4), (0, 2, 1))).reshape(-1, 16)
    T16_dev, score_dev, incr_dev = torch.tensor(cm(g["T"]), device="cuda"), torch.tensor(g["score"], device="cuda"), torch.tensor(cm(g["incr_T"]), device="cuda")
    before = live_resources()
    results = []
    for wide_form in (False, True):
        gate, bank = N.LinkGate(n, m), N.PGO(1, n, k + m)
        results.append(N.optimize_gated(bank, 0, gate, g["start"], g["incr_ref"], g["incr_mov"], incr_dev, g["ref"], g["mov"], T16_dev, score_dev,
                                        max_rounds=8, wide=wide_form))
        assert live_resources() != before
        gate.close()
        bank.close()
        assert live_resources() == before
    (rounds1, p1), (roundsw, pw) = results
    print("rounds kept: one workgroup %s, wide %s" % ([len(r) for r in rounds1], [len(r) for r in roundsw]))
    assert len(rounds1) == len(roundsw) >= 2 and all(np.array_equal(x, y) for x, y in zip(rounds1, roundsw))
    kept = rounds1[-1]
    assert 20 < kept.size < m
    links = np.concatenate([cm(g["incr_T"]), cm(g["T"])[kept]])
    last = M.Graph(g["start"], np.concatenate([g["incr_ref"], g["ref"][kept]]), np.concatenate([g["incr_mov"], g["mov"][kept]]),
                   np.array([M.link_from_registration(T)[0] for T in links]))
    floor = WG.measure_floor(last)[0]
    d = pose_diff(pw, p1)
    print("largest pose difference %.3g, the last graph's floor %.3g (allowed %.3g)" % (d, floor, 2 * 10 * floor))
    assert np.spacing(4.0) <= floor <= 1e-13                          # (a floor of a few units in the last place of a coordinate)
    assert d <= 2 * 10 * floor
