"""ndtgpu_pgo3_optimize_wide: the chip-wide form of the SE(3) pose-graph optimiser on the device (-m gpu) against the NumPy model
(tests/pgo3_model.py, dense solve), against the one-workgroup form, and against itself bit for bit.

Tolerance of "compare with the model": as in tests/test_gpu_pgo3.py, ten times the floor of the graph -- the largest entrywise
pose difference, and the relative difference of cost_final, between the model's dense run and its run with the restated
conjugate gradients.  The four graphs of pgo3_model.model_graphs() keep pgo3_model.TOL / COST_RTOL; the graphs on the tile's
edges and the hub graph have floors of their own (tests/pgo3_wide_graphs.py, measured on the CPU by
tests/test_pgo3_wide_model.py).  The two device forms are compared at twice a graph's tolerance: each sits within one tolerance
of the model.  Where two wide runs are compared the bits must match."""
import numpy as np
import pytest

import pgo3_model as M
import pgo3_wide_graphs as WG

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
    bank = N.PGO3(1, G.n_nodes, max(G.n_edges, 1))
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize_wide(0, check_every=check_every, **params)
    out = bank.poses(0)
    bank.close()
    return out


def pose_diff(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def same_result(a, b):
    """two result records bit for bit (NaN fields included)"""
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in set(a) | set(b))


def test_smallest_graphs(N):
    """1: two nodes and one link reach the closed form T_1 = T_0 Z; a five-node chain set at its solution stays at cost 0; one node
    without a link -- the link pass has one workgroup with nothing to do"""
    two, want = M.two_nodes()
    T2, r2 = wide(N, two)
    assert r2["exit_code"] == M.CONVERGED and (r2["n_nodes"], r2["n_edges"]) == (2, 1)
    assert pose_diff(T2[1], want) <= 16 * np.spacing(np.max(np.abs(want)))
    assert pose_diff(T2[0], two.poses[0]) <= 16 * np.spacing(np.max(np.abs(want)))      # (the prior holds node 0 where it was set)
    assert r2["cost_final"] <= 1e-24 < r2["cost_initial"]
    chain = M.chain(5)
    Tc, rc = wide(N, chain)
    assert rc["exit_code"] == M.CONVERGED and rc["cost_initial"] <= 1e-24 and rc["cost_final"] <= 1e-24
    assert pose_diff(Tc, chain.truth) <= 16 * np.spacing(np.max(np.abs(chain.truth))) and rc["max_step"] <= 1e-8
    one = M.Graph(M.euler_T(0.7, -0.4, 1.1, 0.3, -0.2, 2.9)[None], [], [], np.zeros((0, 4, 4)))
    T1, r1 = wide(N, one)
    assert r1["exit_code"] == M.CONVERGED and (r1["n_nodes"], r1["n_edges"]) == (1, 0) and np.array_equal(T1, one.poses)
    assert r1["cost_initial"] == 0.0 and r1["cost_final"] == 0.0 and r1["max_step"] == 0.0 and r1["linear_iterations"] == 0


@pytest.mark.parametrize("name", ["helix_ring", "grid3d", "doubled", "weighted", "random_255", "random_256", "random_257", "links_255",
                                  "links_256", "hub"])
def test_against_the_model(graphs, reference, alone, name):
    """2: exit code, the last step, cost_initial, and poses and cost within the graph's tolerance"""
    G, (Tm, rm), (T, r) = graphs[name], reference[name], alone[name]
    tol, cost_rtol = WG.tolerance(name)
    d, dc = pose_diff(T, Tm), abs(r["cost_final"] - rm["cost_final"]) / rm["cost_final"]
    print("%s: %d nodes (%d tiles), %d links (%d tiles with the prior), %d updates (model %d), %d inner iterations, exit %d, cost %.9g "
          "(model %.9g, relative difference %.3g, allowed %.3g), largest pose difference %.3g (allowed %.3g)"
          % (name, G.n_nodes, WG.tiles(G.n_nodes), G.n_edges, WG.link_tiles(G.n_edges), r["iterations"], rm["iterations"],
             r["linear_iterations"], r["exit_code"], r["cost_final"], rm["cost_final"], dc, cost_rtol, d, tol))
    assert r["exit_code"] == M.CONVERGED and (r["n_nodes"], r["n_edges"]) == (G.n_nodes, G.n_edges)
    assert r["max_step"] <= 1e-8 and r["iterations"] >= 1 and r["linear_iterations"] >= r["iterations"]
    assert abs(r["cost_initial"] - rm["cost_initial"]) <= 1e-12 * rm["cost_initial"]
    assert np.array_equal(T[:, 3], np.tile([0, 0, 0, 1.0], (G.n_nodes, 1)))
    assert d <= tol
    assert dc <= cost_rtol


@pytest.mark.parametrize("name", ["grid3d", "hub"])
def test_against_the_one_workgroup_form(N, graphs, alone, name):
    """3: both forms sit within one tolerance of the model, so within two of each other; the iteration counts need not match"""
    G = graphs[name]
    bank = N.PGO3(1, G.n_nodes, G.n_edges)
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize()
    T1, r1 = bank.poses(0)
    bank.close()
    T, r = alone[name]
    tol, cost_rtol = WG.tolerance(name)
    d, dc = pose_diff(T, T1), abs(r["cost_final"] - r1["cost_final"]) / r1["cost_final"]
    print("%s: wide %d updates / %d inner iterations, one workgroup %d / %d, largest pose difference %.3g (allowed %.3g), cost %.3g relative "
          "(allowed %.3g)" % (name, r["iterations"], r["linear_iterations"], r1["iterations"], r1["linear_iterations"], d, 2 * tol, dc, 2 * cost_rtol))
    assert r["exit_code"] == r1["exit_code"] == M.CONVERGED and r["cost_initial"] > 0
    assert d <= 2 * tol and dc <= 2 * cost_rtol


@pytest.mark.parametrize("name", ["grid3d", "random_257"])
def test_same_bits(N, graphs, alone, name):
    """4: the bits do not depend on check_every, the run, the bank's capacity, the slot or what the neighbours have just done"""
    G = graphs[name]
    T0, r0 = alone[name]
    for every in (1, 7, None):
        T, r = wide(N, G, check_every=every)
        assert np.array_equal(T, T0) and same_result(r, r0), (every, r, r0)
    bank = N.PGO3(5, 3000, 9000)
    other = graphs["random_255"]
    for with_neighbours in (False, True):
        bank.set_graph(3, G.poses, G.ref, G.mov, G.meas, G.info)
        if with_neighbours:
            for k in (2, 4):
                bank.set_graph(k, other.poses, other.ref, other.mov, other.meas, other.info)
            bank.optimize(first=2, count=1)
            bank.optimize(first=4, count=1)
        bank.optimize_wide(3, check_every=7 if with_neighbours else None)
        T, r = bank.poses(3)
        assert np.array_equal(T, T0) and same_result(r, r0), (with_neighbours, r, r0)
    bank.close()


def test_exit_codes(N, graphs, alone):
    """5: the caps, a cap below check_every (the launches enqueued past it do nothing), a NaN measurement and a half turn, each for
    its graph alone"""
    G = M.helix_ring()
    Tm, rm = M.optimize(G, max_iterations=1)
    T, r = wide(N, G, max_iterations=1)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 1 and r["max_step"] > 1e-3
    S = M._System(G, G.poses, G.W(), 100.0 * np.eye(6))                  # (the bound of tests/test_gpu_pgo3.py::test_exit_codes)
    bound = float(np.linalg.cond(S.dense())) * 1e-8 * rm["max_step"]
    print("one step: largest pose difference %.3g (bound %.3g), step %.6g (model %.6g)" % (pose_diff(T, Tm), bound, r["max_step"], rm["max_step"]))
    assert pose_diff(T, Tm) <= bound and abs(r["max_step"] - rm["max_step"]) <= bound
    T, r = wide(N, G, max_iterations=0)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 0 and r["linear_iterations"] == 0 and np.array_equal(T, G.poses)
    assert r["cost_final"] == r["cost_initial"] > 0
    T, r = wide(N, graphs["grid3d"], max_linear_iterations=3, max_iterations=4)      # (the default check_every is larger than the cap)
    assert N.pgo_wide_params().check_every > 3
    assert r["exit_code"] == M.LINEAR_CAP and r["iterations"] == 4 and r["linear_iterations"] == 12
    assert r["cost_final"] < r["cost_initial"]
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1, 3] = np.nan
    half = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())                  # (the half-turn graph of tests/test_gpu_pgo3.py)
    half.meas[2] = M.inv_T(M.make_T(np.diag([1.0, -1.0, -1.0]), [0.1, 0.0, 0.0])) @ (M.inv_T(G.poses[G.ref[2]]) @ G.poses[G.mov[2]])
    assert M.optimize(half)[1]["exit_code"] == M.HALF_TURN
    good = M.helix()
    Ta, ra = wide(N, good)
    bank = N.PGO3(3, good.n_nodes, good.n_edges)
    for k, g in enumerate((bad, half, good)):
        bank.set_graph(k, g.poses, g.ref, g.mov, g.meas, g.info)
    for k in range(3):
        bank.optimize_wide(k)                                            # (raises unless the call returns NDTGPU_OK)
    (Tb, rb), (Th, rh), (Tg, rg) = (bank.poses(k) for k in range(3))
    bank.close()
    assert rb["exit_code"] == M.NOT_FINITE and rb["iterations"] == 0 and np.array_equal(Tb, G.poses)
    assert not np.isfinite(rb["cost_initial"])
    assert rh["exit_code"] == M.HALF_TURN == N.PGO3_HALF_TURN == 4 and rh["iterations"] == 0 and np.array_equal(Th, G.poses)
    assert np.isnan(rh["cost_initial"])
    assert np.array_equal(Tg, Ta) and same_result(rg, ra) and rg["exit_code"] == M.CONVERGED


def test_the_handle_resources(N, graphs):
    """6: a new bank still counts 12 device buffers; the first wide call adds the per-tile sums and the control blocks; close()
    returns everything"""
    from ndt_feature_graph_amd.binding import live_resources
    G = graphs["helix_ring"]
    before = live_resources()
    bank = N.PGO3(3, 20, 40)
    created = live_resources()
    assert created[0] == before[0] + 12 and created[1] == before[1]
    bank.set_graph(1, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize(first=1, count=1)
    assert live_resources() == created
    bank.optimize_wide(1)
    first = live_resources()
    assert first[0] == created[0] + 2 and first[1] == created[1] + 1     # the per-tile sums, the control blocks; the pinned mirror
    bank.optimize_wide(1)
    assert live_resources() == first                                     # (allocated once, for the handle's capacity)
    bank.close()
    assert live_resources() == before
