"""ndtgpu_pgo3_*: batched SE(3) pose-graph optimisation on the device (-m gpu) against the NumPy model (tests/pgo3_model.py: dense
Gauss-Newton with numpy.linalg.solve on the same factor errors and the same stop rule).

Tolerance of "compare with the model".  It comes from the model alone: tests/test_pgo3_model.py::test_floor runs the model on the
graphs compared here three ways (dense; restated conjugate gradients at the default eps_linear; dense with the error associated
the other way).  The largest entrywise difference of the 4x4 poses between those runs is 1.02e-14 (pgo3_model.PCG3_FLOOR =
1.1e-14), the largest relative difference of cost_final 5.4e-15 (COST3_FLOOR = 5.5e-15).  The tests here allow ten times each
(TOL = 1.1e-13, COST_RTOL = 5.5e-14), the factor covering the device's summation order and its sincos / atan2.  Neither number is
derived from a device's output.  Where two device runs are compared the bits must match."""
import numpy as np
import pytest

import pgo3_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def reference():
    """the model's dense runs of the graphs compared with it, computed once"""
    return {name: (G,) + M.optimize(G) for name, G in M.model_graphs().items()}


def run(N, graphs, **params):
    """every graph in one bank and one call -> [(poses, result)]"""
    bank = N.PGO3(len(graphs), max(G.n_nodes for G in graphs), max(max(G.n_edges for G in graphs), 1))
    for k, G in enumerate(graphs):
        bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize(**params)
    out = [bank.poses(k) for k in range(len(graphs))]
    bank.close()
    return out


def pose_diff(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def same_result(a, b):
    """two result records bit for bit (NaN fields included)"""
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in set(a) | set(b))


def assert_agrees_with_model(name, T, r, Tm, rm, n_edges=None):
    d, dc = pose_diff(T, Tm), abs(r["cost_final"] - rm["cost_final"]) / rm["cost_final"]
    print("%s: %d updates (model %d), %d inner iterations, exit %d, cost %.9g (model %.9g, relative difference %.3g, allowed %.3g), "
          "largest pose difference %.3g (allowed %.3g)" % (name, r["iterations"], rm["iterations"], r["linear_iterations"], r["exit_code"],
                                                          r["cost_final"], rm["cost_final"], dc, M.COST_RTOL, d, M.TOL))
    assert r["exit_code"] == M.CONVERGED and r["n_nodes"] == rm["n_nodes"] and r["n_edges"] == (rm["n_edges"] if n_edges is None else n_edges)
    assert r["max_step"] <= 1e-8 and r["iterations"] == rm["iterations"] and r["linear_iterations"] >= r["iterations"]
    assert abs(r["cost_initial"] - rm["cost_initial"]) <= 1e-12 * rm["cost_initial"]
    assert d <= M.TOL
    assert dc <= M.COST_RTOL


def test_smallest_graphs(N):
    """1: two nodes and one link reach the closed form T_1 = T_0 Z; a five-node chain without a loop closure stays at cost 0"""
    two, want = M.two_nodes()
    chain = M.chain(5)
    (T2, r2), (Tc, rc) = run(N, [two, chain])
    assert r2["exit_code"] == M.CONVERGED and (r2["n_nodes"], r2["n_edges"]) == (2, 1)
    print("two nodes: |T_1 - T_0 Z| = %.3g, cost %.3g -> %.3g; chain: cost %.3g -> %.3g, |T - truth| = %.3g"
          % (pose_diff(T2[1], want), r2["cost_initial"], r2["cost_final"], rc["cost_initial"], rc["cost_final"], pose_diff(Tc, chain.truth)))
    assert pose_diff(T2[1], want) <= 16 * np.spacing(np.max(np.abs(want)))
    assert pose_diff(T2[0], two.poses[0]) <= 16 * np.spacing(np.max(np.abs(want)))      # (the prior holds node 0 where it was set)
    assert r2["cost_final"] <= 1e-24 < r2["cost_initial"]
    assert rc["exit_code"] == M.CONVERGED and rc["cost_initial"] <= 1e-24 and rc["cost_final"] <= 1e-24
    assert pose_diff(Tc, chain.truth) <= 16 * np.spacing(np.max(np.abs(chain.truth))) and rc["max_step"] <= 1e-8
    assert np.array_equal(T2[:, 3], np.tile([0, 0, 0, 1.0], (2, 1)))


def test_helix_ring_against_the_model(N, reference):
    """2: a ring of 8 nodes that climbs, with one inconsistent loop closure, start 0.2 m and 0.1 rad off"""
    G, Tm, rm = reference["helix_ring"]
    assert rm["cost_final"] > 0.1
    (T, r), = run(N, [G])
    assert_agrees_with_model("helix_ring", T, r, Tm, rm)


def test_strided_loops_against_the_model(N, reference):
    """3: more nodes and more links than the workgroup has threads (588 and 1524 against 512)"""
    G, Tm, rm = reference["grid3d"]
    assert G.n_nodes > 512 and G.n_edges > 1024
    (T, r), = run(N, [G])
    assert_agrees_with_model("grid3d", T, r, Tm, rm)


def test_weighting(N, reference):
    """4: a link twice = the link once at twice the information; per-link info36 agrees with the model; NULL = 100 I bit for bit"""
    twice, doubled, explicit = M.weighting_graphs()
    G = M.helix_ring()
    weighted = reference["weighted"][0]
    (Tt, rt), (Td, rd), (Te, re_), (Tn, rn), (Tw, rw) = run(N, [twice, doubled, explicit, G, weighted])
    # 100 e + 100 e against 200 e: the same problem, a rounding apart in every sum; both sit at TOL of the model of either
    _, Tm, rm = reference["doubled"]
    assert_agrees_with_model("link twice", Tt, rt, Tm, rm, n_edges=twice.n_edges)
    assert_agrees_with_model("twice the information", Td, rd, Tm, rm)
    assert np.array_equal(Te, Tn) and same_result(re_, rn)
    _, Tm, rm = reference["weighted"]
    assert_agrees_with_model("per-link information", Tw, rw, Tm, rm)


def test_planar_input_stays_planar(N):
    """5: z = 0, yaw-only rotations and information block-diagonal between (x, y, rz) and (z, rx, ry): planar poses come back"""
    G = M.planar_graph()
    (T, r), = run(N, [G])
    Tm, rm = M.optimize(G)
    R = T[:, :3, :3]
    yaw = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    Rz = np.stack([M.euler_T(0, 0, 0, 0, 0, a)[:3, :3] for a in yaw])
    print("planar: |z| %.3g, |R - Rz| %.3g, |R^T R - I| %.3g, against the model %.3g"
          % (np.max(np.abs(T[:, 2, 3])), np.max(np.abs(R - Rz)), np.max(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3))), pose_diff(T, Tm)))
    assert r["exit_code"] == M.CONVERGED and r["iterations"] == rm["iterations"] and r["cost_final"] > 1e-3
    assert np.max(np.abs(T[:, 2, 3])) <= 1e-12 and np.max(np.abs(R - Rz)) <= 1e-12
    assert np.max(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3))) <= 1e-12


def test_batch_independence(N):
    """6: 64 graphs of 2 to 300 nodes in one call, each alone, and with first / count cutting the range: the same bits"""
    graphs = M.batch_graphs()
    together = run(N, graphs)
    assert all(r["exit_code"] == M.CONVERGED for _, r in together)
    bank = N.PGO3(len(graphs), 300, max(G.n_edges for G in graphs))
    for cuts in ([(k, 1) for k in range(len(graphs))], [(0, 5), (5, 30), (35, 1), (36, 28)]):
        for k, G in enumerate(graphs):
            bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
        for first, count in cuts:
            bank.optimize(first=first, count=count)
        for k in range(len(graphs)):
            T, r = bank.poses(k)
            assert np.array_equal(T, together[k][0]), (cuts[0], k)
            assert same_result(r, together[k][1]), (cuts[0], k, r, together[k][1])
    bank.close()
    # a graph alone in a bank of another capacity as well
    k = 17
    (T, r), = run(N, [graphs[k]])
    assert np.array_equal(T, together[k][0]) and same_result(r, together[k][1])


def test_exit_codes(N):
    """7: the iteration cap returns the iterate after one step; a NaN measurement and a half turn are reported for their graphs alone;
    an inner solve that stops at its cap is reported"""
    G = M.helix_ring()
    Tm, rm = M.optimize(G, max_iterations=1)
    (T, r), = run(N, [G], max_iterations=1)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 1 and r["max_step"] > 1e-3
    # One Gauss-Newton step from the same start.  The device's solve stops at the relative residual eps_linear, which bounds its
    # distance from the dense solve by cond(H) * eps_linear * |step| (H and the step taken from the model).
    S = M._System(G, G.poses, G.W(), 100.0 * np.eye(6))
    bound = float(np.linalg.cond(S.dense())) * 1e-8 * rm["max_step"]
    print("one step: largest pose difference %.3g (bound %.3g), step %.6g (model %.6g)" % (pose_diff(T, Tm), bound, r["max_step"], rm["max_step"]))
    assert pose_diff(T, Tm) <= bound and abs(r["max_step"] - rm["max_step"]) <= bound
    # cost_final is the cost at the poses returned: the model's cost there, to the rounding of its terms
    at_T = M._System(G, T, G.W(), 100.0 * np.eye(6)).cost
    assert abs(r["cost_final"] - at_T) <= 1e-13 * at_T and r["cost_final"] < r["cost_initial"]
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1, 3] = np.nan
    half = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    half.meas[2] = M.inv_T(M.make_T(np.diag([1.0, -1.0, -1.0]), [0.1, 0.0, 0.0])) @ (M.inv_T(G.poses[G.ref[2]]) @ G.poses[G.mov[2]])
    assert M.optimize(half)[1]["exit_code"] == M.HALF_TURN
    good = M.helix()
    alone, = run(N, [good])
    (Ta, ra), (Tb, rb), (Th, rh), (Tc, rc) = run(N, [good, bad, half, good])             # (run raises unless the call returns NDTGPU_OK)
    assert rb["exit_code"] == M.NOT_FINITE and rb["iterations"] == 0 and np.array_equal(Tb, G.poses)
    assert not np.isfinite(rb["cost_initial"])
    assert rh["exit_code"] == M.HALF_TURN == N.PGO3_HALF_TURN and rh["iterations"] == 0 and np.array_equal(Th, G.poses)
    for T, r in ((Ta, ra), (Tc, rc)):
        assert np.array_equal(T, alone[0]) and same_result(r, alone[1]) and r["exit_code"] == M.CONVERGED
    # an inner solve that stops at its cap is reported, and the run still goes on
    (T, r), = run(N, [M.grid3d()], max_linear_iterations=3, max_iterations=4)
    assert r["exit_code"] == M.LINEAR_CAP and r["iterations"] == 4 and r["linear_iterations"] == 12
    assert r["cost_final"] < r["cost_initial"]


def test_device_links(N):
    """8: links straight from ndtgpu_register_batch_cov_device (16 scan pairs round a loop, registered in 6 DoF) against the same
    values read back, converted on the host (ndtgpu_pgo3_link_from_registration, which tests/test_pgo3_abi.py holds bit for bit
    against the model) and given to set_graph: the same bits.  Made-up flags, each of the three bits, and a zeroed cov36: 50 I."""
    import torch
    from ndt_feature_graph_amd import synth
    import pgo_model as M2
    dev = torch.device("cuda", 0)
    n = 16
    a = 2.0 * np.pi * np.arange(n) / n
    truth2 = np.stack([2.0 * np.cos(a), 1.5 * np.sin(a), M2.wrap(a + 2.0)], -1)
    truth = np.stack([M.euler_T(p[0], p[1], 0.0, 0.0, 0.0, p[2]) for p in truth2])
    scans = synth.scan_2d([1] * n, torch.tensor(truth2, dtype=torch.float64), 20000).to(dev)
    ref, mov = np.arange(n), (np.arange(n) + 1) % n
    rng = np.random.default_rng(8)
    guess = M2.ominus(truth2[mov], truth2[ref]) + rng.uniform(-0.05, 0.05, size=(n, 3))
    T16 = synth.pose2d_to_T(torch.tensor(guess)).transpose(1, 2).contiguous().reshape(n, 16).to(dev)
    res = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    cov = torch.zeros((n, 36), dtype=torch.float64, device=dev)
    flg = torch.zeros((n,), dtype=torch.int32, device=dev)
    reg = N.Registrar(0.5, [0, 0, 0], [100.0, 100.0, 1.0], pairs_per_batch=n, depth=1, max_cells=4096)
    reg.submit(scans[ref].contiguous(), scans[mov].contiguous(), T16, res, range_limit=30.0, covariance_mode=0, cov36_dev=cov,
               cov_flags_dev=flg)
    reg.sync()
    T_h = np.transpose(T16.cpu().numpy().reshape(n, 4, 4), (0, 2, 1))
    cov_h, flg_h = cov.cpu().numpy(), flg.cpu().numpy()
    Z_true = M.inv_T(truth[ref]) @ truth[mov]
    assert np.max(np.abs(T_h[:, :3, 3] - Z_true[:, :3, 3])) < 0.1
    assert np.count_nonzero(flg_h == 0) >= n - 2                        # (the registrations ran: real covariances are converted)
    start = M._perturbed(truth, rng)

    def both(cov_dev, flags_dev, cov_host, flags_host):
        bank = N.PGO3(2, n, n)
        bank.set_links_device(0, start, ref, mov, T16, cov_dev, flags_dev)
        conv = [N.pgo3_link_from_registration(T_h[k], None if cov_host is None else cov_host[k], 0 if flags_host is None else int(flags_host[k]))
                for k in range(n)]
        bank.set_graph(1, start, ref, mov, np.array([c[0] for c in conv]), np.array([c[1] for c in conv]))
        bank.optimize()
        (T0, r0), (T1, r1) = bank.poses(0), bank.poses(1)
        bank.close()
        assert np.array_equal(T0, T1) and same_result(r0, r1), (pose_diff(T0, T1), r0, r1)
        assert r0["exit_code"] == M.CONVERGED
        return T0, r0, conv

    T, r, conv = both(cov, flg, cov_h, flg_h)
    inverted = sum(1 for k in range(n) if not np.array_equal(conv[k][1], 50.0 * np.eye(6)))
    print("registered links: %d of %d carry the inverse of their own cov36 (the rest 50 I), cost %.6g -> %.6g in %d updates"
          % (inverted, n, r["cost_initial"], r["cost_final"], r["iterations"]))
    assert pose_diff(T[:, :2, 3], truth[:, :2, 3]) < 0.2
    # made-up flags, each of the three bits, and a zeroed cov36
    fake = flg_h.copy()
    fake[2], fake[5], fake[9] = M.COV_SINGULAR, M.COV_POSE_UNCHANGED, M.COV_NOT_COMPUTED
    cov_f = cov_h.copy()
    cov_f[12] = 0.0
    Tf, rf, conv_f = both(torch.tensor(cov_f, device=dev), torch.tensor(fake, device=dev), cov_f, fake)
    for k in (2, 5, 9, 12):
        assert np.array_equal(conv_f[k][1], 50.0 * np.eye(6))
    # no covariances: every link 100 I, the same bits as set_graph with info36 = NULL
    Tn, rn, _ = both(None, None, None, None)
    bank = N.PGO3(1, n, n)
    bank.set_graph(0, start, ref, mov, np.array([c[0] for c in conv]), None)
    bank.optimize()
    T1, r1 = bank.poses(0)
    bank.close()
    assert np.array_equal(Tn, T1) and same_result(rn, r1)


def test_poses_go_into_the_world_assembly(N):
    """9: poses() feeds assemble_world unchanged: four small node maps under the optimised poses of a four-node graph"""
    import world_model as W
    poses2 = list(W.PLANAR_POSES) + [(2.2, 1.1, -2.0)]
    src = N.MapSet(W.NODE_RES, [0, 0, 0], W.NODE_SIZE_M, n_maps=4, max_cells=4096)
    src.build(W.planar_scans(poses=poses2))
    truth = np.stack([W.pose2d(*p) for p in poses2])
    rng = np.random.default_rng(9)
    ref, mov = np.array([0, 1, 2, 3, 0]), np.array([1, 2, 3, 0, 2])
    G = M.Graph(M._perturbed(truth, rng, 0.1, 0.05), ref, mov, M._measure(truth, ref, mov))
    (T, r), = run(N, [G])
    assert r["exit_code"] == M.CONVERGED and pose_diff(T, truth) < 1e-6
    dst = N.MapSet(W.NODE_RES, [0, 0, 0], W.WORLD_SIZE_M, n_maps=1, max_cells=4096)
    res, = N.assemble_world(dst, 0, src, [[0, 1, 2, 3]], [T])
    mean, cov, idx, n = dst.export_cells(0)
    print("world of 4 nodes under the optimised poses: %d cells from %d contributions" % (res["n_cells"], res["n_contributions"]))
    assert res["n_nodes"] == 4 and res["n_cells"] > 0 and res["n_contributions"] >= res["n_cells"] and res["overflow"] == 0
    assert mean.shape[0] == res["n_cells"]
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))


def test_a_bank_leaves_no_resources_behind(N):
    from ndt_feature_graph_amd.binding import live_resources
    before = live_resources()
    bank = N.PGO3(3, 20, 40)
    during = live_resources()
    assert during[0] == before[0] + 12 and during[2] > before[2] and during[3] == before[3] + 1      # 12 device buffers, the fence, the stream
    bank.close()
    assert live_resources() == before
