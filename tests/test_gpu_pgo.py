"""ndtgpu_pgo_*: batched SE(2) pose-graph optimisation on the device (-m gpu) against the NumPy model (tests/pgo_model.py: dense
Gauss-Newton with numpy.linalg.solve on the same factor errors and the same stop rule).

Tolerance of "compare with the model".  The device and the model both stop at eps_step but solve their linear systems
differently, so the tolerance comes from the model alone: tests/test_pgo_model.py::test_pcg_floor runs the model on the graphs of
tests 2 to 4 once with the dense solve and once with a NumPy restatement of the device's block-Jacobi conjugate gradients at the
default eps_linear.  The largest pose difference between the two runs -- the floor -- is 3.55e-15 (m or rad; on the grid world,
two units in the last place of its largest coordinate; 9.0e-16 on the rings), kept as pgo_model.PCG_FLOOR = 3.6e-15.  The tests
here allow ten times the floor, TOL = 3.6e-14, the factor covering the device's other summation order.  cost_final is held the
same way: the largest relative difference between the two model runs is 8.9e-15 (COST_FLOOR = 9e-15), allowed COST_RTOL = 9e-14.
Neither number is derived from a device's output.  Where two device runs are compared the bits must match."""
import numpy as np
import pytest

import pgo_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def reference():
    """the model's dense runs of the graphs of tests 2 to 4, computed once"""
    return {name: (G,) + M.optimize(G) for name, G in M.model_graphs().items()}


def run(N, graphs, **params):
    """every graph in one bank and one call -> [(poses, result)]"""
    bank = N.PGO(len(graphs), max(G.n_nodes for G in graphs), max(max(G.n_edges for G in graphs), 1))
    for k, G in enumerate(graphs):
        bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize(**params)
    out = [bank.poses(k) for k in range(len(graphs))]
    bank.close()
    return out


def pose_diff(a, b):
    d = np.asarray(a) - np.asarray(b)
    d[:, 2] = M.wrap(d[:, 2])
    return float(np.max(np.abs(d)))


def assert_agrees_with_model(name, p, r, pm, rm, n_edges=None):
    d, dc = pose_diff(p, pm), abs(r["cost_final"] - rm["cost_final"]) / rm["cost_final"]
    print("%s: %d updates (model %d), %d inner iterations, exit %d, cost %.9g (model %.9g, relative difference %.3g), largest pose "
          "difference %.3g (allowed %.3g)" % (name, r["iterations"], rm["iterations"], r["linear_iterations"], r["exit_code"],
                                              r["cost_final"], rm["cost_final"], dc, d, M.TOL))
    assert r["exit_code"] == M.CONVERGED and r["n_nodes"] == rm["n_nodes"] and r["n_edges"] == (rm["n_edges"] if n_edges is None else n_edges)
    assert r["max_step"] <= 1e-8 and r["iterations"] >= 1 and r["linear_iterations"] >= r["iterations"]
    assert abs(r["cost_initial"] - rm["cost_initial"]) <= 1e-12 * rm["cost_initial"]
    assert d <= M.TOL
    assert dc <= M.COST_RTOL


def test_smallest_graphs(N):
    """1: two nodes and one link reach the closed form; a five-node chain without a loop closure stays at cost 0"""
    two, want = M.two_nodes()
    chain = M.chain(5)
    (p2, r2), (pc, rc) = run(N, [two, chain])
    assert r2["exit_code"] == M.CONVERGED and (r2["n_nodes"], r2["n_edges"]) == (2, 1)
    assert np.array_equal(p2[0], two.poses[0])
    assert np.max(np.abs(p2[1] - want)) <= 16 * np.spacing(4.0)         # (either way to the closed form is a few roundings of numbers below 4)
    assert r2["cost_final"] <= 1e-24 < r2["cost_initial"]
    assert rc["exit_code"] == M.CONVERGED and rc["cost_initial"] <= 1e-24 and rc["cost_final"] <= 1e-24
    assert np.max(np.abs(pc - chain.truth)) <= 16 * np.spacing(4.0) and rc["max_step"] <= 1e-8


def test_inconsistent_ring_against_the_model(N, reference):
    """2: a ring of 8 nodes with one inconsistent loop closure, start 0.2 m and 0.1 rad off"""
    G, pm, rm = reference["ring_inconsistent"]
    assert rm["cost_final"] > 0.1
    (p, r), = run(N, [G])
    assert_agrees_with_model("ring_inconsistent", p, r, pm, rm)


def test_angle_wrap_against_the_model(N, reference):
    """3: yaws that run once round the circle: errors and updates cross +-pi, one link is measured across the cut"""
    G, pm, rm = reference["ring_wrap"]
    (p, r), = run(N, [G])
    assert np.all(p[:, 2] > -np.pi) and np.all(p[:, 2] <= np.pi)
    assert_agrees_with_model("ring_wrap", p, r, pm, rm)


def test_strided_loops_against_the_model(N, reference):
    """4: more nodes and more links than the workgroup has threads (1122 and 2561 against 1024)"""
    G, pm, rm = reference["grid_world"]
    assert G.n_nodes > 1024 and G.n_edges > 2048
    (p, r), = run(N, [G])
    assert_agrees_with_model("grid_world", p, r, pm, rm)


def test_weighting(N):
    """5: a link twice = the link once at twice the information; per-link info9 agrees with the model; NULL = 100 I bit for bit"""
    G = M.ring_inconsistent()
    W = np.tile(100.0 * np.eye(3), (G.n_edges, 1, 1))
    twice = M.Graph(G.poses, np.append(G.ref, G.ref[-1]), np.append(G.mov, G.mov[-1]), np.vstack([G.meas, G.meas[-1:]]))
    W2 = W.copy()
    W2[-1] *= 2.0
    doubled = M.Graph(G.poses, G.ref, G.mov, G.meas, W2)
    explicit = M.Graph(G.poses, G.ref, G.mov, G.meas, W)
    weighted = M.random_graph(40, 7, per_link_info=True)
    (pt, rt), (pd, rd), (pe, re_), (pn, rn), (pw, rw) = run(N, [twice, doubled, explicit, G, weighted])
    # 100 e + 100 e against 200 e: the same problem, a rounding apart in every sum; both sit at TOL of the model of either
    pm, rm = M.optimize(doubled)
    assert_agrees_with_model("link twice", pt, rt, pm, rm, n_edges=twice.n_edges)
    assert_agrees_with_model("twice the information", pd, rd, pm, rm)
    assert np.array_equal(pe, pn) and re_ == rn
    pm, rm = M.optimize(weighted)
    assert_agrees_with_model("per-link information", pw, rw, pm, rm)


def test_batch_independence(N):
    """6: 64 graphs of 2 to 300 nodes in one call, each alone, and with first / count cutting the range: the same bits"""
    graphs = M.batch_graphs()
    together = run(N, graphs)
    assert all(r["exit_code"] == M.CONVERGED for _, r in together)
    bank = N.PGO(len(graphs), 300, max(G.n_edges for G in graphs))
    for cuts in ([(k, 1) for k in range(len(graphs))], [(0, 5), (5, 30), (35, 1), (36, 28)]):
        for k, G in enumerate(graphs):
            bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
        for first, count in cuts:
            bank.optimize(first=first, count=count)
        for k in range(len(graphs)):
            p, r = bank.poses(k)
            assert np.array_equal(p, together[k][0]), (cuts[0], k)
            assert r == together[k][1], (cuts[0], k, r, together[k][1])
    bank.close()
    # a graph alone in a bank of another capacity as well
    k = 17
    (p, r), = run(N, [graphs[k]])
    assert np.array_equal(p, together[k][0]) and r == together[k][1]


def test_exit_codes(N):
    """7: the iteration cap returns the iterate after one step; a NaN measurement is reported for its graph alone"""
    G = M.ring_inconsistent()
    pm, rm = M.optimize(G, max_iterations=1)
    (p, r), = run(N, [G], max_iterations=1)
    assert r["exit_code"] == M.MAX_ITERATIONS and r["iterations"] == 1 and r["max_step"] > 1e-3
    # One Gauss-Newton step from the same start.  The device's solve stops at the relative residual eps_linear, which bounds its
    # distance from the dense solve by cond(H) * eps_linear * |step| (H and the step taken from the model).
    S = M._System(G, G.poses, G.W(), 100.0 * np.eye(3))
    bound = float(np.linalg.cond(S.dense())) * 1e-8 * rm["max_step"]
    print("one step: largest pose difference %.3g (bound %.3g), step %.6g (model %.6g)" % (pose_diff(p, pm), bound, r["max_step"], rm["max_step"]))
    assert pose_diff(p, pm) <= bound and abs(r["max_step"] - rm["max_step"]) <= bound
    # cost_final is the cost at the poses returned: the model's cost there, to the rounding of 8 terms
    at_p = M._System(M.Graph(G.poses, G.ref, G.mov, G.meas), p, G.W(), 100.0 * np.eye(3)).cost
    assert abs(r["cost_final"] - at_p) <= 1e-13 * at_p and r["cost_final"] < r["cost_initial"]
    bad = M.Graph(G.poses, G.ref, G.mov, G.meas.copy())
    bad.meas[3, 1] = np.nan
    good = M.ring_wrap()
    alone, = run(N, [good])
    (pa, ra), (pb, rb), (pc, rc) = run(N, [good, bad, good])             # (run raises unless the call returns NDTGPU_OK)
    assert rb["exit_code"] == M.NOT_FINITE and rb["iterations"] == 0 and np.array_equal(pb, G.poses)
    assert not np.isfinite(rb["cost_initial"])
    for p, r in ((pa, ra), (pc, rc)):
        assert np.array_equal(p, alone[0]) and r == alone[1] and r["exit_code"] == M.CONVERGED
    # an inner solve that stops at its cap is reported, and the run still goes on
    (p, r), = run(N, [M.grid_world()], max_linear_iterations=3, max_iterations=4)
    assert r["exit_code"] == M.LINEAR_CAP and r["iterations"] == 4 and r["linear_iterations"] == 12
    assert r["cost_final"] < r["cost_initial"]


def test_device_links(N):
    """8: links straight from ndtgpu_register_batch_cov_device (16 scan pairs round a loop) against the same values read back,
    converted in NumPy (pgo_model.link_from_registration) and given to set_graph: the same bits.  Made-up flags, each of the three
    bits: those links take the covariance 0.02 I."""
    import torch
    from ndt_feature_graph_amd import synth
    dev = torch.device("cuda", 0)
    n = 16
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([2.0 * np.cos(a), 1.5 * np.sin(a), M.wrap(a + 2.0)], -1)
    scans = synth.scan_2d([1] * n, torch.tensor(truth, dtype=torch.float64), 20000).to(dev)
    ref, mov = np.arange(n), (np.arange(n) + 1) % n
    rng = np.random.default_rng(8)
    guess = M.ominus(truth[mov], truth[ref]) + rng.uniform(-0.05, 0.05, size=(n, 3))
    T16 = synth.pose2d_to_T(torch.tensor(guess)).transpose(1, 2).contiguous().reshape(n, 16).to(dev)
    res = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    cov = torch.zeros((n, 36), dtype=torch.float64, device=dev)
    flg = torch.zeros((n,), dtype=torch.int32, device=dev)
    reg = N.Registrar(0.5, [0, 0, 0], [100.0, 100.0, 1.0], pairs_per_batch=n, depth=1, max_cells=4096)
    reg.submit(scans[ref].contiguous(), scans[mov].contiguous(), T16, res, range_limit=30.0, covariance_mode=0, cov36_dev=cov,
               cov_flags_dev=flg)
    reg.sync()
    T_h, cov_h, flg_h = T16.cpu().numpy(), cov.cpu().numpy(), flg.cpu().numpy()
    z_true = M.ominus(truth[mov], truth[ref])
    z_reg = np.array([M.link_from_registration(T_h[k])[0] for k in range(n)])
    assert np.max(np.abs(z_reg[:, :2] - z_true[:, :2])) < 0.1 and np.max(np.abs(M.wrap(z_reg[:, 2] - z_true[:, 2]))) < 0.05
    assert np.count_nonzero(flg_h == 0) >= n - 2                        # (the registrations ran: real covariances are inverted)
    start = M._perturbed(truth, rng)

    def both(cov_dev, flags_dev, cov_host, flags_host):
        bank = N.PGO(2, n, n)
        bank.set_links_device(0, start, ref, mov, T16, cov_dev, flags_dev)
        conv = [M.link_from_registration(T_h[k], None if cov_host is None else cov_host[k], 0 if flags_host is None else int(flags_host[k]))
                for k in range(n)]
        bank.set_graph(1, start, ref, mov, np.array([c[0] for c in conv]), np.array([c[1] for c in conv]))
        bank.optimize()
        (p0, r0), (p1, r1) = bank.poses(0), bank.poses(1)
        bank.close()
        assert np.array_equal(p0, p1) and r0 == r1, (pose_diff(p0, p1), r0, r1)
        assert r0["exit_code"] == M.CONVERGED
        return p0, r0, conv

    p, r, conv = both(cov, flg, cov_h, flg_h)
    assert pose_diff(p, truth) < 0.2
    # made-up flags, each of the three bits, and a block that does not invert
    fake = flg_h.copy()
    fake[2], fake[5], fake[9] = M.COV_SINGULAR, M.COV_POSE_UNCHANGED, M.COV_NOT_COMPUTED
    cov_f = cov_h.copy()
    cov_f[12] = 0.0
    pf, rf, conv_f = both(torch.tensor(cov_f, device=dev), torch.tensor(fake, device=dev), cov_f, fake)
    for k in (2, 5, 9, 12):
        assert np.max(np.abs(conv_f[k][1] - 50.0 * np.eye(3))) < 1e-12
    assert not np.array_equal(pf, p)
    # no covariances: every link 100 I, the same bits as set_graph with info9 = NULL
    pn, rn, _ = both(None, None, None, None)
    bank = N.PGO(1, n, n)
    bank.set_graph(0, start, ref, mov, np.array([c[0] for c in conv]), None)
    bank.optimize()
    p1, r1 = bank.poses(0)
    assert np.array_equal(pn, p1) and rn == r1
