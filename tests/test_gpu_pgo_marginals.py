"""ndtgpu_pgo_marginals: node marginal covariances of the SE(2) pose-graph bank on the device (-m gpu).

Every comparison is against numpy.linalg.inv of the model's dense H (tests/pgo_marginals_model.py) built at the poses THE DEVICE
holds.  The tolerance comes from the model alone: ten times the graph's floor (pgo_marginals_model.FLOOR2, guarded by
tests/test_pgo_marginals_model.py::test_floors), as the largest entry difference of a block relative to the block's largest
entry.  Where two device runs are compared the bits must match."""
import numpy as np
import pytest

import pgo_marginals_checks as K
import pgo_marginals_model as MM
import pgo_model as M

pytestmark = pytest.mark.gpu
DOF = 3


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


def against_dense(N, names, **params):
    """the named graphs of the model in one bank, optimised in one call, their queries in ONE marginals call"""
    sets = [MM.graphs(DOF)[n] for n in names]
    bank = K.make_bank(N, DOF, [s[0] for s in sets])
    gi = np.concatenate([np.full(len(s[1]), k) for k, s in enumerate(sets)])
    qs, os_ = np.concatenate([s[1] for s in sets]), np.concatenate([s[2] for s in sets])
    cov, cross, res = bank.marginals(gi, qs, os_, **params)
    out = {}
    for k, (name, (G, q, o)) in enumerate(zip(names, sets)):
        sel = gi == k
        S, Hi, P = K.dense_at_device_poses(bank, k, G)
        out[name] = (G, q, o, cov[sel], cross[sel], res[sel], Hi, P)
    bank.close()
    return out


def test_trees_reach_the_closed_forms(N):
    """two nodes and a five-node chain, every node: (H^-1)[0, 0] is the prior's inverse, the relative covariance along a link is the
    link's W^-1 = 0.01 I, every column converges within dof * n_nodes + 3 iterations"""
    for name, (G, q, o, cov, cross, res, Hi, P) in against_dense(N, ["two_nodes", "chain"]).items():
        tol = 10 * MM.FLOOR2[name]
        K.assert_blocks(name, tol, cov, cross, Hi, q, o)
        assert np.all(res["exit_code"] == M.CONVERGED) and np.all(res["capped_columns"] == 0)
        assert np.all(res["max_column_iterations"] <= DOF * G.n_nodes + 3) and np.all(res["linear_iterations"] >= DOF)
        assert MM.block_diff(cov[0], 0.01 * np.eye(3)) <= tol
        for e in range(G.n_edges):                       # link e is e -> e + 1, and query e asked for the cross block [e + 1, e]
            R = N.pgo_relative_covariance(P[e], P[e + 1], cov[e], cov[e + 1], cross[e])
            # out = J S J^T with J 3x6: an entry of out moves by at most (6 max |J|)^2 times what an entry of S moves by
            jmax = max(1.0, float(np.max(np.abs(M.ominus(P[e + 1], P[e])[:2]))))
            bound = 36 * jmax * jmax * tol * max(np.max(np.abs(cov[e])), np.max(np.abs(cov[e + 1])), np.max(np.abs(cross[e])))
            print("%s link %d: relative covariance off 0.01 I by %.3g (allowed %.3g)" % (name, e, np.max(np.abs(R - 0.01 * np.eye(3))), bound))
            assert np.max(np.abs(R - 0.01 * np.eye(3))) <= bound


@pytest.mark.parametrize("name", ["ring_inconsistent", "ring_wrap", "weighted"])
def test_loops_against_the_dense_inverse(N, name):
    """every node of the inconsistent ring, the ring that wraps and the 40-node graph with per-link information, other = the next
    node; the loop makes the relative covariance strictly smaller than a link's own 0.01 I"""
    G, q, o, cov, cross, res, Hi, P = against_dense(N, [name])[name]
    print("%s: iterations per query %s" % (name, list(res["linear_iterations"])))
    assert np.all(res["exit_code"] == M.CONVERGED) and np.all(res["capped_columns"] == 0)
    assert np.all(res["linear_iterations"] >= res["max_column_iterations"]) and np.all(res["max_column_iterations"] > 0)
    K.assert_blocks(name, 10 * MM.FLOOR2[name], cov, cross, Hi, q, o)
    if name == "ring_inconsistent":
        R = N.pgo_relative_covariance(P[0], P[1], cov[0], cov[1], cross[0])
        assert np.all(np.linalg.eigvalsh(0.01 * np.eye(3) - 0.5 * (R + R.T)) > 0.0)


def test_result_record_is_consistent_with_the_raw_block(N):
    """other == node returns the raw diagonal block: cov is its symmetric part and asymmetry its max |B - B^T|, bit for bit"""
    G, q, _ = MM.graphs(DOF)["ring_wrap"]
    bank = K.make_bank(N, DOF, [G])
    cov, raw, res = bank.marginals(0, q, q)
    bank.close()
    Bt = np.swapaxes(raw, 1, 2)
    assert K.same_bits(cov, 0.5 * (raw + Bt))
    assert K.same_bits(res["asymmetry"], np.max(np.abs(raw - Bt), axis=(1, 2)))


def test_strided_loops(N):
    """more nodes and links than the workgroup has threads (1122 and 2561 against 1024): queries 0, 1, 560, 1121"""
    G, q, o, cov, cross, res, Hi, P = against_dense(N, ["grid_world"])["grid_world"]
    assert G.n_nodes > 1024 and G.n_edges > 2048 and list(q) == [0, 1, 560, 1121]
    K.assert_blocks("grid_world", 10 * MM.FLOOR2["grid_world"], cov, cross, Hi, q, o)
    assert np.all(res["exit_code"] == M.CONVERGED)
    assert MM.block_diff(cov[0], 0.01 * np.eye(3)) <= 10 * MM.FLOOR2["grid_world"]


def test_per_link_information_300_nodes(N):
    G, q, o, cov, cross, res, Hi, P = against_dense(N, ["random300"])["random300"]
    assert G.info is not None and len(q) == 4
    K.assert_blocks("random300", 10 * MM.FLOOR2["random300"], cov, cross, Hi, q, o)
    assert np.all(res["exit_code"] == M.CONVERGED)


def test_batch_independence(N):
    """64 graphs of 2 to 300 nodes optimised in one call; the last node of each queried in one call, one by one and in reversed
    order: the same bits"""
    graphs = M.batch_graphs(64, 2, 300)
    assert graphs[0].n_nodes == 2
    bank = K.make_bank(N, DOF, graphs)
    gi = np.arange(len(graphs))
    last = np.array([G.n_nodes - 1 for G in graphs])
    cov, cross, res = bank.marginals(gi, last)
    assert cross is None and np.all(res["exit_code"] == M.CONVERGED) and np.all(np.isfinite(cov))
    rc, _, rr = bank.marginals(gi[::-1], last[::-1])
    assert K.same_bits(rc[::-1].copy(), cov) and K.same_bits(rr[::-1].copy(), res)
    for k in (0, 1, 17, 63):
        c1, _, r1 = bank.marginals(k, [last[k]])
        assert K.same_bits(c1[0], cov[k]) and K.same_bits(r1, res[k:k + 1]), k
    bank.close()


def test_chunking_and_repeated_queries(N):
    """the ring's eight queries with one slot (24 solve launches) and under the default budget (one launch): the same bits; a
    query given twice gives equal bits"""
    G, q, o = MM.graphs(DOF)["ring_inconsistent"]
    bank = K.make_bank(N, DOF, [G])
    assert N.pgo_marginal_plan(G.n_nodes, G.n_edges, len(q), DOF, 1)[1:] == (1, DOF * len(q))
    assert N.pgo_marginal_plan(G.n_nodes, G.n_edges, len(q), DOF)[1:] == (DOF * len(q), 1)
    cov, cross, res = bank.marginals(0, q, o)
    cov1, cross1, res1 = bank.marginals(0, q, o, max_workspace_bytes=1)
    assert K.same_bits(cov, cov1) and K.same_bits(cross, cross1) and K.same_bits(res, res1)
    slot = N.pgo_marginal_plan(G.n_nodes, G.n_edges, len(q), DOF)[0]
    cov5, cross5, res5 = bank.marginals(0, q, o, max_workspace_bytes=5 * slot)        # (five slots: a last launch that is not full)
    assert K.same_bits(cov, cov5) and K.same_bits(cross, cross5) and K.same_bits(res, res5)
    cov2, cross2, res2 = bank.marginals(0, [3, 5, 3], [4, 6, 4])
    assert K.same_bits(cov2[0], cov2[2]) and K.same_bits(cross2[0], cross2[2]) and K.same_bits(res2[0:1], res2[2:3])
    assert K.same_bits(cov2[0], cov[3]) and K.same_bits(cross2[1], cross[5])
    bank.close()


def test_marginals_do_not_interfere_with_the_optimiser(N):
    """poses and ndtgpu_pgo_result are unchanged by a marginals call; optimising a re-set graph after one gives a fresh handle's bits"""
    G, q, o = MM.graphs(DOF)["ring_wrap"]
    bank = K.make_bank(N, DOF, [G])
    p0, r0 = bank.poses(0)
    bank.marginals(0, q, o)
    p1, r1 = bank.poses(0)
    assert K.same_bits(p0, p1) and r0 == r1
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize()
    p2, r2 = bank.poses(0)
    bank.close()
    assert K.same_bits(p0, p2) and r0 == r2


def test_exit_codes(N):
    """max_linear_iterations = 3 on the grid world: LINEAR_CAP, finite iterates, the capped columns counted; a NaN measurement in one
    graph of a bank: NOT_FINITE and NaN for its queries, another graph's query in the same call untouched"""
    G, q, o = MM.graphs(DOF)["grid_world"]
    bad = M.ring_inconsistent()
    z = bad.meas.copy()
    z[2, 1] = np.nan
    bad = M.Graph(bad.poses, bad.ref, bad.mov, z)
    bank = K.make_bank(N, DOF, [G, bad], optimize=False)
    cov, cross, res = bank.marginals(0, q, o, max_linear_iterations=3)
    assert np.all(res["exit_code"] == M.LINEAR_CAP) and np.all(res["capped_columns"] == 3) and np.all(res["max_column_iterations"] == 3)
    assert np.all(res["linear_iterations"] == 9) and np.all(np.isfinite(cov)) and np.all(np.isfinite(cross))
    S = MM.system(G, bank.poses(0)[0])
    B, X, its, capped = MM.marginal(S, int(q[2]), int(o[2]), max_linear_iterations=3)
    assert capped == 3 and its == [3, 3, 3]
    # three iterations of the same recurrence: sums of at most 2561 terms in another order, each good to 2561 * 2^-53 = 3e-13
    assert MM.block_diff(cov[2], MM.cov_of(B)) <= 1e-12 and MM.block_diff(cross[2], X) <= 1e-12
    good, _, rgood = bank.marginals([0], [q[1]], [o[1]])
    cov2, cross2, res2 = bank.marginals([1, 0, 1], [0, q[1], 5], [1, o[1], 6])
    bank.close()
    assert list(res2["exit_code"]) == [M.NOT_FINITE, M.CONVERGED, M.NOT_FINITE]
    assert np.all(np.isnan(cov2[[0, 2]])) and np.all(np.isnan(cross2[[0, 2]])) and np.all(np.isnan(res2["asymmetry"][[0, 2]]))
    assert K.same_bits(cov2[1], good[0]) and K.same_bits(res2[1:2], rgood)


def test_device_form(N):
    """outputs in caller buffers on a caller stream equal the host form's bits; relative_covariance of device results on the
    chain gives the links' W^-1"""
    import torch
    G, q, o = MM.graphs(DOF)["chain"]
    bank = K.make_bank(N, DOF, [G])
    cov, cross, res = bank.marginals(0, q, o)
    n = len(q)
    cov_d = torch.zeros(n * 9, dtype=torch.float64, device="cuda")
    cross_d = torch.zeros(n * 9, dtype=torch.float64, device="cuda")
    res_d = torch.zeros(n * N.PGO_MARGINAL_RESULT.itemsize, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    bank.marginals_device(0, q, o, cov_d, cross_d, res_d, stream=st)
    st.synchronize()
    cov2, cross2 = cov_d.cpu().numpy().reshape(n, 3, 3), cross_d.cpu().numpy().reshape(n, 3, 3)
    assert K.same_bits(cov2, cov) and K.same_bits(cross2, cross)
    assert K.same_bits(res_d.cpu().numpy().view(N.PGO_MARGINAL_RESULT), res)
    P = bank.poses(0)[0]
    bank.close()
    for e in range(G.n_edges):
        R = N.pgo_relative_covariance(P[e], P[e + 1], cov2[e], cov2[e + 1], cross2[e])
        jmax = max(1.0, float(np.max(np.abs(M.ominus(P[e + 1], P[e])[:2]))))
        bound = 36 * jmax * jmax * 10 * MM.FLOOR2["chain"] * max(np.max(np.abs(cov2[e])), np.max(np.abs(cov2[e + 1])), np.max(np.abs(cross2[e])))
        assert np.max(np.abs(R - 0.01 * np.eye(3))) <= bound


def test_bad_queries_are_refused(N):
    G, q, o = MM.graphs(DOF)["chain"]
    bank = N.PGO(2, 8, 8)
    bank.set_graph(0, G.poses, G.ref, G.mov, G.meas)
    for gi, qi, oi, word in (([2], [0], None, "out of range"), ([1], [0], None, "not been set"), ([0], [5], None, "n_nodes"),
                             ([0], [4], [5], "n_nodes")):
        with pytest.raises(N.NdtGpuError) as e:
            bank.marginals(gi, qi, oi)
        assert e.value.status == -1 and word in str(e.value), (gi, qi, oi)
    cov, _, res = bank.marginals([0], [4])                # (the handle still works)
    bank.close()
    assert res["exit_code"][0] == M.CONVERGED and np.all(np.isfinite(cov))


def test_lifecycle(N):
    """the library owns the same resources before create and after destroy, with marginals calls in between"""
    G, q, o = MM.graphs(DOF)["ring_inconsistent"]
    before = N.binding.live_resources()
    bank = K.make_bank(N, DOF, [G])
    bank.marginals(0, q, o)
    bank.marginals(0, q, None, max_workspace_bytes=1)
    assert N.binding.live_resources() != before
    bank.close()
    assert N.binding.live_resources() == before
