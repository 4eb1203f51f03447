"""What tests/test_gpu_pgo_robust.py (SE(2), dof 3) and tests/test_gpu_pgo3_robust.py (SE(3), dof 6) share: the checks of the robust
weighting on the device against tests/pgo_robust_model.py.  Where two device runs are compared the bits must match; the weights
and flags are the model's functions of the DEVICE's own chi2, bit for bit; chi2 itself is held in the carried-bound unit of
tests/pgo_robust_bounds.py; poses and robust cost against the model's dense IRLS within ten times the floors of the model file."""
import numpy as np

import pgo3_model as M3
import pgo_marginals_model as MM
import pgo_model as M2
import pgo_robust_bounds as B
import pgo_robust_model as R

EDGES = (1, 255, 256, 257, 513)          # the tile's edges: one link, one short of a tile, a tile, one more, two tiles and one


def mod_of(dof):
    return M2 if dof == 3 else M3


def bank_of(N, dof, graphs, n_graphs=None, max_nodes=None, max_edges=None, first=0):
    cls = N.PGO if dof == 3 else N.PGO3
    bank = cls(n_graphs or len(graphs), max_nodes or max(G.n_nodes for G in graphs), max_edges or max(max(G.n_edges for G in graphs), 1))
    for k, G in enumerate(graphs):
        bank.set_graph(first + k, G.poses, G.ref, G.mov, G.meas, G.info)
    return bank


def pack(W):
    """[m, d, d] symmetric -> the bank's layout: SE(2) (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); SE(3) the lower triangle row by row"""
    d = W.shape[-1]
    idx = [(i, j) for i in range(3) for j in range(i, 3)] if d == 3 else [(i, j) for i in range(6) for j in range(i + 1)]
    return np.stack([W[:, i, j] for i, j in idx], axis=1)


def state(bank, g):
    """everything a robust call leaves for graph g, as bytes-comparable arrays"""
    P, _ = bank.poses(g)
    chi2, w, inl, res = bank.robust_links(g)
    return P.copy(), chi2.copy(), w.copy(), inl.copy(), res


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def diff(dof, P, Q):
    d = np.asarray(P) - np.asarray(Q)
    if dof == 3:
        d[:, 2] = M2.wrap(d[:, 2])
    return float(np.max(np.abs(d)))


def check_evaluate_only(N, dof, n_edges):
    """max_rounds = 0 on a graph of exactly n_edges links, nothing protected (min_index_gap 1) so that every link is weighed"""
    mod = mod_of(dof)
    G = R.edge_graph(mod, n_edges)
    W0 = G.W()
    chi2_m, _ = R.link_chi2(mod, G, G.poses, W0)
    bound = (B.chi2_bound2 if dof == 3 else B.chi2_bound3)(G, G.poses, W0)
    bank = bank_of(N, dof, [G])
    info0, poses0 = bank.information(0), bank.poses(0)[0]
    assert info0.tobytes() == pack(W0).tobytes()
    med = float(np.median(chi2_m))
    scales = {"huber": [np.sqrt(med)], "cauchy": [1.0], "dcs": [med]}
    if n_edges == 1:                                    # one link takes one branch at a time
        scales = {"huber": [np.sqrt(med) * 0.5, np.sqrt(med) * 2.0], "cauchy": [1.0], "dcs": [med * 0.5, med * 2.0]}
    worst = 0.0
    for kind, ss in scales.items():
        ones = below = 0
        for scale in ss:
            bank.optimize_robust(robust=dict(kind=kind, scale=float(scale), max_rounds=0, min_index_gap=1))
            chi2, w, inl, res = bank.robust_links(0)
            assert chi2.shape == (n_edges,) and np.all(np.isfinite(chi2))
            worst = max(worst, float(np.max(np.abs(chi2 - chi2_m) / bound)))
            want = R.weights(kind, scale, chi2)
            assert w.tobytes() == want.tobytes(), (kind, scale)
            assert w.tobytes() == N.pgo_robust_weight(kind, scale, chi2).tobytes()       # (and the host form of the library)
            assert np.array_equal(inl, want >= 0.5)
            ones, below = ones + int(np.sum(w == 1.0)), below + int(np.sum(w < 1.0))
            cost = float(np.sum([R.rho(kind, scale, c) for c in chi2]))
            assert res["exit_code"] == R.MAX_ROUNDS and res["rounds"] == res["updates"] == res["linear_iterations"] == 0
            assert res["outliers"] == int(np.sum(~inl))
            assert res["cost_initial"] == res["cost_final"] and abs(res["cost_final"] - cost) <= 1e-13 * cost
            assert abs(res["chi2_final"] - float(np.sum(chi2))) <= 1e-13 * float(np.sum(chi2))
            # nothing in the bank has changed
            assert bank.information(0).tobytes() == info0.tobytes() and bank.poses(0)[0].tobytes() == poses0.tobytes()
        if kind != "cauchy":
            assert ones and below, (kind, ones, below)          # both branches were taken
    bank.close()
    print("E = %d: chi2 against the model %.3f of its carried bound (bound 1)" % (n_edges, worst))
    assert worst <= 1.0


def check_protected_and_restore(N, dof):
    mod = mod_of(dof)
    G = mod.random_graph(40, 10, per_link_info=True)
    bank = bank_of(N, dof, [G])
    info0 = bank.information(0)
    bank.optimize_robust(robust=dict(kind="cauchy", scale=1.0, max_rounds=3))
    chi2, w, inl, res = bank.robust_links(0)
    info1 = bank.information(0)
    prot = R.protected(G)
    assert G.n_nodes - 1 <= prot.sum() < G.n_edges and np.all(w[prot] == 1.0) and np.all(w[~prot] < 1.0)
    assert info1[prot].tobytes() == info0[prot].tobytes()
    assert info1[~prot].tobytes() == (w[~prot, None] * info0[~prot]).tobytes()      # the bank holds the weights the call reports
    assert res["rounds"] == 3 and res["exit_code"] == R.MAX_ROUNDS and res["updates"] == 3
    # a larger gap protects more
    bank.optimize_robust(robust=dict(kind="cauchy", scale=1.0, max_rounds=0, min_index_gap=1000))
    assert np.all(bank.robust_links(0)[1] == 1.0) and bank.information(0).tobytes() == info1.tobytes()
    bank.robust_restore(0)
    assert bank.information(0).tobytes() == info0.tobytes()
    bank.close()


def check_reduces_to_plain(N, dof):
    """Huber with a scale no chi2 reaches, one round of 50 updates: the plain optimiser's bits, in either form"""
    mod = mod_of(dof)
    G = mod.model_graphs()["ring_inconsistent" if dof == 3 else "helix_ring"]
    robust = dict(kind="huber", scale=1e300, max_rounds=1, updates_per_round=50)
    for wide in (False, True):
        plain = bank_of(N, dof, [G])
        (plain.optimize_wide(0) if wide else plain.optimize())
        P0, r0 = plain.poses(0)
        plain.close()
        bank = bank_of(N, dof, [G])
        bank.optimize_robust(robust=robust, wide=wide)
        P1, r1 = bank.poses(0)
        _, w, _, res = bank.robust_links(0)
        bank.close()
        assert P1.tobytes() == P0.tobytes() and r1["iterations"] == r0["iterations"] and r1["cost_final"] == r0["cost_final"]
        assert res["exit_code"] == R.MAX_ROUNDS and res["rounds"] == 1 and res["updates"] == r0["iterations"] > 1
        assert res["linear_iterations"] == r0["linear_iterations"] and np.all(w == 1.0)


_REFERENCE = {}


def reference(name, kind):
    """the model's dense IRLS of an outlier graph, computed once"""
    key = (name, kind)
    if key not in _REFERENCE:
        case = {c[0]: c for c in R.floor_cases()}[name]
        if name not in _REFERENCE:
            clean, dirty, false = case[2](*case[3])
            _REFERENCE[name] = (clean, dirty, false, case[1].optimize(clean)[0], case[1].optimize(dirty)[0])
        _REFERENCE[key] = R.irls(case[1], _REFERENCE[name][1], robust=dict(kind=kind))
    return _REFERENCE[name] + _REFERENCE[key]


def check_outlier_graph(N, dof, name, kind):
    """the conditions of tests/test_pgo_robust_model.py on the device, and the device against the model"""
    mod = mod_of(dof)
    clean, dirty, false, Pc, Pp, Pm, om = reference(name, kind)
    tol, rtol = (R.TOL, R.COST_RTOL) if dof == 3 else (R.TOL3, R.COST3_RTOL)
    bank = bank_of(N, dof, [dirty])
    bank.optimize_robust(robust=dict(kind=kind))
    P, chi2, w, inl, res = state(bank, 0)
    rm = om["result"]
    d, dc = diff(dof, P, Pm), abs(res["cost_final"] - rm["cost_final"]) / rm["cost_final"]
    print("%s %s: %d rounds (model %d), exit %d, distance to the clean optimum %.3g, false closures' weights <= %.3g, true links' >= %.3g, "
          "largest pose difference to the model %.3g (allowed %.3g), robust cost %.12g (model %.12g, relative difference %.3g, allowed %.3g)"
          % (name, kind, res["rounds"], rm["rounds"], res["exit_code"], R.distance(mod, P, Pc), w[false].max(), w[~false].min(), d, tol,
             res["cost_final"], rm["cost_final"], dc, rtol))
    assert res["exit_code"] == R.CONVERGED and res["rounds"] == rm["rounds"] and res["updates"] == rm["updates"]
    if kind == "dcs":
        assert R.distance(mod, P, Pc) <= (1e-3 if dof == 3 else 3e-4)
        assert w[false].max() <= (1e-3 if dof == 3 else 1.6e-4) and w[~false].min() >= (0.5 if dof == 3 else 0.1)
        assert np.array_equal(inl, ~false) and res["outliers"] == int(false.sum())
    elif kind == "cauchy":
        assert R.distance(mod, P, Pc) <= (0.05 if dof == 3 else 0.069)
    plain = bank_of(N, dof, [dirty])
    plain.optimize()
    Pd = plain.poses(0)[0]
    plain.close()
    print("the plain optimiser on the device ends %.3g m from the clean optimum (the model's %.3g)" % (R.distance(mod, Pd, Pc), R.distance(mod, Pp, Pc)))
    assert R.distance(mod, Pd, Pc) >= (1.0 if dof == 3 else 0.16)
    assert w.tobytes() == np.where(R.protected(dirty), 1.0, R.weights(kind, 1.0, chi2)).tobytes()
    assert d <= tol
    assert dc <= rtol
    if kind == "dcs" and name != "grid17x16":
        # the bank is left weighted: a node's marginal is the dense inverse of the model's H with the weights the device reports, at
        # the device's poses, within the marginals tests' tolerance for the grid worlds (ten times their floor)
        q = dirty.n_nodes - 1
        cov, _, mres = bank.marginals(0, [q])
        Gw = mod.Graph(dirty.poses, dirty.ref, dirty.mov, dirty.meas, w[:, None, None] * dirty.W())
        Hi = MM.dense_inverse(MM.system(Gw, P))
        md = MM.block_diff(cov[0], Hi[q, q])
        mtol = 10 * MM.floors(dof)["grid_world" if dof == 3 else "grid3d"]
        print("marginal of node %d on the weighted bank: relative block difference %.3g (allowed %.3g)" % (q, md, mtol))
        assert mres["exit_code"][0] == 0 and md <= mtol
        bank.robust_restore(0)
        cov0, _, _ = bank.marginals(0, [q])
        Hi0 = MM.dense_inverse(MM.system(dirty, P))
        assert MM.block_diff(cov0[0], Hi0[q, q]) <= mtol and MM.block_diff(cov0[0], Hi[q, q]) > mtol     # (restored: the plain problem again)
    bank.close()


def batch_graphs(dof):
    """8 graphs of different sizes: random graphs whose last loop closure is made false"""
    mod = mod_of(dof)
    out = []
    for k, n in enumerate((3, 9, 20, 33, 47, 64, 90, 173)):
        G = mod.random_graph(n, 300 + k)
        meas = G.meas.copy()
        meas[-1] = meas[0]                                # the last closure measures what the first odometry link does
        out.append(mod.Graph(G.poses, G.ref, G.mov, meas, truth=G.truth))
    return out


def check_batch_and_rerun(N, dof):
    graphs = batch_graphs(dof)
    robust = dict(kind="dcs", max_rounds=8)
    bank = bank_of(N, dof, graphs)
    start = N.binding.live_resources()
    info0 = [bank.information(k) for k in range(len(graphs))]
    bank.optimize_robust(robust=robust)
    assert N.binding.live_resources() != start          # (the robust buffers are the handle's, and counted)
    together = [state(bank, k) for k in range(len(graphs))]
    assert len({s[4]["rounds"] for s in together}) > 1  # (the graphs stop in different rounds: the later rounds run on a part of the batch)
    assert all(s[4]["exit_code"] in (R.CONVERGED, R.MAX_ROUNDS) for s in together)
    # a robust call weighs the information as set, not the weighted one the bank now holds: an evaluation on the still-weighted
    # bank gives the final weighing of the call before it, bit for bit (weighing the weighted information would square the weights)
    weighted = [bank.information(k) for k in range(len(graphs))]
    assert sum(weighted[k].tobytes() != info0[k].tobytes() for k in range(len(graphs))) >= 6               # (the bank is left weighted)
    bank.optimize_robust(robust=dict(robust, max_rounds=0))
    for k in range(len(graphs)):
        again = state(bank, k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:4], together[k][:4])), k
        assert again[4]["cost_final"] == together[k][4]["cost_final"] and again[4]["outliers"] == together[k][4]["outliers"]
        assert bank.information(k).tobytes() == weighted[k].tobytes()
    # ... and so does a whole second call from the same start
    for k, G in enumerate(graphs):
        bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
    bank.optimize_robust(robust=robust)
    assert all(same(state(bank, k), together[k]) for k in range(len(graphs)))
    for k in range(len(graphs)):
        bank.robust_restore(k)
        assert bank.information(k).tobytes() == info0[k].tobytes()
    bank.close()
    # one by one, each in a bank of its own
    for k, G in enumerate(graphs):
        solo = bank_of(N, dof, [G])
        solo.optimize_robust(robust=robust)
        assert same(state(solo, 0), together[k]), k
        solo.close()
    # at another first, in a larger bank, in two calls
    big = bank_of(N, dof, graphs, n_graphs=13, max_nodes=200, max_edges=700, first=4)
    big.optimize_robust(4, 3, robust=robust)
    big.optimize_robust(7, 5, robust=robust)
    assert all(same(state(big, 4 + k), together[k]) for k in range(len(graphs)))
    big.close()


def check_wide(N, dof):
    name = "grid9x10" if dof == 3 else "grid3d"
    dirty = reference(name, "dcs")[1]
    got = []
    for check_every in (1, 32):
        bank = bank_of(N, dof, [dirty])
        bank.optimize_robust(0, 1, robust=dict(kind="dcs"), wide=True, check_every=check_every)
        got.append(state(bank, 0))
        bank.close()
    assert same(got[0], got[1])
    assert got[0][4]["exit_code"] == R.CONVERGED and np.array_equal(got[0][3], ~reference(name, "dcs")[2])


def check_bad_graph(N, dof, bad, code):
    """a graph whose chi2 is not finite ends with `code`, holds its information as set, and leaves its neighbours' bits alone"""
    graphs = batch_graphs(dof)[2:5]
    robust = dict(kind="dcs", max_rounds=6)
    bank = bank_of(N, dof, graphs)
    bank.optimize_robust(robust=robust)
    want = [state(bank, k) for k in range(3)]
    bank.close()
    bank = bank_of(N, dof, [graphs[0], bad, graphs[2]])
    info = bank.information(1)
    bank.optimize_robust(robust=robust)
    assert same(state(bank, 0), want[0]) and same(state(bank, 2), want[2])
    P, chi2, w, inl, res = state(bank, 1)
    assert res["exit_code"] == code and res["rounds"] == 0 and res["updates"] == 0
    assert diff(dof, P, bad.poses) == 0.0 and np.array_equal(bank.information(1), info, equal_nan=True)
    bank.close()


def check_live_resources(N, dof):
    start = N.binding.live_resources()
    bank = bank_of(N, dof, batch_graphs(dof)[:2])
    bank.optimize_robust(robust=dict(max_rounds=2))
    bank.optimize_robust(0, 1, robust=dict(max_rounds=1), wide=True)
    assert N.binding.live_resources() != start
    bank.close()
    assert N.binding.live_resources() == start
