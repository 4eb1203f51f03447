"""The robust weighting's NumPy model (tests/pgo_robust_model.py) against what it restates: the weights against their cost terms
in mpmath, the outlier graphs' conditions, and the floors the GPU tests' tolerances are built on.  CPU only.

d rho / d chi2 = w holds for Huber and Cauchy, by central differences.  For DCS as it is published and specified -- s = min(1,
2 Phi / (Phi + chi2)), w = s^2, cost s^2 chi2 + Phi (1 - s)^2 -- it CANNOT hold beyond chi2 = Phi: with that s the cost is
identically Phi there (4 Phi^2 chi2 + Phi (chi2 - Phi)^2 = Phi (chi2 + Phi)^2), so its total derivative is 0 while w = s^2 > 0.  What
holds, and is tested, is the statement DCS makes: w is the derivative of the cost with the scaling s FROZEN, which is how a round
of the re-weighting uses it; below Phi, where s = 1, the total derivative is 1 = w as well.  Likewise the minimiser over s of
s^2 chi2 + Phi (1 - s)^2 is s* = Phi / (Phi + chi2), and DCS's s is min(1, 2 s*), twice the minimiser and clipped: w is held
against min(1, 2 s*)^2, with s* found by mpmath's root finder, not against s*^2."""
import math

import mpmath as MP
import numpy as np
import pytest

import pgo3_model as M3
import pgo_model as M2
import pgo_robust_model as R

MP.mp.dps = 50
CHI2 = [0.0, 1e-6, 0.01, 0.3, 0.999, 1.001, 2.0, 3.7, 25.0, 1e3, 1e6]
SCALES = [0.5, 1.0, 3.0]


def _rho_mp(kind, scale, x, s=None):
    k, x = MP.mpf(scale), MP.mpf(x)
    if kind == "huber":
        r = MP.sqrt(x)
        return x if r <= k else 2 * k * r - k * k
    if kind == "cauchy":
        return k * k * MP.log(1 + x / (k * k))
    if s is None:
        s = min(MP.mpf(1), 2 * k / (k + x))
    return s * s * x + k * (1 - s) ** 2


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_weight_is_the_derivative_of_rho(kind):
    worst = 0.0
    for scale in SCALES:
        for x in CHI2[1:]:
            if kind == "huber" and abs(math.sqrt(x) - scale) < 1e-2:
                continue                                    # (the kink: the one-sided derivatives differ)
            h = MP.mpf(x) * MP.mpf("1e-12")
            d = (_rho_mp(kind, scale, x + h) - _rho_mp(kind, scale, x - h)) / (2 * h)
            worst = max(worst, abs(float(d) - R.weight(kind, scale, x)))
    print("%s: |d rho / d chi2 - w| %.3g" % (kind, worst))
    assert worst <= 1e-15


def test_dcs_weight_and_cost():
    """see the module's docstring"""
    for scale in SCALES:
        for x in CHI2[1:]:
            w = R.weight("dcs", scale, x)
            s = MP.mpf(R.dcs_s(scale, x))
            h = MP.mpf(x) * MP.mpf("1e-12")
            # the derivative with s frozen
            d = (_rho_mp("dcs", scale, x + h, s) - _rho_mp("dcs", scale, x - h, s)) / (2 * h)
            assert abs(float(d) - w) <= 1e-15
            # the total derivative: 1 below Phi, 0 above it, where the cost is Phi
            if abs(x - scale) > 1e-2:
                t = (_rho_mp("dcs", scale, x + h) - _rho_mp("dcs", scale, x - h)) / (2 * h)
                assert abs(float(t) - (1.0 if x < scale else 0.0)) <= 1e-15
            if x > scale:
                assert abs(R.rho("dcs", scale, x) - scale) <= 4e-16 * scale
            # s against the minimiser over s of s^2 chi2 + Phi (1 - s)^2, found numerically
            star = MP.findroot(lambda q: MP.diff(lambda u: u * u * MP.mpf(x) + MP.mpf(scale) * (1 - u) ** 2, q), MP.mpf("0.5"))
            assert abs(float(star) - scale / (scale + x)) <= 1e-15
            assert abs(w - float(min(MP.mpf(1), 2 * star) ** 2)) <= 4e-16


def test_weights_branches_and_limits():
    assert R.weight("huber", 1.0, 1.0) == 1.0 and R.weight("huber", 1.0, 4.0) == 0.5
    assert R.weight("cauchy", 2.0, 4.0) == 0.5
    assert R.weight("dcs", 1.0, 1.0) == 1.0 and R.weight("dcs", 1.0, 3.0) == 0.25
    for kind in ("huber", "cauchy", "dcs"):
        assert R.weight(kind, 1.0, 0.0) == 1.0 and math.isnan(R.weight(kind, 1.0, math.nan))
        w = R.weights(kind, 1.3, CHI2)
        assert np.all(np.diff(w) <= 0.0) and np.all((w > 0.0) & (w <= 1.0))


def test_protected_links():
    G = M2.random_graph(12, 3)
    assert np.array_equal(R.protected(G), np.abs(G.mov - G.ref) < 2)
    assert np.all(R.protected(G, 100)) and R.protected(G)[: G.n_nodes - 1].all()


_CASE = {}


def _case(mod):
    if mod not in _CASE:
        clean, dirty, false = R.outlier_graph() if mod is M2 else R.outlier_graph3()
        Pc, _ = mod.optimize(clean)
        Pp, _ = mod.optimize(dirty)
        runs = {kind: R.irls(mod, dirty, robust=dict(kind=kind)) for kind in ("dcs", "cauchy", "huber")}
        _CASE[mod] = (clean, dirty, false, Pc, Pp, runs)
    return _CASE[mod]


def test_outlier_graph_se2():
    """grid_world(9, 10), 90 nodes, 6 false closures drawn with default_rng(77).  Measured here (distance to the clean optimum, rounds,
    largest weight of a false closure, smallest of a true link): plain 3.63 m; DCS 2.3e-5, 6, 5.1e-6, exactly 1; Cauchy 8.2e-3, 7,
    1.1e-3, 0.926; Huber 0.33, 35, 0.038, 0.75."""
    clean, dirty, false, Pc, Pp, runs = _case(M2)
    assert dirty.n_nodes == 90 and int(false.sum()) == 6
    assert np.all(np.abs(dirty.mov[false] - dirty.ref[false]) >= 2)
    assert np.all(np.linalg.norm(dirty.truth[dirty.mov[false], :2] - dirty.truth[dirty.ref[false], :2], axis=1) >= 2.0)
    assert R.distance(M2, Pp, Pc) >= 1.0
    P, out = runs["dcs"]
    print("dcs", R.distance(M2, P, Pc), out["result"], out["weight"][false].max(), out["weight"][~false].min())
    assert out["result"]["exit_code"] == R.CONVERGED and out["result"]["rounds"] <= 12
    assert R.distance(M2, P, Pc) <= 1e-3
    assert out["weight"][false].max() <= 1e-3 and out["weight"][~false].min() >= 0.5
    assert np.all(out["weight"][~false] == 1.0)
    assert np.array_equal(out["inlier"], ~false) and out["result"]["outliers"] == 6
    P, out = runs["cauchy"]
    print("cauchy", R.distance(M2, P, Pc), out["result"], out["weight"][false].max(), out["weight"][~false].min())
    assert out["result"]["exit_code"] == R.CONVERGED and R.distance(M2, P, Pc) <= 0.05
    assert out["weight"][false].max() <= 1e-2 and out["weight"][~false].min() >= 0.5
    P, out = runs["huber"]
    print("huber", R.distance(M2, P, Pc), out["result"], out["weight"][false].max())
    assert out["result"]["exit_code"] == R.CONVERGED and out["weight"][false].max() <= 0.5
    assert R.distance(M2, P, Pc) < R.distance(M2, Pp, Pc)       # (Huber's influence does not redescend: better, not clean)


def test_outlier_graph_se3():
    """pgo3_model.grid3d(2, 6, 7), 84 nodes and 194 links, 6 false closures drawn with default_rng(78), +-0.5 m and +-0.3 rad in every
    component.  Measured here: plain 1.66 m from the clean optimum; DCS 3.1e-5 in 6 rounds, false closures' weights at most 1.6e-5,
    every true link exactly 1; Cauchy 6.9e-3 in 7 rounds, at most 2.0e-3, at least 0.946; Huber 0.20 in 11 rounds, at most 0.047.
    Each condition below has a factor 10 of room or more."""
    clean, dirty, false, Pc, Pp, runs = _case(M3)
    assert dirty.n_nodes == 84 and int(false.sum()) == 6
    assert R.distance(M3, Pp, Pc) >= 0.16
    P, out = runs["dcs"]
    print("dcs", R.distance(M3, P, Pc), out["result"], out["weight"][false].max(), out["weight"][~false].min())
    assert out["result"]["exit_code"] == R.CONVERGED
    assert R.distance(M3, P, Pc) <= 3e-4
    assert out["weight"][false].max() <= 1.6e-4 and out["weight"][~false].min() >= 0.1
    assert np.array_equal(out["inlier"], ~false) and out["result"]["outliers"] == 6
    P, out = runs["cauchy"]
    print("cauchy", R.distance(M3, P, Pc), out["result"], out["weight"][false].max(), out["weight"][~false].min())
    assert out["result"]["exit_code"] == R.CONVERGED and R.distance(M3, P, Pc) <= 0.069
    P, out = runs["huber"]
    assert out["result"]["exit_code"] == R.CONVERGED and out["weight"][false].max() <= 0.47


def test_evaluate_only_and_reduction():
    """max_rounds = 0 leaves the poses; Huber with a scale no chi2 reaches is the plain optimiser"""
    _, dirty, false = R.outlier_graph()
    P, out = R.irls(M2, dirty, robust=dict(max_rounds=0))
    assert np.array_equal(P, dirty.poses) and out["result"]["rounds"] == 0 and out["result"]["exit_code"] == R.MAX_ROUNDS
    assert out["result"]["cost_initial"] == out["result"]["cost_final"]
    P, out = R.irls(M2, dirty, robust=dict(kind="huber", scale=1e300, max_rounds=1, updates_per_round=50))
    Pp, rp = M2.optimize(dirty)
    assert np.array_equal(P, Pp) and out["result"]["exit_code"] == R.MAX_ROUNDS and out["result"]["updates"] == rp["iterations"]
    assert np.all(out["weight"] == 1.0)


def test_not_finite_and_half_turn():
    G = M2.random_graph(10, 4)
    G.meas[3, 1] = np.nan
    P, out = R.irls(M2, G)
    assert out["result"]["exit_code"] == R.NOT_FINITE and out["result"]["rounds"] == 0 and np.array_equal(P, G.poses)
    G = M3.chain(4)
    Z = G.meas.copy()
    Z[1] = Z[1] @ M3.make_T(np.diag([1.0, -1.0, -1.0]), np.zeros(3))
    P, out = R.irls(M3, M3.Graph(G.poses, G.ref, G.mov, Z))
    assert out["result"]["exit_code"] == R.HALF_TURN


def test_floor():
    """the constants the GPU tests' tolerances are built on: dense IRLS against IRLS with the restated conjugate gradients"""
    worst = {2: [0.0, 0.0], 3: [0.0, 0.0]}
    for name, mod, gen, args, kinds in R.floor_cases():
        _, dirty, _ = gen(*args)
        for kind in kinds:
            Pd, od = R.irls(mod, dirty, robust=dict(kind=kind))
            Pq, oq = R.irls(mod, dirty, solver="pcg", robust=dict(kind=kind))
            assert od["result"]["exit_code"] == oq["result"]["exit_code"] == R.CONVERGED
            assert od["result"]["rounds"] == oq["result"]["rounds"]
            dp = float(np.max(np.abs(Pd - Pq)))
            dc = abs(od["result"]["cost_final"] - oq["result"]["cost_final"]) / od["result"]["cost_final"]
            print("%s %s: poses %.3g cost %.3g" % (name, kind, dp, dc))
            w = worst[2 if mod is M2 else 3]
            w[0], w[1] = max(w[0], dp), max(w[1], dc)
    print(worst)
    assert worst[2][0] <= R.ROBUST_FLOOR and worst[2][1] <= R.ROBUST_COST_FLOOR
    assert worst[3][0] <= R.ROBUST3_FLOOR and worst[3][1] <= R.ROBUST3_COST_FLOOR
