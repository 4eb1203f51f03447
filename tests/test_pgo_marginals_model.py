"""The NumPy model of the marginal covariances (tests/pgo_marginals_model.py) against closed forms, and the floors that set the
tolerance of tests/test_gpu_pgo_marginals.py and tests/test_gpu_pgo3_marginals.py.  No device."""
import numpy as np
import pytest

import pgo3_model as M3
import pgo_marginals_model as MM
import pgo_model as M2


def spd(n, seed):
    A = np.random.default_rng(seed).normal(size=(n, n))
    return A @ A.T * 20.0 + 30.0 * np.eye(n)


def optimum(G):
    return (M2 if G.poses.ndim == 2 else M3).optimize(G)[0]


SE2 = {"two_nodes": lambda: M2.two_nodes()[0], "chain": lambda: M2.chain(5), "ring_inconsistent": M2.ring_inconsistent,
       "ring_wrap": M2.ring_wrap, "random300": lambda: M2.random_graph(300, 8, True)}
SE3 = {"two_nodes": lambda: M3.two_nodes()[0], "chain": lambda: M3.chain(5), "helix_ring": M3.helix_ring,
       "weighted": lambda: M3.random_graph(40, 10, True)}


@pytest.mark.parametrize("bank,name", [("se2", k) for k in SE2] + [("se3", k) for k in SE3])
def test_block_of_node_0_is_the_inverse_of_the_prior(bank, name):
    """relative links carry no absolute information: (H^-1)[0, 0] = prior_information^-1 on every graph, for the default prior and
    for a general symmetric positive definite one.  The bound is the dense inverse's own: an entry of the computed H^-1 is good to
    cond(H) * 2^-52 * |H^-1|, taken relative to the block's largest entry as the difference is."""
    G = (SE2 if bank == "se2" else SE3)[name]()
    d = 3 if bank == "se2" else 6
    P = optimum(G)
    for prior in (None, spd(d, 5)):
        S = MM.system(G, P, prior)
        Hi = MM.dense_inverse(S)
        want = np.linalg.inv(100.0 * np.eye(d) if prior is None else prior)
        sv = np.linalg.svd(S.dense(), compute_uv=False)
        bound = (sv[0] / sv[-1]) * 2.0 ** -52 * (1.0 / sv[-1]) / np.max(np.abs(want))
        diff = MM.block_diff(Hi[0, 0], want)
        print("%s %s: (H^-1)[0, 0] off the prior's inverse by %.3g (cond(H) %.3g, allowed %.3g)" % (bank, name, diff, sv[0] / sv[-1], bound))
        assert diff <= bound


@pytest.mark.parametrize("dof,name", [(3, "two_nodes"), (3, "chain"), (6, "two_nodes"), (6, "chain")])
def test_relative_covariance_along_a_tree_link_is_the_links_own(dof, name):
    """on a tree the relative covariance along a link is that link's W^-1 = 0.01 I (to a few roundings of the dense inverse)"""
    G = MM.graphs(dof)[name][0]
    P = MM.optimised(dof, name)
    Hi = MM.dense_inverse(MM.system(G, P))
    rel = MM.relative_covariance if dof == 3 else MM.relative_covariance3
    for r, m in zip(G.ref, G.mov):
        R = rel(P[r], P[m], Hi[r, r], Hi[m, m], Hi[m, r])
        assert np.max(np.abs(R - 0.01 * np.eye(dof))) <= 1e-14, (r, m)


def test_a_loop_adds_information():
    """on the inconsistent ring the relative covariance of neighbours is strictly smaller than 0.01 I"""
    for dof, name in ((3, "ring_inconsistent"), (6, "helix_ring")):
        G = MM.graphs(dof)[name][0]
        P = MM.optimised(dof, name)
        Hi = MM.dense_inverse(MM.system(G, P))
        rel = MM.relative_covariance if dof == 3 else MM.relative_covariance3
        R = rel(P[0], P[1], Hi[0, 0], Hi[1, 1], Hi[1, 0])
        assert np.all(np.linalg.eigvalsh(0.01 * np.eye(dof) - 0.5 * (R + R.T)) > 1e-5)


def test_column_solve_is_the_optimisers_solve():
    """column_solve restates _System.pcg: with b the unit vector the two give the same bits"""
    for dof, name in ((3, "ring_wrap"), (6, "helix_ring")):
        G = MM.graphs(dof)[name][0]
        S = MM.system(G, MM.optimised(dof, name))
        x, it, capped = MM.column_solve(S, 3, 1)
        S.b = np.zeros_like(S.b)
        S.b[3, 1] = 1.0
        x2, it2, capped2 = S.pcg(1e-8, 2000)
        assert x.tobytes() == x2.tobytes() and (it, capped) == (it2, capped2) and it > 0
        _, it3, capped3 = MM.column_solve(S, 3, 1, max_linear_iterations=3)
        assert (it3, capped3) == (3, True)


def test_relabelling_keeps_the_problem():
    G = MM.graphs(3)["ring_wrap"][0]
    G2, new = MM.relabelled(G, 17)
    assert new[0] == 0 and sorted(new) == list(range(G.n_nodes)) and not np.array_equal(new, np.arange(G.n_nodes))
    P = MM.optimised(3, "ring_wrap")
    a, b = MM.system(G, P), MM.system(G2, P[np.argsort(new)])
    assert abs(a.cost - b.cost) <= 1e-12 * a.cost
    Ha, Hb = MM.dense_inverse(a), MM.dense_inverse(b)
    assert MM.block_diff(Hb[new[5], new[7]], Ha[5, 7]) <= 1e-11


@pytest.mark.parametrize("dof,name", [(3, k) for k in MM.FLOOR2] + [(6, k) for k in MM.FLOOR3])
def test_floors(dof, name):
    """the floors of the GPU tests' tolerance: the constants are the measured values, up to the factor 2 that another BLAS' rounding
    may move numbers this close to the last place"""
    a, b, its = MM.measure_floor(dof, name)
    floor = MM.floors(dof)[name]
    print("%s dof %d: column solve against the dense inverse %.3g, against itself relabelled %.3g (constant %.3g); %d to %d inner "
          "iterations a column" % (name, dof, a, b, floor, min(its), max(its)))
    assert floor / 2 <= max(a, b) <= 2 * floor
    assert max(its) < 2000
    assert set(MM.graphs(dof)) == set(MM.floors(dof))
