"""The NumPy model of the world-map assembly (tests/world_model.py) against an independent route: every Gaussian expanded into an
explicit point set with that mean and sample covariance, the sets of a cell concatenated, np.mean / np.cov of the lot."""
import itertools

import numpy as np
import pytest

import world_model as W

RES = 0.5
CELLS = [8, 8, 8]
CENTRE = [0.0, 0.0, 0.0]


def point_set(rng, mean, cov, n):
    """n >= 4 points whose np.mean is `mean` and whose np.cov (ddof 1) is `cov`, to rounding"""
    X = rng.normal(size=(n, 3))
    X -= X.mean(axis=0)
    L = np.linalg.cholesky(np.cov(X.T))
    X = X @ np.linalg.inv(L).T @ np.linalg.cholesky(cov).T
    return X + mean


def spd(rng, scale):
    A = rng.normal(size=(3, 3))
    return scale * (A @ A.T + 0.3 * np.eye(3))


def pose(rng, t_scale=0.3):
    a, b, c = rng.uniform(-1, 1, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = rng.uniform(-t_scale, t_scale, 3)
    return T


def one_cell_nodes(rng, k, n_lo=4, n_hi=40):
    """k single-cell nodes whose moved means all fall into the cell [0.25, 0.75)^3 (LazyGrid cells are centred on multiples of res)"""
    nodes, poses = [], []
    for _ in range(k):
        T = pose(rng)
        target = np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.2, 0.2, 3)
        mean = T[:3, :3].T @ (target - T[:3, 3])
        nodes.append((mean[None], spd(rng, 0.004)[None], np.array([rng.integers(n_lo, n_hi)])))
        poses.append(T)
    return nodes, poses


def test_merge_equals_mean_and_cov_of_the_concatenated_point_sets():
    rng = np.random.default_rng(11)
    nodes, poses = one_cell_nodes(rng, 5)
    out = W.assemble(nodes, poses, RES, CENTRE, CELLS, eval_factor=1e12)      # (no eigenvalue is raised: cov == cov_raw)
    assert len(out["cells"]) == 1 and out["n_dropped"] == 0 and out["n_rejected"] == 0
    cell = next(iter(out["cells"].values()))
    pts = []
    for (mean, cov, n), T in zip(nodes, poses):
        X = point_set(rng, mean[0], cov[0], int(n[0]))
        assert np.allclose(X.mean(axis=0), mean[0], atol=1e-12) and np.allclose(np.cov(X.T), cov[0], atol=1e-12)
        pts.append(X @ T[:3, :3].T + T[:3, 3])
    pts = np.concatenate(pts)
    assert cell["N"] == cell["n"] == pts.shape[0] == out["n_points"] and cell["count"] == 5
    assert np.allclose(cell["mean"], pts.mean(axis=0), rtol=0, atol=1e-11)
    assert np.allclose(cell["cov_raw"], np.cov(pts.T), rtol=0, atol=1e-11)
    assert np.array_equal(cell["cov"], cell["cov_raw"])
    mb, cb = W.error_bounds(out["s1_shift"], out["s2_shift"], cell["N"], 5, RES, CELLS)
    assert mb < 1e-11 and cb < 1e-11


def test_a_single_contribution_reproduces_itself():
    rng = np.random.default_rng(3)
    mean, cov = np.array([[0.31, -0.62, 0.12]]), spd(rng, 0.003)[None]
    out = W.assemble([(mean, cov, np.array([17]))], [np.eye(4)], RES, CENTRE, CELLS)
    cell = next(iter(out["cells"].values()))
    mb, cb = W.error_bounds(out["s1_shift"], out["s2_shift"], 17, 1, RES, CELLS)
    assert cell["n"] == 17 and np.abs(cell["mean"] - mean[0]).max() <= mb
    assert np.abs(cell["cov_raw"] - cov[0]).max() <= cb
    ref = W.rescale_covariance(cov[0], 1000.0)
    assert np.abs(cell["cov"] - ref).max() <= 4 * cb


def test_two_identical_contributions():
    rng = np.random.default_rng(4)
    mean, cov, n = np.array([[0.4, 0.45, 0.6]]), spd(rng, 0.003)[None], 9
    out = W.assemble([(mean, cov, np.array([n]))] * 2, [np.eye(4)] * 2, RES, CENTRE, CELLS, eval_factor=1e12)
    cell = next(iter(out["cells"].values()))
    # (N - 1) C = 2 (n - 1) Sigma: the mean does not move, the covariance shrinks by (2n - 2) / (2n - 1)
    assert cell["N"] == 2 * n and np.allclose(cell["mean"], mean[0], atol=1e-12)
    assert np.allclose(cell["cov_raw"], cov[0] * (2 * n - 2) / (2 * n - 1), rtol=0, atol=1e-12)


def test_small_counts_merge_as_two_points():
    # rank-one covariances: a 2-point set has one -- mean +- d with d d^T * 2 = Sigma
    d1, d2 = np.array([0.05, 0.02, -0.01]), np.array([-0.03, 0.04, 0.02])
    m1, m2 = np.array([0.45, 0.55, 0.4]), np.array([0.55, 0.45, 0.5])
    nodes = lambda n: [(m1[None], (2 * np.outer(d1, d1))[None], np.array([n])), (m2[None], (2 * np.outer(d2, d2))[None], np.array([n]))]
    a = W.assemble(nodes(1), [np.eye(4)] * 2, RES, CENTRE, CELLS, eval_factor=1e12)
    b = W.assemble(nodes(2), [np.eye(4)] * 2, RES, CENTRE, CELLS, eval_factor=1e12)
    z = W.assemble(nodes(0), [np.eye(4)] * 2, RES, CENTRE, CELLS, eval_factor=1e12)
    assert a["sums"] == b["sums"] == z["sums"] and a["n_points"] == 4 and a["n_bound"] == 4
    pts = np.stack([m1 + d1, m1 - d1, m2 + d2, m2 - d2])
    (slot, (N, s1, s2)), = a["sums"].items()
    assert N == 4
    # (the pooled covariance of four coplanar points is rank deficient: no Gaussian, but the moments are those of the points)
    u = pts / RES - np.floor(pts / RES + 0.5)[0]
    assert np.allclose(np.array(s1) * 2.0 ** -a["s1_shift"], u.sum(axis=0), atol=1e-12)
    S = u.T @ u
    assert np.allclose(np.array(s2) * 2.0 ** -a["s2_shift"], [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]], atol=1e-12)
    # a third, full-rank contribution makes it a Gaussian with N = 2 + 2 + n
    rng = np.random.default_rng(5)
    full = (np.array([[0.5, 0.5, 0.5]]), spd(rng, 0.002)[None], np.array([6]))
    c = W.assemble(nodes(1) + [full], [np.eye(4)] * 3, RES, CENTRE, CELLS)
    assert next(iter(c["cells"].values()))["N"] == 10


def test_maxnumpoints_clamps_the_stored_count_only_at_the_end():
    rng = np.random.default_rng(6)
    nodes, poses = one_cell_nodes(rng, 4, 30, 40)
    free = W.assemble(nodes, poses, RES, CENTRE, CELLS, maxnumpoints=0)
    clamped = W.assemble(nodes, poses, RES, CENTRE, CELLS, maxnumpoints=50)
    a, b = next(iter(free["cells"].values())), next(iter(clamped["cells"].values()))
    assert a["n"] == a["N"] > 50 and b["n"] == 50 and b["N"] == a["N"]
    assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["cov"], b["cov"])
    assert W.DEFAULTS["maxnumpoints"] == 1e5                                    # fuser_hmt.cpp:486


def test_integer_sums_do_not_depend_on_the_order():
    rng = np.random.default_rng(7)
    nodes, poses = one_cell_nodes(rng, 4)
    ref = W.assemble(nodes, poses, RES, CENTRE, CELLS)
    for perm in itertools.permutations(range(4)):
        out = W.assemble([nodes[i] for i in perm], [poses[i] for i in perm], RES, CENTRE, CELLS)
        assert out["sums"] == ref["sums"] and (out["s1_shift"], out["s2_shift"]) == (ref["s1_shift"], ref["s2_shift"])
        for s in ref["cells"]:
            assert np.array_equal(out["cells"][s]["mean"], ref["cells"][s]["mean"])
            assert np.array_equal(out["cells"][s]["cov"], ref["cells"][s]["cov"])


def test_drops_rejections_and_face_distances():
    rng = np.random.default_rng(8)
    mean = np.array([[0.5, 0.5, 0.5], [5.0, 0.0, 0.0], [0.1, 0.1, 0.1], [np.nan, 0.0, 0.0], [0.2500000000001, 0.5, 0.5]])
    cov = np.stack([spd(rng, 0.002), spd(rng, 0.002), 50.0 * np.eye(3), spd(rng, 0.002), spd(rng, 0.002)])
    out = W.assemble([(mean, cov, np.full(5, 8))], [np.eye(4)], RES, CENTRE, CELLS)
    assert list(out["contribution_slot"][1:4]) == [W.DROPPED, W.REJECTED, W.REJECTED]
    assert (out["n_dropped"], out["n_rejected"], out["n_contributions"], out["n_points"]) == (1, 2, 5, 16)
    assert out["face_distance"][0] == pytest.approx(0.5) and 0 < out["face_distance"][4] < 1e-9
    assert out["contribution_slot"][0] == out["contribution_slot"][4] == ((5 * 8) + 5) * 8 + 5


def test_shifts_are_the_builds():
    assert W.build_shifts([40, 40, 2], 2000) == (45, 45) and W.build_shifts([40, 40, 1], 2000) == (45, 45)
    assert W.build_shifts([40, 40, 2], 1 << 20) == (42, 42) and W.build_shifts([40, 40, 1], 1 << 20) == (40, 38)
    assert W.grid_cells(0.5, [20, 20, 0.5]) == [40, 40, 1]


def test_the_baseline_route_agrees_with_the_model():
    rng = np.random.default_rng(9)
    nodes, poses = one_cell_nodes(rng, 6)
    out = W.assemble(nodes, poses, RES, CENTRE, CELLS)
    mean, cov = W.baseline_merge(nodes, poses, RES, CENTRE, CELLS)
    cell = next(iter(out["cells"].values()))
    assert mean.shape == (1, 3) and np.allclose(mean[0], cell["mean"], atol=1e-12) and np.allclose(cov[0], cell["cov"], atol=1e-12)


def test_the_planar_case_has_no_contribution_on_a_cell_face():
    """the seed of the device test's three-node case (world_model.PLANAR_SEED), checked here: no moved mean lies within FACE_EPS of
    a face of the world grid, so the device and the model bin every contribution alike"""
    scans = W.planar_scans()
    ncells, wcells = W.grid_cells(W.NODE_RES, W.NODE_SIZE_M), W.grid_cells(W.NODE_RES, W.WORLD_SIZE_M)
    assert ncells == [40, 40, 1] and wcells == [96, 96, 1]
    nodes = [W.numpy_node_cells(s, W.NODE_RES, [0, 0, 0], ncells) for s in scans]
    assert all(nd[0].shape[0] > 10 for nd in nodes)
    out = W.assemble(nodes, [W.pose2d(*p) for p in W.PLANAR_POSES], W.NODE_RES, [0, 0, 0], wcells)
    assert out["n_contributions"] == sum(nd[0].shape[0] for nd in nodes) and out["n_rejected"] == 0
    assert (out["face_distance"] >= W.FACE_EPS).all()
    assert max(c["count"] for c in out["cells"].values()) >= 2           # the nodes do overlap
