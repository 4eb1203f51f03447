"""The NumPy restatement of the extrinsic calibration (tests/calib_model.py) against what the reference's program does
(laser2d_extrinsic_calibration.cpp): the contract form of the score against the literal one, the lattice against the three loops, the
tie rule, the identity the kernel rests on, and the planted offset.  No device, no library."""
import math

import numpy as np
import pytest

import calib_fixtures as X
import calib_model as M

EPS = 2.0 ** -52


def T3(p):
    c, s = math.cos(p[2]), math.sin(p[2])
    return np.array([[c, -s, p[0]], [s, c, p[1]], [0.0, 0.0, 1.0]])


def random_pair(rng, n1, n2, spread):
    """two scans of the same random scene from two poses of a base that carries the sensor at ts; poses up to `spread` from the origin"""
    ts = (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2))
    pose1 = (rng.uniform(-spread, spread), rng.uniform(-spread, spread), rng.uniform(-3, 3))
    pose2 = (pose1[0] + rng.uniform(-0.4, 0.4), pose1[1] + rng.uniform(-0.4, 0.4), pose1[2] + rng.uniform(0.5, 1.0))
    world = np.concatenate([rng.uniform(-8, 8, size=(max(n1, n2), 2)) + np.array(pose1[:2]), rng.uniform(0.0, 0.02, size=(max(n1, n2), 1))], axis=1)
    clouds = []
    for pose, n in ((pose1, n1), (pose2, n2)):
        inv = np.linalg.inv(T3(pose) @ T3(ts))
        xy = world[:n, :2] @ inv[:2, :2].T + inv[:2, 2] + rng.normal(0, 0.02, size=(n, 2))
        clouds.append(np.concatenate([xy, world[:n, 2:3]], axis=1).astype(np.float32))
    return clouds[0], pose1, clouds[1], pose2, ts


@pytest.mark.parametrize("spread", [1.0, 30.0])
def test_contract_form_against_the_literal_form(spread):
    """The bound, from the coordinates' magnitude alone.  W bounds every world coordinate (pose + sensor offset + range).  A world
    coordinate of the literal form passes through at most 8 rounded fp64 operations on magnitudes <= 2 W, a coordinate of the
    contract form through no more, and a difference of two coordinates takes one of each cloud in each form: the two forms' coordinate
    differences disagree by at most delta = 64 eps W.  term = min(d2, th2) is 1-Lipschitz in d2 and the minimum over the neighbours is
    1-Lipschitz in each d2; where d2 <= th2 every |coordinate difference| <= th, so d2 moves by at most 3 (2 th delta + delta^2).
    n terms add that up, plus the rounding of the sums themselves, n eps times the largest possible sum n th2."""
    rng = np.random.default_rng(int(spread))
    th = 0.1
    worst = 0.0
    for case in range(6):
        n1, n2 = int(rng.integers(20, 60)), int(rng.integers(20, 60))
        c1, p1, c2, p2, ts = random_pair(rng, n1, n2, spread)
        lit = M.literal_score(c1, p1, c2, p2, ts, th)
        lat = dict(xs=np.array([ts[0]]), ys=np.array([ts[1]]), cs=np.array([math.cos(ts[2])]), sn=np.array([math.sin(ts[2])]))
        p4 = M.poses4([p1, p2])
        con = M.search([c1, c2], [n1, n2], p4, [(0, 1)], lat, th)["score"]
        W = spread + 0.4 + 0.5 + 8.0 * math.sqrt(2.0) + 1.0
        delta = 64 * EPS * W
        bound = n2 * 3 * (2 * th * delta + delta * delta) + n2 * EPS * (n2 * th * th)
        assert 0.0 < lit < n2 * th * th, "the case must have points within max_dist, or it checks nothing"
        assert abs(lit - con) <= bound, (case, lit, con, bound)
        worst = max(worst, abs(lit - con) / bound)
    print("largest |literal - contract| / bound: %.3g" % worst)


def replay_loops(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r):
    """the three for loops of bruteForceOptimization, literally: every (x, y, yaw) in loop order"""
    out = []
    x = ix - x_s
    while x < ix + x_s:
        y = iy - y_s
        while y < iy + y_s:
            yaw = iyaw - yaw_s
            while yaw < iyaw + yaw_s:
                out.append((x, y, yaw))
                yaw += yaw_r
            y += t_r
        x += t_r
    return out


@pytest.mark.parametrize("args", [X.LATTICE, (0.0, 0.0, 0.0, 0.05, 0.05, 0.04, 0.01, 0.001), (0.1, -0.2, 0.3, 0.3, 0.35, 0.2, 0.1, 0.07),
                                  (1.0, 2.0, -1.0, 0.01, 0.03, 0.5, 0.02, 1.0)])
def test_lattice_against_the_three_loops(args):
    lat = M.lattice(*args)
    want = replay_loops(*args)
    nx, ny, nyaw = len(lat["xs"]), len(lat["ys"]), len(lat["yaws"])
    assert len(want) == nx * ny * nyaw
    got = [(x, y, w) for x in lat["xs"] for y in lat["ys"] for w in lat["yaws"]]
    assert got == want                                                  # the same doubles in the same (linear index) order
    assert [math.cos(w) for w in lat["yaws"]] == lat["cs"].tolist() and [math.sin(w) for w in lat["yaws"]] == lat["sn"].tolist()


def test_rounding_decides_the_last_node():
    """0.19 - 0.1 + ten times 0.02 is 0.29 and 0.19 + 0.1 is 0.29000000000000004: an eleventh node exists that the real numbers do
    not have; 0.2 +- 0.05 by 0.01 has the ten they have"""
    assert len(M.lattice_axis(0.19, 0.1, 0.02)) == 11 and round(2 * 0.1 / 0.02) == 10
    assert M.lattice_axis(0.19, 0.1, 0.02)[-1] < 0.19 + 0.1
    assert len(M.lattice_axis(0.2, 0.05, 0.01)) == 10
    assert len(M.lattice(*X.LATTICE)["xs"]) == 11


def test_equal_scores_go_to_the_first_candidate():
    """pairs with D = I (the same pose twice, yaw 0: cd is exactly 1): every candidate's translation is exactly 0, all scores are
    equal bit for bit, and the strict < of the reference keeps the first: linear index 0"""
    rng = np.random.default_rng(3)
    c1 = rng.uniform(-3, 3, size=(30, 3)).astype(np.float32)
    c2 = (c1[:25] + rng.normal(0, 0.03, size=(25, 3))).astype(np.float32)
    lat = M.lattice(0.0, 0.0, 0.0, 0.3, 0.3, 0.2, 0.1, 0.1)
    p4 = M.poses4([(1.5, -2.0, 0.0), (1.5, -2.0, 0.0)])
    tx, ty = M.translations(M.pair_motion(p4[0], p4[1]), lat)
    assert (tx == 0.0).all() and (ty == 0.0).all()
    r = M.search([c1, c2], [30, 25], p4, [(0, 1)], lat)
    assert (r["volume"] == r["volume"].reshape(-1)[0]).all() and 0.0 < r["score"] < 25 * 0.01
    assert r["index"] == 0


def test_rotations_commute_so_a_candidate_is_a_translation():
    """|p1 a - p2 b| = |a - M b| with M = Ts^-1 D Ts, D = pose1^-1 pose2; M's rotation is D's, and its translation is
    R(-yaw) (t_D + (R_D - I) t_s), which is what the model's translations() evaluates"""
    rng = np.random.default_rng(11)
    for _ in range(20):
        p1, p2, ts = (rng.uniform(-5, 5, 3) for _ in range(3))
        a, b = rng.uniform(-10, 10, 2), rng.uniform(-10, 10, 2)
        P1, P2, Ts = T3(p1), T3(p2), T3(ts)
        D = np.linalg.inv(P1) @ P2
        Mx = np.linalg.inv(Ts) @ D @ Ts
        wa = (P1 @ Ts @ np.append(a, 1.0))[:2]
        wb = (P2 @ Ts @ np.append(b, 1.0))[:2]
        mb = (Mx @ np.append(b, 1.0))[:2]
        assert abs(np.linalg.norm(wa - wb) - np.linalg.norm(a - mb)) < 1e-12
        assert np.allclose(Mx[:2, :2], D[:2, :2], atol=1e-14)
        R = lambda t: np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
        t = R(-ts[2]) @ (D[:2, 2] + (D[:2, :2] - np.eye(2)) @ ts[:2])
        assert np.allclose(Mx[:2, 2], t, atol=1e-13)
        lat = dict(xs=np.array([ts[0]]), ys=np.array([ts[1]]), cs=np.array([math.cos(ts[2])]), sn=np.array([math.sin(ts[2])]))
        tx, ty = M.translations(M.pair_motion(M.poses4([p1])[0], M.poses4([p2])[0]), lat)
        assert abs(tx[0, 0, 0] - t[0]) < 1e-13 and abs(ty[0, 0, 0] - t[1]) < 1e-13


def test_select_pairs_walk():
    """one pair per turn of more than 25 degrees within a metre; a step of more than a metre resets the anchor without a pair"""
    deg = math.pi / 180.0
    poses = [(0, 0, 0), (0.1, 0, 10 * deg), (0.2, 0, 24.9 * deg), (0.3, 0, 25.1 * deg), (0.35, 0, 30 * deg), (2.0, 0, 80 * deg),
             (2.1, 0, 100 * deg), (2.2, 0.1, 50 * deg), (2.2, 0.1, 50 * deg), (2.0, 0.3, 76 * deg)]
    assert M.select_pairs(M.poses4(poses)).tolist() == [[0, 3], [5, 7], [7, 9]]
    assert M.select_pairs(M.poses4(poses[:1])).shape == (0, 2)
    assert X.planted()["pairs"].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]]


def test_planted_offset_wins_in_the_model():
    """Six 181-beam scans of hall 5 from a base 1.2 m inside a corner, the laser at (0.23, 0.02, 0.01) on it, five pairs, the
    11 x 10 x 4 lattice of calib_fixtures.LATTICE.  Measured with the model alone: the planted node (7, 6, 2) scores 1.7957, the best
    node that is not one of its neighbours 1.8839 (a margin of 0.088, 4.9 %), the second best node of all 1.8147, the worst 5.500.
    The margin is a condition on these inputs -- a scan set on which the model itself cannot tell the nodes apart would test
    nothing --, not a tolerance on any implementation."""
    f = X.planted()
    r = X.planted_model()
    v = r["volume"]
    idx = np.unravel_index(r["index"], v.shape)
    assert v.shape == (11, 10, 4) and tuple(int(i) for i in idx) == X.PLANTED_NODE
    lat = f["lattice"]
    assert abs(lat["xs"][idx[0]] - X.PLANTED[0]) < 1e-12 and abs(lat["ys"][idx[1]] - X.PLANTED[1]) < 1e-12
    assert abs(lat["yaws"][idx[2]] - X.PLANTED[2]) < 1e-12
    ii = np.indices(v.shape)
    far = (abs(ii[0] - idx[0]) > 1) | (abs(ii[1] - idx[1]) > 1) | (abs(ii[2] - idx[2]) > 1)
    print("planted %.4f, best non-neighbour %.4f, second %.4f, worst %.4f" % (r["score"], v[far].min(), np.sort(v.reshape(-1))[1], v.max()))
    assert v[far].min() - r["score"] > 0.05
    assert r["flags"] == 0 and r["n_skipped"] == 0
