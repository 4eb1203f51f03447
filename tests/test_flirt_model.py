"""The laser-scan feature extraction as tests/flirt_model.py restates it (include/ndtgpu.h "laser-scan feature extraction", steps
1-8), checked on scans whose answer is known: a corner, a wall, a rotated scan, a descriptor enumerated by hand, gaps, and the chain
scan -> features -> RANSAC pose (tests/featmatch_model.py).  No GPU; the last test needs the library for the C struct's defaults."""
import math

import numpy as np
import pytest

import featmatch_model as FM
import flirt_fixtures as X
import flirt_model as F


def test_l_corner_gives_one_point_at_the_corner():
    """Walls x = 3 and y = 4 from the origin, 181 beams at 1 degree, the middle beam on the corner: exactly one interest point,
    within one beam of the corner, theta within 0.1 rad of the inward bisector (-135 degrees), and a response near the closed form
    of the continuum, sqrt(2 / pi) sin(45 deg) = 0.5642.  Measured once on this model: response 0.61296 at level 4, that is
    0.0488 above the closed form, so the test allows twice that, 0.098; theta -2.44468, 0.0885 rad from the bisector (the wall at
    the shorter distance is sampled more densely and pulls the smoothed point to its side).  With the beams on whole degrees
    instead (angle_min -90 degrees) the point is beam 143 at (3, 3.981), response 0.59991 and theta 0.1010 rad from the bisector."""
    o = F.extract(*X.l_corner())
    assert o["status"] == F.OK and o["n_valid"] == 181 and o["n_segments"] == 1
    assert o["n_found"] == 1 and o["n_stored"] == 1
    assert abs(int(o["beam"][0]) - 90) <= 1
    # (one beam along the wall x = 3 at the corner: r^2 / 3 * 1 degree = 0.145 m)
    assert np.hypot(o["pos"][0, 0] - X.CORNER[0], o["pos"][0, 1] - X.CORNER[1]) <= 25.0 / 3.0 * math.radians(1.0)
    print("theta %.6f response %.6f level %d" % (o["pos"][0, 2], o["response"][0], o["level"][0]))
    assert abs(o["pos"][0, 2] - (-0.75 * math.pi)) < 0.1
    closed_form = math.sqrt(2.0 / math.pi) * math.sin(math.radians(45.0))
    assert abs(o["response"][0] - closed_form) <= 0.098
    assert o["desc"].shape == (1, 48) and np.all(o["desc"] > 0.0) and np.all(o["desc"] < 1.0)


def test_a_straight_wall_gives_no_point():
    o = F.extract(*X.wall())
    assert o["status"] == F.OK and o["n_valid"] == 121 and o["n_segments"] == 1
    assert o["n_peaks"] == 0 and o["n_found"] == 0 and o["pos"].shape == (0, 3)       # in particular none at the segment's ends


@pytest.mark.parametrize("scan", ["corner", "hall"])
@pytest.mark.parametrize("shift", [0.3, -1.234, 2.5])
def test_rotation_symmetry(scan, shift):
    r, a0, inc = X.l_corner() if scan == "corner" else X.hall(1, 360)
    a, b = F.extract(r, a0, inc), F.extract(r, a0 + shift, inc)
    assert min(a["margins"].values()) > 1e-9 and min(b["margins"].values()) > 1e-9
    assert a["n_found"] >= 1
    for f in ("status", "n_valid", "n_segments", "n_peaks", "n_found"):
        assert a[f] == b[f], f
    assert np.array_equal(a["beam"], b["beam"]) and np.array_equal(a["level"], b["level"])
    assert np.max(np.abs(a["response"] - b["response"])) <= 1e-12
    assert np.max(np.abs(a["desc"] - b["desc"])) <= 1e-12
    c, s = math.cos(shift), math.sin(shift)
    assert np.max(np.abs(c * a["pos"][:, 0] - s * a["pos"][:, 1] - b["pos"][:, 0])) <= 1e-12 * 30.0
    assert np.max(np.abs(s * a["pos"][:, 0] + c * a["pos"][:, 1] - b["pos"][:, 1])) <= 1e-12 * 30.0
    dth = b["pos"][:, 2] - a["pos"][:, 2] - shift
    assert np.max(np.abs(np.arctan2(np.sin(dth), np.cos(dth)))) <= 1e-12


def test_a_descriptor_enumerated_by_hand():
    """Keypoint K = (2, 0) with theta = 15 degrees, so that the directions along the x axis fall on sector centres: +x is sector 5,
    -x sector 11.  Rings: [0.02, 0.265), [0.265, 0.51), [0.51, 0.755), [0.755, 1); delta = 0.1225.  Three scan points:
      A = (2.1, 0): 0.1 from K along +x: ring 0, sector 5: HIT bin 5.  Its beam's samples x = 2.1 - 0.1225 u pass K at -0.0225,
        -0.145 (ring 0), -0.2675, -0.39 (ring 1), -0.5125, -0.635 (ring 2), -0.7575, -0.88 (ring 3), -1.0025 (outside): MISS bins
        11, 23, 35, 47.
      C = (5, 0): 3 from K: no hit.  Its samples x = 5 - 0.1225 u: u = 17 .. 24 are +0.9175, +0.795 (ring 3), +0.6725, +0.55 (ring
        2), +0.4275, +0.305 (ring 1), +0.1825, +0.06 (ring 0) in sector 5: MISS bins 41, 29, 17, 5; u = 25 .. 32 are -0.0625,
        -0.185, -0.3075, -0.43, -0.5525, -0.675, -0.7975, -0.92 in sector 11: MISS bins 11, 23, 35, 47; u = 16 and 33 are outside.
      B = (2.1, 0.6): (0.1, 0.6) from K, rho 0.608 (ring 2), 80.5 - 15 = 65.5 degrees (sector 8): HIT bin 32.  Its samples move
        towards the origin: u = 1, 2 stay in bin 32 (76.8 and 89.3 degrees, ring 2) -- the hit bin, no miss --, u = 3, 4 ring 2
        sector 9 (101.9, 113.6 degrees): bin 33; u = 5, 6 ring 2 sector 10: bin 34; u = 7, 8 ring 3 sector 10: bin 46; u = 9 is at
        rho 1.005, outside."""
    pts = np.array([[2.1, 0.0], [2.1, 0.6], [5.0, 0.0]])
    desc, hit, miss, margins = F.describe(pts, 2.0, 0.0, math.radians(15.0), dict(F.DEFAULTS))
    want_hit, want_miss = np.zeros(48, dtype=int), np.zeros(48, dtype=int)
    want_hit[[5, 32]] = 1
    want_miss[[11, 23, 35, 47]] = 2
    want_miss[[41, 29, 17, 5, 33, 34, 46]] = 1
    assert np.array_equal(hit, want_hit), np.nonzero(hit)
    assert np.array_equal(miss, want_miss), (np.nonzero(miss), miss[np.nonzero(miss)])
    assert min(margins.values()) > 1e-3
    assert desc[5] == 2.0 / 4.0 and desc[32] == 2.0 / 3.0 and desc[11] == 1.0 / 4.0 and desc[41] == 1.0 / 3.0 and desc[0] == 0.5
    assert np.array_equal(desc, (want_hit + 1.0) / (want_hit + want_miss + 2.0))


def test_gaps_and_segments():
    r, a0, inc = X.wall()
    far = r.copy()
    far[100:] += 3.0                                      # the last 21 beams see a wall 3 m behind: a gap above dmst = 2
    o = F.extract(far, a0, inc)
    assert o["n_segments"] == 2 and o["n_valid"] == 121
    assert np.array_equal(o["segment"], np.r_[np.zeros(100, dtype=int), np.ones(21, dtype=int)])
    one = r.copy()
    one[120] += 3.0                                       # a single point cut off is a segment of its own
    assert F.extract(one, a0, inc)["n_segments"] == 2
    hole = r.copy()
    hole[60] = float("nan")                               # a dropped beam in the middle of the wall: its neighbours are 0.105 m apart
    o = F.extract(hole, a0, inc)
    assert o["n_segments"] == 1 and o["n_valid"] == 120 and o["n_found"] == 0
    hole[61], hole[62] = float("inf"), 31.0               # (inf and out of range are dropped like NaN)
    o = F.extract(hole, a0, inc)
    assert o["n_segments"] == 1 and o["n_valid"] == 118
    few = np.full(121, float("nan"))
    few[[3, 50]] = 2.0
    o = F.extract(few, a0, inc)
    assert o["status"] == F.TOO_FEW_POINTS and o["n_valid"] == 2 and o["n_found"] == 0 and o["pos"].shape == (0, 3)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_chain_recovers_the_planted_pose(seed):
    """scan -> features -> RANSAC: two scans of one hall, 720 beams, from (0, 0, 0) and PLANTED; the pose that maps the second
    scan's features into the first's is PLANTED within 0.10 m and 0.01 rad (DESIGN.md 6f records the errors)."""
    a = F.extract(*X.hall(seed, 720))
    b = F.extract(*X.hall(seed, 720, X.PLANTED))
    assert 4 <= a["n_found"] <= 16 and 4 <= b["n_found"] <= 16
    m = FM.match(a["pos"], a["desc"], b["pos"], b["desc"], inlier_probability=0.5, success_probability=0.99)
    assert m["status"] == FM.OK
    print("seed %d: %d / %d points, errors %.4f m %.4f m %.5f rad" % (seed, a["n_found"], b["n_found"], m["x"] - X.PLANTED[0],
                                                                      m["y"] - X.PLANTED[1], m["theta"] - X.PLANTED[2]))
    assert abs(m["x"] - X.PLANTED[0]) < 0.10 and abs(m["y"] - X.PLANTED[1]) < 0.10 and abs(m["theta"] - X.PLANTED[2]) < 0.01


def test_overflow_keeps_the_first_points_in_beam_order():
    full = F.extract(*X.hall(1, 360))
    cut = F.extract(*X.hall(1, 360), max_points=4)
    assert full["n_found"] > 4 and cut["status"] == F.OVERFLOW and cut["n_found"] == full["n_found"] and cut["n_stored"] == 4
    assert np.array_equal(cut["beam"], full["beam"][:4]) and np.array_equal(cut["desc"], full["desc"][:4])


def test_the_c_defaults_are_flirtlib_utils():
    """ndtgpu_default_featextract_params against flirtlib_utils.h:15-42 (needs the library, no device)"""
    import ndt_feature_graph_amd as N
    from ndt_feature_graph_amd import binding
    N.build_library()
    p = binding.featextract_params()
    # SimpleMinMaxPeakFinder(0.34, 0.001); CurvatureDetector(peak, 5, 0.2, 1.4, 2.0); BetaGridGenerator(0.02, 1.0, 4, 12)
    assert (p.min_value, p.min_diff) == (0.34, 0.001)
    assert (p.scales, p.base_sigma, p.sigma_step, p.dmst) == (5, 0.2, 1.4, 2.0)
    assert (p.min_rho, p.max_rho, p.bin_rho, p.bin_phi) == (0.02, 1.0, 4, 12)
    assert (p.min_separation, p.r_min, p.r_max) == (0.2, 0.5, 30.0)
    assert {k: getattr(p, k) for k in F.DEFAULTS} == F.DEFAULTS
    with pytest.raises(TypeError):
        binding.featextract_params(no_such_field=1)
    with pytest.raises(TypeError):
        F.extract(*X.wall(), no_such_field=1)
