"""Inputs shared by tests/test_scansim_model.py, tests/test_scansim_abi.py (CPU) and tests/test_gpu_scansim.py: the room of the
simulation tests, its poses, random grids with every kind of pixel, and the chain test's scene (chosen on the CPU, see CHAIN)."""
import math

import numpy as np

RES = 0.05
ROOM_W, ROOM_H = 65, 67                       # an odd width puts every row at another alignment
ROOM_ORIGIN = (-1.0, -2.0)


def room():
    """int8 [67, 65]: walls (100) with a doorway, two posts (70, 55), a weak wall (30: no obstacle), an unknown patch (-1), free elsewhere"""
    g = np.zeros((ROOM_H, ROOM_W), dtype=np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    g[0, 25:35] = 0                                  # a doorway: rays leave the map through it
    g[30, 40:50] = 70
    g[12:15, 20:23] = 55
    g[45:48, 8:30] = 30
    g[50:58, 44:52] = -1
    return g


def second_room():
    """another grid of the same size: the room turned upside down with one more post"""
    g = room()[::-1].copy()
    g[33:36, 30:33] = 100
    return g


def centre(i, j, origin=ROOM_ORIGIN, res=RES):
    return origin[0] + (i + 0.5) * res, origin[1] + (j + 0.5) * res


def room_poses():
    """24 poses (x, y, c, s) and their grid indices: interior, rim, off the map, on an obstacle, on unknown, a grid index out of range"""
    rng = np.random.default_rng(7)
    rows, gi = [], []
    for k in range(12):                               # interior, any point of a cell, any heading; every other one near the left wall
        x, y = ROOM_ORIGIN[0] + rng.uniform(2, 5 if k % 2 else ROOM_W - 2) * RES, ROOM_ORIGIN[1] + rng.uniform(2, ROOM_H - 2) * RES
        th = rng.uniform(-math.pi, math.pi)
        rows.append((x, y, math.cos(th), math.sin(th)))
        gi.append(0)
    for (i, j, th) in ((1, 1, 0.3), (ROOM_W - 2, ROOM_H - 2, -2.0), (30, 5, 0.0), (ROOM_W - 1, 33, math.pi)):    # the rim; (30, 5): beam 0 leaves by the doorway
        rows.append(centre(i, j) + (math.cos(th), math.sin(th)))
        gi.append(0)
    rows += [(50.0, 50.0, 1.0, 0.0), (ROOM_ORIGIN[0] - 1e-9, 0.0, 1.0, 0.0), (float("nan"), 0.0, 1.0, 0.0)]             # off the map
    gi += [0, 0, 0]
    rows += [centre(44, 30) + (0.0, 1.0), centre(21, 13) + (1.0, 0.0)]                                                  # on an obstacle
    gi += [0, 0]
    rows += [centre(47, 53) + (math.cos(2.5), math.sin(2.5))]                                                           # on unknown
    gi += [0]
    rows += [centre(30, 30) + (1.0, 0.0), centre(30, 30) + (1.0, 0.0)]                                                  # grid 1, grid 2 (out of range)
    gi += [1, 2]
    assert len(rows) == 24
    return np.array(rows, dtype=np.float64), np.array(gi, dtype=np.uint32)


# The chain test (grid -> lattice -> simulated reference scans and one current scan -> FLIRT extraction -> RANSAC match -> pick ->
# badness).  Chosen on the CPU with tests/scansim_model.py, flirt_model.extract (r_min 0.02, r_max 10.5: a miss of 11.0 is dropped),
# featmatch_model.match (inlier_probability 0.25: the default 0.1 asks for 20 candidates) and locmon_model: a hall of 6 m x 5 m at
# 0.05 m (120 x 100 pixels: 10961 free, 963 obstacle, 76 unknown) with six pillars and two buttresses, 181 beams over +- pi / 2,
# range_max 10 (R = 200), skip 20 (1 m) and headings by angle_step 3.2 (theta 0 and 3.2).  The models gave: 38 lattice poses (19
# positions kept of 30); every beam of every pose hits; stored features per pose 0 .. 12, [9, 5, 12, 5, 9, 5, 6, 4, 9, 3, 8, 7, 7, 8,
# 6, 8, 7, 11, 12, 6, 11, 0, 10, 8, 3, 2, 8, 9, 5, 10, 3, 4, 2, 7, 2, 8, 2, 9]; the scan of pose 2, (-1.975, -0.475, heading 0),
# against every reference: 12 inliers and the identity against reference 2 (12 > min_num_matches 8), status TOO_FEW against each of
# the other 37, so no pose ties; the badness of the picked pose is 0.0 (median key 0, all 181 beams kept), below 0.25.
CHAIN = dict(width=120, height=100, origin=(-3.0, -2.5), n_beams=181, angle_min=-math.pi / 2, angle_increment=math.pi / 180, range_max=10.0,
             miss=11.0, skip=20, angle_step=3.2, capacity=48, n_passed=38, chosen=2, chosen_pose=(-1.975, -0.475, 1.0, 0.0), n_stored=12,
             n_inliers=12, extract=dict(r_min=0.02, r_max=10.5), match=dict(inlier_probability=0.25), max_points=64, max_dist=0.375,
             key=0, badness_below=0.25)


def chain_grid():
    c = CHAIN
    g = np.zeros((c["height"], c["width"]), dtype=np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    for (i, j, a, b) in ((30, 25, 8, 6), (70, 20, 6, 10), (50, 55, 10, 8), (90, 60, 7, 7), (20, 70, 9, 5), (75, 80, 5, 9)):    # pillars
        g[j:j + b, i:i + a] = 100
    g[40:60, 1:6] = 100          # a buttress on the left wall
    g[94:99, 55:75] = 100        # and one on the top wall
    g[60:64, 100:119] = -1
    return g


def random_grid(rng, h, w, p_occ):
    """unknown (-1), free (0), weakly occupied (30) and occupied (55, 70, 100) pixels"""
    return rng.choice(np.array([-1, 0, 30, 55, 70, 100], dtype=np.int8), size=(h, w), p=[0.05, 0.9 - 3 * p_occ, 0.05, p_occ, p_occ, p_occ])


def assert_not_vacuous(rec, n_beams, R):
    """on the model's records of room_poses(): among the poses that are on the map, at least a quarter of the beams hit and at least
    one misses.  A reach of one cell allows no quarter (of the 20 poses on the map only those beside a wall, a post or the patch can
    hit at all): there, at least one hit and one miss."""
    on_map = rec["flags"] == 0
    hits, total = int(rec["n_hits"][on_map].sum()), int(on_map.sum()) * n_beams
    assert on_map.sum() == 20
    assert hits < total, (n_beams, R, hits, total)
    assert (hits >= 1) if R == 1 else (4 * hits >= total), (n_beams, R, hits, total)
