"""The inputs that the calibration tests share (tests/test_calib_model.py, tests/test_gpu_calib.py): synthetic hall scans taken by a
laser that sits at a planted offset on a base which turns by more than 25 degrees within a metre between scans."""
import functools
import math

import numpy as np

import calib_model as M
import scanproject_model as P

PLANTED = (0.23, 0.02, 0.01)                      # the laser on the base: (x, y, yaw), a node of LATTICE
LATTICE = (0.19, 0.0, 0.01, 0.1, 0.1, 0.1, 0.02, 0.05)      # ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r: 10 x 10 x 4 nodes
PLANTED_NODE = (7, 6, 2)                          # xs[7] ~ 0.23, ys[6] ~ 0.02, yaws[2] ~ 0.01
# the base relative to a point CORNER metres inside a corner of the hall: near walls, where 181 beams still sample them more
# finely than max_dist.  Consecutive poses turn by more than 25 degrees within a metre: five pairs.
REL = ((0.0, 0.0, 0.0), (0.15, 0.05, 0.6), (0.25, -0.1, 1.3), (0.1, 0.15, 0.55), (-0.05, 0.0, -0.2), (0.1, 0.1, -0.9))
CORNER = 1.2
SEED = 5


def base_poses(seed=SEED):
    from ndt_feature_graph_amd import synth
    half, _ = synth.room_2d([seed])
    hx, hy = half[0].tolist()
    return tuple((hx - CORNER + x, hy - CORNER + y, t) for x, y, t in REL)


def sensor_poses(base, ts=PLANTED):
    """base o Ts for every base pose"""
    out = []
    for x, y, t in base:
        c, s = math.cos(t), math.sin(t)
        out.append((x + c * ts[0] - s * ts[1], y + s * ts[0] + c * ts[1], t + ts[2]))
    return out


@functools.lru_cache(maxsize=None)
def planted(n_beams=181, seed=SEED):
    """-> dict(ranges [n, n_beams], angle_min, angle_increment, xyz float32 [n, n_beams, 3], n_kept, poses4 [n, 4], pairs [m, 2],
    lattice): the clouds are tests/scanproject_model.py's of the ranges (kept rows in front of NaN pads, z jitter)"""
    from ndt_feature_graph_amd import synth
    base = base_poses(seed)
    sp = sensor_poses(base)
    r, a0, inc = synth.scan_2d_ranges([seed] * len(sp), sp, n_beams, noise_sigma=0.005)
    ranges = r.numpy()
    xyz, n_kept = P.project(ranges, a0, inc, r_min=0.3, r_max=20.0)       # the callback's gate (r > 0.3 && r < 20)
    p4 = M.poses4(base)
    return dict(ranges=ranges, angle_min=a0, angle_increment=inc, xyz=xyz, n_kept=n_kept, poses4=p4, pairs=M.select_pairs(p4),
                lattice=M.lattice(*LATTICE))


@functools.lru_cache(maxsize=None)
def planted_model(n_beams=181, seed=SEED):
    """the contract form's search of planted(): computed once, shared, not modified"""
    f = planted(n_beams, seed)
    r = M.search(f["xyz"], f["n_kept"], f["poses4"], f["pairs"], f["lattice"])
    r["volume"].setflags(write=False)
    return r
