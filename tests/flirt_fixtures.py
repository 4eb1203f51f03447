"""The scans that the feature-extraction tests share (tests/test_flirt_model.py, tests/test_gpu_featextract.py): each is
(ranges float64 [n_beams], angle_min, angle_increment)."""
import math

import numpy as np

CORNER = (3.0, 4.0)
# the middle beam (90) of the L scan looks at the corner, so both walls get 90 beams and the corner itself is sampled
L_ANGLE_MIN = math.atan2(CORNER[1], CORNER[0]) - math.pi / 2.0
PLANTED = (0.3, -0.2, 0.1)


def l_corner(angle_min=L_ANGLE_MIN, n_beams=181):
    """walls x = 3 and y = 4 seen from the origin, 1 degree a beam, noise-free"""
    a = angle_min + np.arange(n_beams) * math.radians(1.0)
    c, s = np.cos(a), np.sin(a)
    rx = np.where(c > 1e-9, CORNER[0] / np.where(c > 1e-9, c, 1.0), np.inf)
    ry = np.where(s > 1e-9, CORNER[1] / np.where(s > 1e-9, s, 1.0), np.inf)
    return np.minimum(rx, ry), angle_min, math.radians(1.0)


def wall(n_beams=121, angle_min=math.radians(-60.0)):
    """the wall x = 3 alone, 1 degree a beam, noise-free"""
    a = angle_min + np.arange(n_beams) * math.radians(1.0)
    return 3.0 / np.cos(a), angle_min, math.radians(1.0)


def hall(seed, n_beams, pose=(0.0, 0.0, 0.0)):
    """synth.scan_2d_ranges of one hall: range noise 0.005 m"""
    from ndt_feature_graph_amd import synth
    r, a0, inc = synth.scan_2d_ranges([seed], [pose], n_beams, noise_sigma=0.005)
    return r[0].numpy(), a0, inc
