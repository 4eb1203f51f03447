"""Inputs shared by tests/test_locmon_model.py, tests/test_locmon_abi.py (CPU) and tests/test_gpu_locmon.py: random occupancy grids
with every kind of pixel, query records, and the chain test's scene (chosen on the CPU, see CHAIN below)."""
import numpy as np

QUERY_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("c", "<f8"), ("s", "<f8"), ("scan", "<u4"), ("grid", "<u4")])

# The chain test (ranges -> ScanProjector -> MapSet.build -> occupancy grid -> distance field -> badness).  Chosen on the CPU with the
# oracle's cells (oracle.binding.OracleMap) rasterised by tests/occgrid_model.py and evaluated by tests/locmon_model.py: hall 4102 of
# synth.scan_2d_ranges seen from (0, 0, 0) with range noise 0.005 m, 1440 beams (all kept), a map of 120 x 120 x 2 cells of 0.5 m
# around the sensor, pixels of 0.1 m (600 x 600), max_dist 0.375 -> R = 3.  The oracle's map has 225 Gaussian cells, 5625 obstacle
# pixels; 97.8 % of the true pose's endpoints lie on obstacle pixels (key 0) and the median key is 0 (badness 0.0); from 3 m
# further along x the median key is 0x10000 (far, badness 0.375).  With 720 beams of the same hall only 35 % of the endpoints lie
# on obstacle pixels (too few points per cell for a Gaussian) and the median is 9: too sparse, not used.
CHAIN = dict(seed=4102, n_beams=1440, noise_sigma=0.005, map_res=0.5, size_m=(60.0, 60.0, 1.0), cells=(120, 120, 2), pixel=0.1,
             max_dist=0.375, r_min=0.5, r_max=30.0, displaced=(3.0, 0.0), key_true=0, key_displaced=0x10000, min_on_obstacle=0.75)


def random_grid(rng, h, w, p_occ):
    """unknown (-1), free (0), weakly occupied (30: no obstacle at 55) and occupied (55, 70, 100) pixels"""
    return rng.choice(np.array([-1, 0, 30, 55, 70, 100], dtype=np.int8), size=(h, w), p=[0.2, 0.8 - 3 * p_occ - 0.05, 0.05, p_occ, p_occ, p_occ])


def queries(scan, grid, x, y, yaw):
    cols = np.broadcast_arrays(scan, grid, x, y, yaw)
    q = np.zeros(cols[0].shape, dtype=QUERY_DTYPE).reshape(-1)
    q["scan"], q["grid"], q["x"], q["y"] = (np.asarray(c).reshape(-1) for c in cols[:4])
    q["c"], q["s"] = np.cos(np.asarray(cols[4], dtype=np.float64).reshape(-1)), np.sin(np.asarray(cols[4], dtype=np.float64).reshape(-1))
    return q
