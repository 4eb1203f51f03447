"""NumPy model of the laser-scan projection (include/ndtgpu.h "laser-scan projection"; csrc/ndt_scanproject.h): the gate, the point
and the cloud of a batch of scans.  fp64 products rounded to float once; the cosine and sine are NumPy's, so x and y may differ from
another correctly working implementation by one float32 unit in the last place; the kept flags, the order, n_kept, z and the pads
are exact."""
import numpy as np

DEFAULTS = dict(r_min=0.5, r_max=30.0, varz=0.02, seed=0)       # gustav_laser_tf.launch:20-23


def hash_uniform(seed, scan_id, idx):
    """csrc/ndt_mcl.h ndt_hash_uniform(seed, scan_id, idx) through synth.hash_uniform (64-bit wrap-around arithmetic)"""
    import torch
    from ndt_feature_graph_amd import synth

    def i64(v):
        v = int(v) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v
    return synth.hash_uniform(i64(seed), i64(scan_id), torch.as_tensor(np.asarray(idx, dtype=np.int64))).numpy()


def kept(r, r_min=0.5, r_max=30.0):
    """finite and r_min < r < r_max, both strict"""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r) & (r > r_min) & (r < r_max)


def points(r, angle_min, angle_increment, scan_id=0, idx=None, r_min=0.5, r_max=30.0, varz=0.02, seed=0):
    """every beam's (kept flag, point float32 [n, 3]); beam k has index idx[k] (None: 0 .. n - 1); the point of a dropped beam is
    unspecified"""
    r = np.asarray(r, dtype=np.float64)
    i = np.arange(r.shape[0], dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    a = angle_min + i.astype(np.float64) * angle_increment
    rr = np.where(kept(r, r_min, r_max), r, 1.0)
    xyz = np.empty((r.shape[0], 3), dtype=np.float32)
    with np.errstate(over="ignore"):                 # (a range near the largest double becomes an infinite float, as in C)
        xyz[:, 0] = (rr * np.cos(a)).astype(np.float32)
        xyz[:, 1] = (rr * np.sin(a)).astype(np.float32)
    xyz[:, 2] = (varz * hash_uniform(seed, scan_id, i)).astype(np.float32)
    return kept(r, r_min, r_max), xyz


def project(ranges, angle_min, angle_increment, scan_ids=None, **params):
    """ranges [n, n_beams] -> (xyz float32 [n, n_beams, 3]: the kept points in beam order, NaN rows behind them; n_kept uint32 [n])"""
    ranges = np.asarray(ranges, dtype=np.float64)
    n, nb = ranges.shape
    prm = dict(DEFAULTS, **params)
    xyz = np.full((n, nb, 3), np.nan, dtype=np.float32)
    n_kept = np.zeros(n, dtype=np.uint32)
    for b in range(n):
        k, p = points(ranges[b], angle_min, angle_increment, scan_id=b if scan_ids is None else scan_ids[b], **prm)
        n_kept[b] = int(k.sum())
        xyz[b, :n_kept[b]] = p[k]
    return xyz, n_kept
