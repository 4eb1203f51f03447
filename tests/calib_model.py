"""NumPy restatement of the laser-to-base extrinsic calibration (include/ndtgpu.h "extrinsic calibration",
csrc/ndt_calib.h): the checker of tests/test_calib_model.py, tests/test_calib_abi.py and tests/test_gpu_calib.py.

Two forms of the score:
  contract form  the arithmetic of csrc/ndt_calib.h operation for operation -- fp64 on the float32 coordinates, cloud1 as it is,
                 cloud2 rotated once per pair and translated per candidate, every sum sequential (a cumsum / a loop).  Nothing is
                 pruned: every row of cloud1 is visited for every row of cloud2.  The device's scores equal it bit for bit.
  literal form   what laser2d_extrinsic_calibration.cpp:85-122 does: both clouds moved into the world frame by pose Ts, then the
                 nearest neighbour (brute force, in fp64).
NumPy evaluates a * b + c as a product and a sum, each rounded: no contraction."""
import math

import numpy as np

CAP = 1e6


def lattice_axis(centre, span, step):
    """for (double v = centre - span; v < centre + span; v += step), literally"""
    out = []
    v = centre - span
    end = centre + span
    while v < end:
        out.append(v)
        v += step
    return np.array(out, dtype=np.float64)


def lattice(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r):
    yaws = lattice_axis(iyaw, yaw_s, yaw_r)
    return dict(xs=lattice_axis(ix, x_s, t_r), ys=lattice_axis(iy, y_s, t_r), yaws=yaws,
                cs=np.array([math.cos(v) for v in yaws]), sn=np.array([math.sin(v) for v in yaws]))


def poses4(xyyaw):
    """(x, y, yaw) [n, 3] -> (x, y, cos, sin) [n, 4]"""
    p = np.asarray(xyyaw, dtype=np.float64).reshape(-1, 3)
    return np.stack([p[:, 0], p[:, 1], np.array([math.cos(t) for t in p[:, 2]]), np.array([math.sin(t) for t in p[:, 2]])], axis=1)


def pair_motion(p1, p2):
    """D = pose1^-1 pose2 as (dx, dy, cd, sd), the order of ndt_calib_pair_motion"""
    p1 = np.asarray(p1, dtype=np.float64)
    p2 = np.asarray(p2, dtype=np.float64)
    ex, ey = p2[0] - p1[0], p2[1] - p1[1]
    return np.array([p1[2] * ex + p1[3] * ey, p1[2] * ey - p1[3] * ex, p1[2] * p2[2] + p1[3] * p2[3], p1[2] * p2[3] - p1[3] * p2[2]])


def select_pairs(p4, max_translation=1.0, min_yaw=25.0 * math.pi / 180.0):
    """the callback's anchor and gate walk (laser2d_extrinsic_calibration.cpp:312-349) with the robust yaw"""
    p4 = np.asarray(p4, dtype=np.float64).reshape(-1, 4)
    pairs, anchor = [], 0
    for k in range(1, p4.shape[0]):
        D = pair_motion(p4[anchor], p4[k])
        if math.sqrt(D[0] * D[0] + D[1] * D[1]) > max_translation:
            anchor = k
            continue
        if math.acos(min(1.0, max(-1.0, D[2]))) < min_yaw:
            continue
        pairs.append((anchor, k))
        anchor = k
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def usable_rows(cloud, n_kept):
    """the rows in front of n_kept whose coordinates are all finite, in order, as float64 [m, 3]; and how many were skipped"""
    c = np.asarray(cloud, dtype=np.float32)[:min(int(n_kept), len(cloud)), :3]
    ok = np.isfinite(c).all(axis=1)
    return c[ok].astype(np.float64), int((~ok).sum())


def translations(D, lat):
    """t(Ts) of every candidate -> (tx, ty) [nx, ny, nyaw], the order of ndt_calib_translation"""
    xs = lat["xs"][:, None, None]
    ys = lat["ys"][None, :, None]
    c = lat["cs"][None, None, :]
    s = lat["sn"][None, None, :]
    ux = D[0] + (D[2] * xs - D[3] * ys) - xs
    uy = D[1] + (D[3] * xs + D[2] * ys) - ys
    return c * ux + s * uy, c * uy - s * ux


def pair_volume(a, b, D, lat, th2, block=2048):
    """the contract form of one pair over the whole lattice -> float64 [nx, ny, nyaw].  a, b: usable rows float64 [n, 3]"""
    tx, ty = translations(D, lat)
    shape = tx.shape
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros(shape)
    brx = D[2] * b[:, 0] - D[3] * b[:, 1]
    bry = D[3] * b[:, 0] + D[2] * b[:, 1]
    tx, ty = tx.reshape(-1), ty.reshape(-1)
    out = np.zeros(tx.shape[0])
    for c0 in range(0, tx.shape[0], block):
        cx = brx[None, :] + tx[c0:c0 + block, None]                   # [C, nb]
        cy = bry[None, :] + ty[c0:c0 + block, None]
        m = None
        for i in range(a.shape[0]):                                   # the minimum over the rows of a (order free: no NaN)
            ex, ey, ez = a[i, 0] - cx, a[i, 1] - cy, a[i, 2] - b[None, :, 2]
            d = (ex * ex + ey * ey) + ez * ez
            m = d if m is None else np.minimum(m, d)
        term = np.where(m > th2, th2, m)
        out[c0:c0 + block] = np.cumsum(term, axis=1)[:, -1]           # sequential, in row order, from 0.0 (0.0 + t0 is t0)
    return out.reshape(shape)


def search(clouds, n_kept, p4, pairs, lat, max_dist=0.1):
    """the contract form of ndtgpu_calib_search -> dict(volume [nx, ny, nyaw], index, score, flags, n_skipped)"""
    th2 = max_dist * max_dist
    p4 = np.asarray(p4, dtype=np.float64).reshape(-1, 4)
    vol, skipped = None, 0
    for i1, i2 in np.asarray(pairs).reshape(-1, 2):
        a, s1 = usable_rows(clouds[i1], n_kept[i1])
        b, s2 = usable_rows(clouds[i2], n_kept[i2])
        skipped += s1 + s2
        v = pair_volume(a, b, pair_motion(p4[i1], p4[i2]), lat, th2)
        vol = (0.0 + v) if vol is None else vol + v                    # in pair order, from 0.0
    index = int(np.argmin(vol.reshape(-1)))                           # (the first of the smallest: the lowest linear index)
    score = float(vol.reshape(-1)[index])
    return dict(volume=vol, index=index, score=score, flags=1 if score >= CAP else 0, n_skipped=skipped)


def literal_score(cloud1, pose1, cloud2, pose2, ts, max_dist=0.1):
    """scoreICP as the reference writes it, in fp64: poses (x, y, yaw), ts = (x, y, yaw); clouds float [n, 3] of usable rows"""
    def T(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return np.array([[c, -s, p[0]], [s, c, p[1]], [0.0, 0.0, 1.0]])
    th2 = max_dist * max_dist
    e = 0.0
    if len(cloud1) == 0:
        return e
    w = []
    for cloud, pose in ((cloud1, pose1), (cloud2, pose2)):
        M = T(pose) @ T(ts)
        c = np.asarray(cloud, dtype=np.float64)
        xy = c[:, :2] @ M[:2, :2].T + M[:2, 2]
        w.append(np.concatenate([xy, c[:, 2:3]], axis=1))
    for q in w[1]:
        d = ((w[0] - q) ** 2).sum(axis=1).min()
        e += th2 if d > th2 else d
    return e
