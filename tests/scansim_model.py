"""NumPy model of the scan simulator (include/ndtgpu.h "scan simulation", csrc/ndt_scansim.h): the reach, the cell of a point, the ray
of a beam, the cells of its steps by the closed form (vectorised over k), the stop rule, the scan record and the lattice of
reference poses.  Every fp64 expression is one NumPy operation per operation of the header, in its order; everything behind the two
cells of a ray is integer.  The device's outputs equal this model's bit for bit."""
import math

import numpy as np

OFFMAP, BAD_INDEX, NO_POSE = 1, 2, 4
MAX_DELTA = 32768.0
RESULT_DTYPE = np.dtype([("n_hits", "<u4"), ("flags", "<u4")])


def reach(range_max, resolution):
    q = math.floor(range_max / resolution)
    return int(q) if 1 <= q <= 4094 else 0


def skip_of(ref_pos_resolution, resolution):
    q = ref_pos_resolution / resolution
    return int(q) if 1.0 <= q < 32769.0 else 0


def beam_table(n_beams, angle_min, angle_increment):
    a = angle_min + np.arange(n_beams, dtype=np.float64) * angle_increment
    return np.cos(a), np.sin(a)


def headings(angle_step):
    th, theta = [], 0.0
    while theta < 6.28:
        th.append(theta)
        theta += angle_step
    th = np.array(th)
    return np.cos(th), np.sin(th)


def point_cell(px, py, origin, res, width, height):
    """(in the grid, i, j)"""
    with np.errstate(all="ignore"):
        fi = np.floor((np.float64(px) - origin[0]) / res)
        fj = np.floor((np.float64(py) - origin[1]) / res)
    if not (0 <= fi < width and 0 <= fj < height):
        return False, 0, 0
    return True, int(fi), int(fj)


def ray_cells(di, dj):
    """the cells of steps 1 .. n of a ray of (di, dj) cells, relative to its start: (a [n], b [n], m [n]); m the minor axis' advance"""
    ai, aj = abs(di), abs(dj)
    n = max(ai, aj)
    k = np.arange(1, n + 1, dtype=np.int64)
    si, sj = int(np.sign(di)), int(np.sign(dj))
    if ai >= aj:
        m = (2 * k * aj + n) // (2 * n) if n else k
        return si * k, sj * m, m
    m = (2 * k * ai + n) // (2 * n)
    return si * m, sj * k, m


def cell(di, dj, k):
    if k == 0:
        return 0, 0
    a, b, _ = ray_cells(di, dj)
    return int(a[k - 1]), int(b[k - 1])


def blocked(grid, occupied_min=55, unknown_is_obstacle=1):
    g = grid.astype(np.int64)
    return (g >= occupied_min) | ((g < 0) if unknown_is_obstacle else np.zeros(g.shape, dtype=bool))


def beam(grid, origin, res, pose, cb, sb, range_max=10.0, miss=11.0, occupied_min=55, unknown_is_obstacle=1):
    """one beam from a pose whose cell is in the grid -> (range, hit); None where the pose is off the map"""
    h, w = grid.shape
    x, y, c, s = (float(v) for v in pose)
    ok, i0, j0 = point_cell(x, y, origin, res, w, h)
    if not ok:
        return None
    R = reach(range_max, res)
    ex = c * cb - s * sb
    ey = s * cb + c * sb
    px = x + ex * range_max
    py = y + ey * range_max
    with np.errstate(all="ignore"):
        fdi = np.floor((np.float64(px) - origin[0]) / res) - float(i0)
        fdj = np.floor((np.float64(py) - origin[1]) / res) - float(j0)
    if not (abs(fdi) <= MAX_DELTA and abs(fdj) <= MAX_DELTA):
        return miss, 0
    a, b, m = ray_cells(int(fdi), int(fdj))
    if a.shape[0] == 0:
        return miss, 0
    i, j = i0 + a, j0 + b
    inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
    d2 = a * a + b * b
    stop_miss = ~inside | (d2 > R * R)
    v = blocked(grid[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)], occupied_min, unknown_is_obstacle)
    stop = stop_miss | v
    if not stop.any():
        return miss, 0
    first = int(np.argmax(stop))
    if stop_miss[first]:
        return miss, 0
    return float(res * np.sqrt(np.float64(d2[first]))), 1


def simulate(grids, origins, res, poses, cb, sb, grid_idx=None, count=None, **prm):
    """grids int8 [n_grids, height, width] -> (ranges [n_poses, n_beams], RESULT_DTYPE [n_poses])"""
    grids = np.asarray(grids, dtype=np.int8)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4)
    miss = prm.get("miss", 11.0)
    n, nb = poses.shape[0], len(cb)
    ranges = np.full((n, nb), miss)
    rec = np.zeros(n, dtype=RESULT_DTYPE)
    for p in range(n):
        if count is not None and p >= count:
            rec[p]["flags"] = NO_POSE
            continue
        g = 0 if grid_idx is None else int(grid_idx[p])
        if g >= grids.shape[0]:
            rec[p]["flags"] = BAD_INDEX
            continue
        hits = 0
        for bi in range(nb):
            out = beam(grids[g], origins[g], res, poses[p], float(cb[bi]), float(sb[bi]), **prm)
            if out is None:
                rec[p]["flags"] = OFFMAP
                break
            ranges[p, bi] = out[0]
            hits += out[1]
        rec[p]["n_hits"] = hits
    return ranges, rec


def lattice(grid, origin, res, skip, cs, sn, box=None, capacity=None):
    """-> dict(poses [written, 4], index [written], written, passed)"""
    h, w = grid.shape
    box = (-math.inf, -math.inf, math.inf, math.inf) if box is None else box
    npx, npy, nyaw = (w + skip - 1) // skip, (h + skip - 1) // skip, len(cs)
    px, py = np.meshgrid(np.arange(npx), np.arange(npy), indexing="ij")
    ix, iy = px * skip, py * skip
    cx = origin[0] + (ix.astype(np.float64) + 0.5) * res
    cy = origin[1] + (iy.astype(np.float64) + 0.5) * res
    keep = (grid[iy, ix] == 0) & (cx >= box[0]) & (cx <= box[2]) & (cy >= box[1]) & (cy <= box[3])
    pos = np.flatnonzero(keep.reshape(-1))
    poses = np.zeros((pos.shape[0], nyaw, 4))
    poses[:, :, 0] = cx.reshape(-1)[pos][:, None]
    poses[:, :, 1] = cy.reshape(-1)[pos][:, None]
    poses[:, :, 2] = np.asarray(cs)[None, :]
    poses[:, :, 3] = np.asarray(sn)[None, :]
    index = (pos[:, None] * nyaw + np.arange(nyaw)[None, :]).reshape(-1).astype(np.uint32)
    passed = index.shape[0]
    written = passed if capacity is None else min(passed, capacity)
    return dict(poses=poses.reshape(-1, 4)[:written], index=index[:written], written=written, passed=passed)
