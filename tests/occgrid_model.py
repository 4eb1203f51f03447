"""NumPy model of the occupancy-grid export (include/ndtgpu.h "occupancy-grid export"): lslgeneric::toOccupancyGrid restated,
written from the semantics and independently of csrc/ndt_occgrid.hip (vectorised over the whole grid, LU inverse from
numpy.linalg instead of the adjugate).  Input: the cells a map exports (export_cells: mean, cov, idx) and optionally its
occupancies (export_occupancy); output: the grid, per pixel the real-valued 100 v, and the distance of the pixel centre to the
nearest cell face -- what the comparison band of tests/test_gpu_occgrid.py is defined on."""
import numpy as np

VALUE_BAND = 1e-8        # |100 v - nearest integer|: the device's exp and quadratic form may differ from NumPy's by a few ulps
FACE_BAND = 1e-9         # metres between a pixel centre and a cell face


def grid_dims(res, size, centre, r):
    """(width, height, origin xy) of the grid of a map of size[] cells of res metres around centre, pixel size r"""
    size_m = [np.float64(size[k]) * np.float64(res) for k in range(2)]
    width, height = int(size_m[0] / np.float64(r)), int(size_m[1] / np.float64(r))
    return width, height, (np.float64(centre[0]) - size_m[0] / 2, np.float64(centre[1]) - size_m[1] / 2)


def cell_index(p, c, res, n):
    """LazyGrid::getIndexForPoint along one axis: floor((p - c) / res + 0.5) + n / 2.0 truncated to int; -1 outside [0, n)"""
    v = np.floor((np.asarray(p, dtype=np.float64) - c) / res + 0.5) + n / 2.0
    k = np.trunc(v)
    return np.where((k >= 0) & (k < n) & np.isfinite(v), k, -1).astype(np.int64)


def face_distance(p, c, res):
    """distance of p to the nearest face of LazyGrid's cells along one axis (faces where (p - c) / res + 0.5 is an integer)"""
    t = (np.asarray(p, dtype=np.float64) - c) / res + 0.5
    return np.abs(t - np.round(t)) * res


def rasterise(res, size, centre, r, mean, cov, idx, occ=None, z=0.0, occupied_no_gaussian=100):
    """-> (grid int8 [height, width], v100 float64 [height, width] (NaN where the pixel has no likelihood), face float64 [height, width])
    mean [n, 3], cov [n, 3, 3], idx [n, 3]: the Gaussian cells; occ [sx, sy, sz] or None (a Gaussian cell counts as occ > 0)."""
    res = np.float64(res)
    r = np.float64(r)
    sx, sy, sz = (int(s) for s in size)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
    cov = np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    width, height, (ox, oy) = grid_dims(res, size, centre, r)
    px = ox + (np.arange(width, dtype=np.float64) + 0.5) * r
    py = oy + (np.arange(height, dtype=np.float64) + 0.5) * r
    ix, iy = cell_index(px, centre[0], res, sx), cell_index(py, centre[1], res, sy)
    iz = int(cell_index(np.float64(z), centre[2], res, sz))
    face = np.minimum(np.minimum(face_distance(px, centre[0], res)[None, :], face_distance(py, centre[1], res)[:, None]),
                      face_distance(np.float64(z), centre[2], res))
    grid = np.full((height, width), -1, dtype=np.int8)
    v100 = np.full((height, width), np.nan)
    if iz < 0:
        return grid, v100, face
    IX, IY = np.meshgrid(ix, iy)                                     # [height, width]
    inside = (IX >= 0) & (IY >= 0)
    cx, cy = np.where(inside, IX, 0), np.where(inside, IY, 0)
    cell_of = np.full((sx, sy, sz), -1, dtype=np.int64)
    cell_of[idx[:, 0], idx[:, 1], idx[:, 2]] = np.arange(idx.shape[0])
    k = np.where(inside, cell_of[cx, cy, iz], -1)                    # the pixel's Gaussian cell
    o = np.where(k >= 0, 1.0, 0.0) if occ is None else np.asarray(occ, dtype=np.float64).reshape(sx, sy, sz)[cx, cy, iz]
    o = np.where(inside, o, 0.0)
    grid[o < 0] = 0
    grid[(o > 0) & (k < 0)] = occupied_no_gaussian
    g = (o > 0) & (k >= 0)
    if g.any():
        det = np.linalg.det(cov)
        ok = np.isfinite(det) & (det > 0)
        inv = np.zeros_like(cov)
        inv[ok] = np.linalg.inv(cov[ok])
        jj, ii = np.nonzero(g)
        kk = k[jj, ii]
        d = np.stack([px[ii], py[jj], np.full(ii.shape, np.float64(z))], axis=1) - mean[kk]
        with np.errstate(all="ignore"):
            l = np.einsum("na,nab,nb->n", d, inv[kk], d)
            l = np.where(ok[kk], l, np.nan)
            v = 0.5 + 0.5 * (np.exp(-l / 2) + 0.1)
            val = np.where(v > 1, 100, np.trunc(v * 100))
        fin = np.isfinite(l)
        grid[jj, ii] = np.where(fin, val, -1).astype(np.int8)
        v100[jj, ii] = np.where(fin, v * 100, np.nan)
    return grid, v100, face


def bands(v100, face):
    """-> (value_band, face_band): the pixels a comparison against the device leaves out.  value_band: 100 v within VALUE_BAND of an
    integer where that integer decides the value (beyond 100 + VALUE_BAND the value is 100 on either side); face_band: the pixel
    centre within FACE_BAND of a cell face."""
    with np.errstate(invalid="ignore"):
        value_band = np.isfinite(v100) & (np.abs(v100 - np.round(v100)) <= VALUE_BAND) & (v100 <= 100 + VALUE_BAND)
    return value_band, face <= FACE_BAND
