"""Inputs shared by tests/test_occgrid_model.py (CPU) and tests/test_gpu_occgrid.py: the set of 3 maps on a grid of 25 x 20 x 2 cells
of 0.5 m (an odd axis, and at r = 0.1 an odd width of 125), small synthetic scans, and a NumPy cell builder for the CPU side.

The scans FILL whole cells (60 points spread evenly over each chosen cell): every Gaussian is then about as wide as its cell,
the likelihood of any pixel of the cell stays above e^-8, and 100 v never comes within 1e-8 of an integer except by chance.  A
scan of a wall would leave most pixels of its cells at 55 + 50 e^(-l / 2) with e^(-l / 2) below 2e-10 -- inside the comparison
band by construction, where nothing is compared."""
import numpy as np

RES = 0.5
SIZE_M = (12.5, 10.0, 1.0)
CELLS = (25, 20, 2)
CENTRES = [(0.0, 0.0, 0.0), (1.0, -0.5, 0.0), (0.25, 0.25, 0.0)]      # dyadic: at r = 0.125 no pixel centre lies on a cell face
N_MAPS = 3
CELLS_PER_SCAN = 50
POINTS_PER_CELL = 60


def cell_lower(k, c, n):
    """lower face of cell k along an axis of n cells around c (LazyGrid: floor((p - c) / res + 0.5) + n / 2.0 == k + (n % 2) / 2)"""
    return c + (k - n // 2 - 0.5) * RES


def scans(seed=7):
    """[N_MAPS, CELLS_PER_SCAN * POINTS_PER_CELL, 3] float32 in each map's frame, and the chosen cells [N_MAPS, CELLS_PER_SCAN, 3]"""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((N_MAPS, CELLS_PER_SCAN * POINTS_PER_CELL, 3), dtype=np.float32)
    chosen = np.zeros((N_MAPS, CELLS_PER_SCAN, 3), dtype=np.int64)
    for m in range(N_MAPS):
        flat = rng.choice((CELLS[0] - 2) * (CELLS[1] - 2), CELLS_PER_SCAN, replace=False)
        ix, iy = 1 + flat // (CELLS[1] - 2), 1 + flat % (CELLS[1] - 2)
        iz = np.where(np.arange(CELLS_PER_SCAN) % 5 == 4, 0, 1)         # most in the layer that holds z = 0
        chosen[m] = np.stack([ix, iy, iz], axis=1)
        for k in range(CELLS_PER_SCAN):
            lo = np.array([cell_lower(chosen[m, k, a], CENTRES[m][a], CELLS[a]) for a in range(3)])
            u = rng.uniform(0.04, 0.96, size=(POINTS_PER_CELL, 3))
            xyz[m, k * POINTS_PER_CELL:(k + 1) * POINTS_PER_CELL] = (lo + u * RES).astype(np.float32)
    return xyz, chosen


def build_cells(xyz, centre):
    """loadPointCloud + computeNDTCells of one scan in NumPy for clouds that need no eigenvalue floor (asserted): per cell the mean
    and the sample covariance of its points.  -> mean [n, 3], cov [n, 3, 3], idx [n, 3] in slot order."""
    from occgrid_model import cell_index
    p = np.asarray(xyz, dtype=np.float64)
    idx = np.stack([cell_index(p[:, a], centre[a], RES, CELLS[a]) for a in range(3)], axis=1)
    p, idx = p[(idx >= 0).all(axis=1)], idx[(idx >= 0).all(axis=1)]
    slot = (idx[:, 0] * CELLS[1] + idx[:, 1]) * CELLS[2] + idx[:, 2]
    mean, cov, out_idx = [], [], []
    for s in np.unique(slot):
        q = p[slot == s]
        if q.shape[0] < 3:
            continue
        c = np.cov(q.T)
        ev = np.linalg.eigvalsh(c)
        assert ev[0] > 0 and ev[2] < 1000.0 * ev[0], "this builder does not floor eigenvalues"
        mean.append(q.mean(axis=0))
        cov.append(c)
        out_idx.append(idx[slot == s][0])
    return np.array(mean), np.array(cov), np.array(out_idx)
