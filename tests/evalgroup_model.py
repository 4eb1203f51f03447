"""What csrc/ndt_evalgroup.h has to compute, from the definitions (tests/test_evalgroup_model.py holds it to the oracle on the
CPU, tests/test_gpu_evalgroup.py holds the device to it).

The cell of a mean.  LazyGrid::getIndexForPoint: floor((p - c) / res + 0.5) + size / 2.0, truncated to an int -- evaluated here
in NumPy doubles, the IEEE operations the kernel runs with contraction off (lazygrid_index_h; lazygrid_index_p2 must agree with
it wherever res is a power of two).

The pair list of a group of up to 64 source cells: lanes in order; per lane the in-grid cells ix-n..ix+n, iy-n..iy+n, iz-n..iz+n
in slot order (x, then y, then z; slot = (x sy + y) sz + z); of those the occupied ones; entry = lane << 24 | rank, the rank of
a cell being its place among the occupied slots in slot order.  No bit windows, words or popcounts here.

Index -1.  The kernel's index functions return -1 when the value is NaN or not inside (-2e9, 2e9).  eval_group has no test of
its own for that -1: its bounds checks (xx >= 0 && xx < sx, the same for y, the clamp of z) treat it as the cell -1, one cell
outside the low face.  With n neighbours the in-grid cells 0..n-1 of that axis therefore ARE neighbours of such a mean, their
pairs enter the list and count in w.terms.  The oracle's derivatives (the reference project's code, restated) converts the
same double to an int with a C cast, which is undefined there and gives INT_MIN on x86: no neighbour is in the grid and no
pair is formed.  The two disagree in the pair COUNT only: every pair of such a mean has a non-finite or astronomically large
x = m - mu, for which pair_term adds +0 to every sum (tests/test_gpu_pairterm.py, the guards), so score, gradient and Hessian
are the same.  A mean more than 2e9 cells from the map does not occur in a registration; the model follows the kernel.
"""
import numpy as np

LIMIT = 2.0e9


def cell_index(p, centre, res, size):
    """index of coordinate p along an axis of `size` cells (NumPy doubles; -1 as the kernel's functions give it)"""
    with np.errstate(all="ignore"):
        v = np.floor((np.float64(p) - np.float64(centre)) / np.float64(res) + np.float64(0.5)) + np.float64(size) / np.float64(2.0)
    if not (v > -LIMIT and v < LIMIT):
        return -1
    return int(v)


class Grid:
    """a target map: sizes in cells, centre, cell size and the occupied slots"""

    def __init__(self, size_cells, centre, res, slots):
        self.size = tuple(int(s) for s in size_cells)
        self.centre = tuple(float(c) for c in centre)
        self.res = float(res)
        self.slots = sorted(int(s) for s in slots)
        assert len(set(self.slots)) == len(self.slots)
        assert not self.slots or (self.slots[0] >= 0 and self.slots[-1] < self.n_slots)
        self.rank = {s: k for k, s in enumerate(self.slots)}

    @property
    def n_slots(self):
        return self.size[0] * self.size[1] * self.size[2]

    def slot(self, ix, iy, iz):
        return (ix * self.size[1] + iy) * self.size[2] + iz

    def cell_centre(self, ix, iy, iz):
        """centre of cell (ix, iy, iz): c + (i - floor(size / 2)) res; the cell spans half a cell either side of it"""
        return tuple(self.centre[a] + (i - self.size[a] // 2) * self.res for a, i in enumerate((ix, iy, iz)))

    def indices(self, means):
        """[n, 3] cell indices of [n, 3] means"""
        return np.array([[cell_index(m[a], self.centre[a], self.res, self.size[a]) for a in range(3)] for m in np.asarray(means)],
                        dtype=np.int64).reshape(-1, 3)

    def neighbours(self, idx, nn):
        """ranks of the occupied in-grid cells around idx, in slot order"""
        out = []
        for x in range(idx[0] - nn, idx[0] + nn + 1):
            if x < 0 or x >= self.size[0]:
                continue
            for y in range(idx[1] - nn, idx[1] + nn + 1):
                if y < 0 or y >= self.size[1]:
                    continue
                for z in range(idx[2] - nn, idx[2] + nn + 1):
                    if z < 0 or z >= self.size[2]:
                        continue
                    k = self.rank.get(self.slot(x, y, z))
                    if k is not None:
                        out.append(k)
        return out


def pair_list(grid, lane_means, nn):
    """the list of a group: lane_means[l] is the transformed mean of lane l, or None for a lane that holds no cell"""
    out = []
    for lane, m in enumerate(lane_means):
        if m is None:
            continue
        idx = [cell_index(m[a], grid.centre[a], grid.res, grid.size[a]) for a in range(3)]
        out.extend((lane << 24) | k for k in grid.neighbours(idx, nn))
    return out


def lanes_of(base, stride, end):
    """source cell of every lane of a group (None: the lane holds none)"""
    return [base + l * stride if base + l * stride < end else None for l in range(64)]


def last_pass(entries, ql):
    """what the list holds after the group: the last of its passes of ql entries"""
    if not entries:
        return []
    return entries[(len(entries) - 1) // ql * ql:]


# ---- the lattices of tests/test_gpu_parity.py::test_probe_rank_bitmap_windows --------------------------------------------------
PROBE_LATTICES = [((12, 9, 7), 1), ((12, 9, 7), 2), ((12, 9, 7), 3), ((40, 33, 2), 2), ((40, 33, 1), 3), ((5, 70, 3), 2), ((6, 6, 6), 0)]
PROBE_RES = 0.5


def probe_lattice(size_cells, nn, m=700):
    """the random lattice of that test for (size_cells, nn), drawn the same way: about half of the slots filled, m source cells
    everywhere including outside the grid and on its border.  Returns grid, target mean / cov in rank order, source mean / cov."""
    rng = np.random.default_rng(size_cells[0] * 100 + size_cells[2] * 10 + nn)
    res = PROBE_RES
    size_m = [c * res for c in size_cells]
    sx, sy, sz = size_cells
    ix, iy, iz = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
    keep = rng.random(ix.shape) < 0.5
    idx = np.stack([ix[keep], iy[keep], iz[keep]], axis=1)            # (C order of the mask: slot order)
    ctr = (idx - np.array(size_cells) // 2) * res
    mean = ctr + rng.uniform(-0.2, 0.2, ctr.shape) * res
    A = rng.normal(size=(len(idx), 3, 3)) * 0.1
    cov = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(3)
    half = np.array(size_m) / 2.0
    smean = rng.uniform(-half - 1.2 * res, half + 1.2 * res, (m, 3))
    smean[:40] = np.clip(smean[:40], -half + 1e-3, half - 1e-3)
    B = rng.normal(size=(m, 3, 3)) * 0.1
    scov = B @ B.transpose(0, 2, 1) + 0.01 * np.eye(3)
    grid = Grid(size_cells, (0.0, 0.0, 0.0), res, [(int(a) * sy + int(b)) * sz + int(c) for a, b, c in idx])
    return grid, mean, cov, smean, scov


def six(M33):
    return [M33[0, 0], M33[0, 1], M33[0, 2], M33[1, 1], M33[1, 2], M33[2, 2]]


def scores(m, C, mu, Cj, d1=1.0, d2=0.05):
    """the score entry of pairterm_model.formula in doubles for n pairs at once: m, mu [n, 3]; C, Cj [n, 3, 3].
    s = -d1 exp(-d2 / 2 x^T B x), B = (C + Cj)^-1 by adjugate / determinant, x = m - mu"""
    x = m - mu
    S = C + Cj
    c = np.empty_like(S)
    for i in range(3):
        for j in range(3):
            c[:, i, j] = (S[:, (i + 1) % 3, (j + 1) % 3] * S[:, (i + 2) % 3, (j + 2) % 3]
                          - S[:, (i + 1) % 3, (j + 2) % 3] * S[:, (i + 2) % 3, (j + 1) % 3])
    det = S[:, 0, 0] * c[:, 0, 0] + S[:, 0, 1] * c[:, 0, 1] + S[:, 0, 2] * c[:, 0, 2]
    B = c.transpose(0, 2, 1) / det[:, None, None]
    Bx = B[:, :, 0] * x[:, 0:1] + B[:, :, 1] * x[:, 1:2] + B[:, :, 2] * x[:, 2:3]
    l = x[:, 0] * Bx[:, 0] + x[:, 1] * Bx[:, 1] + x[:, 2] * Bx[:, 2]
    return -d1 * np.exp(-d2 * 0.5 * l)
