"""Inputs shared by tests/test_marker_model.py, tests/test_marker_abi.py (CPU) and tests/test_gpu_marker.py: a DESIGNED set of 3 maps
on the 25 x 20 x 2 grid of occgrid_fixtures, the built maps of occgrid_fixtures as the realistic case, poses, links and particles.

The designed set: map 0 holds 600 cells (two full tiles of 256 and one of 88), map 1 is EMPTY, map 2 holds 257 (one past a tile).
Each cell sits at the centre of a slot of its own (plus a small offset), and the cells cycle through six families of covariance:
  (a) rotated SPD, eigenvalues 0.04 / 0.01 / 2.5e-3                 -> 3 segments
  (b) rotated, 0.02 / 2e-5 / 2e-5                                    -> 1 segment, a degenerate pair skipped
  (c) DIAGONAL, exactly 1e-4 / 0.01 / 5e-5                           -> 2 segments: the threshold itself is emitted, one axis skipped;
                                                                        no rotation, so the solver does not run and both sides are exact
  (d) rotated, 5e-5 / 2e-5 / 1e-5                                    -> 0 segments
  (e) rotated, 0.01 / 0.01 / 2.5e-3                                  -> 3 segments, an emitted degenerate pair
  (f) a full matrix whose xz entry is exactly zero                   -> 3 segments, a rotation of the first sweep skipped
ndtgpu_mapset_set_cells (what the GPU tests load these with) keeps mean and covariance AS THEY ARE -- it floors nothing and refuses
nothing here -- sorts the cells by slot and drops a cell outside the grid; these cells are made in slot order, one per slot, inside
the grid, so export_cells returns what was set.  The GPU tests feed the model with what export_cells returns all the same."""
import numpy as np

import occgrid_fixtures as F

N_MAPS = 3
N_CELLS = (600, 0, 257)
MAX_CELLS = 1000                        # = the grid's slots: 4 tiles a map
FAMILIES = "abcdef"
SEGMENTS = dict(a=3, b=1, c=2, d=0, e=3, f=3)
EIGENVALUES = dict(a=(0.04, 0.01, 2.5e-3), b=(0.02, 2e-5, 2e-5), c=(1e-4, 0.01, 5e-5), d=(5e-5, 2e-5, 1e-5), e=(0.01, 0.01, 2.5e-3))


def rotation(rng):
    """a rotation matrix, uniformly enough: QR of a Gaussian matrix with the determinant made +1"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def family_cov(fam, rng):
    if fam == "c":
        return np.diag(EIGENVALUES["c"])
    if fam == "f":
        s = rng.uniform(0.5, 2.0)
        return s * np.array([[0.03, 0.01, 0.0], [0.01, 0.02, 0.004], [0.0, 0.004, 0.01]])
    R = rotation(rng)
    c = R @ np.diag(EIGENVALUES[fam]) @ R.T
    return 0.5 * (c + c.T)


def designed_cells(m, seed=11):
    """-> mean [n, 3] in map m's frame, cov [n, 3, 3], family [n] (letters), in slot order"""
    n = N_CELLS[m]
    rng = np.random.default_rng(seed + m)
    slots = np.sort(rng.choice(F.CELLS[0] * F.CELLS[1] * F.CELLS[2], n, replace=False))
    mean, cov, fam = np.zeros((n, 3)), np.zeros((n, 3, 3)), []
    for k, slot in enumerate(slots):
        idx = (slot // (F.CELLS[1] * F.CELLS[2]), (slot // F.CELLS[2]) % F.CELLS[1], slot % F.CELLS[2])
        lo = np.array([F.cell_lower(idx[a], F.CENTRES[m][a], F.CELLS[a]) for a in range(3)])
        mean[k] = lo + (0.5 + rng.uniform(-0.3, 0.3, size=3)) * F.RES
        fam.append(FAMILIES[k % len(FAMILIES)])
        cov[k] = family_cov(fam[-1], rng)
    return mean, cov, np.array(fam)


def pose(x, y, z, yaw, roll=0.0):
    cy, sy, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = (x, y, z)
    return T


# one pose per map: three rigid yaw + translation; and the same with a roll on the first
POSES_YAW = np.stack([pose(1.25, -0.75, 0.0, 0.3), pose(-3.0, 2.0, 0.1, -1.2), pose(0.5, 0.25, -0.05, 2.9)])
POSES_ROLL = np.stack([pose(1.25, -0.75, 0.2, 0.3, roll=0.4), POSES_YAW[1], POSES_YAW[2]])
POSE_SETS = dict(none=None, yaw=POSES_YAW, roll=POSES_ROLL)


def built_cells():
    """the realistic case on the CPU: occgrid_fixtures' scans (3 maps, 3000 points each) through its NumPy cell builder ->
    [(mean, cov) per map]"""
    xyz, _ = F.scans()
    out = []
    for m in range(F.N_MAPS):
        mean, cov, _ = F.build_cells(xyz[m], F.CENTRES[m])
        out.append((mean, cov))
    return out


def links(seed=5):
    """40 nodes, 300 links (two tiles of 256), a third of the scores negative -> poses [40, 4, 4], ref [300], mov [300], score [300]"""
    rng = np.random.default_rng(seed)
    n_nodes, n_links = 40, 300
    poses = np.stack([pose(*rng.uniform(-20, 20, size=2), rng.uniform(-0.2, 0.2), rng.uniform(-np.pi, np.pi)) for _ in range(n_nodes)])
    ref = rng.integers(0, n_nodes, n_links).astype(np.uint32)
    mov = rng.integers(0, n_nodes, n_links).astype(np.uint32)
    score = rng.uniform(0.0, 1.0, n_links)
    score[::3] = -score[::3] - 0.01
    return poses, ref, mov, score


def particles(seed=9):
    """2 filters x 300 particles -> T [2, 300, 4, 4]"""
    rng = np.random.default_rng(seed)
    T = np.zeros((2, 300, 4, 4))
    for f in range(2):
        for i in range(300):
            T[f, i] = pose(*rng.uniform(-5, 5, size=2), rng.uniform(-0.1, 0.1), rng.uniform(-np.pi, np.pi), roll=rng.uniform(-0.05, 0.05))
    return T
