"""NumPy restatement, operation for operation, of csrc/ndt_marker.h (include/ndtgpu.h "marker export"): the cyclic Jacobi of a cell's
covariance, the stable ascending order, the sign rule, the axis segments of a cell under a pose, the segments of links and particles,
and the ordered compaction of a call.  Vectorised over cells: every lane of an array goes through the scalar code's operations in the
scalar code's order (NumPy's float64 + - * / and sqrt are IEEE operations and nothing here is fused), and a lane that the scalar code
would not touch is left alone by a mask.  check_against_eigh is the independent check: numpy.linalg.eigh knows nothing of this file."""
import numpy as np

MIN_EVAL = 0.0001
PARTICLE_LENGTH = 0.3
NONFINITE, BAD_INDEX = 1, 2
SWEEPS = 64
DBL_MAX = np.finfo(np.float64).max


def cov6_of(cov):
    """[n, 3, 3] -> [n, 6] = (xx xy xz yy yz zz): what the cell record holds"""
    c = np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=1)


def _rotate(a, v, p, q, active):
    apq = a[p][q]
    m = active & (apq != 0.0)
    if not m.any():
        return
    with np.errstate(all="ignore"):
        theta = (a[q][q] - a[p][p]) / (2.0 * apq)
        t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        for k in range(3):
            akp, akq = a[k][p], a[k][q]
            a[k][p] = np.where(m, c * akp - s * akq, akp)
            a[k][q] = np.where(m, s * akp + c * akq, akq)
        for k in range(3):
            apk, aqk = a[p][k], a[q][k]
            a[p][k] = np.where(m, c * apk - s * aqk, apk)
            a[q][k] = np.where(m, s * apk + c * aqk, aqk)
        for k in range(3):
            vkp, vkq = v[k][p], v[k][q]
            v[k][p] = np.where(m, c * vkp - s * vkq, vkp)
            v[k][q] = np.where(m, s * vkp + c * vkq, vkq)


def _exchange(d, v, i, j):
    with np.errstate(invalid="ignore"):
        m = d[j] < d[i]
    d[i], d[j] = np.where(m, d[j], d[i]), np.where(m, d[i], d[j])
    for k in range(3):
        v[k][i], v[k][j] = np.where(m, v[k][j], v[k][i]), np.where(m, v[k][i], v[k][j])


def eig3(cov6):
    """ndt_marker_eig3 of cov6 [n, 6] -> evals [n, 3] ascending, V [n, 3, 3] (V[:, k, j]: component k of the eigenvector of evals[:, j])"""
    c = np.asarray(cov6, dtype=np.float64).reshape(-1, 6)
    n = c.shape[0]
    idx = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    a = [[c[:, idx[i][j]].copy() for j in range(3)] for i in range(3)]
    v = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        with np.errstate(all="ignore"):
            off = np.zeros(n)
            off = off + a[0][1] * a[0][1]
            off = off + a[0][2] * a[0][2]
            off = off + a[1][2] * a[1][2]
            diag = np.zeros(n)
            diag = diag + a[0][0] * a[0][0]
            diag = diag + a[1][1] * a[1][1]
            diag = diag + a[2][2] * a[2][2]
            active = ~((off == 0.0) | (off <= 1e-30 * diag))
        if not active.any():
            break
        _rotate(a, v, 0, 1, active)
        _rotate(a, v, 0, 2, active)
        _rotate(a, v, 1, 2, active)
    d = [a[0][0].copy(), a[1][1].copy(), a[2][2].copy()]
    _exchange(d, v, 0, 1)
    _exchange(d, v, 1, 2)
    _exchange(d, v, 0, 1)
    for j in range(3):
        m0, m1, m2 = np.abs(v[0][j]), np.abs(v[1][j]), np.abs(v[2][j])
        lead, big = v[0][j], m0
        with np.errstate(invalid="ignore"):
            g = m1 > big
            lead, big = np.where(g, v[1][j], lead), np.where(g, m1, big)
            g = m2 > big
            lead, big = np.where(g, v[2][j], lead), np.where(g, m2, big)
            neg = lead < 0.0
        for k in range(3):
            v[k][j] = np.where(neg, -v[k][j], v[k][j])
    evals = np.stack(d, axis=1)
    V = np.stack([np.stack(v[k], axis=1) for k in range(3)], axis=1)
    return evals, V


def pose12(T):
    """a pose [4, 4] (math convention) -> (R [3, 3], t [3]): what ndt_marker_pose12 reads of the column-major 16"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return T[:3, :3].copy(), T[:3, 3].copy()


def point(R, t, p):
    """R p + t of points p [n, 3], as written: ((R_i0 p0 + R_i1 p1) + R_i2 p2) + t_i"""
    with np.errstate(all="ignore"):
        return np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + t[i] for i in range(3)], axis=1)


def cell_segments(mean, cov6, pose=None, min_eval=MIN_EVAL):
    """ndt_marker_cell of cells mean [n, 3], cov6 [n, 6] under one pose ([4, 4] or None) ->
    (seg [n, 3, 2, 3] per AXIS (not compacted), kept bool [n, 3], evals [n, 3], flags)"""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
    evals, V = eig3(cov6)
    with np.errstate(invalid="ignore"):
        finite = np.abs(evals) <= DBL_MAX
        kept = finite & ~(evals < min_eval)
    flags = NONFINITE if (~finite).any() else 0
    seg = np.zeros((mean.shape[0], 3, 2, 3))
    for j in range(3):
        with np.errstate(invalid="ignore"):
            r = np.sqrt(evals[:, j])
            o = V[:, :, j] * r[:, None]
            p1, p2 = mean - o, mean + o
        if pose is not None:
            R, t = pose12(pose)
            p1, p2 = point(R, t, p1), point(R, t, p2)
        seg[:, j, 0], seg[:, j, 1] = p1, p2
    return seg, kept, evals, flags


def map_markers(cells, poses=None, first=0, min_eval=MIN_EVAL):
    """the call: cells = [(mean [n_m, 3], cov [n_m, 3, 3]) per map of the call]; poses: [count, 4, 4] or None ->
    (points [n, 2, 3], src uint32 [n, 2] = (first + map of the call, cell rank), flags) in (map, cell, axis) order"""
    pts, src, flags = [], [], 0
    for m, (mean, cov) in enumerate(cells):
        mean = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
        if mean.shape[0] == 0:
            continue
        seg, kept, _, f = cell_segments(mean, cov6_of(cov), None if poses is None else poses[m], min_eval)
        flags |= f
        cell, axis = np.nonzero(kept)                  # (row-major: cell, then axis)
        pts.append(seg[cell, axis])
        src.append(np.stack([np.full(cell.shape[0], first + m), cell], axis=1))
    if not pts:
        return np.zeros((0, 2, 3)), np.zeros((0, 2), dtype=np.uint32), flags
    return np.concatenate(pts), np.concatenate(src).astype(np.uint32), flags


def link_markers(poses, ref, mov, score=None, skip_negative=0):
    """markerNDTFeatureLinks: poses [n_nodes, 4, 4] -> (points [n, 2, 3], flags); a kept link with a node index out of range emits
    nothing and raises BAD_INDEX"""
    T = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    ref, mov = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(mov, dtype=np.int64).reshape(-1)
    keep = np.ones(ref.shape[0], dtype=bool)
    if skip_negative and score is not None:
        keep &= ~(np.asarray(score, dtype=np.float64).reshape(-1) < 0.0)
    bad = keep & ((ref >= T.shape[0]) | (mov >= T.shape[0]))
    keep &= ~bad
    pts = np.stack([T[ref[keep], :3, 3], T[mov[keep], :3, 3]], axis=1) if keep.any() else np.zeros((0, 2, 3))
    return pts, (BAD_INDEX if bad.any() else 0)


def particle_markers(T, length=PARTICLE_LENGTH):
    """markerParticlesNDTMCL3D: T [..., 4, 4] -> points [..., 2, 3]: the translation, and T * (length, 0, 0) through point()"""
    T = np.asarray(T, dtype=np.float64)
    flat = T.reshape(-1, 4, 4)
    out = np.zeros((flat.shape[0], 2, 3))
    out[:, 0] = flat[:, :3, 3]
    tip = np.array([[length, 0.0, 0.0]])
    for i in range(flat.shape[0]):
        out[i, 1] = point(flat[i, :3, :3], flat[i, :3, 3], tip)[0]
    return out.reshape(T.shape[:-2] + (2, 3))


def check_against_eigh(cov, evals, V, kept, min_eval=MIN_EVAL, band=1e-9):
    """The independent check of eigen-pairs (cov [n, 3, 3]) against numpy.linalg.eigh; no eigenvector is compared with eigh's: the
    residual form holds inside a degenerate eigenspace too.  -> dict of the worst figures:
      eval_rel   max |lambda - lambda_eigh| / lambda_max
      unit       max | ||d|| - 1 | over the kept directions
      residual   max ||cov d - lambda d|| / lambda_max over the kept directions
      ortho      max |d_i . d_j| over the kept directions of a cell
      count_bad  cells outside the band whose segment count differs from eigh's;  in_band: cells left out of that comparison"""
    cov = np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3)
    w = np.linalg.eigh(cov)[0]
    lmax = np.abs(w).max(axis=1)
    out = dict(eval_rel=float((np.abs(evals - w).max(axis=1) / lmax).max()))
    unit = res = ortho = 0.0
    for j in range(3):
        d = V[:, :, j]
        k = kept[:, j]
        if k.any():
            unit = max(unit, float(np.abs(np.linalg.norm(d[k], axis=1) - 1.0).max()))
            r = np.einsum("nij,nj->ni", cov[k], d[k]) - evals[k, j][:, None] * d[k]
            res = max(res, float((np.linalg.norm(r, axis=1) / lmax[k]).max()))
        for i in range(j):
            both = k & kept[:, i]
            if both.any():
                ortho = max(ortho, float(np.abs((d[both] * V[both][:, :, i]).sum(axis=1)).max()))
    in_band = (np.abs(w - min_eval) <= band * min_eval).any(axis=1)
    count_eigh = (w >= min_eval).sum(axis=1)
    out.update(unit=unit, residual=res, ortho=ortho, in_band=int(in_band.sum()),
               count_bad=int(((kept.sum(axis=1) != count_eigh) & ~in_band).sum()))
    return out
