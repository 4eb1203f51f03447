"""NumPy model of the link gate (csrc/ndt_linkgate.h, include/ndtgpu.h "link gating"): distanceBetweenAffine3d, the candidate gate
of computeAllPossibleLinks' pairs, getValidLinks, the gather and the gated optimisation loop, in the header's operation order --
every product and sum is one IEEE operation (NumPy does not fuse a * b + c across ufunc calls), the square root is correctly
rounded and the arc cosine is ndt_pgo_acos (pgo_model.acos_fd, vectorised here and checked against it bit for bit by
tests/test_linkgate_model.py).  Poses are [.., 4, 4] arrays in the usual row-major NumPy layout (T[r, c]); the library's T16 is
their column-major flattening.

The scalar forms (one pair, one link: Python floats) are the definition; the vector forms evaluate the same expressions on
arrays and are what the large cases use."""
import math

import numpy as np

import pgo_model

DEFAULTS = dict(max_score=0.1, max_dist=1.0, max_angle=0.2, min_idx_dist=2, clip_cosine=0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown link-gate parameter %r" % k)
        p[k] = v
    return p


# ---- scalar forms ---------------------------------------------------------------------------------------------------------------

def distance(p1, p2, clip_cosine=0):
    """ndt_linkgate_distance -> (dist, ang, r00 before clipping)"""
    p1, p2 = [[float(v) for v in row] for row in p1], [[float(v) for v in row] for row in p2]
    dx, dy, dz = p2[0][3] - p1[0][3], p2[1][3] - p1[1][3], p2[2][3] - p1[2][3]
    dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
    r00 = (p1[0][0] * p2[0][0] + p1[1][0] * p2[1][0]) + p1[2][0] * p2[2][0]
    c = r00
    if clip_cosine:
        c = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)
    ang = abs(pgo_model.acos_fd(c)) if -1.0 <= c <= 1.0 else float("nan")
    return dist, ang, r00


def compose(R, L):
    """ndt_linkgate_compose: T_ref * T_link for rigid poses"""
    out = np.zeros((4, 4))
    R, L = np.asarray(R, dtype=np.float64), np.asarray(L, dtype=np.float64)
    for c in range(3):
        for k in range(3):
            out[k, c] = (float(R[k, 0]) * float(L[0, c]) + float(R[k, 1]) * float(L[1, c])) + float(R[k, 2]) * float(L[2, c])
    for k in range(3):
        out[k, 3] = ((float(R[k, 0]) * float(L[0, 3]) + float(R[k, 1]) * float(L[1, 3])) + float(R[k, 2]) * float(L[2, 3])) + float(R[k, 3])
    out[3, 3] = 1.0
    return out


def relative(Ti, Tj):
    """ndt_linkgate_relative: T_i^-1 * T_j by the rigid inverse"""
    out = np.zeros((4, 4))
    Ti, Tj = np.asarray(Ti, dtype=np.float64), np.asarray(Tj, dtype=np.float64)
    for c in range(3):
        for k in range(3):
            out[k, c] = (float(Ti[0, k]) * float(Tj[0, c]) + float(Ti[1, k]) * float(Tj[1, c])) + float(Ti[2, k]) * float(Tj[2, c])
    d = [float(Tj[a, 3]) - float(Ti[a, 3]) for a in range(3)]
    for k in range(3):
        out[k, 3] = (float(Ti[0, k]) * d[0] + float(Ti[1, k]) * d[1]) + float(Ti[2, k]) * d[2]
    out[3, 3] = 1.0
    return out


def pairs_before(i, n):
    return i * (2 * n - i - 1) // 2


def decode_pair(p, n):
    """ndt_linkgate_decode_pair: the row proposed by a double-precision square root, settled in integers"""
    b = 2.0 * float(n) - 1.0
    disc = b * b - 8.0 * float(p)
    r = 0.5 * (b - math.sqrt(disc if disc > 0.0 else 0.0))
    row = min(int(r) if r >= 0.0 else 0, n - 2)
    while row > 0 and pairs_before(row, n) > p:
        row -= 1
    while row + 2 < n and pairs_before(row + 1, n) <= p:
        row += 1
    return row, row + 1 + (p - pairs_before(row, n))


def candidate(node_T, i, j, prm):
    """ndt_linkgate_candidate"""
    if j - i < prm["min_idx_dist"]:
        return False
    dist, ang, _ = distance(node_T[i], node_T[j], prm["clip_cosine"])
    return dist < prm["max_dist"] and ang < prm["max_angle"]


def link_valid(node_T, ref, mov, T_link, score, prm):
    """ndt_linkgate_link_valid; score None: not tested"""
    if score is not None and not (score <= prm["max_score"]):
        return False
    if ref >= len(node_T) or mov >= len(node_T):
        return False
    if abs(int(mov) - int(ref)) < prm["min_idx_dist"]:
        return False
    dist, ang, _ = distance(node_T[mov], compose(node_T[ref], T_link), prm["clip_cosine"])
    return dist < prm["max_dist"] and ang < prm["max_angle"]


def candidates_scalar(node_T, **kw):
    """-> (ref, mov, T [k, 4, 4]) by the scalar forms, over the decoded pair index"""
    prm = params(**kw)
    n = len(node_T)
    ref, mov, T = [], [], []
    for p in range(n * (n - 1) // 2):
        i, j = decode_pair(p, n)
        if candidate(node_T, i, j, prm):
            ref.append(i)
            mov.append(j)
            T.append(relative(node_T[i], node_T[j]))
    return np.asarray(ref, dtype=np.int64), np.asarray(mov, dtype=np.int64), np.asarray(T).reshape(-1, 4, 4)


def valid_scalar(ref, mov, T_links, node_T, scores=None, **kw):
    prm = params(**kw)
    return np.asarray([k for k in range(len(ref))
                       if link_valid(node_T, int(ref[k]), int(mov[k]), T_links[k], None if scores is None else float(scores[k]), prm)],
                      dtype=np.int64)


# ---- vector forms: the same expressions on arrays -------------------------------------------------------------------------------

def acos_vec(x):
    """pgo_model.acos_fd on an array of values in [-1, 1] (NaN stays NaN)"""
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
    pS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
          7.91534994289814532176e-04, 3.47933107596021167570e-05)
    qS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)
    shape = np.shape(x)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    P = lambda z: z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
    Q = lambda z: 1.0 + z * (qS[0] + z * (qS[1] + z * (qS[2] + z * qS[3])))
    with np.errstate(invalid="ignore", divide="ignore"):
        ax = np.abs(x)
        # |x| < 0.5
        z = x * x
        small = pio2_hi - (x - (pio2_lo - x * (P(z) / Q(z))))
        small = np.where(ax <= 6.938893903907228e-18, pio2_hi + pio2_lo, small)
        # x <= -0.5
        z = (1.0 + x) * 0.5
        s = np.sqrt(np.where(z > 0.0, z, 0.0))
        neg = pi - 2.0 * (s + ((P(z) / Q(z)) * s - pio2_lo))
        # x >= 0.5
        z = (1.0 - x) * 0.5
        s = np.sqrt(np.where(z > 0.0, z, 0.0))
        df = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(np.float64)       # s with its low word cleared
        c = (z - df * df) / (s + df)
        pos = 2.0 * (df + ((P(z) / Q(z)) * s + c))
        out = np.where(ax < 0.5, small, np.where(x < 0.0, neg, pos))
        out = np.where(x >= 1.0, 0.0, out)
        out = np.where(x <= -1.0, pi + 2.0 * pio2_lo, out)
        out = np.where(np.isnan(x), x, out)
    return out.reshape(shape)


def distance_vec(p1, p2, clip_cosine=0):
    """distance over arrays [.., 4, 4] -> (dist, ang, r00 before clipping)"""
    dx, dy, dz = p2[..., 0, 3] - p1[..., 0, 3], p2[..., 1, 3] - p1[..., 1, 3], p2[..., 2, 3] - p1[..., 2, 3]
    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
    r00 = (p1[..., 0, 0] * p2[..., 0, 0] + p1[..., 1, 0] * p2[..., 1, 0]) + p1[..., 2, 0] * p2[..., 2, 0]
    c = np.where(r00 > 1.0, 1.0, np.where(r00 < -1.0, -1.0, r00)) if clip_cosine else r00
    inside = (c >= -1.0) & (c <= 1.0)
    ang = np.where(inside, np.abs(acos_vec(np.where(inside, c, 0.0))), np.nan)
    return dist, ang, r00


def compose_vec(R, L):
    out = np.zeros(np.broadcast(R, L).shape)
    for c in range(3):
        for k in range(3):
            out[..., k, c] = (R[..., k, 0] * L[..., 0, c] + R[..., k, 1] * L[..., 1, c]) + R[..., k, 2] * L[..., 2, c]
    for k in range(3):
        out[..., k, 3] = ((R[..., k, 0] * L[..., 0, 3] + R[..., k, 1] * L[..., 1, 3]) + R[..., k, 2] * L[..., 2, 3]) + R[..., k, 3]
    out[..., 3, 3] = 1.0
    return out


def relative_vec(Ti, Tj):
    out = np.zeros(np.broadcast(Ti, Tj).shape)
    for c in range(3):
        for k in range(3):
            out[..., k, c] = (Ti[..., 0, k] * Tj[..., 0, c] + Ti[..., 1, k] * Tj[..., 1, c]) + Ti[..., 2, k] * Tj[..., 2, c]
    d = [Tj[..., a, 3] - Ti[..., a, 3] for a in range(3)]
    for k in range(3):
        out[..., k, 3] = (Ti[..., 0, k] * d[0] + Ti[..., 1, k] * d[1]) + Ti[..., 2, k] * d[2]
    out[..., 3, 3] = 1.0
    return out


def all_pairs(n):
    """computeAllPossibleLinks' enumeration (i ascending, then j) as two int64 arrays"""
    i, j = np.triu_indices(n, k=1)
    return i.astype(np.int64), j.astype(np.int64)


def band(dist, ang, r00, prm, eps=1e-9):
    """the items device and model may decide differently (the comparison band: |dist - max_dist| < 1e-9, |ang - max_angle| < 1e-9, and
    |r00| > 1 - 1e-12 with clip_cosine = 0)"""
    with np.errstate(invalid="ignore"):
        b = (np.abs(dist - prm["max_dist"]) < eps) | (np.abs(ang - prm["max_angle"]) < eps)
        if not prm["clip_cosine"]:
            b |= np.abs(r00) > 1.0 - 1e-12
    return b


def candidates(node_T, with_T=True, **kw):
    """-> dict(ref, mov, T [k, 4, 4] or None, kept mask over all pairs, band mask over all pairs (among the pairs far enough in index and not beyond max_dist + 1e-9))"""
    prm = params(**kw)
    node_T = np.asarray(node_T, dtype=np.float64)
    i, j = all_pairs(len(node_T))
    far = (j - i) >= prm["min_idx_dist"]
    keep = np.zeros(len(i), dtype=bool)
    bnd = np.zeros(len(i), dtype=bool)
    # by rows of the pair list, in chunks: 18 M pairs do not need 18 M 4x4 matrices at once
    step = 1 << 20
    tx, ty, tz = (np.ascontiguousarray(node_T[:, a, 3]) for a in range(3))
    for a in range(0, len(i), step):
        s = slice(a, a + step)
        # a pair whose distance is beyond the threshold and its band is rejected whatever its angle: the angle is evaluated for
        # the others only (the same decisions, and 18 M arc cosines less at 6000 nodes)
        ii, jj = i[s], j[s]
        dx, dy, dz = tx[jj] - tx[ii], ty[jj] - ty[ii], tz[jj] - tz[ii]
        with np.errstate(invalid="ignore"):
            near = np.nonzero(far[s] & ~(np.sqrt((dx * dx + dy * dy) + dz * dz) >= prm["max_dist"] + 1e-9))[0]
        if not len(near):
            continue
        dist, ang, r00 = distance_vec(node_T[ii[near]], node_T[jj[near]], prm["clip_cosine"])
        with np.errstate(invalid="ignore"):
            keep[a + near] = (dist < prm["max_dist"]) & (ang < prm["max_angle"])
        bnd[a + near] = band(dist, ang, r00, prm)
    ref, mov = i[keep], j[keep]
    T = relative_vec(node_T[ref], node_T[mov]) if with_T else None
    return dict(ref=ref, mov=mov, T=T, keep=keep, band=bnd)


def valid(ref, mov, T_links, node_T, scores=None, **kw):
    """-> dict(keep: ascending indices of the links that stay, mask, band mask (among the links that pass score, range and index))"""
    prm = params(**kw)
    node_T = np.asarray(node_T, dtype=np.float64)
    ref, mov = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(mov, dtype=np.int64).reshape(-1)
    T_links = np.asarray(T_links, dtype=np.float64).reshape(-1, 4, 4)
    m, n = len(ref), len(node_T)
    pre = (ref < n) & (mov < n) & (np.abs(mov - ref) >= prm["min_idx_dist"])
    if scores is not None:
        with np.errstate(invalid="ignore"):
            pre &= np.asarray(scores, dtype=np.float64).reshape(-1) <= prm["max_score"]
    mask = np.zeros(m, dtype=bool)
    bnd = np.zeros(m, dtype=bool)
    k = np.nonzero(pre)[0]
    if len(k):
        dist, ang, r00 = distance_vec(node_T[mov[k]], compose_vec(node_T[ref[k]], T_links[k]), prm["clip_cosine"])
        with np.errstate(invalid="ignore"):
            mask[k] = (dist < prm["max_dist"]) & (ang < prm["max_angle"])
        bnd[k] = band(dist, ang, r00, prm)
    return dict(keep=np.nonzero(mask)[0].astype(np.int64), mask=mask, band=bnd)


def gather(keep, src, dst, dst_first_row=0):
    """ndtgpu_linkgate_gather: row keep[k] of src -> row dst_first_row + k of dst (in place)"""
    keep = np.asarray(keep, dtype=np.int64)
    dst[dst_first_row:dst_first_row + len(keep)] = src[keep]
    return dst


def pose_T(poses):
    """[n, 3] (x, y, yaw) -> [n, 4, 4]: convertIsamPose2dToEigenAffine3d"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    T = np.tile(np.eye(4), (len(poses), 1, 1))
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 0, 3], T[:, 1, 3] = c, -s, s, c, poses[:, 0], poses[:, 1]
    return T


def gated_loop(optimise, start_poses, ref, mov, T_links, scores=None, max_rounds=10, gate=None, **kw):
    """The loop of ndt_feature_graph_opt.cpp:152-173: gate the matched links under the current poses, optimise with the links that
    stay (optimise(poses, kept) -> new poses [n, 3]; it adds the incremental links itself), gate again; stop when the kept count
    repeats, when nothing is kept, or after max_rounds (ours).  gate(ref, mov, T_links, node_T, scores, **kw) -> kept indices:
    default the model's valid.  -> (kept index arrays per round, final poses)"""
    if gate is None:
        gate = lambda r, m, T, nT, sc, **k: valid(r, m, T, nT, sc, **k)["keep"]
    poses = np.asarray(start_poses, dtype=np.float64).reshape(-1, 3).copy()
    rounds, prev = [], None
    for _ in range(int(max_rounds)):
        kept = np.asarray(gate(ref, mov, T_links, pose_T(poses), scores, **kw), dtype=np.int64)
        rounds.append(kept)
        if kept.size == 0:
            break
        poses = np.asarray(optimise(poses, kept), dtype=np.float64).reshape(-1, 3)
        if prev == kept.size:
            break
        prev = kept.size
    return rounds, poses
