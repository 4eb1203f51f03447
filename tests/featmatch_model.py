"""NumPy restatement of the feature-set RANSAC matcher (include/ndtgpu.h, ndtgpu_featbank_*; steps 1-8 of its section): flirtlib's
RansacFeatureSetMatcher::matchSets as matchFeatureMap calls it (ndt_feature_map.h:104-122), sequential and plain.  It is the
checker of the GPU tests.  Every product and sum of a distance is written operation for operation as the kernel writes it
(csrc/ndt_featmatch.hip, contraction off), so the descriptor distances, the hypotheses' poses and every point-to-point distance of
a sweep with a hypothesis's pose are the device's bits; the sums over many points (a sweep's score, the refinement's moments) are
taken in ascending order here and by a tree there, which is what the GPU tests' tolerance covers.  match() also reports the
MARGINS that make its integer outputs safe to compare."""
import math

import numpy as np

OK, TOO_FEW, NO_HYPOTHESIS, BAD_INDEX = 0, 1, 2, 3
DEFAULTS = dict(acceptance_threshold=0.0599, success_probability=0.9, inlier_probability=0.1, distance_threshold=0.6,
                rigidity_threshold=0.0499, seed=0)
FAIL_SCORE = 1e17
_M = (1 << 64) - 1


def splitmix(x):
    z = (x + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def hash_uniform(seed, stream, idx):
    """ndt_hash_uniform (csrc/ndt_mcl.h) = synth.hash_uniform, in Python integers"""
    key = splitmix((seed * 1000003 + stream) & _M)
    z = splitmix(key ^ ((idx * 0x9E3779B97F4A7C15) & _M))
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def n_hypotheses(success_probability, inlier_probability):
    return int(math.ceil(math.log(1.0 - success_probability) / math.log(1.0 - inlier_probability * inlier_probability)))


def sample(seed, h, n_c):
    """the two candidates of hypothesis h (step 3)"""
    a = int(math.floor(hash_uniform(seed, 0, h) * n_c))
    b = int(math.floor(hash_uniform(seed, 1, h) * (n_c - 1)))
    if b >= a:
        b += 1
    return a, b


def chi2(mov_desc, ref_desc):
    """step 1 for every (mov, ref): [n_mov, n_ref], each sum in ascending k"""
    acc = np.zeros((mov_desc.shape[0], ref_desc.shape[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(mov_desc.shape[1]):
            a, b = mov_desc[:, k, None], ref_desc[None, :, k]
            s, d = a + b, a - b
            acc = acc + np.where(s > 0.0, d * d / s, 0.0)
    return 0.5 * acc


def candidates(mov_desc, ref_desc, distance_threshold):
    """step 2: (list of (i, j), the smallest distance of every mov point)"""
    d = chi2(mov_desc, ref_desc)
    j = np.argmin(d, axis=1)                       # (the first of equal minima: the lowest j)
    best = d[np.arange(d.shape[0]), j]
    return [(int(i), int(j[i])) for i in range(d.shape[0]) if best[i] < distance_threshold], best


def compute_pose(p, q):
    """step 5: (c, s, tx, ty) from correspondences p -> q, every sum in ascending order"""
    n = len(p)
    mpx = mpy = mqx = mqy = 0.0
    for k in range(n):
        mpx += p[k][0]; mpy += p[k][1]; mqx += q[k][0]; mqy += q[k][1]
    mpx /= float(n); mpy /= float(n); mqx /= float(n); mqy /= float(n)
    A = B = 0.0
    for k in range(n):
        px, py, qx, qy = p[k][0] - mpx, p[k][1] - mpy, q[k][0] - mqx, q[k][1] - mqy
        A += px * qx + py * qy
        B += px * qy - py * qx
    h = math.sqrt(A * A + B * B)
    c, s = (1.0, 0.0) if h == 0.0 else (A / h, B / h)
    return c, s, mqx - (c * mpx - s * mpy), mqy - (s * mpx + c * mpy)


def verify(pose, mov_xy, ref_xy, acceptance_threshold):
    """step 6: (score, nearest ref point of every mov point, inlier flags, squared distances)"""
    c, s, tx, ty = pose
    ax = (c * mov_xy[:, 0] - s * mov_xy[:, 1]) + tx
    ay = (s * mov_xy[:, 0] + c * mov_xy[:, 1]) + ty
    dx, dy = ax[:, None] - ref_xy[None, :, 0], ay[:, None] - ref_xy[None, :, 1]
    d2 = dx * dx + dy * dy
    j = np.argmin(d2, axis=1)
    best = d2[np.arange(d2.shape[0]), j]
    inl = best < acceptance_threshold
    score = 0.0
    for i in range(best.shape[0]):
        score += float(best[i]) if inl[i] else acceptance_threshold
    return score, j, inl, best


def _fail(status, n_c, H):
    return dict(status=status, score=FAIL_SCORE, c=1.0, s=0.0, x=0.0, y=0.0, theta=0.0, n_candidates=n_c, n_hypotheses=H, n_tested=0,
                best_hypothesis=-1, n_inliers=0, corr=np.zeros((0, 2), dtype=np.uint32), margins=None)


def match(ref_pos, ref_desc, mov_pos, mov_desc, **params):
    """one pair.  margins: `descriptor` the smallest |d - distance_threshold| of step 2; `score` the relative gap between the best
    and the next distinct hypothesis score (inf where there is one score only); `acceptance` the smallest |d^2 -
    acceptance_threshold| of the two sweeps that decide the inlier sets (the best hypothesis's and step 8's)."""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown parameter %r" % k)
        p[k] = v
    ref_xy = np.asarray(ref_pos, dtype=np.float64).reshape(-1, 3)[:, :2]
    mov_xy = np.asarray(mov_pos, dtype=np.float64).reshape(-1, 3)[:, :2]
    ref_desc, mov_desc = np.asarray(ref_desc, dtype=np.float64), np.asarray(mov_desc, dtype=np.float64)
    H = n_hypotheses(p["success_probability"], p["inlier_probability"])
    if ref_xy.shape[0] == 0 or mov_xy.shape[0] == 0:
        return _fail(TOO_FEW, 0, H)
    cand, best_d = candidates(mov_desc, ref_desc.reshape(ref_xy.shape[0], -1), p["distance_threshold"])
    n_c = len(cand)
    if n_c < 2 or n_c * p["inlier_probability"] < 2:
        return _fail(TOO_FEW, n_c, H)
    scores, best = {}, None
    for h in range(H):
        a, b = sample(p["seed"], h, n_c)
        (i1, j1), (i2, j2) = cand[a], cand[b]
        fx, fy = mov_xy[i1, 0] - mov_xy[i2, 0], mov_xy[i1, 1] - mov_xy[i2, 1]
        gx, gy = ref_xy[j1, 0] - ref_xy[j2, 0], ref_xy[j1, 1] - ref_xy[j2, 1]
        f, g = fx * fx + fy * fy, gx * gx + gy * gy
        if f + g == 0.0:
            continue
        d = f - g
        if d * d / (8.0 * (f + g)) > p["rigidity_threshold"]:
            continue
        pose = compute_pose([mov_xy[i1], mov_xy[i2]], [ref_xy[j1], ref_xy[j2]])
        scores[h] = verify(pose, mov_xy, ref_xy, p["acceptance_threshold"])[0]
        if best is None or scores[h] < scores[best]:
            best = h
    if best is None:
        return _fail(NO_HYPOTHESIS, n_c, H)
    a, b = sample(p["seed"], best, n_c)
    pose = compute_pose([mov_xy[cand[a][0]], mov_xy[cand[b][0]]], [ref_xy[cand[a][1]], ref_xy[cand[b][1]]])
    _, j, inl, d2_best = verify(pose, mov_xy, ref_xy, p["acceptance_threshold"])
    idx = np.nonzero(inl)[0]
    if idx.shape[0] > 0:
        pose = compute_pose([mov_xy[i] for i in idx], [ref_xy[j[i]] for i in idx])
    score, j, inl, d2_final = verify(pose, mov_xy, ref_xy, p["acceptance_threshold"])
    idx = np.nonzero(inl)[0]
    distinct = sorted(set(scores.values()))
    margins = dict(descriptor=float(np.min(np.abs(best_d - p["distance_threshold"]))),
                   score=float("inf") if len(distinct) < 2 else (distinct[1] - distinct[0]) / distinct[0],
                   acceptance=float(min(np.min(np.abs(d2_best - p["acceptance_threshold"])),
                                        np.min(np.abs(d2_final - p["acceptance_threshold"])))))
    return dict(status=OK, score=score, c=pose[0], s=pose[1], x=pose[2], y=pose[3], theta=math.atan2(pose[1], pose[0]), n_candidates=n_c,
                n_hypotheses=H, n_tested=len(scores), best_hypothesis=best, n_inliers=int(idx.shape[0]),
                corr=np.stack([idx, j[idx]], axis=1).astype(np.uint32).reshape(-1, 2), margins=margins, candidates=cand)
