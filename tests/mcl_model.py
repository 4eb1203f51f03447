"""NumPy restatement of the NDT Monte Carlo localisation bank (include/ndtgpu.h, "NDT Monte Carlo localisation"): NDTMCL3D's
initializeFilter / updateAndPredictEff / pf.getMean as the header restates them, with the library's counter-based random numbers
(csrc/ndt_mcl.h).  The tests compare the device against these functions; the arithmetic follows the kernels' order of operations
(no fused multiply-adds) so that likelihoods agree to rounding."""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)
DRAW_POSE, DRAW_SUBSAMPLE, DRAW_SIR = 0, 6, 7
FX_SHIFT = 52


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def splitmix(x):
    with np.errstate(over="ignore"):
        z = _u64(x) + _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
        return z ^ (z >> np.uint64(31))


def hash_uniform(seed, stream, idx):
    """U[0,1) from (seed, stream, idx): synth.hash_uniform on uint64 arithmetic"""
    with np.errstate(over="ignore"):
        key = splitmix(_u64(seed) * np.uint64(1000003) + _u64(stream))
        z = splitmix(key ^ (_u64(idx) * _GAMMA))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_normal(seed, stream, idx):
    u1 = np.maximum(hash_uniform(seed, stream, idx), 1e-300)
    u2 = hash_uniform(seed, _u64(stream) + np.uint64(1), idx)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * 3.141592653589793 * u2)


def stream(f, c, d):
    """the key of draw d of filter slot f at draw counter c (ndt_mcl_stream)"""
    return np.uint64((((int(f) << 32) | (int(c) & 0xFFFFFFFF)) << 4 | (2 * d)) & 0xFFFFFFFFFFFFFFFF)


def xyz_rotation(a, b, c):
    """AngleAxis(a, X) * AngleAxis(b, Y) * AngleAxis(c, Z), closed form; a, b, c arrays -> [..., 3, 3]"""
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    R = np.empty(np.shape(a) + (3, 3))
    R[..., 0, 0] = cb * cc
    R[..., 0, 1] = -(cb * sc)
    R[..., 0, 2] = sb
    R[..., 1, 0] = ca * sc + sa * sb * cc
    R[..., 1, 1] = ca * cc - sa * sb * sc
    R[..., 1, 2] = -(sa * cb)
    R[..., 2, 0] = sa * sc - ca * sb * cc
    R[..., 2, 1] = sa * cc + ca * sb * sc
    R[..., 2, 2] = ca * cb
    return R


def pose(t, a, b, c):
    T = np.zeros(np.shape(a) + (4, 4))
    T[..., :3, :3] = xyz_rotation(a, b, c)
    T[..., 0, 3], T[..., 1, 3], T[..., 2, 3] = t[0], t[1], t[2]
    T[..., 3, 3] = 1.0
    return T


def euler012(R):
    """Eigen 3.3 MatrixBase::eulerAngles(0, 1, 2) of one 3x3 rotation (csrc/ndt_pose.h ndt_euler012)"""
    pi = 3.141592653589793
    r0 = np.arctan2(R[1, 2], R[2, 2])
    c2 = np.sqrt(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1])
    if r0 > 0.0:
        r0 -= pi
        r1 = np.arctan2(-R[0, 2], -c2)
    else:
        r1 = np.arctan2(-R[0, 2], c2)
    s1, c1 = np.sin(r0), np.cos(r0)
    r2 = np.arctan2(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    return np.array([-r0, -r1, -r2])


def motion(Tmotion, motion_model, offset):
    """updateAndPredictEff step 3: (tr, rot, sigma)"""
    tr = np.array(Tmotion[:3, 3], dtype=np.float64)
    rot = euler012(Tmotion[:3, :3])
    incr = np.abs(np.concatenate([tr, rot]))
    mm = np.asarray(motion_model, dtype=np.float64).reshape(6, 6)
    sigma = np.zeros(6)
    for i in range(6):
        s = 0.0
        for j in range(6):
            s = s + mm[i, j] * incr[j]
        sigma[i] = s + offset[i]
    return tr, rot, sigma


def initialize(seed, f, c, n, pose6, sigma6):
    """initializeFilter's particles [n, 4, 4] for filter slot f at draw counter c"""
    i = np.arange(n, dtype=np.uint64)
    v = [pose6[d] + sigma6[d] * hash_normal(seed, stream(f, c, DRAW_POSE + d), i) for d in range(6)]
    return pose(v[:3], v[3], v[4], v[5])


def predict(seed, f, c, T, tr, rot, sigma):
    """updateAndPredictEff step 4 on particles T [n, 4, 4]"""
    n = T.shape[0]
    i = np.arange(n, dtype=np.uint64)
    v = [(tr[d] if d < 3 else rot[d - 3]) + sigma[d] * hash_normal(seed, stream(f, c, DRAW_POSE + d), i) for d in range(6)]
    inc = pose(v[:3], v[3], v[4], v[5])
    return T @ inc


def subsample_mask(seed, f, c, n_cells, level):
    if not level < 1.0:
        return np.ones(n_cells, dtype=bool)
    return hash_uniform(seed, stream(f, c, DRAW_SUBSAMPLE), np.arange(n_cells, dtype=np.uint64)) < level


def rotate_cov(R, c):
    """R C R^T (csrc/ndt_math.h rotate_cov); c: [..., 6] (xx xy xz yy yz zz) -> [..., 6]"""
    xx, xy, xz, yy, yz, zz = (c[..., k] for k in range(6))
    a = np.empty(c.shape[:-1] + (9,))
    for i in range(3):
        a[..., i * 3 + 0] = R[i, 0] * xx + R[i, 1] * xy + R[i, 2] * xz
        a[..., i * 3 + 1] = R[i, 0] * xy + R[i, 1] * yy + R[i, 2] * yz
        a[..., i * 3 + 2] = R[i, 0] * xz + R[i, 1] * yz + R[i, 2] * zz
    o = np.empty(c.shape)
    o[..., 0] = a[..., 0] * R[0, 0] + a[..., 1] * R[0, 1] + a[..., 2] * R[0, 2]
    o[..., 1] = a[..., 0] * R[1, 0] + a[..., 1] * R[1, 1] + a[..., 2] * R[1, 2]
    o[..., 2] = a[..., 0] * R[2, 0] + a[..., 1] * R[2, 1] + a[..., 2] * R[2, 2]
    o[..., 3] = a[..., 3] * R[1, 0] + a[..., 4] * R[1, 1] + a[..., 5] * R[1, 2]
    o[..., 4] = a[..., 3] * R[2, 0] + a[..., 4] * R[2, 1] + a[..., 5] * R[2, 2]
    o[..., 5] = a[..., 6] * R[2, 0] + a[..., 7] * R[2, 1] + a[..., 8] * R[2, 2]
    return o


def inverse_check(a):
    """(inv [..., 6], ok [...]): computeInverseAndDetWithCheck, |det| > 1e-12 (csrc/ndt_math.h inverse_check)"""
    xx, xy, xz, yy, yz, zz = (a[..., k] for k in range(6))
    c00 = yy * zz - yz * yz
    c01 = yz * xz - xy * zz
    c02 = xy * yz - yy * xz
    det = xx * c00 + xy * c01 + xz * c02
    ok = np.abs(det) > 1e-12
    with np.errstate(divide="ignore", invalid="ignore"):
        idt = 1.0 / det
        inv = np.stack([c00 * idt, c01 * idt, c02 * idt, (xx * zz - xz * xz) * idt, (xy * xz - xx * yz) * idt,
                        (xx * yy - xy * xy) * idt], axis=-1)
    return inv, ok


def sym6(cov33):
    c = np.asarray(cov33, dtype=np.float64).reshape(-1, 3, 3)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=-1)


class MapModel:
    """A map as the filters see it: the Gaussian cells of one map of a MapSet (export_cells), keyed by LazyGrid slot."""

    def __init__(self, res, centre, cells_per_axis, mean, cov33, idx3):
        self.res, self.centre, self.size = float(res), np.asarray(centre, dtype=np.float64), np.asarray(cells_per_axis)
        self.slot_rank = {}
        for r, (ix, iy, iz) in enumerate(np.asarray(idx3)):
            self.slot_rank[(int(ix) * int(self.size[1]) + int(iy)) * int(self.size[2]) + int(iz)] = r
        self.mean, self.cov = np.asarray(mean, dtype=np.float64), sym6(cov33)

    def ranks(self, m):
        """rank of the Gaussian cell at pcl::PointXYZ(m) for points m [n, 3] (float coordinates), -1 where there is none"""
        p = m.astype(np.float32).astype(np.float64)
        out = np.full(m.shape[0], -1, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            v = np.floor((p - self.centre) / self.res + 0.5) + self.size / 2.0
            fine = np.all((v > -2.0e9) & (v < 2.0e9), axis=1)
            idx = np.where(fine[:, None], np.trunc(np.where(fine[:, None], v, 0.0)), -1).astype(np.int64)
        inside = fine & np.all((idx >= 0) & (idx < self.size), axis=1)
        for k in np.nonzero(inside)[0]:
            out[k] = self.slot_rank.get(int((idx[k, 0] * self.size[1] + idx[k, 1]) * self.size[2] + idx[k, 2]), -1)
        return out


def likelihood(T, scan_mean, scan_cov6, keep, mp, zfilt_min, chunk):
    """updateAndPredictEff step 6 for particles T [n, 4, 4]: (lik [n], terms) -- per chunk of `chunk` scan cells a sum in cell
    order, then the chunks in order (the kernels' order)"""
    n = T.shape[0]
    M = scan_mean.shape[0]
    lik = np.zeros(n)
    terms = 0
    for i in range(n):
        R, t = T[i, :3, :3], T[i, :3, 3]
        x, y, z = scan_mean[:, 0], scan_mean[:, 1], scan_mean[:, 2]
        m = np.stack([R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0], R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1],
                      R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]], axis=1)
        ok = keep & ~(m[:, 2] < zfilt_min)
        rk = np.where(ok, mp.ranks(np.where(ok[:, None], m, 0.0)), -1)
        ok &= rk >= 0
        rkc = np.where(ok, rk, 0)
        S = mp.cov[rkc] + rotate_cov(R, scan_cov6)
        Si, inv_ok = inverse_check(S)
        ok &= inv_ok
        dm = mp.mean[rkc] - m
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.stack([Si[:, 0] * dm[:, 0] + Si[:, 1] * dm[:, 1] + Si[:, 2] * dm[:, 2],
                          Si[:, 1] * dm[:, 0] + Si[:, 3] * dm[:, 1] + Si[:, 4] * dm[:, 2],
                          Si[:, 2] * dm[:, 0] + Si[:, 4] * dm[:, 1] + Si[:, 5] * dm[:, 2]], axis=1)
            l = dm[:, 0] * q[:, 0] + dm[:, 1] * q[:, 1] + dm[:, 2] * q[:, 2]
            ok &= (l * 0.0 == 0.0)
            term = np.where(ok, 0.1 + 0.9 * np.exp(-0.05 * np.where(ok, l, 0.0) / 2.0), 0.0)
        total = 0.0
        for c0 in range(0, M, chunk):
            s = 0.0
            for v in term[c0:c0 + chunk][ok[c0:c0 + chunk]]:
                s += v
            total += s
        lik[i] = total
        terms += int(ok.sum())
    return lik, terms


def normalise(w, lik):
    """pf.normalize(): (weights, sum p)"""
    p = w * lik
    S = p.sum()
    if not S > 0.0:
        return np.full_like(w, 1.0 / w.shape[0]), S
    return p / S, S


def var_p(w):
    n = w.shape[0]
    return np.sqrt(np.sum((w - 1.0 / n) ** 2) / n)


def sir_decision(vp, since_sir, force_sir, threshold, max_iters):
    """(resample, since_sir after)"""
    if force_sir:
        return True, since_sir
    if vp > threshold or since_sir > max_iters:
        return True, 0
    return False, since_sir + 1


def cumulative_fx(w):
    """the cumulative weights in units of 2^-52 (exact integer sums)"""
    return np.cumsum(np.rint(np.ldexp(w, FX_SHIFT)).astype(np.int64))


def thresholds(u0, n):
    return np.ldexp((u0 + np.arange(n, dtype=np.float64)) / float(n), FX_SHIFT)


def systematic_resample(w, u0):
    """SIRUpdate: indices of the survivors -- output k takes the first particle whose cumulative weight exceeds (u0 + k) / N"""
    n = w.shape[0]
    cum = cumulative_fx(w).astype(np.float64)
    j = np.searchsorted(cum, thresholds(u0, n), side="right")
    return np.minimum(j, n - 1)


def sir_offset(seed, f, c):
    return float(hash_uniform(seed, stream(f, c, DRAW_SIR), np.uint64(0)))


def mean(T, w):
    """pf.getMean()"""
    t = np.zeros(3)
    cs, sn = np.zeros(3), np.zeros(3)
    for i in range(T.shape[0]):
        t += w[i] * T[i, :3, 3]
        e = euler012(T[i, :3, :3])
        cs += w[i] * np.cos(e)
        sn += w[i] * np.sin(e)
    a = np.arctan2(sn, cs)
    return pose(t, a[0], a[1], a[2])
