"""NumPy restatement of the laser-scan feature extraction (include/ndtgpu.h, ndtgpu_featbank_extract; steps 1-8 of its section):
a curvature detector on the chain of consecutive valid beams and the BetaGrid descriptor, the parameters of flirtlib_utils.h:15-42.
Sequential and plain; it is the checker of the GPU tests.  The arithmetic of every decision is written operation for operation as
the kernel writes it (csrc/ndt_featextract.hip, contraction off); what differs is the last bit of cos / sin / exp / atan2 and the
association of the arc-length prefix sum, which is what the GPU tests' tolerance covers.  extract() also reports the MARGINS that
make its integer outputs safe to compare: per decision class the smallest absolute distance of a decision from its threshold."""
import math

import numpy as np

OK, TOO_FEW_POINTS, OVERFLOW, BAD_INDEX = 0, 1, 2, 3
# flirtlib_utils.h:15-42: SimpleMinMaxPeakFinder(0.34, 0.001), CurvatureDetector(peak, 5, 0.2, 1.4, 2.0), BetaGridGenerator(0.02,
# 1.0, 4, 12); min_separation is this project's, r_min / r_max the launch files' min and sensor range
DEFAULTS = dict(scales=5, base_sigma=0.2, sigma_step=1.4, dmst=2.0, min_value=0.34, min_diff=0.001, min_rho=0.02, max_rho=1.0,
                bin_rho=4, bin_phi=12, min_separation=0.2, r_min=0.5, r_max=30.0)
MARGIN_CLASSES = ("validity", "break", "window", "eligibility", "peak_value", "peak_left", "peak_right", "level", "separation_r",
                  "separation", "bin_rho", "bin_phi", "ray")


def sigmas(p):
    """sigma_s = base_sigma * sigma_step^s, by repeated multiplication"""
    out, s = [], p["base_sigma"]
    for _ in range(p["scales"]):
        out.append(s)
        s = s * p["sigma_step"]
    return out


def smooth(pts, g, first, last, k, sigma):
    """step 3 for point k at one level: (n_x, n_y, R, eligible, window margin, eligibility margin)"""
    h = 3.0 * sigma
    two_s2 = (2.0 * sigma) * sigma
    lo = k
    while lo > first[k] and g[k] - g[lo - 1] <= h:
        lo -= 1
    hi = k
    while hi < last[k] and g[hi + 1] - g[k] <= h:
        hi += 1
    dg = g[lo:hi + 1] - g[k]
    w = np.exp(-(dg * dg) / two_s2)
    sw = np.cumsum(w)[-1]                                  # (cumsum: ascending j, one term at a time)
    sx = np.cumsum(w * pts[lo:hi + 1, 0])[-1]
    sy = np.cumsum(w * pts[lo:hi + 1, 1])[-1]
    nx, ny = sx / sw - pts[k, 0], sy / sw - pts[k, 1]
    R = math.sqrt(nx * nx + ny * ny) / sigma
    left, right = g[k] - g[first[k]], g[last[k]] - g[k]
    seg = np.abs(g[first[k]:last[k] + 1] - g[k])
    return nx, ny, R, (left >= h and right >= h), float(np.min(np.abs(seg - h))), min(abs(left - h), abs(right - h))


class Grid:
    """step 8's bin assignment around one keypoint"""

    def __init__(self, x, y, theta, p):
        self.x, self.y, self.c, self.s = x, y, math.cos(theta), math.sin(theta)
        self.p = p
        self.drho = (p["max_rho"] - p["min_rho"]) / p["bin_rho"]
        self.dphi = 2.0 * math.pi / p["bin_phi"]

    def bins(self, qx, qy):
        """(bin or -1, distance of rho to the nearest ring edge, distance of phi to the nearest sector edge where rho has a ring)"""
        p = self.p
        dx, dy = qx - self.x, qy - self.y
        lx = self.c * dx + self.s * dy
        ly = self.c * dy - self.s * dx
        rho = np.sqrt(lx * lx + ly * ly)
        phi = np.arctan2(ly, lx)
        inside = (rho >= p["min_rho"]) & (rho < p["max_rho"])
        a = np.minimum(np.floor((rho - p["min_rho"]) / self.drho), p["bin_rho"] - 1)
        t = (phi + math.pi) / self.dphi
        c = np.minimum(np.floor(t), p["bin_phi"] - 1)
        b = np.where(inside, a * p["bin_phi"] + c, -1).astype(np.int64)
        edges = p["min_rho"] + self.drho * np.arange(p["bin_rho"] + 1)
        edges[-1] = p["max_rho"]
        m_rho = np.min(np.abs(rho[..., None] - edges), axis=-1)
        m_phi = np.where(inside, np.abs(t - np.round(t)) * self.dphi, np.inf)
        return b, m_rho, m_phi


def describe(pts, x, y, theta, p):
    """step 8: (descriptor, hit counts, miss counts, margins) of the keypoint (x, y, theta) in the scan's valid points"""
    n_bins = p["bin_rho"] * p["bin_phi"]
    grid = Grid(x, y, theta, p)
    delta = grid.drho / 2.0
    hb, m_rho, m_phi = grid.bins(pts[:, 0], pts[:, 1])
    hit = np.bincount(hb[hb >= 0], minlength=n_bins)
    qn = np.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1])
    ud = np.arange(1, int(np.max(qn) / delta) + 3)[None, :] * delta          # u delta, every u that any beam can need
    live = ud < qn[:, None]
    t = 1.0 - ud / qn[:, None]
    sb, s_rho, s_phi = grid.bins(pts[:, 0, None] * t, pts[:, 1, None] * t)
    visited = np.zeros((pts.shape[0], n_bins + 1), dtype=bool)               # (column n_bins takes the samples without a bin)
    rows = np.broadcast_to(np.arange(pts.shape[0])[:, None], sb.shape)
    visited[rows[live], np.where(sb[live] >= 0, sb[live], n_bins)] = True
    visited[np.arange(pts.shape[0]), np.where(hb >= 0, hb, n_bins)] = False  # the bin that q itself hits gets no miss from q's beam
    miss = visited[:, :n_bins].sum(axis=0)
    desc = (hit + 1.0) / (hit + miss + 2.0)
    margins = dict(bin_rho=float(min(np.min(m_rho), np.min(np.where(live, s_rho, np.inf)))),
                   bin_phi=float(min(np.min(m_phi), np.min(np.where(live, s_phi, np.inf)))),
                   ray=float(np.min(np.abs(ud - qn[:, None]))))
    return desc, hit, miss, margins


def extract(ranges, angle_min, angle_increment, max_points=None, **params):
    """one scan -> dict(status, n_valid, n_segments, n_peaks, n_found, n_stored, pos [n, 3], desc [n, bins], beam, level, response,
    margins); max_points: the bank's capacity (None: no limit)"""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown parameter %r" % k)
        p[k] = v
    n_bins = p["bin_rho"] * p["bin_phi"]
    margins = {c: float("inf") for c in MARGIN_CLASSES}

    def note(cls, values):
        values = np.asarray(values, dtype=np.float64).reshape(-1)
        if values.size:
            margins[cls] = min(margins[cls], float(np.min(values)))

    r = np.asarray(ranges, dtype=np.float64).reshape(-1)
    # step 1
    finite = np.isfinite(r)
    valid = finite & (np.where(finite, r, 0.0) > p["r_min"]) & (np.where(finite, r, 0.0) < p["r_max"])
    note("validity", np.minimum(np.abs(r[finite] - p["r_min"]), np.abs(r[finite] - p["r_max"])))
    beams = np.nonzero(valid)[0]
    m = beams.shape[0]
    out = dict(status=OK, n_valid=m, n_segments=0, n_peaks=0, n_found=0, n_stored=0, pos=np.zeros((0, 3)), desc=np.zeros((0, n_bins)),
               beam=np.zeros(0, dtype=np.uint32), level=np.zeros(0, dtype=np.int32), response=np.zeros(0), margins=margins)
    if m < 3:
        out["status"] = TOO_FEW_POINTS
        return out
    phi = angle_min + beams * angle_increment
    pts = np.stack([r[beams] * np.cos(phi), r[beams] * np.sin(phi)], axis=1)
    # step 2
    dx, dy = pts[1:, 0] - pts[:-1, 0], pts[1:, 1] - pts[:-1, 1]
    d = np.concatenate([[0.0], np.sqrt(dx * dx + dy * dy)])
    note("break", np.abs(d[1:] - p["dmst"]))
    brk = d > p["dmst"]
    g = np.cumsum(d)
    seg = np.cumsum(brk)
    first = np.array([np.nonzero(seg == s)[0][0] for s in seg])
    last = np.array([np.nonzero(seg == s)[0][-1] for s in seg])
    out["n_segments"] = int(seg[-1]) + 1
    # steps 3-5
    best_R = np.zeros(m)
    best_s = np.full(m, -1)
    peak_R = [[] for _ in range(m)]
    for s, sigma in enumerate(sigmas(p)):
        R = np.zeros(m)
        elig = np.zeros(m, dtype=bool)
        for k in range(m):
            _, _, R[k], elig[k], m_win, m_el = smooth(pts, g, first, last, k, sigma)
            note("window", m_win)
            note("eligibility", m_el)
        for k in np.nonzero(elig)[0]:                       # (an eligible point has both neighbours in its segment)
            note("peak_value", abs(R[k] - p["min_value"]))
            note("peak_left", abs((R[k] - R[k - 1]) - p["min_diff"]))
            note("peak_right", abs((R[k] - R[k + 1]) - p["min_diff"]))
            if R[k] > p["min_value"] and R[k] - R[k - 1] > p["min_diff"] and R[k] - R[k + 1] > p["min_diff"]:
                out["n_peaks"] += 1
                note("level", [abs(R[k] - x) for x in peak_R[k]])
                peak_R[k].append(R[k])
                if best_s[k] < 0 or R[k] > best_R[k]:
                    best_R[k], best_s[k] = R[k], s
    # step 6: one pass over the step-5 set
    kept5 = np.nonzero(best_s >= 0)[0]
    found = []
    for k in kept5:
        dropped = False
        for k2 in kept5:
            if k2 == k or seg[k2] != seg[k]:
                continue
            gap = abs(g[k2] - g[k])
            note("separation", abs(gap - p["min_separation"]))
            if gap < p["min_separation"]:
                note("separation_r", abs(best_R[k2] - best_R[k]))
                if best_R[k2] > best_R[k] or (best_R[k2] == best_R[k] and k2 < k):
                    dropped = True
        if not dropped:
            found.append(int(k))
    out["n_found"] = len(found)
    stored = found if max_points is None else found[:max_points]
    if len(stored) < len(found):
        out["status"] = OVERFLOW
    out["n_stored"] = len(stored)
    # steps 7-8
    sig = sigmas(p)
    pos, desc, hits, misses = [], [], [], []
    for k in stored:
        nx, ny, R, _, _, _ = smooth(pts, g, first, last, k, sig[best_s[k]])
        theta = math.atan2(ny, nx)
        pos.append((pts[k, 0], pts[k, 1], theta))
        dsc, hit, miss, mg = describe(pts, pts[k, 0], pts[k, 1], theta, p)
        for c, v in mg.items():
            note(c, v)
        desc.append(dsc)
        hits.append(hit)
        misses.append(miss)
    out.update(pos=np.array(pos).reshape(-1, 3), desc=np.array(desc).reshape(-1, n_bins), beam=beams[stored].astype(np.uint32),
               level=best_s[stored].astype(np.int32), response=best_R[stored].astype(np.float64), hit=hits, miss=misses,
               points=pts, g=g, segment=seg)
    return out
