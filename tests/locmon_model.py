"""NumPy model of the localisation monitor (include/ndtgpu.h "localisation monitor", csrc/ndt_locmon.h): the distance field as the
brute-force minimum over the (2R + 1)^2 offsets inside the disc, the key arithmetic operation for operation in fp64 (NumPy does not
contract), the median by sorting, the arg-min and arg-max ordered.  The device's outputs equal this model's bit for bit."""
import math

import numpy as np

FIELD_FAR, KEY_FAR, KEY_OFFMAP, NO_SCAN = 0xFFFF, 0x10000, 0x10001, 0xFFFFFFFF
NO_BEAMS, BAD_INDEX, NO_QUERY, NO_RESULT, NO_PICK = 1, 2, 4, 8, 16
OFFMAP_BADNESS = 1e9
RESULT_DTYPE = np.dtype([("badness", "<f8"), ("key", "<u4"), ("n_kept", "<u4"), ("n_offmap", "<u4"), ("flags", "<u4")])


def radius(max_dist, resolution):
    """R = (int)floor(max_dist / resolution); 0 where it is not 1 .. 254"""
    q = math.floor(max_dist / resolution)
    return int(q) if 1 <= q <= 254 else 0


def field(grid, R, occupied_min=55):
    """grid int8 [height, width] -> uint16 [height, width]: min dx^2 + dy^2 over the obstacle pixels within the disc of radius R,
    0xFFFF where there is none.  Pixels outside the grid are not obstacles."""
    g = np.asarray(grid, dtype=np.int8)
    h, w = g.shape
    obst = np.zeros((h + 2 * R, w + 2 * R), dtype=bool)
    obst[R:R + h, R:R + w] = g >= occupied_min
    out = np.full((h, w), FIELD_FAR, dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            k = dx * dx + dy * dy
            if k > R * R:
                continue
            hit = obst[R + dy:R + dy + h, R + dx:R + dx + w]
            out = np.where(hit & (k < out), k, out)
    return out.astype(np.uint16)


def beam_table(n_beams, angle_min, angle_increment):
    a = np.float64(angle_min) + np.arange(n_beams, dtype=np.float64) * np.float64(angle_increment)
    return np.cos(a), np.sin(a)


def kept(r, r_min=0.0, r_max=math.inf):
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r) & (r > r_min) & (r < r_max)


def pixels(pose4, cb, sb, r, origin2, resolution, width, height):
    """-> (in_bounds bool [n], fi int64 [n], fj int64 [n]) of beams with table entries cb, sb and ranges r (all kept)"""
    x, y, c, s = (np.float64(v) for v in pose4)
    with np.errstate(invalid="ignore", over="ignore"):
        ex = c * cb - s * sb
        ey = s * cb + c * sb
        px = x + ex * r
        py = y + ey * r
        di = np.floor((px - np.float64(origin2[0])) / np.float64(resolution))
        dj = np.floor((py - np.float64(origin2[1])) / np.float64(resolution))
        inb = (di >= 0.0) & (di < float(width)) & (dj >= 0.0) & (dj < float(height))
    fi = np.where(inb, di, 0.0).astype(np.int64)
    fj = np.where(inb, dj, 0.0).astype(np.int64)
    return inb, fi, fj


def metres(key, resolution, max_dist):
    if key >= KEY_OFFMAP:
        return OFFMAP_BADNESS
    if key == KEY_FAR:
        return float(max_dist)
    return float(np.float64(resolution) * np.sqrt(np.float64(key)))


def beam_keys(fld, pose4, cb, sb, r, origin2, resolution, r_min=0.0, r_max=math.inf):
    """the keys of the kept beams, in beam order"""
    k = kept(r, r_min, r_max)
    rr = np.asarray(r, dtype=np.float64)[k]
    h, w = fld.shape
    inb, fi, fj = pixels(pose4, cb[k], sb[k], rr, origin2, resolution, w, h)
    f = fld[fj, fi].astype(np.int64)
    return np.where(inb, np.where(f == FIELD_FAR, KEY_FAR, f), KEY_OFFMAP)


def evaluate(fields, origins, resolution, max_dist, cb, sb, ranges, queries, r_min=0.0, r_max=math.inf):
    """fields: list of uint16 [height, width]; queries: records with scan, grid, x, y, c, s -> RESULT_DTYPE [n]"""
    out = np.zeros(len(queries), dtype=RESULT_DTYPE)
    for n, q in enumerate(queries):
        scan, grid = int(q["scan"]), int(q["grid"])
        rec = out[n]
        rec["badness"], rec["key"] = OFFMAP_BADNESS, KEY_OFFMAP
        if scan == NO_SCAN:
            rec["flags"] = NO_QUERY
            continue
        if scan >= len(ranges) or grid >= len(fields):
            rec["flags"] = BAD_INDEX
            continue
        keys = beam_keys(fields[grid], (q["x"], q["y"], q["c"], q["s"]), cb, sb, ranges[scan], origins[grid], resolution, r_min, r_max)
        rec["n_kept"], rec["n_offmap"] = len(keys), int((keys == KEY_OFFMAP).sum())
        if len(keys) == 0:
            rec["flags"] = NO_BEAMS
            continue
        key = int(np.sort(keys)[len(keys) // 2])
        rec["key"], rec["badness"] = key, metres(key, resolution, max_dist)
    return out


def adjust(fld, origin2, resolution, max_dist, cb, sb, r, lattice, r_min=0.0, r_max=math.inf):
    """-> dict(index, key, badness, flags, volume uint32 [nx, ny, nyaw]): the smallest key, ties to the lowest linear index"""
    xs, ys, cs, sn = (np.asarray(lattice[k], dtype=np.float64) for k in ("xs", "ys", "cs", "sn"))
    vol = np.zeros((len(xs), len(ys), len(cs)), dtype=np.uint32)
    for ix, x in enumerate(xs):
        for iy, y in enumerate(ys):
            for iyaw in range(len(cs)):
                keys = beam_keys(fld, (x, y, cs[iyaw], sn[iyaw]), cb, sb, r, origin2, resolution, r_min, r_max)
                vol[ix, iy, iyaw] = int(np.sort(keys)[len(keys) // 2]) if len(keys) else KEY_OFFMAP
    flat = vol.reshape(-1)
    index = int(np.argmin(flat))                       # (the first of equals)
    key = int(flat[index])
    bad = metres(key, resolution, max_dist)
    return dict(index=index, key=key, badness=bad, flags=NO_RESULT if bad >= 1e8 else 0, volume=vol)


def compose(ref, m, post=(-0.275, 0.0)):
    xr, yr, cr, sr = (np.float64(v) for v in ref)
    xm, ym, cm, sm = (np.float64(v) for v in m)
    px, py = np.float64(post[0]), np.float64(post[1])
    ax = xr + (cr * xm - sr * ym)
    ay = yr + (sr * xm + cr * ym)
    ac = cr * cm - sr * sm
    as_ = sr * cm + cr * sm
    return np.array([ax + (ac * px - as_ * py), ay + (as_ * px + ac * py), ac, as_])


def pick(status, n_inliers, match4, ref_poses, scan, grid, min_num_matches=8, post=(-0.275, 0.0)):
    """-> (query dict(scan, grid, x, y, c, s), pick dict(pair, n_inliers, flags)): the most inliers among status 0 and
    n_inliers > min_num_matches, strict >, so the first of equals"""
    best, best_n = -1, 0
    for p in range(len(status)):
        if int(status[p]) == 0 and int(n_inliers[p]) > min_num_matches and int(n_inliers[p]) > best_n:
            best, best_n = p, int(n_inliers[p])
    if best < 0:
        return dict(scan=NO_SCAN, grid=grid, x=0.0, y=0.0, c=1.0, s=0.0), dict(pair=-1, n_inliers=0, flags=NO_PICK)
    o = compose(ref_poses[best], match4[best], post)
    return dict(scan=scan, grid=grid, x=o[0], y=o[1], c=o[2], s=o[3]), dict(pair=best, n_inliers=best_n, flags=0)
