"""The NumPy model of the scan simulator (tests/scansim_model.py) against independently written step-by-step loops: the walk of a
ray, the closed form of a step against the accumulator, exact ranges in a walled room, the flags and the lattice."""
import math

import numpy as np
import pytest

import scansim_fixtures as F
import scansim_model as M


def walk_loop(grid, origin, res, pose, cb, sb, range_max, miss, occupied_min=55, unknown=1):
    """one beam, a literal loop with the accumulator; None: the pose is off the map"""
    h, w = grid.shape
    x, y, c, s = pose
    fi0, fj0 = math.floor((x - origin[0]) / res), math.floor((y - origin[1]) / res)
    if not (0 <= fi0 < w and 0 <= fj0 < h):
        return None
    R = int(math.floor(range_max / res))
    ex, ey = c * cb - s * sb, s * cb + c * sb
    di = math.floor((x + ex * range_max - origin[0]) / res) - fi0
    dj = math.floor((y + ey * range_max - origin[1]) / res) - fj0
    n, xmajor = max(abs(di), abs(dj)), abs(di) >= abs(dj)
    dmin = min(abs(di), abs(dj))
    si, sj = (di > 0) - (di < 0), (dj > 0) - (dj < 0)
    acc, m = n, 0
    for k in range(1, n + 1):
        acc += 2 * dmin
        if acc >= 2 * n:
            acc -= 2 * n
            m += 1
        a, b = (si * k, sj * m) if xmajor else (si * m, sj * k)
        i, j = fi0 + a, fj0 + b
        if not (0 <= i < w and 0 <= j < h):
            return miss
        if a * a + b * b > R * R:
            return miss
        v = int(grid[j, i])
        if v >= occupied_min or (unknown and v < 0):
            return res * math.sqrt(float(a * a + b * b))
    return miss


def test_model_equals_a_step_by_step_loop_on_random_grids():
    rng = np.random.default_rng(3)
    n_hit = n_miss = n_off = 0
    for trial in range(40):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        g = F.random_grid(rng, h, w, 0.02)
        origin = (rng.uniform(-3, 3), rng.uniform(-3, 3))
        res = (0.05, 0.1, 0.125)[trial % 3]
        rm = res * int(rng.integers(1, 60)) + 0.3 * res
        unk, om = trial % 2, (55, 70)[(trial // 2) % 2]
        for _ in range(30):
            th, a = rng.uniform(-4, 4, 2)
            pose = (origin[0] + rng.uniform(-0.1, 1.1) * w * res, origin[1] + rng.uniform(-0.1, 1.1) * h * res, math.cos(th), math.sin(th))
            want = walk_loop(g, origin, res, pose, math.cos(a), math.sin(a), rm, rm + 1.0, om, unk)
            got = M.beam(g, origin, res, pose, math.cos(a), math.sin(a), range_max=rm, miss=rm + 1.0, occupied_min=om, unknown_is_obstacle=unk)
            if want is None:
                assert got is None
                n_off += 1
                continue
            assert np.float64(got[0]).view(np.uint64) == np.float64(want).view(np.uint64)
            assert got[1] == (want != rm + 1.0)
            n_hit += got[1]
            n_miss += 1 - got[1]
    assert n_hit > 100 and n_miss > 100 and n_off > 50, (n_hit, n_miss, n_off)


def test_closed_form_equals_the_accumulator():
    """for all |di|, |dj| <= 40: the same cells, ends on (di, dj), steps of at most one cell, point symmetry"""
    for di in range(-40, 41):
        for dj in range(-40, 41):
            a, b, m = M.ray_cells(di, dj)
            n, dmin = max(abs(di), abs(dj)), min(abs(di), abs(dj))
            assert a.shape[0] == n
            if n == 0:
                continue
            acc, mm, acc_m = n, 0, []
            for k in range(1, n + 1):
                acc += 2 * dmin
                if acc >= 2 * n:
                    acc -= 2 * n
                    mm += 1
                acc_m.append(mm)
            assert m.tolist() == acc_m, (di, dj)
            assert (int(a[-1]), int(b[-1])) == (di, dj)
            assert np.abs(np.diff(np.r_[0, a])).max() <= 1 and np.abs(np.diff(np.r_[0, b])).max() <= 1
            a2, b2, _ = M.ray_cells(-di, -dj)
            assert np.array_equal(a2, -a) and np.array_equal(b2, -b)
            if abs(di) == abs(dj):                       # x is the major axis: both advance a cell a step
                assert np.array_equal(np.abs(a), np.arange(1, n + 1)) and np.array_equal(np.abs(b), np.arange(1, n + 1))
    assert M.cell(4, 2, 1) == (1, 1) and M.cell(4, 2, 2) == (2, 1) and M.cell(4, 2, 3) == (3, 2) and M.cell(4, 2, 4) == (4, 2)
    assert M.cell(-2, 4, 3) == (-2, 3) and M.cell(5, 0, 0) == (0, 0)


def walled_room(n=41):
    g = np.zeros((n, n), dtype=np.int8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 100
    return g


def test_exact_ranges_in_a_walled_room():
    """the pose at a cell centre: beams along the four axes return res * sqrt((double)(k * k)), the diagonals res * sqrt((double)(2 k k))"""
    g, res, origin = walled_room(), 0.05, (-0.3, 0.7)
    i0, j0 = 17, 25
    pose = F.centre(i0, j0, origin, res) + (1.0, 0.0)
    axes = {0: 40 - i0, 90: 40 - j0, 180: i0, 270: j0}
    diag = {45: min(40 - i0, 40 - j0), 135: min(i0, 40 - j0), 225: min(i0, j0), 315: min(40 - i0, j0)}
    for deg, k in list(axes.items()) + list(diag.items()):
        a = math.radians(deg)
        cb, sb = (round(math.cos(a)), round(math.sin(a))) if deg in axes else (math.cos(a), math.sin(a))
        r, hit = M.beam(g, origin, res, pose, float(cb), float(sb), range_max=3.0, miss=4.0)
        want = res * math.sqrt(float(k * k if deg in axes else 2 * k * k))
        assert hit == 1 and np.float64(r).view(np.uint64) == np.float64(want).view(np.uint64), (deg, r, want)


def test_miss_offmap_start_cell_and_unknown():
    g, res, origin = walled_room(), 0.05, (0.0, 0.0)
    pose = F.centre(20, 20, origin, res) + (1.0, 0.0)
    # the wall is 20 cells away: out of reach at R = 19, a hit at R = 20
    assert M.beam(g, origin, res, pose, 1.0, 0.0, range_max=19 * res + 0.01, miss=7.5) == (7.5, 0)
    assert M.beam(g, origin, res, pose, 1.0, 0.0, range_max=20 * res + 0.01, miss=7.5) == (res * math.sqrt(400.0), 1)
    # off the map: no beam, the flag; a NaN is off the map
    for bad in ((-0.01, 0.5), (0.5, 41 * res), (float("nan"), 0.5)):
        assert M.beam(g, origin, res, bad + (1.0, 0.0), 1.0, 0.0) is None
    r, rec = M.simulate(g[None], [origin], res, [(-0.01, 0.5, 1.0, 0.0)], [1.0, 0.0], [0.0, 1.0], miss=11.0)
    assert rec["flags"][0] == M.OFFMAP and rec["n_hits"][0] == 0 and (r == 11.0).all()
    r, rec = M.simulate(g[None], [origin], res, [pose, pose, pose], [1.0], [0.0], grid_idx=[0, 1, 0], count=2, range_max=3.0, miss=4.0)
    assert rec["flags"].tolist() == [0, M.BAD_INDEX, M.NO_POSE] and rec["n_hits"].tolist() == [1, 0, 0] and r[1:, 0].tolist() == [4.0, 4.0]
    # the start cell is never tested: from a wall cell the beam along the wall hits the next wall cell, the beam inwards crosses the room
    on_wall = F.centre(0, 20, origin, res) + (1.0, 0.0)
    assert M.beam(g, origin, res, on_wall, 0.0, 1.0, range_max=3.0) == (res * 1.0, 1)
    assert M.beam(g, origin, res, on_wall, 1.0, 0.0, range_max=3.0) == (res * math.sqrt(1600.0), 1)
    # unknown pixels
    g2 = g.copy()
    g2[20, 30] = -1
    assert M.beam(g2, origin, res, pose, 1.0, 0.0, range_max=3.0, unknown_is_obstacle=1) == (res * math.sqrt(100.0), 1)
    assert M.beam(g2, origin, res, pose, 1.0, 0.0, range_max=3.0, unknown_is_obstacle=0) == (res * math.sqrt(400.0), 1)
    # occupied_min
    g2[20, 25] = 60
    assert M.beam(g2, origin, res, pose, 1.0, 0.0, range_max=3.0, occupied_min=55)[0] == res * math.sqrt(25.0)
    assert M.beam(g2, origin, res, pose, 1.0, 0.0, range_max=3.0, occupied_min=70)[0] == res * math.sqrt(100.0)
    # a direction that is no unit vector: a miss without a walk
    assert M.beam(g, origin, res, pose, 1e9, 0.0, range_max=3.0, miss=4.0) == (4.0, 0)
    assert M.reach(10.0, 0.05) == 200 and M.reach(0.04, 0.05) == 0 and M.reach(4094.5, 1.0) == 4094 and M.reach(4095.0, 1.0) == 0
    assert M.skip_of(1.0, 0.05) == 20 and M.skip_of(0.04, 0.05) == 0 and M.skip_of(0.35, 0.05) == 6      # (0.35 / 0.05 = 6.999...)


@pytest.mark.parametrize("skip,w,h", [(1, 9, 7), (2, 9, 7), (7, 5, 9), (3, 1, 1)])
def test_lattice_equals_three_literal_loops(skip, w, h):
    rng = np.random.default_rng(skip * 100 + w)
    g = F.random_grid(rng, h, w, 0.1)
    origin, res = (-0.2, 0.4), 0.05
    for angle_step, box in ((math.pi / 4, None), (2.1, (-0.1, 0.45, 0.1, 0.6)), (7.0, None)):
        cs, sn = M.headings(angle_step)
        poses, index = [], []
        nyaw_count = 0
        theta = 0.0
        while theta < 6.28:
            nyaw_count += 1
            theta += angle_step
        assert len(cs) == nyaw_count
        npy = (h + skip - 1) // skip
        for ix in range(0, w, skip):
            for iy in range(0, h, skip):
                theta, t = 0.0, 0
                while theta < 6.28:
                    cx, cy = origin[0] + (ix + 0.5) * res, origin[1] + (iy + 0.5) * res
                    if g[iy, ix] == 0 and (box is None or (box[0] <= cx <= box[2] and box[1] <= cy <= box[3])):
                        poses.append((cx, cy, math.cos(theta), math.sin(theta)))
                        index.append(((ix // skip) * npy + iy // skip) * nyaw_count + t)
                    theta += angle_step
                    t += 1
        got = M.lattice(g, origin, res, skip, cs, sn, box)
        assert got["passed"] == got["written"] == len(poses)
        assert np.array_equal(got["poses"].view(np.uint64), np.array(poses, dtype=np.float64).reshape(-1, 4).view(np.uint64))
        assert got["index"].tolist() == index
        cap = max(1, len(poses) // 2)
        capped = M.lattice(g, origin, res, skip, cs, sn, box, capacity=cap)
        assert capped["written"] == min(cap, len(poses)) and capped["passed"] == len(poses)
        assert np.array_equal(capped["poses"], got["poses"][:cap])
