"""The localisation monitor's NumPy model (tests/locmon_model.py) against independent statements of the same thing: its distance field
against SciPy's exact Euclidean distance transform, its median against a literal restatement of the reference's loop, its ordered
selections against hand-made cases.  No device, no library."""
import math

import numpy as np
import pytest

import locmon_model as M
from locmon_fixtures import random_grid


@pytest.mark.parametrize("h,w,R", [(1, 1, 1), (3, 5, 2), (65, 67, 7), (130, 259, 20)])
def test_field_equals_scipy_exact_edt(h, w, R):
    """rint(d^2) of distance_transform_edt, capped at R^2, on random grids"""
    from scipy.ndimage import distance_transform_edt
    rng = np.random.default_rng(1000 * h + R)
    for p_occ, occ_min in ((0.0005, 55), (0.01, 55), (0.01, 70), (0.2, 55)):
        g = random_grid(rng, h, w, p_occ)
        if h * w > 1:
            g[rng.integers(h), rng.integers(w)] = 100          # (the transform of a grid with no obstacle is not defined)
        obst = g >= occ_min
        got = M.field(g, R, occ_min)
        if not obst.any():
            assert (got == M.FIELD_FAR).all()
            continue
        d2 = np.rint(distance_transform_edt(~obst) ** 2).astype(np.int64)
        want = np.where(d2 <= R * R, d2, M.FIELD_FAR).astype(np.uint16)
        assert np.array_equal(got, want), (h, w, R, p_occ, occ_min)


def test_field_edges():
    assert (M.field(np.zeros((4, 6), dtype=np.int8), 3) == M.FIELD_FAR).all()
    assert (M.field(np.full((4, 6), 100, dtype=np.int8), 3) == 0).all()
    assert (M.field(np.full((4, 6), -1, dtype=np.int8), 3) == M.FIELD_FAR).all()
    g = np.zeros((5, 9), dtype=np.int8)
    g[0, 0] = 55
    f = M.field(g, 3)
    assert f[0, 0] == 0 and f[0, 3] == 9 and f[0, 4] == M.FIELD_FAR and f[2, 2] == 8 and f[3, 1] == M.FIELD_FAR and f[3, 0] == 9
    assert M.field(g, 3, occupied_min=56).min() == M.FIELD_FAR
    assert M.radius(0.375, 0.05) == 7 and M.radius(0.375, 0.1) == 3 and M.radius(0.04, 0.05) == 0 and M.radius(100.0, 0.05) == 0
    assert M.radius(12.7, 0.05) == 254 or M.radius(12.7, 0.05) == 253


def test_median_is_the_reference_loop():
    """distances[size / 2] of the sorted per-beam distances with cos(theta0 + a_i) as the reference writes it, against the model's
    angle-addition form: an endpoint within rounding of a pixel edge may fall either way, so the medians agree to within the step
    between neighbouring field values (below 1.5 pixels), not bit for bit"""
    rng = np.random.default_rng(5)
    res, R = 0.05, 7
    g = np.zeros((80, 90), dtype=np.int8)
    g[10, :] = 100
    g[:, 70] = 100
    fld = M.field(g, R)
    origin = (-1.0, -2.0)
    n = 181
    amin, ainc = -math.pi / 2, math.pi / 180
    cb, sb = M.beam_table(n, amin, ainc)
    for trial in range(20):
        x0, y0, th = rng.uniform(0.5, 2.0), rng.uniform(-1.0, 1.0), rng.uniform(-3, 3)
        r = rng.uniform(0.2, 3.0, n)
        d = []
        for i in range(n):
            a = th + amin + i * ainc
            px, py = x0 + math.cos(a) * r[i], y0 + math.sin(a) * r[i]
            ci, cj = math.floor((px - origin[0]) / res), math.floor((py - origin[1]) / res)
            if 0 <= ci < 90 and 0 <= cj < 80:
                f = int(fld[cj, ci])
                d.append(0.375 if f == M.FIELD_FAR else res * math.sqrt(f))
            else:
                d.append(1e9)
        want = sorted(d)[n // 2]
        q = np.zeros(1, dtype=[("scan", "<u4"), ("grid", "<u4"), ("x", "<f8"), ("y", "<f8"), ("c", "<f8"), ("s", "<f8")])
        q["x"], q["y"], q["c"], q["s"] = x0, y0, math.cos(th), math.sin(th)
        got = M.evaluate([fld], [origin], res, 0.375, cb, sb, r[None], q)[0]
        assert got["n_kept"] == n and got["flags"] == 0
        assert abs(got["badness"] - want) <= res * 1.5, (trial, got, want)       # (a beam on a pixel edge may fall either way)


def test_flags_and_gates():
    fld = M.field(np.full((4, 4), 100, dtype=np.int8), 2)
    cb, sb = M.beam_table(4, 0.0, 0.1)
    r = np.array([[np.nan, np.inf, 0.0, -1.0], [0.1, 0.1, 0.1, 500.0], [0.1, 0.1, 500.0, 500.0]])
    q = np.zeros(6, dtype=[("scan", "<u4"), ("grid", "<u4"), ("x", "<f8"), ("y", "<f8"), ("c", "<f8"), ("s", "<f8")])
    q["c"] = 1.0
    q["scan"] = [0, 1, 2, 3, 0, M.NO_SCAN]
    q["grid"] = [0, 0, 0, 0, 1, 0]
    out = M.evaluate([fld], [(0.0, 0.0)], 0.05, 0.1, cb, sb, r, q)
    assert out["flags"].tolist() == [M.NO_BEAMS, 0, 0, M.BAD_INDEX, M.BAD_INDEX, M.NO_QUERY]
    assert out["key"].tolist() == [M.KEY_OFFMAP, 0, M.KEY_OFFMAP, M.KEY_OFFMAP, M.KEY_OFFMAP, M.KEY_OFFMAP]
    assert out["n_kept"].tolist() == [0, 4, 4, 0, 0, 0] and out["n_offmap"].tolist() == [0, 1, 2, 0, 0, 0]
    assert out["badness"].tolist() == [1e9, 0.0, 1e9, 1e9, 1e9, 1e9]
    gated = M.evaluate([fld], [(0.0, 0.0)], 0.05, 0.1, cb, sb, r, q[1:2], r_min=0.1, r_max=500.0)
    assert gated["flags"][0] == M.NO_BEAMS                                    # at r_min and at r_max: dropped
    assert M.metres(M.KEY_FAR, 0.05, 0.375) == 0.375 and M.metres(49, 0.05, 0.375) == 0.05 * 7.0


def test_ordered_selections():
    status = [0, 0, 1, 0, 0]
    n_in = [8, 12, 40, 12, 9]
    m4 = np.tile(np.array([0.0, 0.0, 1.0, 0.0]), (5, 1))
    refs = np.array([[k, 0.0, 1.0, 0.0] for k in range(5)], dtype=np.float64)
    q, p = M.pick(status, n_in, m4, refs, 3, 0)
    assert p == dict(pair=1, n_inliers=12, flags=0) and q["scan"] == 3 and q["x"] == 1.0 - 0.275
    q, p = M.pick([0], [8], m4[:1], refs[:1], 3, 0)
    assert p["pair"] == -1 and p["flags"] == M.NO_PICK and q["scan"] == M.NO_SCAN
    q, p = M.pick([], [], m4[:0], refs[:0], 3, 0)
    assert p["pair"] == -1
    th = 0.3
    o = M.compose((1.0, 2.0, math.cos(0.5), math.sin(0.5)), (0.4, -0.1, math.cos(th), math.sin(th)), (-0.275, 0.0))
    c, s = math.cos(0.5), math.sin(0.5)
    wx, wy = 1.0 + c * 0.4 + s * 0.1, 2.0 + s * 0.4 - c * 0.1
    assert abs(o[0] - (wx - 0.275 * math.cos(0.8))) < 1e-12 and abs(o[1] - (wy - 0.275 * math.sin(0.8))) < 1e-12
    assert abs(o[2] - math.cos(0.8)) < 1e-12 and abs(o[3] - math.sin(0.8)) < 1e-12
