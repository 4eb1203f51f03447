"""The NumPy model of the laser-scan projection (tests/scanproject_model.py) against its own specification (include/ndtgpu.h
"laser-scan projection"), and the library's pure host function ndtgpu_scanproj_beam against the model.  No device is needed.

THE TOLERANCE of x and y, derived and not measured: both sides round the same fp64 a_i = angle_min + i * angle_increment; their
cosines and sines (two correctly working fp64 libraries) and so their fp64 products differ by a few fp64 units in the last place,
2^-28 of a float32 step; the two roundings to float can therefore only land on the same float or on neighbours: at most ONE float32
unit in the last place of the model's value (np.spacing).  The kept flags and z (no library function) are equal bit for bit."""
import math

import numpy as np
import pytest

import scanproject_model as M


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def edge_ranges(r_min=0.5, r_max=30.0):
    inf, nan = float("inf"), float("nan")
    return [r_min, np.nextafter(r_min, inf), np.nextafter(r_min, -inf), r_max, np.nextafter(r_max, inf), np.nextafter(r_max, -inf),
            nan, inf, -inf, 0.0, -0.0, -1.0, -29.0, 5e-324, 1.0, 29.999]


def test_gates_are_strict():
    r = np.array(edge_ranges())
    k = M.kept(r)
    assert k.tolist() == [False, True, False, False, False, True, False, False, False, False, False, False, False, False, True, True]
    # no upper gate with r_max = +inf: every finite range above r_min stays, +inf itself does not
    k = M.kept(np.array([0.5, 0.6, 1e300, float("inf"), float("nan"), -float("inf")]), 0.5, float("inf"))
    assert k.tolist() == [False, True, True, False, False, False]
    assert M.kept(np.array([0.0, 5e-324]), 0.0, 1.0).tolist() == [False, True]


def test_cloud_order_pads_and_z():
    rng = np.random.default_rng(3)
    r = rng.uniform(0.0, 35.0, size=(3, 257))
    r[0, ::7] = np.nan
    r[1, :] = 31.0                                   # none kept
    r[2, :] = 2.0                                    # all kept
    a0, inc = -2.0, 0.013
    xyz, n_kept = M.project(r, a0, inc, seed=9)
    assert n_kept.tolist() == [int(M.kept(r[0]).sum()), 0, 257]
    for b in range(3):
        assert not np.isnan(xyz[b, :n_kept[b]]).any() and np.isnan(xyz[b, n_kept[b]:]).all()
        assert (xyz[b, :n_kept[b], 2] >= 0).all() and (xyz[b, :n_kept[b], 2].astype(np.float64) < 0.02).all()
    # ascending beam order: the kept points' bearings are those of the kept beams, in order
    beams = np.nonzero(M.kept(r[0]))[0]
    ang = np.arctan2(xyz[0, :n_kept[0], 1].astype(np.float64), xyz[0, :n_kept[0], 0].astype(np.float64))
    want = np.arctan2(np.sin(a0 + beams * inc), np.cos(a0 + beams * inc))
    assert np.max(np.abs(np.angle(np.exp(1j * (ang - want))))) < 1e-6
    assert np.allclose(np.hypot(xyz[0, :n_kept[0], 0], xyz[0, :n_kept[0], 1]), r[0, beams], rtol=1e-6)
    # z is drawn by the beam index, the scan id and the seed
    u = M.hash_uniform(9, 0, beams)
    assert np.array_equal(xyz[0, :n_kept[0], 2], (0.02 * u).astype(np.float32))
    assert not np.array_equal(M.project(r[:1], a0, inc, seed=10)[0][0, :, 2], xyz[0, :, 2])
    assert not np.array_equal(M.project(r[:1], a0, inc, scan_ids=[5], seed=9)[0][0, :, 2], xyz[0, :, 2])
    assert np.array_equal(M.project(r, a0, inc, varz=0.0)[0][2, :, 2], np.zeros(257, dtype=np.float32))


def test_a_beams_point_does_not_depend_on_the_other_beams():
    rng = np.random.default_rng(4)
    r = rng.uniform(0.6, 29.0, size=300)
    a0, inc = 0.3, -0.02
    k0, p0 = M.points(r, a0, inc, scan_id=7, seed=2)
    r2 = r.copy()
    r2[::2] = np.nan                                 # every second beam dropped: the others move up in the cloud, unchanged
    k2, p2 = M.points(r2, a0, inc, scan_id=7, seed=2)
    assert np.array_equal(p0[1::2], p2[1::2]) and k2[1::2].all() and not k2[::2].any()
    xyz, n_kept = M.project(r2[None], a0, inc, scan_ids=[7], seed=2)
    assert n_kept[0] == 150 and np.array_equal(xyz[0, :150], p0[1::2])
    # ... nor on the batch: the scan alone, and as the third of three
    batch = np.stack([r, r2, r])
    xb, nb = M.project(batch, a0, inc, scan_ids=[1, 2, 7], seed=2)
    assert np.array_equal(xb[2], M.project(r[None], a0, inc, scan_ids=[7], seed=2)[0][0])


def ulp_ok(got, want):
    """equal (a range near the largest double overflows to the same infinity on both sides), or one float32 step apart"""
    with np.errstate(invalid="ignore"):
        return (got == want) | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def test_library_beam_against_the_model(N):
    """ndtgpu_scanproj_beam over a few thousand random and edge ranges: flags and z bits equal, x and y within one float32 ulp"""
    rng = np.random.default_rng(5)
    cases = 0
    worst = 0.0
    for a0, inc, scan_id, seed, prm in ((-math.pi, 2.0 * math.pi / 1440, 0, 0, {}), (0.37, -0.0043, 123456789012, 77, dict(varz=0.5)),
                                        (-2.35619449, 0.00436332, 3, 2 ** 63 + 5, dict(r_min=0.0, r_max=float("inf"), varz=0.0)),
                                        (1e3, 0.1, 2 ** 64 - 1, 1, dict(r_min=1.0, r_max=2.0))):
        p = dict(M.DEFAULTS, **prm)
        r = np.concatenate([rng.uniform(0.0, 1.2 * min(p["r_max"], 40.0), size=800), rng.uniform(p["r_min"], min(p["r_max"], 40.0), size=200),
                            np.array(edge_ranges(p["r_min"], p["r_max"]))])
        idx = np.concatenate([rng.integers(0, 1 << 20, size=r.shape[0] - 3), [0, (1 << 20) - 1, 1439]])
        k, pts = M.points(r, a0, inc, scan_id=scan_id, idx=idx, seed=seed, **prm)
        for j in range(r.shape[0]):
            got = N.scan_project_beam(a0, inc, scan_id, int(idx[j]), float(r[j]), seed=seed, **prm)
            assert (got is not None) == bool(k[j]), (a0, j, r[j])
            if got is None:
                continue
            assert got[2].tobytes() == pts[j, 2].tobytes(), (a0, j)
            assert ulp_ok(got[:2], pts[j, :2]).all(), (a0, j, got, pts[j])
            if np.isfinite(pts[j, :2]).all():
                worst = max(worst, float(np.max(np.abs(got[:2].astype(np.float64) - pts[j, :2]) / np.spacing(np.abs(pts[j, :2])))))
            cases += 1
    print("ndtgpu_scanproj_beam against the model: %d kept beams, worst |dx| %.0f float32 ulp" % (cases, worst))
    assert cases > 2000
