"""csrc/ndt_binning.h and csrc/ndt_wave.h checked directly, as host code and on the device.

tests/native/build_checks.hip includes the two headers alone and runs ONE function per row, in a loop on the host or from a
one-thread-per-row kernel on the device.  Every check below is written once, as a function of a run(mode, table) callable, and used
twice: unmarked with the host target, under @pytest.mark.gpu with the device target (workgroups of one wave, `gpu`, and of four,
`gpu256`).  The wave primitives exist on the device only.  References are numpy float64 (numpy does not contract a product into
an add) and Python int / fractions.Fraction:

  bin       NdtBinner::fast, then ::exact where fast asked for it, against LazyGrid's index formula, the range test on
            (double)p - origin and z <= z_max, for 200 000 points in each of BIN_GEOMETRIES: the slot of every point; NaN points;
            scalarize() changes nothing (device); how many points take the exact path.
  fixed     ndt_fixed_from_double against round(Fraction(t)) (half to even), |t| < 2^62.
  gauss     ndt_gaussian_from_moments on int64 moments made in Python integers from points on a dyadic lattice: covariance, mean
            and rescaled covariance against exact rationals, and which cells get a Gaussian at all.
  lanemap   ndt_moment_of_lane names each moment once.
  scan, xor, swapadd, moments    ndt_wave_incl_scan, xor_lane, pl_swap_add, wave_sum_moments by bits against numpy restatements.

Bounds, with their derivations at the checks: covariance 18 units (nine roundings on the path, doubled) of
2^-52 res^2 n / (n - 1) max|u|^2; mean 2 ulp of the exact centre + m res; rescaled covariance 3.01 * 18 of the covariance's units
(the eigenvalue clamp is 1-Lipschitz in the Frobenius norm) plus 512 units of 2^-52 lambda_max, a worst case over 18 Jacobi
rotations that is about 50 times the measurement.  Measured maxima (the device is an MI355X):
                                                   host     device
  covariance, shifts (45, 45)                      1.097    1.097
  covariance, shifts (38, 38)                      0.945    0.945
  covariance, odd grid (40, 38), |u| <= 1.9        1.173    1.173
  mean [ulp]                                       1.846    1.846
  rescaled covariance [share of its bound]         0.0202   0.0202
Share of the uniform points that take the exact path, the largest over the geometries the cap applies to and that keep uniform
points at all: 0.488 % on the host, 0.488 % on the device (cap 1 %).  Geometries 9, 12 and 14 keep no or almost no uniform point
(a range of millimetres, or a sphere above the grid): their share says nothing about the fast path.  Which geometries the cap
applies to is decided by restating init()'s own rule; the slot reference is independent of it.

What the checks found on the commit before this file (host):
  bin       geometry 12 (origin (10000.1, 20000.2, 0.05), range 0.5): 9985 of 200 000 points in the wrong cell -- the band of the
            fp32 range test did not cover the rounding of the origin to fp32; NdtBinner::init now widens it by that much.  Every
            other of the issue's thirteen geometries: 0 mismatches (geometries 13 and 14 are additions: a range so short that no band
            below range^2 covers the origin's rounding -- 26354 points in the wrong cell -- and geometry 9's range inside its grid).
            Geometry 5 (0.05 m cells around (1000.5, -2000.25)) sent 2.412 % of its uniform points to the exact path, over
            the cap of 1 %: the face guard charged 2^-24 each for the roundings of 1 / res and of k to fp32, which are both
            exact there; init() now measures them (0.172 %).  The other capped geometries: 0.43 % at most.  Geometries 15 and 16
            make each measured term necessary: with either dropped from the guard their points next to faces change cell.
  fixed     nothing.
  gauss     164 of 1500 exactly rank-deficient cells got a Gaussian (noise of the moments' fixed-point rounding and of
            S - n m m^T decided); ndt_first_gaussian_rank_deficient now compares with the floor of that noise.  Nothing else.
            (End to end, tests/test_gpu_parity.py::test_rank_deficient_cells_get_no_gaussian: 14 such cells of 2500 on an MI355X
            from the general build kernel, 3 from add_cloud.)
  lanemap   nothing.
"""
import functools
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "build_checks.hip")
WIDTH_IN = {"bin": 2, "fixed": 1, "gauss": 19, "lanemap": 1, "scan": 1, "xor": 1, "swapadd": 2, "moments": 9}
WIDTH_OUT = {"bin": 4, "fixed": 1, "gauss": 10, "lanemap": 1, "scan": 1, "xor": 4, "swapadd": 2, "moments": 1}
EPS = 2.0 ** -52
INF = float("inf")
NDT_DEGENERATE_REL = 1e-9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = str(tmp_path_factory.mktemp("build") / "build_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", SRC, "-o", out])
    return out


def _runner(exe, target):
    cmd = [exe] if target == "host" else ["timeout", "-k", "10", "60", exe]

    def run(mode, table):
        table = np.ascontiguousarray(table, dtype=np.uint64)
        assert table.ndim == 2 and table.shape[1] == WIDTH_IN[mode]
        n = table.shape[0]
        out = subprocess.run(cmd + [mode, target], input=np.uint32(n).tobytes() + table.tobytes(), capture_output=True)
        assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace"))
        return np.frombuffer(out.stdout, dtype=np.uint64).reshape(n, WIDTH_OUT[mode])
    run.target = target
    return run


def _words(a):
    """float64 / int64 values as the 64-bit words of a table"""
    return np.ascontiguousarray(a).view(np.uint64)


# ---- bin ------------------------------------------------------------------------------------------------------------------------
# res, cells per axis, grid centre, range origin, range (0: none), z_max
BIN_GEOMETRIES = [
    (0.5, (160, 160, 2), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, INF),
    (0.5, (160, 160, 2), (12.3, -7.65, 0.2), (1.0, 2.0, 0.0), 30.0, INF),
    (0.5, (161, 160, 3), (12.3, -7.65, 0.2), (1.0, 2.0, 0.0), 30.0, INF),
    (0.5, (159, 77, 5), (0.1, 0.2, 0.3), (0.1, 0.2, 0.3), 12.0, 1.0),
    (0.4, (100, 100, 20), (0.13, -0.07, 0.02), (0.0, 0.0, 0.0), 0.0, INF),
    (0.05, (2000, 2000, 2), (1000.5, -2000.25, 0.0), (1000.5, -2000.25, 0.0), 40.0, INF),
    (0.05, (2000, 2000, 2), (1e5, 3e5, 0.0), (1e5, 3e5, 0.0), 40.0, INF),
    (0.05, (2000, 2000, 2), (1e7, 3e5, 0.0), (1e7, 3e5, 0.0), 0.0, INF),
    (0.1, (512, 512, 64), (0.123456789, 9.87654321, -1.2345), (0.333, 0.777, 0.111), 20.123456789, 2.5),
    (0.5, (160, 160, 2), (0.0, 0.0, 0.0), (0.1, 0.2, 0.3), 0.003, INF),
    (1.0, (4000, 4000, 2), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1500.0, INF),
    (0.5, (160, 160, 2), (1000.1, 2000.2, 0.0), (1000.1, 2000.2, 0.05), 1.0, INF),
    # the fp32 range test against an origin that is far from an fp32 number, relative to the range
    (0.5, (160, 160, 2), (10000.1, 20000.2, 0.0), (10000.1, 20000.2, 0.05), 0.5, INF),
    # ... and so far that no band below range^2 covers it: every point goes through the fp64 range test
    (0.5, (160, 160, 2), (10000.1, 20000.2, 0.0), (10000.1, 20000.2, 0.05), 0.002, INF),
    # a range of millimetres (as in geometry 9) around an origin inside the grid
    (0.5, (160, 160, 2), (0.0, 0.0, 0.0), (0.1, 0.2, 0.1), 0.003, INF),
    # the two terms that init() measures for the face guard, each alone in a geometry's error budget (the fma's own rounding is
    # 1e-5 cell in both): |p / res| |inv32 res - 1| = 4.8e-4 cell with a cell size whose reciprocal is a poor fp32 number, a centre
    # on the cell lattice 20 000 cells out (k is an fp32 number) ...
    (0.3, (160, 160, 2), (6000.0, -4500.0, 0.0), (0.0, 0.0, 0.0), 0.0, INF),
    # ... and |k32 - k| = 2.0e-4 cell with a cell size whose reciprocal is an fp32 number and a centre off the lattice 10 000
    # cells out (0.4 m, not 0.5: the faces then meet the fp32 numbers of the points at every offset).  A guard without the
    # term puts points next to faces (the last eighth, 1e-8 to 1e-2 cell away) into the neighbouring cell.
    (0.4, (160, 160, 2), (-4000.13, 3200.07, 0.0), (0.0, 0.0, 0.0), 0.0, INF),
]
BIN_EIGHTH = 25000


def _bin_fast_path_expected(geom):
    """NdtBinner::init's rule restated: the fp32 index path exists on even grids where 2.4e-7 (size + 1 + |k|), the error bound
    of fma(p, inv32, k32) with k = 0.5 + size / 2 - c / res, is below a quarter cell."""
    res, size, c, _, _, _ = geom
    if any(s & 1 for s in size):
        return False, None
    kmax = max(abs(0.5 + s / 2.0 - cc / res) for s, cc in zip(size, c))
    guard = 2.4e-7 * (max(size) + 1 + kmax)
    assert not 0.2 < guard < 0.3                                           # (no geometry at the threshold)
    return guard < 0.25, guard


@functools.lru_cache(maxsize=None)
def _bin_points(gi):
    res, size, c, o, rng, _ = BIN_GEOMETRIES[gi]
    g = np.random.default_rng(1000 + gi)
    m = BIN_EIGHTH
    size, c, o = np.array(size, dtype=np.float64), np.array(c), np.array(o)
    ext = size * res

    def uniform():
        return c + g.uniform(-0.55, 0.55, (m, 3)) * ext

    def faces(axis):
        # a cell face is where (p - c) / res + 0.5 is an integer t
        t = g.integers(-int(size[axis]) // 2 - 1, int(size[axis]) // 2 + 2, m)
        return c[axis] + (t - 0.5) * res

    def sphere(eps):
        d = g.normal(size=(m, 3)) * np.array([1.0, 1.0, 0.02])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        radius = rng if rng > 0 else 0.4 * min(ext[0], ext[1])
        return o + radius * (1.0 + eps)[:, None] * d
    parts = [uniform()]                                                    # 0: uniform over 1.1 times the grid
    for axis, pert in ((0, 0.0), (1, 5e-8), (2, 0.0)):                     # 1, 2, 3: on x, y (perturbed), z faces
        q = uniform()
        f = faces(axis)
        if pert:
            f = f * (1.0 + g.choice([-pert, pert], m))
        q[:, axis] = f
        parts.append(q)
    parts.append(sphere(g.uniform(-2e-7, 2e-7, m) * (g.random(m) < 0.8)))  # 4: on the range sphere
    special = np.concatenate(parts[1:5]).astype(np.float32)                # 5: such points moved one fp32 ulp
    pick = special[g.integers(0, len(special), m)]
    step = g.integers(-1, 2, (m, 3))
    moved = np.where(step > 0, np.nextafter(pick, np.float32(np.inf)), np.where(step < 0, np.nextafter(pick, np.float32(-np.inf)), pick))
    # 6: at the edges of the band of the fp32 range test (1e-3 of range^2 is 5e-4 of the range) and well clear of it
    parts.append(sphere(g.choice([3e-4, 4.9e-4, 5e-4, 5.1e-4, 2e-3], m) * g.choice([-1.0, 1.0], m)))
    q = uniform()                                                          # 7: next to faces, 1e-8 to 1e-2 cell away
    axis = g.integers(0, 3, m)
    f = np.stack([faces(0), faces(1), faces(2)], axis=1)[np.arange(m), axis]
    q[np.arange(m), axis] = f + res * 10.0 ** g.uniform(-8, -2, m) * g.choice([-1.0, 1.0], m)
    parts.append(q)
    pts = np.concatenate([p.astype(np.float32) for p in parts[:5]] + [moved] + [p.astype(np.float32) for p in parts[5:]])
    assert pts.shape == (8 * m, 3)
    bad = g.integers(m, 8 * m, 900)                                        # NaN and +-Inf, not among the uniform eighth
    pts[bad, g.integers(0, 3, 900)] = g.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 900)
    pts[m] = np.nan
    return pts


def _bin_reference(geom, pts):
    res, size, c, o, rng, z_max = geom
    p = pts.astype(np.float64)
    inb = np.ones(len(p), dtype=bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            v = np.floor((p[:, a] - c[a]) / res + 0.5) + size[a] / 2.0
            ok = (v > -2.0e9) & (v < 2.0e9)                                # lazygrid_index's guard; NaN fails it
            i = np.where(ok, np.trunc(np.where(ok, v, 0.0)), -1.0).astype(np.int64)   # double -> int truncates
            inb &= (i >= 0) & (i < size[a])
            idx.append(i)
        e = p - np.array(o)
        d = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        okr = ~(d > rng) if rng > 0 else np.ones(len(p), dtype=bool)
        okz = pts[:, 2] <= np.float32(z_max)
    slot = (idx[0] * size[1] + idx[1]) * size[2] + idx[2]
    return np.where(inb & okr & okz, slot, -1), okr & okz


def _bin_table(geom, pts):
    res, size, c, o, rng, z_max = geom
    head = np.array([res, size[0], size[1], size[2], c[0], c[1], c[2], o[0], o[1], o[2], rng, z_max], dtype=np.float64)
    t = np.zeros((6 + len(pts), 2), dtype=np.uint64)
    t[:6] = _words(head).reshape(6, 2)
    b = np.ascontiguousarray(pts).view(np.uint32).astype(np.uint64)
    t[6:, 0] = b[:, 0] | (b[:, 1] << np.uint64(32))
    t[6:, 1] = b[:, 2]
    return t


def check_bin(run, gi, label):
    geom = BIN_GEOMETRIES[gi]
    pts = _bin_points(gi)
    out = run("bin", _bin_table(geom, pts))
    frac_lim = out[0, 0:1].view(np.uint32)[0:1].view(np.float32)[0]
    o = np.ascontiguousarray(out[6:]).view(np.int32).reshape(len(pts), 8)
    fast_slot, need, final, named = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
    want, ok_ref = _bin_reference(geom, pts)
    nan = np.isnan(pts).any(axis=1)
    assert nan.sum() > 50 and np.isinf(pts).any(axis=1).sum() > 100
    uni = slice(0, BIN_EIGHTH)
    share = float(np.mean(need[uni] != 0))
    kept_uni = int(np.sum(want[uni] >= 0))                                 # (0: the cap below says nothing about this geometry)
    wrong = int(np.sum(final != want))
    print("bin on %s, geometry %d: %d of %d points in the wrong cell, %.4f %% of the uniform points take the exact path, %d of them kept (frac_lim %g)"
          % (label, gi, wrong, len(pts), 100.0 * share, kept_uni, frac_lim))
    assert np.sum(ok_ref) > 1000 and (np.sum(want >= 0) > 1000 or gi == 9)   # (points are kept; geometry 9's sphere is above its grid)
    # (a) the cell of every point: fast()'s where it did not ask, exact()'s where it did
    assert wrong == 0, np.flatnonzero(final != want)[:10]
    assert np.all((need != 0) | (fast_slot == final))
    assert np.all(named == 1)                                              # the three floats name the same cell
    # (b) NaN: dropped, and not sent to exact()
    assert np.all(final[nan] == -1) and np.all(need[nan] == 0)
    # (c) scalarize() changes nothing
    if run.target != "host":
        assert np.array_equal(o[:, :4], o[:, 4:])
    # (d) the fast path is taken where it exists, and by nobody where it does not
    has_fast, guard = _bin_fast_path_expected(geom)
    assert (frac_lim >= 0) == has_fast
    res, size, c, org, rng, _ = geom
    d32 = np.abs(np.array(org) - np.array(org, dtype=np.float32).astype(np.float64))
    band_ok = rng <= 0 or 2.0 * (2.0 * rng * d32.sum() + d32.sum() ** 2) + 1e-3 * rng * rng < rng * rng
    if has_fast and band_ok:
        assert share < 0.01, share
    else:
        assert np.all(need[uni][ok_ref[uni]] != 0)
    return share if (has_fast and band_ok and kept_uni > 0) else None


@pytest.mark.parametrize("gi", range(len(BIN_GEOMETRIES)))
def test_bin_host(exe, gi):
    check_bin(_runner(exe, "host"), gi, "host")


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["gpu", "gpu256"])
def test_bin_gpu(exe, target):
    run = _runner(exe, target)
    shares = [check_bin(run, gi, "device") for gi in range(len(BIN_GEOMETRIES))]
    print("bin on device: largest share on the exact path %.4f %%" % (100.0 * max(s for s in shares if s is not None)))


# ---- fixed ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_cases():
    g = np.random.default_rng(5)
    n = 200000
    parts = [np.ldexp(g.uniform(1.0, 2.0, n), g.integers(-60, 61, n)) * g.choice([-1.0, 1.0], n)]   # 2^-60 .. 2^61
    k = np.concatenate([np.arange(-64, 65), g.integers(-2 ** 50, 2 ** 50, 2000)]).astype(np.float64)
    parts.append(k + 0.5)                                                  # ties
    k = np.concatenate([np.arange(-64, 65), g.integers(-2 ** 19, 2 ** 19, 2000)]).astype(np.float64) * 4294967296.0
    parts += [k + 0.5, k - 0.5, k - 2.0 ** -20, k - 0.25, k + 0.25]        # the carry where lo rounds up to 2^32
    parts.append(np.array([0.0, -0.0, 2.0 ** 62 - 512.0, -(2.0 ** 62 - 512.0), 2.0 ** 32, -2.0 ** 32, 2.0 ** 32 - 0.5, 4294967295.5,
                           0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 52 + 1.0, 2.0 ** 53, -2.0 ** 61]))
    t = np.concatenate(parts)
    assert np.all(np.abs(t) < 2.0 ** 62)
    want = np.array([round(F(float(v))) for v in t], dtype=np.int64)
    return t, want


def check_fixed(run):
    t, want = _fixed_cases()
    got = run("fixed", _words(t).reshape(-1, 1)).view(np.int64).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(float(t[i]), int(got[i]), int(want[i])) for i in bad[:10]]


def test_fixed_host(exe):
    check_fixed(_runner(exe, "host"))


@pytest.mark.gpu
def test_fixed_gpu(exe):
    check_fixed(_runner(exe, "gpu"))


# ---- gauss ----------------------------------------------------------------------------------------------------------------------
# A cell is a list of points in Python integers on the lattice 2^-L cell around the cell's centre, so that sums of the points and of
# their products are exact.  The three scalings of the accumulators: name -> (s1_shift, s2_shift, L, largest |u|)
SCALINGS = {"45": (45, 45, 22, 0.5), "38": (38, 38, 19, 0.5), "odd": (40, 38, 19, 1.9)}
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
Q3 = [[1, 2, 2], [2, 1, -2], [2, -2, 1]]                                    # three times a rotation, in integers


def _round_shift(num, bits):
    """num * 2^bits rounded to an integer, half to even (what ndt_fixed_from_double makes of an exactly known sum)"""
    return num << bits if bits >= 0 else round(F(num, 1 << -bits))


def _moments(K, L, s1_shift, s2_shift, runs=None):
    """The accumulators of the points K: every run (a list of indices; default: one run of all) is rounded once."""
    s1, s2 = [0, 0, 0], [0] * 6
    for r in (runs if runs is not None else [range(len(K))]):
        for a in range(3):
            s1[a] += _round_shift(sum(K[i][a] for i in r), s1_shift - L)
        for k, (a, b) in enumerate(PAIRS):
            s2[k] += _round_shift(sum(K[i][a] * K[i][b] for i in r), s2_shift - 2 * L)
    return s1, s2


def _exact_stats(K, L, res):
    """mean offset [cell] and covariance [m^2] of the points, in rationals: (n S2 - S1 S1^T) / (n (n - 1)) res^2"""
    n = len(K)
    S1 = [sum(k[a] for k in K) for a in range(3)]
    cov = [[F(n * sum(k[a] * k[b] for k in K) - S1[a] * S1[b], n * (n - 1) << (2 * L)) * F(res) ** 2 for b in range(3)] for a in range(3)]
    return [F(S1[a], n << L) for a in range(3)], cov


def _floor_m2(K, L, res, s1_shift, s2_shift):
    """The noise floor of a first Gaussian's eigenvalues (csrc/ndt_binning.h, ndt_first_gaussian_floor) restated from its derivation:
    n runs round once each to 2^-shift (half a unit), S1's error enters through 2 |m| < 4, sixteen fp64 roundings of at most
    2^-53 * 4 n; a 3 x 3 matrix of entries <= e has eigenvalues <= 3 e; n / (n - 1) <= 2 (one floor for all cells of a launch)."""
    return 6.0 * res * res * (0.5 * 2.0 ** -s2_shift + 2.0 * 2.0 ** -s1_shift + 2.0 ** -47)


def _gauss_row(n, s1, s2, slot, centre, res, n_min, eval_factor, s1_shift, s2_shift):
    row = np.zeros(19, dtype=np.uint64)
    row[:11] = np.array([n] + list(s1) + list(s2) + [slot], dtype=np.int64).view(np.uint64)
    row[11:] = _words(np.array(list(centre) + [res, n_min, eval_factor, s1_shift, s2_shift], dtype=np.float64))
    return row


def _decode_cells(out):
    vals = np.ascontiguousarray(out[:, :9]).view(np.float64)
    n = (out[:, 9] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    slot = (out[:, 9] >> np.uint64(32)).astype(np.int64)
    return vals[:, :3], vals[:, 3:9], n, slot


def _lattice(u, L):
    return [tuple(int(v) for v in row) for row in np.rint(np.asarray(u) * 2.0 ** L)]


def _symmetric_set(d, M, off):
    """Points whose covariance is exactly M diag(2 d_a^2) M^T / (n - 1): +-d_a along each axis, moved by M and off"""
    pts = []
    for a in range(3):
        for s in (1, -1):
            e = [0, 0, 0]
            e[a] = s * d[a]
            pts.append(tuple(sum(M[r][k] * e[k] for k in range(3)) + off[r] for r in range(3)))
    return pts


@functools.lru_cache(maxsize=None)
def _gauss_full_rank_cells():
    """Cells that must get a Gaussian: (scaling, K, centre, res), exact lambda_min >= 1e-6 lambda_max and >= 2 floors (the floor bounds
    the noise, so the computed lambda_min of such a cell is above one floor)."""
    g = np.random.default_rng(23)
    cells = []
    centres = [(0.0, 0.0, 0.0), (12.25, -7.75, 0.25)]
    ident = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for name, (s1, s2, L, umax) in SCALINGS.items():
        lo = -3.6 if L == 22 else -2.6                                       # (thinner clouds sink below the floor)
        for k in range(260):                                               # clouds of every orientation, spread and offset
            n = int(g.choice([4, 5, 6, 8, 13, 32, 64, 200]))
            smax = 10.0 ** g.uniform(lo, -1.0)
            sig = smax * np.array([1.0, 10.0 ** g.uniform(-2, 0), 10.0 ** g.uniform(-2, 0)])[g.permutation(3)]
            Q, _ = np.linalg.qr(g.normal(size=(3, 3)))
            off = g.uniform(-1, 1, 3) * max(0.0, umax - 0.05 - 3.0 * smax)
            u = np.clip(off + (g.normal(size=(n, 3)).clip(-3, 3) * sig) @ Q.T, -umax, umax)
            cells.append((name, _lattice(u, L), centres[k % 2] if umax == 0.5 else centres[0], 0.5 if k % 3 else 0.3))
        a = 1 << (L - 6)                                                   # 1/64 cell
        off = tuple(int(v) for v in np.rint(np.array([0.21, -0.33, 0.4]) * 2.0 ** L))
        for M in (ident, Q3):                                              # the spectra: isotropic, two equal, every order
            for d in [(a, a, a), (a, a, a // 100), (a // 100, a, a), (a, a // 100, a // 100), (a // 100, a // 100, a),
                      (a, a // 10, a // 100), (a, a // 100, a // 10), (a // 10, a, a // 100), (a // 10, a // 100, a),
                      (a // 100, a, a // 10), (a // 100, a // 10, a), (a, a // 40, a // 50)]:
                cells.append((name, _symmetric_set(d, M, off), centres[0], 0.5))
                cells.append((name, _symmetric_set(d, M, (0, 0, 0)), centres[0], 0.5))
    keep = []
    for name, K, centre, res in cells:
        s1, s2, L, umax = SCALINGS[name]
        m, cov = _exact_stats(K, L, res)
        C = np.array([[float(v) for v in r] for r in cov])
        ev = np.linalg.eigvalsh(C)
        if ev[0] >= 1e-6 * ev[2] and ev[0] >= 2.0 * _floor_m2(K, L, res, s1, s2) and max(abs(v) for k in K for v in k) <= umax * 2 ** L:
            keep.append(dict(scaling=name, K=K, centre=centre, res=res, m=m, cov=cov, C=C, ev=ev))
    return keep


def check_gauss_values(run, label):
    cells = _gauss_full_rank_cells()
    by = {name: sum(c["scaling"] == name for c in cells) for name in SCALINGS}
    assert all(v >= 150 for v in by.values()), by
    rows = []
    for k, c in enumerate(cells):
        s1s, s2s, L, _ = SCALINGS[c["scaling"]]
        s1, s2 = _moments(c["K"], L, s1s, s2s)                             # exact: the shifts are not below the lattice's
        assert s1s >= L and s2s >= 2 * L
        for ef in (1e300, 1000.0):
            rows.append(_gauss_row(len(c["K"]), s1, s2, 7 + k, c["centre"], c["res"], 3, ef, s1s, s2s))
    mean, cov, n, slot = _decode_cells(run("gauss", np.stack(rows)))
    worst_cov = {name: 0.0 for name in SCALINGS}
    worst_mean, worst_resc, n_resc, n_clamped = 0.0, 0.0, 0, 0
    spectra = set()
    for k, c in enumerate(cells):
        _, _, L, _ = SCALINGS[c["scaling"]]
        nk, res = len(c["K"]), c["res"]
        for j in (2 * k, 2 * k + 1):                                       # a Gaussian, with the cell's slot and count
            assert n[j] == nk and slot[j] == 7 + k, (k, n[j], slot[j])
        # covariance without the rescale.  Nine roundings on the path (two int64 -> fp64 conversions, the division by n, two
        # products and the difference of S - n m m, res * res, / (n - 1), the product with it), each at most 2^-53 of
        # n max|u|^2 res^2 / (n - 1) or of the entry: 4.5 units of 2^-52 ...; bound: the count doubled, 18 units.
        umax2 = (max(abs(v) for p in c["K"] for v in p) / 2.0 ** L) ** 2
        unit = EPS * res * res * nk / (nk - 1) * umax2
        err = max(abs(F(float(cov[2 * k][q])) - c["cov"][a][b]) for q, (a, b) in enumerate(PAIRS))
        worst_cov[c["scaling"]] = max(worst_cov[c["scaling"]], float(err) / unit)
        assert float(err) <= 18.0 * unit, (k, float(err) / unit)
        # mean: within 2 ulp of the exact centre + m res (the division, the product and the sum round once each)
        for a in range(3):
            ref = F(c["centre"][a]) + c["m"][a] * F(res)
            ulp = np.spacing(abs(float(ref)))
            for j in (2 * k, 2 * k + 1):
                e = float(abs(F(float(mean[j][a])) - ref)) / ulp
                worst_mean = max(worst_mean, e)
                assert e <= 2.0, (k, a, e)
        # rescale at eval_factor 1000 against V diag(max(ev, mx / 1000)) V^T of numpy's eigh of the exact matrix.  The clamp is a
        # 1-Lipschitz function of the eigenvalues (and mx / 1000 moves by 1e-3 of the matrix's error), so the covariance's own
        # error enters at most 1.001 times in the Frobenius norm, 3.003 times an entry's bound.  The Jacobi rotations: at most 6
        # sweeps of 3, and a rotation takes an entry of a and an entry of v through 14 roundings each; the product V ev V^T adds 8
        # per entry: 2 * 18 * 14 + 8 = 512 roundings of 2^-53 lambda_max, 256 units of 2^-52 lambda_max, doubled like the
        # covariance's count: 512 units.  (Loose: the measured maximum is 0.02 of the bound, which a worst case over 18 rotations
        # makes it; a skipped clamp or a wrong eigenvector is an error of lambda_max / 1000, 4e12 units.)
        ev, V = np.linalg.eigh(c["C"])
        mx = ev[2]
        if np.all(np.abs(ev - mx / 1000.0) > 1e-6 * mx / 1000.0):
            want = (V * np.maximum(ev, mx / 1000.0)) @ V.T
            got = np.array([[cov[2 * k + 1][PAIRS.index((min(a, b), max(a, b)))] for b in range(3)] for a in range(3)])
            e = float(np.max(np.abs(got - want)))
            bound = 3.01 * 18.0 * unit + 512.0 * EPS * mx
            worst_resc = max(worst_resc, e / bound)
            assert e <= bound, (k, e / (EPS * mx), bound / (EPS * mx))
            n_resc += 1
            n_clamped += int(ev[0] < mx / 1000.0)
            r = ev / mx
            spectra.add((round(float(r[0]), 5), round(float(r[1]), 5), int(np.argmax(np.diag(c["C"]))), int(np.argmin(np.diag(c["C"])))))
    print("gauss on %s, worst covariance error / unit (bound 18): %s;  mean %.3f ulp (bound 2);  rescaled covariance %.4f of its bound "
          "(%d cells, %d clamped)" % (label, "  ".join("%s %.3f" % kv for kv in worst_cov.items()), worst_mean, worst_resc, n_resc, n_clamped))
    assert n_resc >= 450 and n_clamped >= 150, (n_resc, n_clamped)
    # isotropic, two equal (above and below the third), and every order of three distinct eigenvalues along the axes
    assert any(s[0] == 1.0 for s in spectra) and any(s[0] < 1.0 and s[1] == 1.0 for s in spectra) and any(s[0] == s[1] < 1.0 for s in spectra)
    assert {(s[2], s[3]) for s in spectra if s[0] < s[1] < 1.0} >= {(a, b) for a in range(3) for b in range(3) if a != b}


def test_gauss_values_host(exe):
    check_gauss_values(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_gauss_values_gpu(exe):
    check_gauss_values(_runner(exe, "gpu"), "device")


@functools.lru_cache(maxsize=None)
def _gauss_deficient_cells():
    """Exactly rank-deficient cells: (K, L, s1_shift, s2_shift, runs or None).  On the 2^-22 lattice with exact moments, and off it
    (2^-40) with the moments rounded per run of one, a few, or all points."""
    g = np.random.default_rng(29)
    cells = []
    for k in range(1500):
        kind = k % 3                                                       # identical, collinear, coplanar
        exact = k % 4 == 0
        L = 22 if exact else 40
        n = int(g.choice([3, 4, 5, 8, 20, 64, 200]))
        spread = 10.0 ** g.uniform(-6, -1)
        off = g.uniform(-1, 1, 3) * (0.45 - min(spread, 0.4))
        T = 8
        step = max(1, int(spread * 2.0 ** L / T))
        d1 = [int(v) for v in np.rint(g.uniform(-1, 1, 3) * step)]
        d2 = [int(v) for v in np.rint(g.uniform(-1, 1, 3) * step)]
        u0 = [int(v) for v in np.rint(off * 2.0 ** L)]
        if kind == 0:
            K = [tuple(u0)] * n
        else:
            ab = g.integers(-T, T + 1, (n, 2))
            ab[0], ab[1] = (T, -T), (-T, T)
            K = [tuple(u0[c] + int(a) * d1[c] + (int(b) * d2[c] if kind == 2 else 0) for c in range(3)) for a, b in ab]
        assert max(abs(v) for p in K for v in p) <= 2 ** (L - 1)
        if exact:
            runs = None
        else:
            per = [1, int(g.integers(2, 6)), n][(k // 4) % 3]
            runs = [range(i, min(n, i + per)) for i in range(0, n, per)]
        s1s, s2s = (45, 45) if k % 5 else (38, 38)
        if exact and s2s < 2 * L:
            s1s, s2s = 45, 45
        cells.append((K, L, s1s, s2s, runs))
    return cells


def check_gauss_decisions(run, label):
    full = _gauss_full_rank_cells()
    c5 = next(c for c in full if len(c["K"]) == 5)
    c4 = next(c for c in full if len(c["K"]) == 4)
    rows, expect = [], []

    def add(c, n_pts, n_min, gets):
        s1s, s2s, L, _ = SCALINGS[c["scaling"]]
        K = c["K"][:n_pts]
        s1, s2 = _moments(K, L, s1s, s2s) if K else ([0] * 3, [0] * 6)
        rows.append(_gauss_row(len(K), s1, s2, 1234567 + len(rows), c["centre"], c["res"], n_min, 1000.0, s1s, s2s))
        expect.append((gets, len(K), 1234567 + len(rows) - 1))
    add(c5, 0, 3, False)                                                   # n = 0, 1, n_min - 1: the all-zero record
    add(c5, 1, 1, False)
    add(c5, 1, 3, False)
    add(c5, 2, 3, False)
    add(c5, 4, 5, False)
    add(c4, 3, 4, False)
    add(c5, 5, 5, True)                                                    # n = n_min
    add(c4, 4, 4, True)
    add(c4, 4, 2, True)
    add(c5, 2, 2, False)                                                   # n = 2, n_min = 2: two points are collinear
    n_head = len(rows)
    deficient = _gauss_deficient_cells()
    for K, L, s1s, s2s, runs in deficient:
        s1, s2 = _moments(K, L, s1s, s2s, runs)
        rows.append(_gauss_row(len(K), s1, s2, 99, (0.0, 0.0, 0.0), 0.5, 3, 1000.0, s1s, s2s))
    out = run("gauss", np.stack(rows))
    _, _, n, slot = _decode_cells(out)
    for k, (gets, n_pts, sl) in enumerate(expect):
        if gets:
            assert n[k] == n_pts and slot[k] == sl, (k, n[k], slot[k])
        else:
            assert not out[k].any(), (k, out[k])                           # all 80 bytes
    got = n[n_head:] != 0
    print("gauss on %s: %d of %d exactly rank-deficient cells got a Gaussian" % (label, int(got.sum()), len(deficient)))
    assert not got.any(), np.flatnonzero(got)[:20]
    assert not out[n_head:].any()


def test_gauss_decisions_host(exe):
    check_gauss_decisions(_runner(exe, "host"), "host")


@pytest.mark.gpu
def test_gauss_decisions_gpu(exe):
    check_gauss_decisions(_runner(exe, "gpu"), "device")


# ---- lanemap --------------------------------------------------------------------------------------------------------------------
def check_lanemap(run):
    m = run("lanemap", np.arange(64, dtype=np.uint64).reshape(-1, 1)).view(np.int64).reshape(-1)
    assert sorted(m[m >= 0]) == list(range(9)) and np.all(m[m < 0] == -1)
    return m


def test_lanemap_host(exe):
    check_lanemap(_runner(exe, "host"))


# ---- the wave primitives (device only) ------------------------------------------------------------------------------------------
def _lanes(n_rows):
    lane = np.arange(n_rows) % 64
    return lane, np.arange(n_rows) - lane                                  # lane of a row, first row of its wave


def check_scan(run):
    g = np.random.default_rng(31)
    v = g.integers(0, 2 ** 32, (40, 64), dtype=np.uint64)                  # sums that wrap
    v[0] = 1                                                               # all ones
    v[1] = 0
    v[2] = 0xFFFFFFFF
    v[3] = g.integers(0, 5, 64)
    v[4:12] = g.integers(0, 2 ** 27, (8, 64))                              # sums that do not
    got = run("scan", v.reshape(-1, 1)).reshape(-1, 64)
    assert np.array_equal(got, np.cumsum(v, axis=1) % np.uint64(2 ** 32))


def _payloads(g, n):
    x = g.integers(0, 2 ** 63, n, dtype=np.uint64) | (g.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    x[::7] = np.uint64(0x7FF0000000000000) | g.integers(1, 2 ** 52, len(x[::7]), dtype=np.uint64)    # NaN payloads, quiet and signalling
    x[1::7] = g.integers(1, 2 ** 52, len(x[1::7]), dtype=np.uint64)                                  # subnormals
    x[2::31] = np.uint64(0x8000000000000000)                                                         # -0.0
    return x


def check_xor(run):
    x = _payloads(np.random.default_rng(37), 64 * 32)
    got = run("xor", x.reshape(-1, 1))
    lane, base = _lanes(len(x))
    for j, o in enumerate((1, 2, 4, 8)):
        assert np.array_equal(got[:, j], x[base + (lane ^ o)]), o


def _spread_doubles(g, shape):
    """values whose sum depends on the order: exponents over 40 binades, both signs"""
    return np.ldexp(g.uniform(1.0, 2.0, shape), g.integers(-20, 21, shape)) * g.choice([-1.0, 1.0], shape)


def check_swapadd(run):
    g = np.random.default_rng(41)
    ab = _spread_doubles(g, (64 * 32, 2))
    got = run("swapadd", _words(ab))
    lane, base = _lanes(len(ab))
    for j, bit in enumerate((32, 16)):                                     # rows16 = false, true
        partner = base + (lane ^ bit)
        want = np.where((lane & bit) == 0, ab[:, 0] + ab[partner, 0], ab[:, 1] + ab[partner, 1])
        assert np.array_equal(got[:, j], _words(want)), bit


def check_moments(run):
    g = np.random.default_rng(43)
    v = _spread_doubles(g, (64 * 32, 9))
    got = run("moments", _words(v)).reshape(-1)
    lanemap = check_lanemap(run)
    lane, base = _lanes(len(v))
    tree = v.copy()
    for o in (32, 16, 8, 4, 2, 1):                                         # v += v[l ^ 32], 16, 8, 4, 2, 1
        tree = tree + tree[base + (lane ^ o)]
    assert len(np.unique(_words(tree[:64, 0]))) == 1                       # (every lane of the tree ends with the same bits)
    plain = v.reshape(-1, 64, 9).sum(axis=1)
    assert np.any(_words(plain) != _words(tree[::64]))                     # (and the order matters for these inputs)
    for m in range(9):
        rows = np.flatnonzero(lanemap[lane] == m)
        assert len(rows) == len(v) // 64
        assert np.array_equal(got[rows], _words(tree[rows, m])), m


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["gpu", "gpu256"])
def test_wave_primitives_gpu(exe, target):
    run = _runner(exe, target)
    check_scan(run)
    check_xor(run)
    check_swapadd(run)
    check_moments(run)
