"""csrc/ndt_evalgroup.h on the device against tests/evalgroup_model.py: which pairs the matcher sums, and how.

tests/native/evalgroup_checks.hip includes the header alone; one program per n_neighbours holds every instance of eval_group the
library dispatches (forms: 0 persistent / stream <NN, H, QL, false, false>, 1 the same with the planar pair term, 2 eval_derivs
<.., false, true>, 3 eval_chunks <.., true, true>; with and without the Hessian; QL = 64 and the library's 1024 / 640 / 2048 /
2048).  The gradient-only form is compiled and run for every one of them, not only for the batch-boundary cases.  A case is one
wave, at most 64 source cells, a grid of at most 2 640 slots.  Every pose here is the identity rotation and a translation unless
the test is about the tile, so the transformed mean is mean + t with one rounding on the device and in NumPy alike, and the
model's cells are the device's.

  index     lazygrid_index_h == the NumPy expression, lazygrid_index_p2 == lazygrid_index_h for res = 2^-10 .. 2^6,
            pow2_reciprocal == 1 / res for powers of two with exponent in (-1000, 1000) and 0 otherwise; all exact.
  scan      wave_incl_scan_u32 == cumsum, exact.
  totals    wave_sum_all<8> / <32> within 6 u sum |v| of the exact sum (fractions), u = 2^-53: a value passes six additions, one
            per lane bit, and the usual (1 + u)^6 - 1 <= 6 u / (1 - 6 u) bound applies to sum |v|.  Same bits in every lane that
            holds a value.
  list      count, w.terms, mycell and the list words equal the model's, for all 16 instances of an n at the library's QL (the
            segment form writes no list: its row's count) on the families of the issue: the seven probe lattices cut to groups,
            full / empty / single-slot maps, windows at every reachable bit offset, sources on, outside, n and n + 1 cells
            outside every face, thin maps flat and general, one lane that turns a flat wave general, 1 / 63 / 64 valid lanes,
            strides 5..8 with a base, res 0.5 and 0.3.
  tile      the nine columns against T mean and R C R^T in exact rational arithmetic of the doubles.  Bound k u / (1 - k u)
            times the sum of the magnitudes of the exact terms of the entry.  apply(): r0 x + r1 y + r2 z + t, the longest chain
            is a product and three additions: k = 4 (a fused multiply-add only removes roundings).  rotate_cov(): a = R C is a
            product and two additions (3), o = a R^T multiplies that by R (4) and adds twice (6): k = 6, over the nine terms
            R_ij C_jk R_lk.
  passes    QL = 64 instances at hit totals 0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193 and 500 (n = 0 has one hit per
            lane at the most: 0, 1, 63, 64): w.terms, the last pass in the list, HitCache::key 0 exactly when the total exceeded
            QL, wave totals with the bits of the library-QL instance.
  sums      every wave total against the mpmath sum of the device's own pair terms (mode terms / terms_g) over the model's
            list, bound n 2^-52 sum |term entry|; both forms of the Hessian switch, the planar form against the kept entries.
  reuse     scripts of two or three calls, the marker list tells reuse (w.terms == 1) from PROBE (the model's count).
  segments  seg_lanes 8, 16, 32, 64, QL 64 and 2048: row[28] the model's count of the segment, its sums the bits of the
            eval_derivs instance on the segment's cells alone; rows of segments without cells stay zero.

Measured on an MI355X (worst error in units of the bound, and the cases per run of the group mode; n = 0 / 1 / 2 / 3):
  totals    0.292 of 6 u sum |v| (14 waves of 32 values)
  tile      mean 0.395 (k = 4), covariance 0.391 (k = 6); 6 poses x 2 instances x 64 cells
  sums      0.0094 / 0.0118 / 0.0119 / 0.0105 of n 2^-52 sum |term entry|; 4 / 12 totals x 12 instances
  list      53 / 55 / 55 / 55 families x 8 instances, lists of up to 49 / 834 / 3 264 / 6 659 pairs
  reuse     124 / 132 / 132 / 132 scripts (12 that must reuse, 104 / 112 that must probe, 8 that compare the bits)
  segments  96 / 240 / 240 / 240 cases and 148 / 370 / 370 / 370 segments run alone
By hand, each reverted afterwards: without `!ndt_ballot(moved)` in the reuse condition test_reuse fails ("lane 0 crosses axis 0":
w.terms 1 instead of 266); with nc.key = cache_key always test_passes fails (total 65, QL 64: key 5 instead of 0); with
min(e + lane + 1u, n - 1u) in term_list's fetch test_sums fails (error 0.58 against a bound of 4e-13).
"""
import fractions
import os
import subprocess

import mpmath
import numpy as np
import pytest

import evalgroup_model as E
import pairterm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "evalgroup_checks.hip")
WIDTH_IN = {"index": 4, "scan": 1, "totals": 32, "terms": 20, "terms_g": 20}
TILE, CELL, CACHE, TERMS, TOT, ROWS, LIST, OUTW = 0, 576, 768, 772, 773, 801, 1057, 1057 + 2048
LIB_QL = {0: 1024, 1: 640, 2: 2048, 3: 2048}
KEPT_PLANAR = [0, 1, 2, 6, 7, 8, 12, 13, 17, 27]
U = 2.0 ** -53
PASS_TOTALS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 500]
NNS = [0, 1, 2, 3]


def inst(form, with_h, lib):
    return form * 4 + (2 if with_h else 0) + (1 if lib else 0)


def ql_of(instance):
    return LIB_QL[instance >> 2] if instance & 1 else 64


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    d = tmp_path_factory.mktemp("evalgroup")
    exes = [str(d / ("evalgroup_checks_%d" % nn)) for nn in NNS]
    jobs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-DEG_NN=%d" % nn, SRC, "-o", exe])
            for nn, exe in zip(NNS, exes)]
    codes = [j.wait() for j in jobs]
    assert codes == [0] * len(NNS), codes
    return exes


def _run(exe, mode, blob, n):
    out = subprocess.run(["timeout", "-k", "10", "60", exe, mode], input=np.uint32(n).tobytes() + blob.tobytes(), capture_output=True)
    if out.returncode in (-6, -11, 124, 134, 137, 139):         # a fault or a hang: nothing more is started on the device
        pytest.exit("evalgroup_checks %s ended with %d: %s" % (mode, out.returncode, out.stderr.decode(errors="replace")), 1)
    assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace"))
    return np.frombuffer(out.stdout, dtype=np.float64)


@pytest.fixture(scope="module")
def run(progs):
    def run(mode, table, nn=2):
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, WIDTH_IN[mode])
        return _run(progs[nn], mode, table, table.shape[0]).reshape(table.shape[0], -1)
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- cases of the group mode ------------------------------------------------------------------------------------------------
class Target:
    """a grid and the Gaussians of its occupied cells, in rank order"""

    def __init__(self, size_cells, centre, res, slots, rng):
        self.grid = E.Grid(size_cells, centre, res, slots)
        sx, sy, sz = self.grid.size
        ctr = np.array([self.grid.cell_centre(s // (sy * sz), s // sz % sy, s % sz) for s in self.grid.slots]).reshape(-1, 3)
        self.mean = ctr + rng.uniform(-0.2, 0.2, ctr.shape) * res
        self.cov = _covs(rng, len(ctr))


def _covs(rng, n):
    A = rng.normal(size=(n, 3, 3)) * 0.1
    return A @ A.transpose(0, 2, 1) + 0.01 * np.eye(3)


def _random_slots(rng, size_cells, fill):
    n = int(np.prod(size_cells))
    return np.nonzero(rng.random(n) < fill)[0]


def _at(grid, cells, rng, jitter=0.2):
    """means inside the given cells (indices may lie outside the grid)"""
    cells = np.asarray(cells).reshape(-1, 3)
    ctr = np.array([grid.cell_centre(*c) for c in cells])
    return ctr + rng.uniform(-jitter, jitter, ctr.shape) * grid.res


class Call:
    def __init__(self, instance, t=(0.0, 0.0, 0.0), key=0, base=0, stride=1, end=None, marker=-1, R=None, lfd1=1.0, lfd2=0.05):
        self.instance, self.t, self.key, self.base, self.stride, self.end, self.marker = instance, tuple(t), key, base, stride, end, marker
        self.R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
        self.lfd1, self.lfd2 = lfd1, lfd2


class Case:
    def __init__(self, target, smean, scov, calls, seg_lanes=64, tag=""):
        self.target, self.smean, self.scov, self.calls, self.seg_lanes, self.tag = target, np.asarray(smean), np.asarray(scov), calls, seg_lanes, tag
        for c in calls:
            if c.end is None:
                c.end = len(self.smean)

    def encode(self):
        g = self.target.grid
        out = [list(g.size) + list(g.centre) + [g.res, len(g.slots), len(self.smean), len(self.calls), self.seg_lanes]]
        for k, s in enumerate(g.slots):
            out.append([s] + list(self.target.mean[k]) + E.six(self.target.cov[k]))
        for m, C in zip(self.smean, self.scov):
            out.append(list(m) + E.six(C))
        for c in self.calls:
            out.append(list(c.R.reshape(9)) + list(c.t) + [c.key, c.base, c.stride, c.end, c.lfd1, c.lfd2, c.instance, c.marker])
        return np.concatenate([np.asarray(r, dtype=np.float64) for r in out])

    # the model's view of a call
    def lane_cells(self, call):
        return E.lanes_of(call.base, call.stride, call.end)

    def lane_means(self, call):
        """transformed means (identity rotation: mean + t, one rounding)"""
        assert np.array_equal(call.R, np.eye(3))
        return [None if i is None else self.smean[i] + np.array(call.t) for i in self.lane_cells(call)]

    def model_list(self, call, nn, lanes=(0, 64)):
        """E.pair_list of the call's lanes (of lanes[0] <= lane < lanes[1] only), the neighbours of a mean looked up once per grid"""
        g = self.target.grid
        memo = g.__dict__.setdefault("_memo", {})
        out = []
        for lane, m in enumerate(self.lane_means(call)):
            if m is None or not lanes[0] <= lane < lanes[1]:
                continue
            key = (m.tobytes(), nn)
            if key not in memo:
                memo[key] = g.neighbours(g.indices([m])[0], nn)
            out.extend((lane << 24) | k for k in memo[key])
        return out


class Row:
    def __init__(self, row):
        self.tile = row[TILE:CELL].reshape(9, 64)
        self.cell = row[CELL:CACHE].reshape(3, 64)
        self.key, self.base, self.count = (int(v) for v in row[CACHE:CACHE + 3])
        self.terms = int(row[TERMS])
        self.tot = row[TOT:ROWS]
        self.rows = row[ROWS:LIST].reshape(8, 32)
        self._list = row[LIST:]

    def list(self, ql):
        words = self._list[:min(self.count, ql)]
        assert not np.any(np.isnan(words))
        return [int(v) for v in words]

    def holds(self, want, ql):
        """the list starts with the last pass of `want` (behind a short last pass stands what the pass before left there)"""
        last = E.last_pass(want, ql)
        return self.list(ql)[:len(last)] == last and (self.count <= ql) == (len(want) <= ql)


def run_group(progs, nn, cases):
    """one run of the program of `nn`: per case the rows of its calls"""
    blob = np.concatenate([[float(len(cases))]] + [c.encode() for c in cases])
    out = _run(progs[nn], "group", blob, len(blob)).reshape(-1, OUTW)
    rows, k = [], 0
    for c in cases:
        rows.append([Row(out[k + j]) for j in range(len(c.calls))])
        k += len(c.calls)
    assert k == len(out)
    return rows


def check_cells(case, call, row):
    means = case.lane_means(call)
    for lane, m in enumerate(means):
        if m is None:
            continue
        want = case.target.grid.indices([m])[0]
        assert tuple(int(v) for v in row.cell[:, lane]) == tuple(want), (case.tag, lane)
        assert np.array_equal(_bits(row.tile[0:3, lane]), _bits(m)), (case.tag, lane)


# ---- index ------------------------------------------------------------------------------------------------------------------
def _index_points(res, centre, size):
    half = size / 2.0
    k = np.arange(-size // 2 - 3, size // 2 + 4)
    faces = (k + 0.5) * res + centre
    pts = [faces, np.nextafter(faces, np.inf), np.nextafter(faces, -np.inf), [0.0, -0.0, centre, np.nan, np.inf, -np.inf]]
    edge = np.array([2.0e9, -2.0e9]) - half                                 # floor(..) + half straddles +-2e9
    for e in edge:
        q = (e + np.array([-2.0, -1.0, 0.0, 1.0, 2.0])) * res + centre
        pts += [q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf)]
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in pts]), half


def test_index(run):
    table = []
    for res in [2.0 ** e for e in range(-10, 7)] + [0.3, 0.2, 0.375]:
        for centre in (0.0, 3.25, -1.0e6 / 3.0, 7.0e8):
            for size in (1, 7, 12, 70):
                pts, half = _index_points(res, centre, size)
                table += [[p, centre, res, half] for p in pts]
    table = np.array(table)
    got = run("index", table)
    want = np.array([E.cell_index(p, c, r, 2.0 * h) for p, c, r, h in table])
    assert (want == -1).sum() > 100 and (want > 1.9e9).sum() > 10 and (want < -1.9e9).sum() > 10
    assert np.array_equal(got[:, 0], want.astype(np.float64)), np.nonzero(got[:, 0] != want)[0][:5]
    m, e = np.frexp(table[:, 2])
    pow2 = m == 0.5
    assert pow2.sum() > 1000 and (~pow2).sum() > 100
    assert np.array_equal(got[pow2, 1], got[pow2, 0]), np.nonzero(got[pow2, 1] != got[pow2, 0])[0][:5]
    assert np.array_equal(_bits(got[pow2, 2]), _bits(1.0 / table[pow2, 2])) and np.all(_bits(got[~pow2, 2]) == 0)


def test_pow2_reciprocal(run):
    # frexp(2^k) = (0.5, k + 1): the exponent is inside (-1000, 1000) for k = -1000 .. 998; the two limits are 2^-1001 and 2^999
    ok = [2.0 ** k for k in range(-1000, 999, 37)] + [2.0 ** 998, 1.0, 0.5, 2.0]
    zero = [0.3, 0.2, 3 * 2.0 ** -3, -0.5, -2.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 2.0 ** -1001, 2.0 ** 999, 2.0 ** -1022, 2.0 ** -1074,
            2.0 ** 1023, 1.0 + 2.0 ** -52, 1.5, np.nextafter(0.5, 0.0)]
    for r in ok:
        assert np.frexp(r)[0] == 0.5 and -1000 < np.frexp(r)[1] < 1000
    assert np.frexp(2.0 ** -1001)[1] == -1000 and np.frexp(2.0 ** 999)[1] == 1000
    got = run("index", np.array([[0.0, 0.0, r, 1.0] for r in ok + zero]))[:, 2]
    assert np.array_equal(_bits(got[:len(ok)]), _bits(1.0 / np.array(ok)))
    assert np.all(_bits(got[len(ok):]) == 0), [zero[k] for k in np.nonzero(_bits(got[len(ok):]))[0]]


# ---- scan / totals ----------------------------------------------------------------------------------------------------------
def test_scan(run):
    rng = np.random.default_rng(11)
    waves = [np.zeros(64), np.ones(64)]
    for lane in range(64):
        w = np.zeros(64)
        w[lane] = 1 + lane
        waves.append(w)
    waves += [rng.integers(0, 344, 64).astype(np.float64) for _ in range(40)]
    waves += [rng.integers(900, 1200, 64).astype(np.float64) for _ in range(8)]          # totals that cross 2^16
    waves += [np.full(64, 343.0), np.full(64, 2.0 ** 24)]
    v = np.concatenate(waves)
    got = run("scan", v)[:, 0].reshape(-1, 64)
    want = np.cumsum(np.array(waves), axis=1)
    assert want[-3].max() > 2 ** 16 and want[:-10].max() < 2 ** 16
    assert np.array_equal(got, want)


def test_totals(run):
    rng = np.random.default_rng(12)
    waves = [rng.normal(size=(64, 32)) * 10.0 ** rng.integers(-8, 8, (64, 32)) for _ in range(12)]
    waves.append(np.ones((64, 32)))
    waves.append(-np.abs(rng.normal(size=(64, 32))))                                   # like the scores: one sign
    got = run("totals", np.concatenate(waves)).reshape(len(waves), 64, 2)
    worst = 0.0
    for w, g in zip(waves, got):
        exact = [sum(fractions.Fraction(float(v)) for v in w[:, k]) for k in range(32)]
        mag = [sum(fractions.Fraction(abs(float(v))) for v in w[:, k]) for k in range(32)]
        bound = fractions.Fraction(6 * U) / (1 - fractions.Fraction(6 * U))
        for lane in range(64):
            for col, k in ((0, lane >> 3), (1, lane >> 1)):      # wave_totals: lane l holds value l >> SH
                err = abs(fractions.Fraction(float(g[lane, col])) - exact[k])
                assert err <= bound * mag[k], (lane, col, float(err / (bound * mag[k])))
                worst = max(worst, float(err / (bound * mag[k])))
        for k in range(8):
            assert len(set(_bits(g[8 * k:8 * k + 8, 0]))) == 1
        for k in range(32):
            assert len(set(_bits(g[2 * k:2 * k + 2, 1]))) == 1
    print("totals: worst error %.3f of the bound 6 u sum |v|" % worst)


# ---- pair list, exact -------------------------------------------------------------------------------------------------------
def _families(nn):
    """(tag, target, smean, base, stride, end, t) of every family of the list test"""
    rng = np.random.default_rng(100 + nn)
    fam = []

    def add(tag, target, smean, base=0, stride=1, end=None, t=(0.0, 0.0, 0.0)):
        fam.append((tag, target, np.asarray(smean), base, stride, len(smean) if end is None else end, t))

    def everywhere(g, n, margin):
        lo = np.array([-margin] * 3)
        hi = np.array(g.size) + margin
        return _at(g, rng.integers(lo, hi, (n, 3)), rng)

    # the seven lattices of test_probe_rank_bitmap_windows, two groups of their sources each
    for size_cells, nn_l in E.PROBE_LATTICES:
        grid, mean, cov, smean, _ = E.probe_lattice(size_cells, nn_l, 128)
        tg = Target.__new__(Target)
        tg.grid, tg.mean, tg.cov = grid, mean, cov
        add("lattice %s/%d a" % (size_cells, nn_l), tg, smean[:64])
        add("lattice %s/%d b" % (size_cells, nn_l), tg, smean[64:])
    size = (6, 5, 4)
    n_slots = int(np.prod(size))
    # full and empty maps
    add("full", Target(size, (0, 0, 0), 0.5, range(n_slots), rng), everywhere(E.Grid(size, (0, 0, 0), 0.5, []), 64, nn + 1))
    add("empty", Target(size, (0, 0, 0), 0.5, [], rng), everywhere(E.Grid(size, (0, 0, 0), 0.5, []), 64, nn + 1))
    # one occupied slot: the corners, slots 31, 32, 63 and the last
    g0 = E.Grid(size, (0, 0, 0), 0.5, [])
    corners = [g0.slot(x, y, z) for x in (0, 5) for y in (0, 4) for z in (0, 3)]
    for s in sorted(set(corners + [31, 32, 63, n_slots - 1])):
        c = np.array([s // 20, s // 4 % 5, s % 4])
        near = c + rng.integers(-nn - 1, nn + 2, (48, 3))
        add("single slot %d" % s, Target(size, (0, 0, 0), 0.5, [s], rng), np.concatenate([_at(g0, near, rng), everywhere(g0, 16, nn + 1)]))
    # windows at every reachable bit offset, at their greatest lengths: flat maps (sz <= nn + 1, one window per x covers
    # (2 nn + 1) sz slots) and general ones, sources on runs of consecutive columns / slots
    for sz in sorted({max(1, nn), nn + 1}):
        sizef = (8, 9, sz)
        tg = Target(sizef, (0, 0, 0), 0.5, _random_slots(rng, sizef, 0.7), rng)
        for c0 in (0, 8):
            cols = np.arange(c0, c0 + 64)
            cells = np.stack([cols // 9, cols % 9, rng.integers(0, sz, 64)], axis=1)
            add("offsets flat sz %d from %d" % (sz, c0), tg, _at(tg.grid, cells, rng))
    sizeg = (6, 7, 5)
    tg = Target(sizeg, (0, 0, 0), 0.5, _random_slots(rng, sizeg, 0.7), rng)
    for s0 in (0, 64, 146):
        s = np.arange(s0, s0 + 64)
        add("offsets general from %d" % s0, tg, _at(tg.grid, np.stack([s // 35, s // 5 % 7, s % 5], axis=1), rng))
    for res, centre in ((0.5, (0.0, 0.0, 0.0)), (0.3, (3.25, -8.0, 1.5))):
        # on every face, just outside, n cells outside, n + 1 cells outside
        tg = Target(size, centre, res, _random_slots(rng, size, 0.6), rng)
        cells = []
        for axis in range(3):
            for pos in (0, -1, -nn, -nn - 1, size[axis] - 1, size[axis], size[axis] - 1 + nn, size[axis] + nn):
                c = [int(rng.integers(0, size[a])) for a in range(3)]
                c[axis] = pos
                cells.append(c)
        cells += [[-1, -1, -1], [6, 5, 4], [-nn, 4 + nn, 0], [5 + nn, -nn, 3 + nn]]
        for k in (0, 1):
            add("faces res %g %d" % (res, k), tg, _at(tg.grid, (cells + cells)[16 * k:16 * k + 28] + cells[:8], rng))
        # thin maps: flat (sz = nn + 1) and general (sz = nn + 2)
        for sz in (nn + 1, nn + 2):
            sizet = (9, 8, sz)
            tgt = Target(sizet, centre, res, _random_slots(rng, sizet, 0.5), rng)
            cells = np.stack([rng.integers(-1, 10, 64), rng.integers(-1, 9, 64), rng.integers(0, sz, 64)], axis=1)
            add("thin sz %d res %g" % (sz, res), tgt, _at(tgt.grid, cells, rng))
            if sz == nn + 1:
                # one lane two cells above the plane turns the whole wave to the general form
                for lane, end in ((0, 64), (63, 64), (39, 40)):
                    c2 = cells.copy()
                    c2[lane, 2] = sz + 1
                    c2[lane, 0:2] = (4, 4)
                    add("thin sz %d res %g lane %d above" % (sz, res, lane), tgt, _at(tgt.grid, c2, rng), end=end)
    # 1, 63 and 64 valid lanes
    tg = Target(size, (0, 0, 0), 0.5, _random_slots(rng, size, 0.6), rng)
    sm = everywhere(tg.grid, 64, 1)
    for end in (1, 63, 64):
        add("end %d" % end, tg, sm, end=end)
    # strides 5..8 with a base
    sm = everywhere(tg.grid, 64 * 8 + 8, 1)
    for stride in (5, 6, 7, 8):
        add("stride %d" % stride, tg, sm, base=stride - 2, stride=stride, end=len(sm) - (stride == 6) * 200)
    return fam


@pytest.mark.parametrize("nn", NNS)
def test_pair_list(progs, nn):
    fam = _families(nn)
    rng = np.random.default_rng(7)
    instances = [inst(form, h, True) for form in range(4) for h in (False, True)]
    cases, model = [], []
    for tag, target, smean, base, stride, end, t in fam:
        scov = _covs(rng, len(smean))
        for i in instances:
            cases.append(Case(target, smean, scov, [Call(i, t=t, base=base, stride=stride, end=end)], tag=(tag, i)))
        model.append(cases[-1].model_list(cases[-1].calls[0], nn))
        assert model[-1] == E.pair_list(target.grid, cases[-1].lane_means(cases[-1].calls[0]), nn)
    rows = run_group(progs, nn, cases)
    assert max(len(m) for m in model) > (64 if nn else 32) and min(len(m) for m in model) == 0
    for k, (case, row) in enumerate(zip(cases, rows)):
        want, call, row = model[k // len(instances)], case.calls[0], row[0]
        check_cells(case, call, row)
        if call.instance >> 2 == 3:                         # the segment form: one segment of 64 lanes, its count in the row
            assert row.terms == 0 and row.count == 0 and int(row.rows[0, 28]) == len(want), case.tag
            continue
        assert (row.count, row.terms, row.key, row.base) == (len(want), len(want), 0, call.base), case.tag
        assert row.holds(want, ql_of(call.instance)), case.tag
    print("list: %d families x %d instances, %d .. %d pairs" % (len(fam), len(instances), min(map(len, model)), max(map(len, model))))


# ---- tile -------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def test_tile(progs):
    rng = np.random.default_rng(21)
    size = (6, 5, 4)
    tg = Target(size, (0, 0, 0), 0.5, _random_slots(rng, size, 0.5), rng)
    smean = rng.uniform(-30.0, 30.0, (64, 3))
    scov = _covs(rng, 64)
    poses = [(np.eye(3), (0.0, 0.0, 0.0)), (np.eye(3), (0.25, -1.5, 1e3 / 3)), (_rot(0.0, 0.0, 0.7), (1.0, 2.0, 0.0)),
             (_rot(0.3, -1.1, 2.9), (-5.0, 0.1, 3.0)), (_rot(-3.0, 1.5, 1e-9), (1e-3, 1e3, -7.0)), (_rot(1e-8, -1e-8, 1e-8), (0.0, 0.0, 0.0))]
    cases = [Case(tg, smean, scov, [Call(inst(f, True, True), t=t, R=R)]) for R, t in poses for f in (0, 2)]
    rows = run_group(progs, 1, cases)
    F = fractions.Fraction
    worst = [0.0, 0.0]
    for case, row in zip(cases, rows):
        R, t = case.calls[0].R, case.calls[0].t
        Rf = [[F(float(v)) for v in r] for r in R]
        for lane in range(64):
            m = [F(float(v)) for v in smean[lane]]
            C = [[F(float(v)) for v in r] for r in scov[lane]]
            for i in range(3):
                terms = [Rf[i][j] * m[j] for j in range(3)] + [F(float(t[i]))]
                err = abs(F(float(row[0].tile[i, lane])) - sum(terms))
                bound = F(4 * U) / (1 - F(4 * U)) * sum(abs(v) for v in terms)
                assert err <= bound, (lane, i)
                worst[0] = max(worst[0], float(err / bound) if bound else 0.0)
            for col, (i, l) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                terms = [Rf[i][j] * C[j][k] * Rf[l][k] for j in range(3) for k in range(3)]
                err = abs(F(float(row[0].tile[3 + col, lane])) - sum(terms))
                bound = F(6 * U) / (1 - F(6 * U)) * sum(abs(v) for v in terms)
                assert err <= bound, (lane, col)
                worst[1] = max(worst[1], float(err / bound) if bound else 0.0)
    assert worst[1] > 0.0                                   # (a general rotation rounds)
    print("tile: worst error of the mean %.3f of its bound (k = 4), of the covariance %.3f (k = 6)" % tuple(worst))


# ---- passes and sums --------------------------------------------------------------------------------------------------------
def _with_total(nn, total, rng):
    """a map and 64 sources whose list has exactly `total` entries.  Lane 0 sits alone at the low x face, the others at least
    2 nn + 1 cells of x away in distinct cells: slots are occupied at random while the total allows it, and the slots that only
    lane 0 sees, one hit each, make up the rest."""
    size = (10, 9, 8)
    g0 = E.Grid(size, (0, 0, 0), 0.5, [])
    x0 = 2 * nn + 1
    flat = rng.choice((size[0] - x0) * 72, 63, replace=False)
    cells = np.concatenate([[[0, 4, 4]], np.stack([x0 + flat // 72, flat // 8 % 9, flat % 8], axis=1)])
    smean = _at(g0, cells, rng)
    hits = {}
    for c in cells:
        for x in range(max(c[0] - nn, 0), min(c[0] + nn, size[0] - 1) + 1):
            for y in range(max(c[1] - nn, 0), min(c[1] + nn, size[1] - 1) + 1):
                for z in range(max(c[2] - nn, 0), min(c[2] + nn, size[2] - 1) + 1):
                    hits[g0.slot(x, y, z)] = hits.get(g0.slot(x, y, z), 0) + 1
    own = [s for s in sorted(hits) if s // 72 <= nn]                # lane 0's
    assert all(hits[s] == 1 for s in own)
    order = [s for s in sorted(hits) if s // 72 > nn]
    rng.shuffle(order)
    slots, have = [], 0
    for s in order + own:
        if have + hits[s] <= total:
            slots.append(s)
            have += hits[s]
    assert have == total, (nn, total, have)
    return Target(size, (0, 0, 0), 0.5, slots, rng), smean


def _pass_totals(nn):
    return [t for t in PASS_TOTALS if t <= 64] if nn == 0 else PASS_TOTALS


_PASSES = {}


def _passes(progs, nn):
    """every QL = 64 instance of forms 0..2 and its library-QL twin on lists of the PASS_TOTALS lengths, key 5; one run per nn"""
    if nn not in _PASSES:
        rng = np.random.default_rng(300 + nn)
        cases = []
        for total in _pass_totals(nn):
            target, smean = _with_total(nn, total, rng)
            scov = _covs(rng, 64)
            for form in range(3):
                for h in (False, True):
                    for lib in (False, True):
                        cases.append(Case(target, smean, scov, [Call(inst(form, h, lib), key=5)], tag=(total, form, h, lib)))
        _PASSES[nn] = (cases, run_group(progs, nn, cases))
    return _PASSES[nn]


@pytest.mark.parametrize("nn", NNS)
def test_passes(progs, nn):
    cases, rows = _passes(progs, nn)
    seen = set()
    for k, (case, row) in enumerate(zip(cases, rows)):
        total, form, h, lib = case.tag
        call, row = case.calls[0], row[0]
        want = case.model_list(call, nn)
        ql = ql_of(call.instance)
        assert len(want) == total
        check_cells(case, call, row)
        assert (row.terms, row.count) == (total, total), case.tag
        assert row.key == (0 if total > ql else 5), case.tag
        assert row.holds(want, ql), case.tag
        if not lib:
            twin = rows[k + 1][0]
            assert cases[k + 1].tag == (total, form, h, True)
            n = 28 if h else 7
            assert np.array_equal(_bits(row.tot[:n]), _bits(twin.tot[:n])), case.tag
            seen.add(total > 64)
    assert seen == ({False} if nn == 0 else {False, True})


@pytest.mark.parametrize("nn", NNS)
def test_sums(progs, run, nn):
    cases, rows = _passes(progs, nn)
    # the device's own value of every list entry's term, one table per Hessian switch
    table, where = [], {}
    for k, case in enumerate(cases):
        total, form, h, lib = case.tag
        if total in where:
            continue
        call = case.calls[0]
        means = case.lane_means(call)
        cells = case.lane_cells(call)
        where[total] = (len(table), total)
        for e in case.model_list(call, nn):
            lane, rank = e >> 24, e & 0xFFFFFF
            table.append(list(means[lane]) + E.six(case.scov[cells[lane]]) + list(case.target.mean[rank]) + E.six(case.target.cov[rank])
                         + [call.lfd1, call.lfd2])
    table = np.array(table)
    term = {True: run("terms", table, nn), False: run("terms_g", table, nn)}
    assert np.all(_bits(term[False][:, 7:]) == 0) and np.all(term[True][:, 0] < 0.0)
    worst = 0.0
    with M.workprec():
        for case, row in zip(cases, rows):
            total, form, h, lib = case.tag
            lo, n = where[total]
            t = term[h][lo:lo + n]
            for a in range(28 if h else 7):
                got = M.MP.num(row[0].tot[a])
                if form == 1 and a not in KEPT_PLANAR:      # the planar pair term leaves these sums alone
                    assert _bits(row[0].tot[a]) == 0, (case.tag, a)
                    continue
                want = mpmath.fsum(M.MP.num(v) for v in t[:, a])
                mag = mpmath.fsum(abs(M.MP.num(v)) for v in t[:, a])
                bound = n * 2.0 ** -52 * mag
                err = abs(got - want)
                assert err <= bound, (case.tag, a, float(err), float(bound))
                if n:
                    assert mag > 0
                    worst = max(worst, float(err / bound))
    print("sums nn %d: worst error %.4f of the bound n 2^-52 sum |term|" % (nn, worst))


# ---- reuse ------------------------------------------------------------------------------------------------------------------
def _reuse_cases(nn, rng):
    """scripts and what they must do: per case [(call index, 'reuse' | 'probe')]"""
    size = (10, 9, 8)
    # about eight hits per lane, so that no list outgrows the library's QL (a list that did would not be remembered)
    tg = Target(size, (0, 0, 0), 0.5, _random_slots(rng, size, min(0.6, 8.0 / (2 * nn + 1) ** 3)), rng)
    g = tg.grid
    res = g.res
    n_occ = len(g.slots)
    marker = (5 << 24) | (n_occ // 2)
    out = []
    small = (0.05 * res, -0.04 * res, 0.03 * res)
    for form in (0, 2):
        for h in (False, True):
            I = inst(form, h, True)
            I64 = inst(form, h, False)
            for valid in (64, 40):
                cells = np.stack([rng.integers(0, size[0], 65), rng.integers(0, size[1], 65), rng.integers(0, size[2], 65)], axis=1)
                smean = _at(g, cells, rng, 0.2)
                scov = _covs(rng, 65)
                last = valid - 1

                def case(calls, expect, tag, smean=smean):
                    out.append((Case(tg, smean, scov, calls, tag=(tag, form, h, valid)), expect))

                # every mean keeps its cell: the list is used again (lanes past `end` hold the fill value of mycell and never count)
                case([Call(I, key=7, end=valid), Call(I, key=7, end=valid, t=small, marker=marker)], [(1, "reuse")], "stay, marker")
                case([Call(I, key=7, end=valid), Call(I, key=7, end=valid, t=small), Call(I, key=0, end=valid, t=small)],
                     [(1, "same as 2")], "stay, fresh bits")
                # exactly one lane crosses a face, in one axis
                for lane in (0, 63, last) if valid == 64 else (0, last):
                    for axis in range(3):
                        sm = smean.copy()
                        sm[lane] = np.array(g.cell_centre(*cells[lane]))
                        sm[lane, axis] += 0.49 * res                        # 0.01 cells below the upper face
                        t = [0.0, 0.0, 0.0]
                        t[axis] = 0.02 * res
                        case([Call(I, key=7, end=valid), Call(I, key=7, end=valid, t=t, marker=marker)], [(1, "probe")],
                             "lane %d crosses axis %d" % (lane, axis), sm)
                        if lane == last and axis == 0:
                            # away and back: the cells of call 2 are what call 3 is compared with
                            case([Call(I, key=7, end=valid), Call(I, key=7, end=valid, t=t), Call(I, key=7, end=valid, marker=marker)],
                                 [(2, "probe")], "away and back", sm)
                            # a lane past `end` that would have crossed does not count
                            if valid == 40:
                                sm2 = smean.copy()
                                sm2[valid] = np.array(g.cell_centre(*cells[valid]))
                                sm2[valid, 0] += 0.49 * res
                                case([Call(I, key=7, end=valid), Call(I, key=7, end=valid, t=t, marker=marker)], [(1, "reuse")],
                                     "invalid lane crosses", sm2)
                case([Call(I, key=7, end=valid), Call(I, key=8, end=valid, t=small, marker=marker)], [(1, "probe")], "other key")
                case([Call(I, key=7, end=valid), Call(I, key=0, end=valid, t=small, marker=marker)], [(1, "probe")], "key 0")
                case([Call(I, key=0, end=valid), Call(I, key=7, end=valid, t=small, marker=marker)], [(1, "probe")], "first key 0")
                case([Call(I, key=7, end=valid), Call(I, key=7, base=1, end=valid + 1, t=small, marker=marker)], [(1, "probe")], "other base")
                if nn >= 1:
                    # the list of call 1 overflowed QL = 64: nothing is remembered
                    case([Call(I64, key=7, end=valid), Call(I64, key=7, end=valid, t=small, marker=marker)], [(1, "probe")], "overflowed")
    return out


@pytest.mark.parametrize("nn", NNS)
def test_reuse(progs, nn):
    scripts = _reuse_cases(nn, np.random.default_rng(400 + nn))
    rows = run_group(progs, nn, [c for c, _ in scripts])
    done = {"reuse": 0, "probe": 0, "same as 2": 0}
    for (case, expect), row in zip(scripts, rows):
        h = case.tag[2]
        n = 28 if h else 7
        first = case.model_list(case.calls[0], nn)
        assert row[0].terms == len(first) and len(first) > 1, case.tag
        if case.tag[0] == "overflowed":
            assert len(first) > 64 and row[0].key == 0, case.tag
        else:
            assert len(first) <= ql_of(case.calls[0].instance) and row[0].key == case.calls[0].key, case.tag
        for k, what in expect:
            call = case.calls[k]
            want = case.model_list(call, nn)
            if what == "reuse":
                # the cells of the lanes are those of the call before: nothing moved, by the model too
                before = case.calls[k - 1]
                assert np.array_equal(case.target.grid.indices([m for m in case.lane_means(call) if m is not None]),
                                      case.target.grid.indices([m for m in case.lane_means(before) if m is not None])), case.tag
                assert row[k].terms == 1 and row[k].list(2048) == [call.marker], case.tag
            elif what == "probe":
                assert len(want) > 1
                assert (row[k].terms, row[k].count) == (len(want), len(want)), case.tag
                assert row[k].holds(want, ql_of(call.instance)), case.tag
                check_cells(case, call, row[k])
            else:
                # call 1 used the list of call 0 at the pose of call 2, which probed afresh (key 0): the same bits
                assert want == first and row[k].terms == len(want) and row[2].terms == len(want), case.tag
                assert np.array_equal(_bits(row[k].tot[:n]), _bits(row[2].tot[:n])), case.tag
                assert not np.array_equal(_bits(row[k].tot[:n]), _bits(row[0].tot[:n])), case.tag
            done[what] += 1
    assert min(done.values()) >= 4, done
    print("reuse nn %d: %d scripts, %s" % (nn, len(scripts), done))


# ---- segments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", NNS)
def test_segments(progs, nn):
    rng = np.random.default_rng(500 + nn)
    # hit totals: all segments fit in a list of 64; several whole segments share one; one segment alone exceeds it
    totals = [40, 64] + ([] if nn == 0 else [150, 500, 27 * 64 if nn == 1 else 1500])
    cases, alone = [], []
    for total in totals:
        if total <= 500:
            target, smean = _with_total(nn, total, rng)
        else:
            size = (10, 9, 8)
            target = Target(size, (0, 0, 0), 0.5, range(720) if nn == 1 else _random_slots(rng, size, 0.25), rng)
            smean = _at(target.grid, np.stack([rng.integers(2, 8, 64), rng.integers(2, 7, 64), rng.integers(2, 6, 64)], axis=1), rng)
        scov = _covs(rng, 64)
        for end in (64, 20, 57):
            for seg in (8, 16, 32, 64):
                for h in (False, True):
                    for lib in (False, True):
                        cases.append(Case(target, smean, scov, [Call(inst(3, h, lib), end=end)], seg_lanes=seg, tag=(total, end, seg, h, lib)))
                        if lib:
                            # the eval_derivs instance on every segment's cells alone
                            for sg in range((end + seg - 1) // seg):
                                alone.append(Case(target, smean, scov, [Call(inst(2, h, True), base=sg * seg, end=min(end, (sg + 1) * seg))],
                                                  tag=(total, end, seg, h, sg)))
    rows = run_group(progs, nn, cases)
    arow = {c.tag: r[0] for c, r in zip(alone, run_group(progs, nn, alone))}
    kinds = set()
    for case, row in zip(cases, rows):
        total, end, seg, h, lib = case.tag
        call, row = case.calls[0], row[0]
        n = 28 if h else 7
        ql = ql_of(call.instance)
        check_cells(case, call, row)
        n_seg = (end + seg - 1) // seg
        counts = []
        for sg in range(8):
            if sg >= n_seg:
                assert np.all(_bits(row.rows[sg]) == 0), (case.tag, sg)          # the zeros they were given
                kinds.add("empty")
                continue
            want = case.model_list(call, nn, (sg * seg, (sg + 1) * seg))
            counts.append(len(want))
            ref = arow[(total, end, seg, h, sg)]
            assert int(row.rows[sg, 28]) == len(want) and ref.terms == len(want), (case.tag, sg)
            assert np.array_equal(_bits(row.rows[sg, :n]), _bits(ref.tot[:n])), (case.tag, sg)
            if h is False:
                assert np.all(_bits(row.rows[sg, 7:28]) == 0)
        if sum(counts) <= ql:
            kinds.add("all fit")
        elif max(counts) > ql:
            kinds.add("one exceeds")
        if sum(counts) > ql and any(a + b <= ql for a, b in zip(counts, counts[1:])):
            kinds.add("some share")
    assert kinds >= ({"all fit", "empty"} if nn == 0 else {"all fit", "empty", "one exceeds", "some share"}), kinds
    print("segments nn %d: %d cases, %d segments alone" % (nn, len(cases), len(alone)))
