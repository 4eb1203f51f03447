"""csrc/ndt_pairterm.h on the device against references that rest on definitions (tests/pairterm_model.py).

tests/native/pairterm_checks.hip includes the header alone and runs one case per thread.  What is checked:

  accuracy   pair_term<true, false> and pair_term<false, false> on every case of the families against formula() in
             mpmath (itself held to the central differences of the score by tests/test_pairterm_model.py).  Bound: 8 x the
             family's floor, the error of the plain formula in doubles -- never anything the device gave.  The floor is a
             family's worst case, so the median over a family is held, with the same factor, to the median error of the
             plain formula: a systematic loss of a digit in the ordinary cases does not hide under one hard case.
  PLANAR     accumulators 0, 1, 2, 6, 7, 8, 12, 13, 17, 27 of pair_term<H, true> have the bits of pair_term<H, false>, every
             other one is +0.
  guards     |det| on both sides of 1e-12; a NaN or an infinity in every input component; the exponent in the denormal
             range of the result and past the -745.2 cut-off.  The side of every case is known from the kernel's own
             expression in NumPy doubles, and a test fails if one side is missing.
  exp        exp_nonpos within one ulp of mpmath.exp (2^-1074 in the denormal range) and bit-equal to exp_model().
  rcp        rcp_nr within one ulp of the correctly rounded 1 / x.
  public     ndtgpu_derivatives on prefixes of 700 source cells against the mpmath sum of the per-term references, the
             pair set from the oracle's index_for_point; bound (8 floor + n 2^-52) sum |term entry|, per entry.

  The bound of `public` is taken per entry, with the floor of the lattice's own terms (2.3e-15: its cells are well conditioned).

Measured on an MI355X.  Largest error of pair_term<true, false> per family in units of the family's floor (the bound is 8;
pair_term<false, false> gave the same score and gradient figures), and the median error next to that of the plain formula:
               floor      score  gradient  Hessian    median     plain formula
  generic      2.56e-12   0.876  0.831     0.784      1.79e-15   1.93e-15
  flat         3.15e-14   0.037  0.872     0.538      4.37e-16   5.50e-16
  skewed       3.50e-11   0.441  0.377     0.719      3.33e-13   3.00e-13
  far          2.43e-13   1.008  0.909     1.659      2.60e-15   2.29e-15
  tails        8.69e-11   0.431  0.430     0.429      9.20e-14   1.41e-13
  degenerate   2.24e-12   0.631  2.081     2.066      1.59e-15   2.16e-15
exp_nonpos: 0.837 ulp on the main range, 0.789 x 2^-1074 on the denormal range, the bits of exp_model() at all 17 132 points.
rcp_nr: correctly rounded at all 20 661 values.  PLANAR: the kept sums have the bits of the full term on every case.
public: at most 0.024 of the bound (one term; 0.001 .. 0.005 for 26 .. 990 terms).
"""
import functools
import os
import subprocess

import mpmath
import numpy as np
import pytest

import pairterm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairterm_checks.hip")
WIDTH_IN = {"term": 20, "exp": 1, "rcp": 1}
KEPT_PLANAR = [0, 1, 2, 6, 7, 8, 12, 13, 17, 27]
FAMILY_ORDER = ["generic", "flat", "skewed", "far", "tails", "degenerate"]
MARGIN = 8.0


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path_factory.mktemp("pairterm") / "pairterm_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", SRC, "-o", exe])

    def run(mode, table):
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, WIDTH_IN[mode])
        n = table.shape[0]
        out = subprocess.run(["timeout", "-k", "10", "60", exe, mode], input=np.uint32(n).tobytes() + table.tobytes(),
                             capture_output=True)
        if out.returncode in (-6, -11, 124, 134, 137, 139):         # a fault or a hang: nothing more is started on the device
            pytest.exit("pairterm_checks %s ended with %d: %s" % (mode, out.returncode, out.stderr.decode(errors="replace")), 1)
        assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace"))
        return np.frombuffer(out.stdout, dtype=np.float64).reshape(n, -1)
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def family_out(run):
    """name -> [n, 4, 28]: the four instances on every case of the families, one run of the program"""
    fam = M.families()
    out = run("term", np.concatenate([fam[k] for k in FAMILY_ORDER])).reshape(-1, 4, 28)
    split, lo = {}, 0
    for k in FAMILY_ORDER:
        split[k] = out[lo:lo + len(fam[k])]
        lo += len(fam[k])
    return split


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def test_accuracy(family_out):
    refs, floors, medians = M.references(), M.floors(), M.median_floors()
    bad = []
    with M.workprec():
        for name in FAMILY_ORDER:
            worst, every = {0: [0.0, 0.0, 0.0], 1: [0.0, 0.0, 0.0]}, []
            for k, ref in enumerate(refs[name]):
                for slot in (0, 1):                     # pair_term<false, false>, pair_term<true, false>
                    got = family_out[name][k, slot]
                    assert np.all(np.isfinite(got))
                    if slot == 0:                       # without the Hessian: its 21 sums are never touched
                        assert np.all(_bits(got[7:]) == 0)
                        err = M.part_errors(list(got[:7]) + ref[7:], ref)
                    else:
                        err = M.part_errors(list(got), ref)
                        every.append(max(err))
                    worst[slot] = [max(a, b) for a, b in zip(worst[slot], err)]
                    if max(err) > MARGIN * floors[name]:
                        bad.append((name, k, slot, err))
            print("%-10s floor %.2e   score / gradient / Hessian in floors:  <false> %.3f %.3f   <true> %.3f %.3f %.3f   "
                  "median %.2e, of the formula in doubles %.2e" % (
                      name, floors[name], worst[0][0] / floors[name], worst[0][1] / floors[name], worst[1][0] / floors[name],
                      worst[1][1] / floors[name], worst[1][2] / floors[name], float(np.median(every)), medians[name]))
            # the floor is a family's worst case; its ordinary cases are held to the ordinary error of the plain formula
            if np.median(every) > MARGIN * medians[name]:
                bad.append((name, "median", float(np.median(every)), medians[name]))
    assert not bad, bad[:5]


# ---- PLANAR -----------------------------------------------------------------------------------------------------------------
def test_planar_keeps_the_bits_of_the_full_term(family_out):
    other = [a for a in range(28) if a not in KEPT_PLANAR]
    for name in FAMILY_ORDER:
        out = family_out[name]
        for full, planar in ((0, 2), (1, 3)):
            assert np.array_equal(_bits(out[:, planar, KEPT_PLANAR]), _bits(out[:, full, KEPT_PLANAR])), (name, planar)
            assert np.all(_bits(out[:, planar, other]) == 0), (name, planar)
        assert np.all(out[:, 3, 0] != 0.0) and np.all(out[:, 3, 7] != 0.0)       # (the kept sums are live)


# ---- guards -----------------------------------------------------------------------------------------------------------------
def _diag_case(sxx, syy, szz, x, d1=1.0, d2=0.05):
    """C = Cj = diag / 2 (exact halves: C + Cj is the diagonal itself), mu = 0"""
    half = [0.5 * sxx, 0.0, 0.0, 0.5 * syy, 0.0, 0.5 * szz]
    return np.array(list(x) + half + [0.0, 0.0, 0.0] + half + [d1, d2])


def test_guard_det(run):
    cases = [_diag_case(1e-4 * (1.0 + k * 2.0 ** -50), 1e-4, 1e-4, [1e-3, -2e-3, 5e-4]) for k in range(-12, 13)]
    cases += [_diag_case(-c[3] * 2, c[6] * 2, c[8] * 2, c[0:3]) for c in cases]                  # det < 0: the guard is on |det|
    cases = np.array(cases)
    det = np.array([M.kernel_det(c[3:9], c[12:18]) for c in cases])
    above = np.abs(det) > 1e-12
    assert above.sum() >= 8 and (~above).sum() >= 8 and (det[above] < 0).any() and (det[~above] < 0).any()
    assert np.abs(np.abs(det) / 1e-12 - 1.0).max() < 1e-13                                       # (all of them sit on the guard)
    out = run("term", cases).reshape(-1, 4, 28)
    assert np.all(_bits(out[~above]) == 0)
    floor = M.floors()["generic"]
    with M.workprec():
        for c, o in zip(cases[above], out[above]):
            ref = M.formula(c, M.MP)
            assert max(M.part_errors(list(o[1]), ref)) <= MARGIN * floor
            assert max(M.part_errors(list(o[0, :7]) + ref[7:], ref)) <= MARGIN * floor and np.all(_bits(o[0, 7:]) == 0)


def test_guard_nonfinite_inputs(run):
    base = M.families()["generic"][0]
    cases = []
    for pos in range(18):                                   # every component of m, C, mu, Cj
        for bad in (np.nan, np.inf, -np.inf):
            c = base.copy()
            c[pos] = bad
            cases.append(c)
    out = run("term", np.array(cases))
    assert out.shape == (54, 4 * 28)
    assert np.all(_bits(out) == 0), [(k // 3, k % 3) for k in np.nonzero(np.any(_bits(out) != 0, axis=1))[0]]


def test_guard_exponent_underflow(run):
    # S = I (C = Cj = I / 2), mu = 0, m = (t, 0, 0): A = I, det = 1, B x = x and l = t * t exactly as NumPy rounds it, so the
    # argument of the exponential on the device is the double computed here
    expo = [709.5, 712.0, 720.0, 730.0, 740.0, 744.0, 745.0, 745.19, 745.21, 745.5, 746.0, 800.0, 1e4, 1e8]
    ts = np.sqrt(np.array(expo) / 0.025)
    cases = np.array([_diag_case(1.0, 1.0, 1.0, [t, 0.0, 0.0]) for t in ts])
    arg = (np.float64(-0.05) * (ts * ts)) * np.float64(0.5)
    cut = arg < -745.2
    want = np.array([M.exp_model(a) for a in arg])
    denormal = (want > 0.0) & (want < 2.0 ** -1022)
    assert cut.sum() >= 4 and denormal.sum() >= 4 and np.all(want[cut] == 0.0) and np.all(cut | denormal | (want == 0.0))
    out = run("term", cases).reshape(-1, 4, 28)
    assert np.all(np.isfinite(out))
    for slot in range(4):
        assert np.array_equal(_bits(out[:, slot, 0]), _bits(0.0 - want)), slot       # +0 + (-denormal), or +0 + (-0) = +0 past the cut-off
    assert np.all(out[cut][:, :, 1:] == 0.0)                                         # (zeros of either sign)


# ---- exp --------------------------------------------------------------------------------------------------------------------
def test_exp(run):
    main, den = M.exp_points()
    special = np.array([x for x, _ in M.EXP_SPECIALS])
    x = np.concatenate([main, den, special])
    got = run("exp", x)[:, 0]
    gs = got[len(main) + len(den):]
    for g, (_, want) in zip(gs, M.EXP_SPECIALS):
        assert (np.isnan(g) and np.isnan(want)) or (g == want and not np.signbit(g)), (g, want)
    model = np.array([M.exp_model(v) for v in x[:len(main) + len(den)]])
    finite = got[:len(main) + len(den)]
    with M.workprec():
        err = np.array([M.exp_ulp_error(g, v) for g, v in zip(finite, x)])
    print("exp_nonpos on the device: %.3f ulp on the main range, %.3f x 2^-1074 on the denormal range; differs from "
          "exp_model at %d of %d points" % (err[:len(main)].max(), err[len(main):].max(),
                                            int(np.sum(_bits(finite) != _bits(model))), len(model)))
    assert err.max() <= 1.0
    differ = np.nonzero(_bits(finite) != _bits(model))[0]
    assert len(differ) == 0, [(float(x[k]), float(finite[k]), float(model[k])) for k in differ[:5]]


# ---- rcp --------------------------------------------------------------------------------------------------------------------
def test_rcp(run):
    rng = np.random.default_rng(5)
    x = np.ldexp(rng.uniform(1.0, 2.0, 20000), rng.integers(-1000, 1000, 20000)) * rng.choice([-1.0, 1.0], 20000)
    dets = np.array([M.kernel_det(c[3:9], c[12:18]) for cases in M.families().values() for c in cases])
    x = np.concatenate([x, dets])
    got = run("rcp", x)[:, 0]
    want = np.array([M.rcp_exact(v) for v in x])
    assert np.all(np.signbit(got) == np.signbit(want)) and np.all(np.isfinite(got))
    ulps = np.abs(_bits(np.abs(got)).astype(np.int64) - _bits(np.abs(want)).astype(np.int64))
    print("rcp_nr on the device: not correctly rounded at %d of %d values, at most %d ulp off" % (int(np.sum(ulps != 0)), len(x),
                                                                                                 int(ulps.max())))
    assert ulps.max() <= 1


# ---- through the public entry ---------------------------------------------------------------------------------------------------
COUNTS = [1, 63, 64, 65, 511, 512, 513, 700]
SIZE_CELLS = (12, 9, 7)
RES = 0.5


def _six(M33):
    return [M33[0, 0], M33[0, 1], M33[0, 2], M33[1, 1], M33[1, 2], M33[2, 2]]


@pytest.fixture(scope="module")
def lattice():
    return _lattice()


@functools.lru_cache(maxsize=None)
def _lattice():
    """one random target lattice, 700 source cells, and per (n_neighbours, count) the mpmath sum of the per-term references,
    the sum of their magnitudes, the number of terms and the floor of the lattice's own terms"""
    import oracle as O
    rng = np.random.default_rng(1297)
    size_m = [c * RES for c in SIZE_CELLS]
    slots = rng.choice(int(np.prod(SIZE_CELLS)), 14, replace=False)
    idx = np.stack(np.unravel_index(slots, SIZE_CELLS), axis=1)
    # LazyGrid: cell i is centred at (i - floor(size / 2)) * res
    tmean = (idx - np.array(SIZE_CELLS) // 2) * RES + rng.uniform(-0.2, 0.2, (len(idx), 3)) * RES
    A = rng.normal(size=(len(idx), 3, 3)) * 0.1
    tcov = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(3)
    ot = O.OracleMap(RES, [0, 0, 0], size_m)
    ot.set_cells(tmean, tcov)
    cell_at = {}
    for k in range(len(idx)):
        ic, inside = ot.index_for_point(tmean[k])
        assert inside and tuple(ic) == tuple(idx[k])
        cell_at[tuple(ic)] = k
    m = max(COUNTS)
    half = np.array(size_m) / 2.0
    smean = rng.uniform(-half - 1.2 * RES, half + 1.2 * RES, (m, 3))             # some sources outside the grid
    near = rng.random(m) < 0.35                                                  # a third of them inside an occupied cell
    near[0] = True
    smean[near] = tmean[rng.integers(0, len(idx), near.sum())] + rng.uniform(-0.1, 0.1, (near.sum(), 3)) * RES
    Bm = rng.normal(size=(m, 3, 3)) * 0.1
    scov = Bm @ Bm.transpose(0, 2, 1) + 0.01 * np.eye(3)
    sums, floor = {}, 0.0
    with M.workprec():
        zero = [mpmath.mpf(0)] * 28
        acc = {nn: [list(zero), list(zero), 0] for nn in (0, 2)}                 # sum, sum of magnitudes, terms
        for i in range(m):
            ic, _ = ot.index_for_point(smean[i])
            src = None
            for dx in range(-2, 3):
                for dy in range(-2, 3):
                    for dz in range(-2, 3):
                        k = cell_at.get((ic[0] + dx, ic[1] + dy, ic[2] + dz))
                        if k is None:
                            continue
                        case = np.array(list(smean[i]) + _six(scov[i]) + list(tmean[k]) + _six(tcov[k]) + [1.0, 0.05])
                        if src is None:
                            src = M.source_terms(case, M.MP), M.source_terms(case, M.DOUBLE)
                        ref = M.formula(case, M.MP, src[0])
                        floor = max(floor, max(M.part_errors(M.formula(case, M.DOUBLE, src[1]), ref)))
                        for nn in ((0, 2) if dx == dy == dz == 0 else (2,)):
                            a = acc[nn]
                            a[0] = [s + r for s, r in zip(a[0], ref)]
                            a[1] = [s + abs(r) for s, r in zip(a[1], ref)]
                            a[2] += 1
            if i + 1 in COUNTS:
                for nn in (0, 2):
                    sums[(nn, i + 1)] = (list(acc[nn][0]), list(acc[nn][1]), acc[nn][2])
    assert sums[(0, 1)][2] == 1 and sums[(2, 1)][2] > 1 and sums[(2, 700)][2] > 500 and sums[(0, 63)][2] >= 10 and sums[(0, 700)][2] > 200
    return dict(size_m=size_m, tmean=tmean, tcov=tcov, smean=smean, scov=scov, sums=sums, floor=floor)


@pytest.fixture(scope="module")
def target_map(lattice):
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    tg = N.MapSet(RES, [0, 0, 0], lattice["size_m"], max_cells=4096)
    tg.set_cells(0, lattice["tmean"], lattice["tcov"])
    assert tg.num_cells() == len(lattice["tmean"])
    return N, tg


@pytest.mark.parametrize("nn", [0, 2])
@pytest.mark.parametrize("count", COUNTS)
def test_public_entry_against_the_sum_of_term_references(lattice, target_map, count, nn):
    N, tg = target_map
    want, mag, n_terms = lattice["sums"][(nn, count)]
    for with_h in (True, False):
        s, g, H = N.derivatives(tg, 0, lattice["smean"][:count], lattice["scov"][:count], n_neighbours=nn, compute_hessian=with_h)
        got = [s] + list(g) + ([H[a, b] for a in range(6) for b in range(a, 6)] if with_h else [])
        if with_h:
            assert np.array_equal(H, H.T)
        worst = 0.0
        with M.workprec():
            for k, v in enumerate(got):
                err = abs(M.MP.num(v) - want[k])
                bound = (MARGIN * lattice["floor"] + n_terms * 2.0 ** -52) * mag[k]
                assert err <= bound, (count, nn, with_h, k, float(err), float(bound), n_terms)
                worst = max(worst, float(err / bound))
        print("count %d nn %d hessian %d: %d terms, floor %.2e, worst error %.3f of its bound" % (
            count, nn, with_h, n_terms, lattice["floor"], worst))
