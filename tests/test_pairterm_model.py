"""tests/pairterm_model.py checked against definitions, on the CPU: what tests/test_gpu_pairterm.py then holds the device to.

  * formula() in mpmath against exact(), the central differences of the score itself (400 bits, h = 1e-30), on the first 40
    cases of every family: 1e-25 of the largest entry of each quantity.  The gradient is allowed h * max|Hessian| on top:
    central differences resolve a gradient that is exactly zero (x = 0) only to their own truncation, far below that.
    Measured: 5.5e-51 at the worst (the far-from-origin family).
  * exp_model() against mpmath.exp: within one ulp on the 14 132 points of the main range (measured 0.837) and within
    2^-1074 on the 3 000 points of the denormal range (measured 0.789).
  * the floor of every family -- the largest error of formula() in doubles against formula() in mpmath, over score, gradient
    and Hessian, each relative to its largest reference entry -- is printed (pytest -s) and sane.  Measured:
        generic 2.6e-12   flat 3.1e-14   skewed 3.5e-11   far 2.4e-13   tails 8.7e-11   degenerate 2.2e-12
    A floor is set by its family's worst case: a plain evaluation in doubles loses about cond(C + Cj) * 2^-52 in
    l = x^T B x (more where the cofactors cancel: `skewed`), and the score multiplies that by the exponent d2 l / 2
    (`tails`).  The medians over a family are 5e-16 .. 3e-13.
  * the families are what they say: conditioning, distance from the origin, exponents, exact coincidences, and every case
    clear of the kernel's determinant guard (a pair of small cells, det(C + Cj) <= 1e-12, is skipped by the matcher as by
    the reference; the guard's two sides are cases of the device test).
"""
import math

import numpy as np
import pytest

import pairterm_model as M

N_EXACT = 40


@pytest.mark.parametrize("family", ["generic", "flat", "skewed", "far", "tails", "degenerate"])
def test_formula_is_the_derivative_of_the_score(family):
    cases = M.families()[family]
    assert len(cases) >= N_EXACT
    worst = 0.0
    with M.workprec():
        for case in cases[:N_EXACT]:
            want, got = M.exact(case), M.formula(case, M.MP)
            scale_h = max(abs(v) for v in want[7:28])
            for (lo, hi) in M.PARTS:
                scale = max(abs(v) for v in want[lo:hi])
                slack = scale_h * 10 ** M.FD_STEP_EXP if lo == 1 else 0
                diff = max(abs(g - w) for g, w in zip(got[lo:hi], want[lo:hi]))
                assert diff <= scale * 1e-25 + slack, (family, lo, float(diff), float(scale))
                if slack == 0 or diff > slack:
                    worst = max(worst, float(diff / scale))
    print("formula vs exact, %s: %.2e" % (family, worst))


def test_families_cover_what_they_claim():
    fam = M.families()
    assert 550 <= sum(len(c) for c in fam.values()) <= 700
    expo = {k: np.array([M._exponent(c[3:9], c[12:18], c[0:3] - c[9:12], c[19]) for c in v]) for k, v in fam.items()}
    cond = {k: np.array([np.linalg.cond(M._full(c[3:9]) + M._full(c[12:18])) for c in v]) for k, v in fam.items()}
    assert cond["flat"].max() > 1e6 and cond["flat"].max() < 1e7
    assert cond["skewed"].min() > M.COND_MAX and cond["skewed"].max() > 5e4 and cond["generic"].max() <= M.COND_MAX
    assert all(M.kernel_det(c[3:9], c[12:18]) > M.DET_MIN for v in fam.values() for c in v)
    assert np.linalg.norm(fam["far"][:, 9:12], axis=1).max() > 4000.0
    assert expo["tails"].min() >= 29.0 and expo["tails"].max() > 300.0 and expo["tails"].max() < 660.0
    for k in ("generic", "flat", "skewed", "far", "degenerate"):
        assert expo[k].max() <= 20.0 * (1 + 1e-9)
    deg = fam["degenerate"]
    assert np.sum(np.all(deg[:, 0:3] == deg[:, 9:12], axis=1)) >= 10            # x = 0 exactly
    assert np.sum(np.all(deg[:, 3:9] == deg[:, 12:18], axis=1)) >= 10           # C = Cj
    assert np.sum((deg[:, 18] != 1.0) & (deg[:, 19] != 0.05)) >= 10
    assert all(np.all(np.isfinite(c)) for c in fam.values())


def test_exp_model_within_one_ulp():
    main, den = M.exp_points()
    assert len(main) >= 6000 + 2000 + 6 * 1022 and len(den) == 3000
    with M.workprec():
        worst_main = max(M.exp_ulp_error(M.exp_model(x), x) for x in main)
        worst_den = max(M.exp_ulp_error(M.exp_model(x), x) for x in den)
    print("exp_model: %.3f ulp on [-708.1, 0], %.3f x 2^-1074 on [-745.2, -708.4]" % (worst_main, worst_den))
    assert worst_main <= 1.0 and worst_den <= 1.0
    assert all(0.0 <= M.exp_model(x) < 2.0 ** -1022 for x in den)               # (the range is the denormal one)
    for x, want in M.EXP_SPECIALS:
        got = M.exp_model(x)
        assert (math.isnan(got) and math.isnan(want)) or (got == want and math.copysign(1.0, got) == 1.0)


def test_floors():
    fl = M.floors()
    print("floors: " + "  ".join("%s %.2e" % kv for kv in fl.items()))
    # a floor of 0 would make the device's bound 0; one of 1e-8 would mean the formula in doubles is itself broken
    assert all(2.0 ** -53 < v < 1e-8 for v in fl.values())
