"""tests/marker_model.py against numpy.linalg.eigh on the marker fixtures and 2000 random SPD matrices (CPU).

The bound 1e-9 is not a measurement.  The Jacobi stops at off-diagonal mass <= 1e-30 of the diagonal's, so its error is a few ulps of
||cov|| (about 1e-15 relative); a wrong axis, a transposed V or a wrong rotation is an error of order 1.  No eigenvector is compared
with eigh's: unit length, the residual ||cov d - lambda d|| and orthogonality hold inside a degenerate eigenspace too."""
import numpy as np
import pytest

import marker_fixtures as MF
import marker_model as M


def _figures(cov, min_eval=M.MIN_EVAL):
    cov = np.asarray(cov).reshape(-1, 3, 3)
    _, kept, evals, flags = M.cell_segments(np.zeros((cov.shape[0], 3)), M.cov6_of(cov), None, min_eval)
    _, V = M.eig3(M.cov6_of(cov))
    assert flags == 0
    fig = M.check_against_eigh(cov, evals, V, kept, min_eval)
    print(fig)
    return fig, kept, evals, V


def _assert_bounds(fig):
    assert fig["eval_rel"] <= 1e-9
    assert fig["unit"] <= 1e-12
    assert fig["residual"] <= 1e-9
    assert fig["ortho"] <= 1e-9
    assert fig["count_bad"] == 0


@pytest.fixture(scope="module")
def designed():
    return [MF.designed_cells(m) for m in range(MF.N_MAPS)]


def test_designed_cells_against_eigh(designed):
    cov = np.concatenate([d[1] for d in designed])
    fam = np.concatenate([d[2] for d in designed])
    fig, kept, evals, _ = _figures(cov)
    _assert_bounds(fig)
    assert cov.shape[0] == 857
    # Only family (c) falls in the band around min_eval, where the count is not compared with eigh's.  It is a sixth of the designed
    # cells by construction (not "at most 1 %": that limit holds for the built maps and the random matrices, asserted below), so its
    # count is compared with the exact expectation instead, here, and bit for bit in the ABI and GPU tests.
    assert fig["in_band"] == int((fam == "c").sum())
    n = kept.sum(axis=1)
    for f, want in MF.SEGMENTS.items():
        assert (n[fam == f] == want).all(), f
    c = fam == "c"
    assert (evals[c] == np.array([5e-5, 1e-4, 0.01])).all()          # exact: the solver does not run on a diagonal matrix
    assert (kept[c] == np.array([False, True, True])).all()          # the threshold itself is emitted


def test_built_cells_against_eigh():
    cells = MF.built_cells()
    cov = np.concatenate([c[1] for c in cells])
    assert cov.shape[0] >= 100
    fig, kept, _, _ = _figures(cov)
    _assert_bounds(fig)
    assert fig["in_band"] == 0
    assert kept.all()                      # cells as wide as their cell: every axis is far above 1e-4


def test_random_spd_against_eigh():
    rng = np.random.default_rng(2024)
    cov = np.zeros((2000, 3, 3))
    for k in range(2000):
        R = MF.rotation(rng)
        lam = 10.0 ** rng.uniform(-6, 0, size=3)
        if k % 10 == 0:
            lam[1] = lam[0]                # a degenerate pair now and then
        c = R @ np.diag(lam) @ R.T
        cov[k] = 0.5 * (c + c.T)
    fig, _, _, _ = _figures(cov)
    _assert_bounds(fig)
    assert fig["in_band"] <= 20            # the cells left out of the count comparison: at most 1 % (none is expected)


def test_order_is_ascending_and_stable_and_the_sign_is_fixed():
    # a diagonal matrix with a tie: the solver does not run, the diagonal's order stays among equal values
    ev, V = M.eig3(np.array([[0.02, 0, 0, 0.01, 0, 0.01]]))
    assert (ev[0] == [0.01, 0.01, 0.02]).all()
    assert (V[0] == np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=float)).all()      # columns: e_y, e_z, e_x
    rng = np.random.default_rng(3)
    cov = np.stack([MF.family_cov("a", rng) for _ in range(200)])
    ev, V = M.eig3(M.cov6_of(cov))
    assert (np.diff(ev, axis=1) >= 0).all()
    lead = np.take_along_axis(V, np.abs(V).argmax(axis=1)[:, None, :], axis=1)[:, 0, :]
    assert (lead > 0).all()


def test_a_cell_under_a_pose_and_the_order_of_a_call(designed):
    mean, cov, _ = designed[2]
    pts0, src0, _ = M.map_markers([(mean, cov)], None, first=2)
    T = MF.POSES_ROLL[0]
    pts1, src1, _ = M.map_markers([(mean, cov)], T[None], first=2)
    assert pts0.shape == pts1.shape and (src0 == src1).all() and (src0[:, 0] == 2).all()
    assert np.abs(pts1 - (pts0 @ T[:3, :3].T + T[:3, 3])).max() <= 1e-12
    assert (np.diff(src0[:, 1].astype(np.int64)) >= 0).all()       # cells in order, their axes together
    # the midpoint of a segment is its cell's mean, its half length the axis' standard deviation
    mid = 0.5 * (pts0[:, 0] + pts0[:, 1])
    assert np.abs(mid - mean[src0[:, 1]]).max() <= 1e-12
    # an empty map in the middle contributes nothing and shifts nothing
    a, sa, _ = M.map_markers([designed[0][:2], designed[1][:2], designed[2][:2]], MF.POSES_YAW)
    b, sb, _ = M.map_markers([designed[0][:2]], MF.POSES_YAW[:1])
    c, sc, _ = M.map_markers([designed[2][:2]], MF.POSES_YAW[2:], first=2)
    assert (a == np.concatenate([b, c])).all() and (sa == np.concatenate([sb, sc])).all()


def test_a_non_finite_eigenvalue_emits_nothing_and_raises_the_flag():
    cov6 = np.array([[np.nan, 0, 0, 0.01, 0, 0.02], [0.01, 0, 0, 0.02, 0, np.inf]])
    seg, kept, evals, flags = M.cell_segments(np.zeros((2, 3)), cov6)
    assert flags == M.NONFINITE
    # (a NaN does not compare: it stays where the diagonal had it; an infinity sorts last)
    assert (kept == np.array([[False, True, True], [True, True, False]])).all()


def test_links_and_particles():
    poses, ref, mov, score = MF.links()
    pts, flags = M.link_markers(poses, ref, mov, score, skip_negative=0)
    assert pts.shape == (300, 2, 3) and flags == 0
    assert (pts[:, 0] == poses[ref, :3, 3]).all() and (pts[:, 1] == poses[mov, :3, 3]).all()
    pts1, _ = M.link_markers(poses, ref, mov, score, skip_negative=1)
    keep = score >= 0
    assert pts1.shape[0] == keep.sum() == 200 and (pts1 == pts[keep]).all()
    bad_ref = ref.copy()
    bad_ref[7] = 40
    pts2, flags2 = M.link_markers(poses, bad_ref, mov, score, skip_negative=0)
    assert flags2 == M.BAD_INDEX and pts2.shape[0] == 299
    T = MF.particles()
    p = M.particle_markers(T)
    assert p.shape == (2, 300, 2, 3)
    assert (p[..., 0, :] == T[..., :3, 3]).all()
    assert np.abs(np.linalg.norm(p[..., 1, :] - p[..., 0, :], axis=-1) - 0.3).max() <= 1e-12
