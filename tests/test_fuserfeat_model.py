"""The pure host functions of the fuser bank's feature path (ndtgpu_fuser_feat_prepare, ndtgpu_fuser_feat_move; no device) against
tests/fuserfeat_model.py: records, cell means and covariances BIT FOR BIT -- both sides run the same rounded products in the same
order (csrc/ndt_fuserfeat.h, contraction off), no trigonometry on the compared values; the moved points' theta to 1e-12 rad (a few
ulps of libm's cos / sin / atan2 at |theta| <= pi).  The correspondences come from tests/featmatch_model.py on the hand-made pairs
of fuserfeat_model.hand_made_pair."""
import math

import numpy as np
import pytest

import featmatch_model as FM
import fuserfeat_model as M
from test_gpu_fuser_bank import mm, pose2d, rigid_inv

SENSOR = pose2d(0.25, -0.05, 0.02)
TNOW = pose2d(1.3, -0.7, 0.4)
TMOTION = pose2d(0.21, 0.03, -0.02)


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def record_of(N, m):
    from ndt_feature_graph_amd import binding
    r = np.zeros(1, dtype=binding.FEATMATCH_RESULT_DTYPE)
    for f in binding.FEATMATCH_RESULT_DTYPE.names:
        r[f] = m[f]
    return r[0]


def pose3(T):
    return float(T[0, 3]), float(T[1, 3]), math.atan2(T[1, 0], T[0, 0])


def run_case(N, K, seed, pose, fields=None, ffields=None, prev_moved=False, sensor=SENSOR, expect=None):
    prm = N.fuser_params(sensor_pose=sensor, **(fields or {}))
    fprm = N.fuser_feat_params(**(ffields or {}))
    cur, prev, desc, _ = M.hand_made_pair(K, seed, pose=pose)
    m = FM.match(prev, desc, cur, desc)                                   # (ref = prev, mov = cur)
    rr = record_of(N, m)
    pp = N.fuser_prepare(prm, TNOW, TMOTION, [0.0, 0.0, 0.0])
    rec, cells = N.fuser_feat_prepare(prm, fprm, TNOW, TMOTION, rr, m["corr"], cur, prev, prev_moved=prev_moved)
    mrec, mcells = M.prepare(prm, fprm, TNOW, TMOTION, pp, rr, m["corr"], cur, prev, prev_moved=prev_moved)
    what = (K, seed, fields, ffields)
    for f in ("ransac_run", "consistent", "n_feat_cells", "n_odom_cells", "truncated"):
        assert int(rec[f][0]) == mrec[f], (what, f, int(rec[f][0]), mrec[f])
    for f in ("n_prev", "n_map", "map_appended", "map_overflow", "pad_"):
        assert int(rec[f][0]) == 0, (what, f)
    assert np.array_equal(rec["Tfeat"][0].reshape(4, 4).T, mrec["Tfeat"]), what
    if mrec["ransac_run"]:
        assert rec["ransac"][0].tobytes() == rr.tobytes(), what
    assert cells.shape == mcells.shape, (what, cells.shape, mcells.shape)
    assert np.array_equal(cells, mcells), (what, float(np.max(np.abs(cells - mcells))))
    if expect is not None:
        got = dict(status=int(m["status"]), n_inliers=int(m["n_inliers"]), consistent=mrec["consistent"], n_feat=mrec["n_feat_cells"],
                   n_odom=mrec["n_odom_cells"], truncated=mrec["truncated"])
        for k, v in expect.items():
            assert got[k] == v, (what, k, got)
    return m, mrec, mcells


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_fixture_is_what_the_issue_states(seed):
    """K = 20, 24, 30: OK, K inliers, corr (i, i), pose error <= 2e-15 without the position noise; K = 19: TOO_FEW"""
    for K in (20, 24, 30):
        cur, prev, desc, T = M.hand_made_pair(K, seed)
        m = FM.match(prev, desc, cur, desc)
        assert m["status"] == FM.OK and m["n_inliers"] == K
        assert np.array_equal(m["corr"], np.stack([np.arange(K), np.arange(K)], axis=1))
        cur, prev, desc, T = M.hand_made_pair(K, seed, noise=0.0)
        c, s = T[0, 0], T[1, 0]
        cand, _ = FM.candidates(desc, desc, 0.6)
        assert cand == [(i, i) for i in range(K)]
        pose = FM.compute_pose([cur[i] for i in range(K)], [prev[i] for i in range(K)])
        assert max(abs(pose[0] - c), abs(pose[1] - s), abs(pose[2] - T[0, 3]), abs(pose[3] - T[1, 3])) <= 2e-15
    cur, prev, desc, _ = M.hand_made_pair(19, seed)
    assert FM.match(prev, desc, cur, desc)["status"] == FM.TOO_FEW


@pytest.mark.parametrize("seed", [0, 3])
def test_cells_with_and_without_the_odometry_cells(N, seed):
    pose = (0.3, -0.2, 0.05)
    # K = 24 with use_odom: 24 + 40 = 64 cells, not truncated
    _, _, cells = run_case(N, 24, seed, pose, expect=dict(status=0, n_inliers=24, consistent=1, n_feat=24, n_odom=40, truncated=0))
    assert cells.shape[0] == 64
    # K = 30: 24 taken, truncated
    run_case(N, 30, seed, pose, expect=dict(n_inliers=30, consistent=1, n_feat=24, n_odom=40, truncated=1))
    # K = 30 without use_odom: 30 taken
    _, _, cells = run_case(N, 30, seed, pose, fields=dict(use_odom=0), expect=dict(consistent=1, n_feat=30, n_odom=0, truncated=0))
    assert cells.shape[0] == 30
    # K = 19: inconsistent, the odometry cells only
    _, _, cells = run_case(N, 19, seed, pose, expect=dict(status=1, consistent=0, n_feat=0, n_odom=40, truncated=0))
    assert cells.shape[0] == 40
    # neither: upstream's use_odom_or_features = false
    _, _, cells = run_case(N, 19, seed, pose, fields=dict(use_odom=0), expect=dict(n_feat=0, n_odom=0))
    assert cells.shape[0] == 0
    # fusion2d: no cells, as the plain entry; use_feat = 0: RANSAC is not run
    run_case(N, 24, seed, pose, fields=dict(fusion2d=1), expect=dict(consistent=1, n_feat=0, n_odom=0))
    _, mrec, _ = run_case(N, 24, seed, pose, ffields=dict(use_feat=0), expect=dict(n_feat=0, n_odom=40))
    assert mrec["ransac_run"] == 0
    # the sensor at the origin
    run_case(N, 24, seed, pose, sensor=np.eye(4), expect=dict(n_feat=24, n_odom=40))


def test_the_odometry_cells_are_the_plain_entrys(N):
    """behind the FLIRT cells come exactly the 40 records ndtgpu_fuser_update_batch fills from ndtgpu_fuser_prepare"""
    prm = N.fuser_params(sensor_pose=SENSOR)
    _, _, cells = run_case(N, 24, 1, (0.3, -0.2, 0.05))
    pp = N.fuser_prepare(prm, TNOW, TMOTION, [0.0, 0.0, 0.0])
    for i in range(40):
        c = cells[24 + i]
        assert np.array_equal(c[0:3], pp["feat_src_mean"]) and np.array_equal(c[9:12], pp["feat_tgt_mean"])
        assert np.array_equal(c[3:9], pp["feat_cov_plain"] if i == 39 else pp["feat_cov_rotated"])
        assert np.array_equal(c[12:18], pp["feat_cov_rotated"])


@pytest.mark.parametrize("offset,consistent", [(0.05, 1), (0.3, 0)])
def test_consistency_gate(N, offset, consistent):
    """check_consistency with the odometry 0.05 m / 0.3 m from the feature pose: the threshold is max_translation_norm / 10 = 0.1"""
    # Tfeat = T_ransac * sensor^-1 lands `offset` metres from Tnow * Tmotion
    P = mm(mm(mm(TNOW, TMOTION), pose2d(offset, 0.0, 0.0)), SENSOR)
    run_case(N, 24, 2, pose3(P), fields=dict(check_consistency=1),
             expect=dict(status=0, n_inliers=24, consistent=consistent, n_feat=24 * consistent, n_odom=40))
    # without check_consistency the same features pass
    run_case(N, 24, 2, pose3(P), expect=dict(consistent=1, n_feat=24))


def test_prev_in_map_frame(N):
    pose = (0.3, -0.2, 0.05)
    _, _, quirk = run_case(N, 24, 4, pose, ffields=dict(prev_in_map_frame=0), prev_moved=True)
    _, _, as_is = run_case(N, 24, 4, pose, ffields=dict(prev_in_map_frame=1), prev_moved=True)
    _, _, unmoved = run_case(N, 24, 4, pose, ffields=dict(prev_in_map_frame=1), prev_moved=False)
    assert np.array_equal(quirk, unmoved)                  # (a prev that was not moved is transformed either way)
    assert np.array_equal(quirk[:, :9], as_is[:, :9])      # the source cells do not depend on it
    cur, prev, _, _ = M.hand_made_pair(24, 4, pose=pose)
    for l in range(24):                                    # the target cells: the stored point, the un-rotated covariance
        assert np.array_equal(as_is[l, 9:12], [prev[l, 0], prev[l, 1], 0.0])
        assert np.array_equal(as_is[l, 12:18], [2e-4, 0.0, 0.0, 2e-4, 0.0, 1e-4])
    assert not np.array_equal(quirk[:24, 9:], as_is[:24, 9:])
    assert np.array_equal(quirk[24:], as_is[24:])          # the odometry cells are the same


def test_cells_against_plain_numpy(N):
    """the scalar loops against matrix products: mean' = Tnow S p, cov' = R diag R^T (1e-15 relative)"""
    _, _, cells = run_case(N, 24, 0, (0.3, -0.2, 0.05))
    cur, prev, _, _ = M.hand_made_pair(24, 0, pose=(0.3, -0.2, 0.05))
    A = TNOW @ SENSOR
    C = A[:3, :3] @ np.diag([2e-4, 2e-4, 1e-4]) @ A[:3, :3].T
    for l in range(24):
        assert np.allclose(cells[l, 0:3], (A @ [cur[l, 0], cur[l, 1], 0.0, 1.0])[:3], rtol=0, atol=1e-14)
        assert np.allclose(cells[l, 9:12], (A @ [prev[l, 0], prev[l, 1], 0.0, 1.0])[:3], rtol=0, atol=1e-14)
        for side in (3, 12):
            assert np.allclose(cells[l, side:side + 6], [C[i, j] for i, j in M.IJ], rtol=0, atol=1e-18)


def test_move(N):
    rng = np.random.default_rng(11)
    pos = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-5, 5, 200), rng.uniform(-math.pi, math.pi, 200)], axis=1)
    for T in (mm(TNOW, SENSOR), np.eye(4), pose2d(-2.0, 0.5, 3.0)):
        got, want = N.fuser_feat_move(T, pos), M.move(T, pos)
        assert np.array_equal(got[:, :2], want[:, :2])                 # x, y: products of the inputs only
        d = np.abs(got[:, 2] - want[:, 2])
        assert float(np.max(np.minimum(d, 2 * math.pi - d))) <= 1e-12
        # against the composition of 2D poses
        th = math.atan2(T[1, 0], T[0, 0])
        d = np.abs(np.angle(np.exp(1j * (got[:, 2] - (pos[:, 2] + th)))))
        assert float(np.max(d)) <= 1e-12
    assert N.fuser_feat_move(np.eye(4), np.zeros((0, 3))).shape == (0, 3)


def test_inverse_helper_is_rigid():
    assert np.allclose(rigid_inv(SENSOR) @ SENSOR, np.eye(4), rtol=0, atol=1e-15)
