"""Multi-resolution D2D registration of raw scan pairs (NDTMatcherD2D(irregular, useDefault, resolutions).match(target_pc,
source_pc, T, useInitialGuess); ndt_odom_debug.cpp:159-165, ndt_feature_pcl_eval.cpp:620-642) restated on the CPU as a
composition of the oracle's single-resolution pieces (OracleMap, load_points, compute_cells, match_d2d).

The composition is what the GPU entry (ndtgpu_register_multires_*) is checked against: every float move of the source cloud
and every 4x4 product is written out as explicit left-to-right sums in fp64 (no numpy @, no fused multiply-add), in the order
csrc/ndt_fuser.hip (ndt_cloud_transform_kernel) and csrc/ndt_pose.h (ndt_pose_mul) use.  The GPU test module loads this file
for the same functions."""
import numpy as np
import pytest

DEFAULT_RESOLUTIONS = (0.2, 0.5, 1.0, 2.0)
SIZE = (100.0, 100.0, 1.0)
RNG = 30.0


def move_cloud(T, xyz):
    """transformPointCloudInPlace: (float)(T * (double)p) per point; T 4x4 (row/column math convention)"""
    p = np.asarray(xyz, dtype=np.float32)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = np.empty((p.shape[0], 3), dtype=np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def pose_mul(A, B):
    """A * B with the sums of ndt_pose_mul: s = 0, then s += A[r, k] B[k, c] for k = 0..3, in fp64 scalars"""
    C = np.zeros((4, 4), dtype=np.float64)
    for c in range(4):
        for r in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[r, k]) * float(B[k, c])
            C[r, c] = s
    return C


def range_filter(xyz, range_limit):
    """NDTMap::loadPointCloud's range test on the raw scan (sensor at its origin), fp64: points beyond it become NaN"""
    p = np.array(xyz, dtype=np.float32)[:, :3].copy()
    if range_limit > 0:
        x, y, z = (p[:, k].astype(np.float64) for k in range(3))
        far = np.sqrt((x * x + y * y) + z * z) > range_limit
        p[far] = np.nan
    return p


def oracle_map(O, res, cloud, range_limit=-1.0, centre=(0.0, 0.0, 0.0), size=SIZE):
    m = O.OracleMap(res, list(centre), list(size))
    m.load_points(cloud, range_limit)
    m.compute_cells()
    return m


def multires_match(O, target, source, T0, resolutions, use_initial_guess, range_limit=-1.0, centre=(0.0, 0.0, 0.0), size=SIZE,
                   **prm):
    """-> (T, per-level result dicts in LIST order (None where the level did not run)).  The levels run from the last entry of
    `resolutions` to the first, as listed (not sorted); each level's maps sit on the caller's grid (centre, size) at the level's
    cell size; the target cloud is range-filtered by the map build, the raw source once, before it moves."""
    src = range_filter(source, range_limit)
    T0 = np.asarray(T0, dtype=np.float64)
    if use_initial_guess:
        src = move_cloud(T0, src)
        Tinit = T0
    else:
        Tinit = np.eye(4)
    T = np.eye(4)
    results = [None] * len(resolutions)
    prm = dict(prm)
    prm["use_initial_guess"] = 0
    for j in range(len(resolutions) - 1, -1, -1):
        res = resolutions[j]
        tm = oracle_map(O, res, target, range_limit, centre, size)
        sm = oracle_map(O, res, src, -1.0, centre, size)
        Temp, r = O.match_d2d(tm, sm, np.eye(4), **prm)
        results[j] = r
        src = move_cloud(Temp, src)
        T = pose_mul(Temp, T)
    return pose_mul(T, Tinit), results


def pose_error(T, T_ref):
    dt = float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]))
    dr = float(2.0 * np.arcsin(min(1.0, np.linalg.norm(T[:3, :3] - T_ref[:3, :3]) / (2.0 * np.sqrt(2.0)))))
    return dt, dr


def T2d(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = c, -s, s, c, x, y
    return T


# The basin: pairs of the bench's 2D scenes whose initial guess is off by metres and degrees.  Over seeds 9001-9024 at this
# perturbation the single 0.5 m match ends more than 0.1 m from T_gt on five of them (BASIN_FAR); coarse to fine over
# {0.5, 1, 2, 4} recovers every one of the 24.  (On most pairs of these scenes a single 0.5 m match already converges from such a
# guess: the gain is per pair, not across the board.)
BASIN_RESOLUTIONS = (0.5, 1.0, 2.0, 4.0)
BASIN_POINTS = 20000
BASIN_PERTURB = (1.0, -0.7, np.radians(5.0))
BASIN_FAR = (9001, 9002, 9012, 9018, 9023)


@pytest.fixture(scope="module")
def O():
    import oracle
    oracle.binding.build()
    return oracle


def test_float_move_and_product_are_the_explicit_sums():
    rng = np.random.default_rng(3)
    T = T2d(0.3, -1.2, 0.4)
    T[2, 3] = 0.01
    p = rng.uniform(-30, 30, (1000, 3)).astype(np.float32)
    m = move_cloud(T, p)
    # the same sums one point at a time in Python floats (fp64, no fused multiply-add)
    for i in (0, 17, 999):
        x, y, z = (float(v) for v in p[i])
        for r in range(3):
            v = T[r, 0] * x
            v = v + T[r, 1] * y
            v = v + T[r, 2] * z
            v = v + T[r, 3]
            assert m[i, r] == np.float32(v)
    A, B = T2d(1, 2, 0.3), T2d(-0.5, 0.1, -1.1)
    C = pose_mul(A, B)
    assert np.allclose(C, A @ B, atol=1e-15)


def test_one_level_without_initial_guess_is_the_single_match(O):
    from ndt_feature_graph_amd import synth
    import torch
    pr = synth.pair_2d(torch.tensor([7101, 7102]), 20000)
    for k in range(2):
        f, m = pr["fixed"][k].numpy(), pr["moving"][k].numpy()
        T, res = multires_match(O, f, m, pr["T_init"][k].numpy(), (0.5,), 0, RNG)
        tm = oracle_map(O, 0.5, f, RNG)
        sm = oracle_map(O, 0.5, range_filter(m, RNG))
        To, ro = O.match_d2d(tm, sm, np.eye(4), use_initial_guess=0)
        # T = (Temp * I) * I: the products only normalise the sign of zeros
        assert np.array_equal(T, To + 0.0)
        assert res[0]["iterations"] == ro["iterations"] and res[0]["score"] == ro["score"]


def test_one_level_range_filter_on_the_raw_source_equals_the_build_filter(O):
    from ndt_feature_graph_amd import synth
    import torch
    pr = synth.pair_2d(torch.tensor([7103]), 20000)
    m = pr["moving"][0].numpy()
    a = oracle_map(O, 0.5, m, RNG).export_cells()
    b = oracle_map(O, 0.5, range_filter(m, RNG)).export_cells()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_basin_pairs_where_coarse_to_fine_recovers_what_a_single_match_misses(O):
    from ndt_feature_graph_amd import synth
    import torch
    pr = synth.pair_2d(torch.tensor(BASIN_FAR), BASIN_POINTS)
    f, m, T_gt = pr["fixed"].numpy(), pr["moving"].numpy(), pr["T_gt"].numpy()
    for k, seed in enumerate(BASIN_FAR):
        T0 = pose_mul(T_gt[k], T2d(*BASIN_PERTURB))
        Ts, _ = O.match_d2d(oracle_map(O, 0.5, f[k], RNG), oracle_map(O, 0.5, m[k], RNG), T0)
        assert pose_error(Ts, T_gt[k])[0] > 0.1, seed
        Tm, res = multires_match(O, f[k], m[k], T0, BASIN_RESOLUTIONS, 1, RNG)
        dt, dr = pose_error(Tm, T_gt[k])
        assert dt <= 0.02 and dr <= 0.005, (seed, dt, dr)
        assert all(r["exit_code"] >= 0 for r in res)
