"""World-map assembly on the device (ndtgpu_world_assemble, include/ndtgpu.h) against its NumPy restatement (tests/world_model.py):
single node under the identity, overlapping planar nodes, order and batch independence, a 6-DoF pose in 3D, drops and overflow,
empty worlds, set_cells-installed sources, a Monte Carlo localisation bank as the consumer, and the resources of a call.

Bounds.  Means and covariances are compared within world_model.error_bounds, computed from the s1_shift / s2_shift of the result
record: one rounding of 2^-s cell units per moment and contribution, propagated through mean = s1 / N and
cov = (s2 - N m m^T) / (N - 1), times 4 for the surrounding double arithmetic.  Every comparison prints its largest
error / bound ratio before it asserts."""
import itertools

import numpy as np
import pytest

import world_model as W

pytestmark = pytest.mark.gpu

RES = W.NODE_RES
NODE_CELLS = W.grid_cells(RES, W.NODE_SIZE_M)
WORLD_CELLS = W.grid_cells(RES, W.WORLD_SIZE_M)
CAP = 4096


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    if N.device_count() < 1:
        pytest.fail("no HIP device")
    return N


@pytest.fixture(scope="module")
def planar(N):
    """maps 0..2: the three nodes of the planar case; map 3: never built (a node without cells).  The exported cells, the poses and
    the model's world are computed once and shared."""
    src = N.MapSet(RES, [0, 0, 0], W.NODE_SIZE_M, n_maps=4, max_cells=CAP)
    src.build(W.planar_scans())
    nodes = [src.export_cells(i) for i in range(3)]
    nodes = [(m, c, n) for m, c, _, n in nodes]
    poses = [W.pose2d(*p) for p in W.PLANAR_POSES]
    return dict(src=src, nodes=nodes, poses=poses)


def world_set(N, n_maps=1, max_cells=CAP, size_m=W.WORLD_SIZE_M):
    return N.MapSet(RES, [0, 0, 0], size_m, n_maps=n_maps, max_cells=max_cells)


def exported(ms, i=0):
    mean, cov, idx, n = ms.export_cells(i)
    return mean, cov, idx, n


def as_bytes(ms, i=0):
    return b"".join(a.tobytes() for a in exported(ms, i))


def slots_of(idx, cells):
    idx = idx.astype(np.int64)
    return (idx[:, 0] * cells[1] + idx[:, 1]) * cells[2] + idx[:, 2]


def compare_with_model(ms, i, res, model, cells, max_excluded=0.005):
    """same cell set, n equal, mean / covariance within the bound scaled by the cell's number of contributions.  Contributions
    within FACE_EPS of a cell face are left out together with the cells around them; at most 0.5 % of them."""
    flagged = np.flatnonzero(model["face_distance"] < W.FACE_EPS)
    assert flagged.size <= max_excluded * max(model["n_contributions"], 1)
    skip = set()
    for k in flagged:
        s = int(model["contribution_slot"][k])
        if s < 0:
            continue
        iz, iy, ix = s % cells[2], (s // cells[2]) % cells[1], s // (cells[2] * cells[1])
        for dx, dy, dz in itertools.product((-1, 0, 1), repeat=3):
            skip.add(((ix + dx) * cells[1] + iy + dy) * cells[2] + iz + dz)
    mean, cov, idx, n = exported(ms, i)
    got = {int(s): k for k, s in enumerate(slots_of(idx, cells))}
    assert set(got) - skip == set(model["cells"]) - skip
    worst = [0.0, 0.0]
    for s, c in model["cells"].items():
        if s in skip:
            continue
        k = got[s]
        assert n[k] == c["n"], (s, n[k], c["n"])
        mb, cb = W.error_bounds(res["s1_shift"], res["s2_shift"], c["N"], c["count"], RES, cells)
        dm, dc = np.abs(mean[k] - c["mean"]).max(), np.abs(cov[k] - c["cov"]).max()
        worst = [max(worst[0], dm / mb), max(worst[1], dc / cb)]
        assert dm <= mb and dc <= cb, (s, dm, mb, dc, cb)
    print("largest error / bound: mean %.3g, covariance %.3g over %d cells" % (worst[0], worst[1], len(model["cells"])))
    if not flagged.size:
        assert (res["n_cells"], res["n_dropped"], res["n_rejected"], res["n_points"]) == \
               (len(model["cells"]), model["n_dropped"], model["n_rejected"], model["n_points"])
    assert res["n_contributions"] == model["n_contributions"]
    assert (res["s1_shift"], res["s2_shift"]) == W.build_shifts(cells, model["n_bound"])


def test_single_node_under_the_identity_reproduces_itself(N, planar):
    dst = N.MapSet(RES, [0, 0, 0], W.NODE_SIZE_M, n_maps=1, max_cells=CAP)
    res, = N.assemble_world(dst, 0, planar["src"], [[0]], [np.eye(4)[None]])
    smean, scov, sidx, sn = exported(planar["src"], 0)
    mean, cov, idx, n = exported(dst)
    assert sn.shape[0] > 10 and np.array_equal(idx, sidx) and np.array_equal(n, sn)
    assert res["n_nodes"] == 1 and res["n_cells"] == res["n_contributions"] == sn.shape[0] and res["n_points"] == int(sn.sum())
    assert res["n_dropped"] == res["n_rejected"] == res["overflow"] == 0
    worst = [0.0, 0.0, 0]
    for k in range(sn.shape[0]):
        mb, cb = W.error_bounds(res["s1_shift"], res["s2_shift"], int(sn[k]), 1, RES, NODE_CELLS)
        dm, dc = np.abs(mean[k] - smean[k]).max(), np.abs(cov[k] - scov[k]).max()
        if dm / mb > worst[0]:
            worst = [dm / mb, worst[1], int(sn[k])]
        worst[1] = max(worst[1], dc / cb)
    print("identity: largest error / bound: mean %.3g (a cell of %d points), covariance %.3g over %d cells" % (worst[0], worst[2], worst[1], sn.shape[0]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_three_overlapping_planar_nodes_against_the_model(N, planar):
    dst = world_set(N)
    res, = N.assemble_world(dst, 0, planar["src"], [[0, 1, 2]], [np.stack(planar["poses"])])
    model = W.assemble(planar["nodes"], planar["poses"], RES, [0, 0, 0], WORLD_CELLS, shifts=(res["s1_shift"], res["s2_shift"]))
    assert max(c["count"] for c in model["cells"].values()) >= 2 and res["n_nodes"] == 3 and res["overflow"] == 0
    compare_with_model(dst, 0, res, model, WORLD_CELLS)


def test_order_and_batch_independence(N, planar):
    perms = list(itertools.permutations(range(3)))
    dst = world_set(N, n_maps=7)
    lists = [list(p) for p in perms]
    Ts = [np.stack([planar["poses"][k] for k in p]) for p in perms]
    res = N.assemble_world(dst, 0, planar["src"], lists, Ts)
    ref = as_bytes(dst, 0)
    assert len(ref) > 0 and all(as_bytes(dst, w) == ref for w in range(6))
    assert all(r["n_cells"] == res[0]["n_cells"] and r["s2_shift"] == res[0]["s2_shift"] for r in res)
    for p, T in zip(lists, Ts):                                   # each order alone, into another map
        N.assemble_world(dst, 6, planar["src"], [p], [T])
        assert as_bytes(dst, 6) == ref
    N.assemble_world(dst, 0, planar["src"], lists, Ts)            # and the batch again, over its own result
    assert all(as_bytes(dst, w) == ref for w in range(6))


def test_a_6dof_pose_in_3d_against_the_model(N):
    rng = np.random.default_rng(12)
    size_m = [6.0, 6.0, 3.0]                                       # 12 x 12 x 6 cells
    cells = W.grid_cells(RES, size_m)
    assert cells == [12, 12, 6]
    # three noisy planes through the box
    pts = []
    for normal, off in (((0.1, 0.2, 1.0), -0.6), ((1.0, 0.1, 0.2), 1.1), ((0.2, 1.0, -0.1), -0.9)):
        nrm = np.asarray(normal) / np.linalg.norm(normal)
        p = rng.uniform(-3, 3, (3000, 3)) * [1, 1, 0.5]
        p += (off - p @ nrm)[:, None] * nrm + rng.normal(0, 0.02, (3000, 3))
        pts.append(p)
    pts = np.concatenate(pts).astype(np.float32)
    src = N.MapSet(RES, [0, 0, 0], size_m, n_maps=1, max_cells=CAP)
    src.build(pts[None])
    mean, cov, _, n = src.export_cells(0)
    assert mean.shape[0] > 100
    r, p, y = 0.2, -0.15, 0.7
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = [0.13, -0.21, 0.07]
    dst = N.MapSet(RES, [0, 0, 0], size_m, n_maps=1, max_cells=CAP)
    res, = N.assemble_world(dst, 0, src, [[0]], [T[None]])
    model = W.assemble([(mean, cov, n)], [T], RES, [0, 0, 0], cells, shifts=(res["s1_shift"], res["s2_shift"]))
    assert model["n_dropped"] > 0 and len(model["cells"]) > 50
    compare_with_model(dst, 0, res, model, cells)


def test_drop_and_overflow(N, planar):
    # the world ends at x = 24: the node is put there with its median cell, so about half of it leaves the world
    T = W.pose2d(24.0 - float(np.median(planar["nodes"][0][0][:, 0])) + 0.013, 0.3, 0.0)
    dst = world_set(N)
    res, = N.assemble_world(dst, 0, planar["src"], [[0]], [T[None]])
    model = W.assemble(planar["nodes"][:1], [T], RES, [0, 0, 0], WORLD_CELLS, shifts=(res["s1_shift"], res["s2_shift"]))
    n0 = planar["nodes"][0][0].shape[0]
    assert 0.2 * n0 < model["n_dropped"] < 0.8 * n0 and res["n_dropped"] == model["n_dropped"]
    compare_with_model(dst, 0, res, model, WORLD_CELLS)
    assert dst.counters(0)["n_dropped"] == res["n_dropped"] + res["n_rejected"]
    # a destination with room for 8 cells: reported like a build reports it, and the process lives
    small = world_set(N, max_cells=8)
    res, = N.assemble_world(small, 0, planar["src"], [[0, 1, 2]], [np.stack(planar["poses"])])
    assert res["overflow"] == 1 and small.counters(0)["overflow"] == 1
    with pytest.raises(N.NdtGpuError) as e:
        small.num_cells(0)
    assert e.value.status == -4
    built = world_set(N, max_cells=8)
    built.build(W.planar_scans()[:1])
    assert built.counters(0)["overflow"] == 1                      # (the same scan, the same capacity: the build's own report)
    # the map is usable again afterwards
    res, = N.assemble_world(small, 0, planar["src"], [[]], [np.zeros((0, 4, 4))])
    assert res["overflow"] == 0 and small.num_cells(0) == 0


def test_empty_worlds_leave_a_clean_map(N, planar):
    dst = world_set(N, n_maps=2)
    N.assemble_world(dst, 0, planar["src"], [[0, 1, 2], [2, 1]], [np.stack(planar["poses"]), np.stack(planar["poses"][:2])])
    assert dst.num_cells(0) > 0 and dst.num_cells(1) > 0
    res = N.assemble_world(dst, 0, planar["src"], [[], [3]], [np.zeros((0, 4, 4)), np.eye(4)[None]])
    assert [r["n_cells"] for r in res] == [0, 0] and [r["n_nodes"] for r in res] == [0, 1]
    assert all(r["n_contributions"] == r["n_points"] == r["overflow"] == 0 for r in res)
    assert dst.num_cells(0) == 0 and dst.num_cells(1) == 0
    # the rank map and the scratch are clean: a plain build on these maps gives what it gives on a fresh set
    scans = W.planar_scans()[:2]
    dst.build(scans)
    fresh = world_set(N, n_maps=2)
    fresh.build(scans)
    assert dst.num_cells(0) > 0 and all(as_bytes(dst, i) == as_bytes(fresh, i) for i in range(2))


def test_set_cells_sources_merge_as_two_points_each(N):
    src = N.MapSet(RES, [0, 0, 0], W.NODE_SIZE_M, n_maps=2, max_cells=64)
    cA = np.diag([0.004, 0.002, 0.001])
    cB = np.array([[0.003, 0.001, 0.0], [0.001, 0.002, 0.0], [0.0, 0.0, 0.0015]])
    src.set_cells(0, np.array([[1.0, 1.0, 0.0]]), cA[None])
    src.set_cells(1, np.array([[1.1, 0.9, 0.01], [3.0, 3.0, 0.0]]), np.stack([cB, 50.0 * np.eye(3)]))
    assert list(src.export_cells(0)[3]) == [1] and list(src.export_cells(1)[3]) == [1, 1]     # set_cells installs n = 1
    dst = world_set(N, n_maps=2)
    eye2 = np.stack([np.eye(4)] * 2)
    res, = N.assemble_world(dst, 0, src, [[0, 1]], [eye2])
    # the cell with a covariance beyond the documented bound ((n - 1) |Sigma| / res^2 <= 12 n on this grid: 6 m^2) is rejected
    assert (res["n_contributions"], res["n_rejected"], res["n_dropped"], res["n_points"], res["n_cells"]) == (3, 1, 0, 4, 1)
    nodes = [tuple(src.export_cells(i)[k] for k in (0, 1, 3)) for i in range(2)]
    model = W.assemble(nodes, [np.eye(4)] * 2, RES, [0, 0, 0], WORLD_CELLS, shifts=(res["s1_shift"], res["s2_shift"]))
    assert model["n_rejected"] == 1 and next(iter(model["cells"].values()))["N"] == 4
    compare_with_model(dst, 0, res, model, WORLD_CELLS)
    assert list(dst.export_cells(0)[3]) == [4]
    # ... and nothing else changes: without the rejected cell the world is the same bits
    src.set_cells(1, np.array([[1.1, 0.9, 0.01]]), cB[None])
    res2, = N.assemble_world(dst, 1, src, [[0, 1]], [eye2])
    assert res2["n_rejected"] == 0 and as_bytes(dst, 1) == as_bytes(dst, 0)


def test_a_localisation_bank_consumes_the_world(N):
    seed, pa, pb, truth = 3, (-6.0, -2.0, 0.1), (6.0, 2.0, -0.2), (12.0, 3.0, 0.3)     # node grids of 20 m: neither covers the other's far side
    src = N.MapSet(RES, [0, 0, 0], W.NODE_SIZE_M, n_maps=2, max_cells=CAP)
    src.build(W.planar_scans(poses=[pa, pb], seed=seed))
    dst = world_set(N, n_maps=2)
    Ts = np.stack([W.pose2d(*pa), W.pose2d(*pb)])
    res = N.assemble_world(dst, 0, src, [[0, 1], [0]], [Ts, Ts[:1]])
    assert res[0]["n_cells"] > res[1]["n_cells"] > 0
    scan = W.planar_scans(n_points=4000, poses=[truth], seed=seed)
    quiet = dict(motion_model=np.zeros(36), motion_model_offset=np.zeros(6), sir_varp_threshold=1e9, sir_max_iters_wo_resampling=1 << 30)
    f = N.MCL(dst, [0, 1], 16, scan_size=[16.0, 16.0, 1.0], max_scan_cells=CAP, seed=7, **quiet)
    f.set_particles(np.tile(W.pose2d(*truth), (2, 16, 1, 1)))
    f.update(np.stack([np.eye(4)] * 2), np.concatenate([scan, scan]))
    _, r = f.mean()
    assert r["terms"][0] > 0 and np.isfinite(r["lik_sum"][0])       # in the part of the world that only node 1 covers
    assert r["terms"][1] == 0                                       # the world of node 0 alone has nothing there
    f.close()


def test_a_call_leaves_no_resources_behind(N, planar):
    dst = world_set(N)
    fine = N.MapSet(0.25, [0, 0, 0], [8.0, 8.0, 0.25], n_maps=1)
    N.assemble_world(dst, 0, planar["src"], [[0]], [np.eye(4)[None]])          # (anything the sets allocate lazily exists now)
    before = N.binding.live_resources()
    N.assemble_world(dst, 0, planar["src"], [[0, 1, 2]], [np.stack(planar["poses"])])
    assert N.binding.live_resources() == before
    with pytest.raises(N.NdtGpuError) as e:
        N.assemble_world(dst, 0, planar["src"], [[0, 9]], [np.stack(planar["poses"][:2])])
    assert e.value.status == -1 and N.binding.live_resources() == before
    with pytest.raises(N.NdtGpuError) as e:                                     # the same set, a destination among the nodes
        N.assemble_world(planar["src"], 3, planar["src"], [[0, 3]], [np.stack(planar["poses"][:2])])
    assert e.value.status == -1 and N.binding.live_resources() == before
    with pytest.raises(N.NdtGpuError) as e:
        N.assemble_world(fine, 0, planar["src"], [[0]], [np.eye(4)[None]])
    assert e.value.status == -1 and b"res" in N.lib().ndtgpu_last_error()
