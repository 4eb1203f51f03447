"""The fuser bank's feature path on the device (-m gpu): ndtgpu_fuser_initialize_batch_feat / ndtgpu_fuser_update_batch_feat
(ndt_feature_fuser_hmt.cpp:78-85, 245-334, 497-502) against the calls they replace, slot by slot and update by update.

Shape: 3 fusers, clouds of 2 000 points, the node maps of tests/test_gpu_fuser_bank.py, 5 updates after initialize, so that the map
append at counter 4 is crossed.  The interest points are hand-made (fuserfeat_model.hand_made_pair's construction): K = 24 points
fixed in the map frame, seen from every pose of the path with 1e-3 m of noise, descriptors equal at every step -- real scans carry
6 to 9 points and always end TOO_FEW at the default inlier_probability (the chained test below runs exactly that case).
What is compared bit for bit: the RANSAC record, T16 and corr with FeatureMatcher.match_device on (prev, cur); the cells with
ndtgpu_fuser_feat_prepare on the read-back inputs; the registered increment and the matcher's deterministic fields with
ndtgpu_match_fusion_feat_batch driven by hand with those cells; the descriptors and x, y of the moved points with
tests/fuserfeat_model.py (theta to 1e-12 rad: libm's cos / sin / atan2 on the two sides)."""
import ctypes
import math

import numpy as np
import pytest

import fuserfeat_model as M
from test_gpu_fuser_bank import DET_FIELDS, NODE_SIZE, RANGE, RES, cells_bits_equal, init_pose, mm, move_cloud, node_centres, pose2d

pytestmark = pytest.mark.gpu

NPTS, BN, K, MP = 2000, 3, 24, 64
SENSOR = pose2d(0.25, -0.05, 0.02)
CUR0, PREV0, MAP0 = 0, BN, 2 * BN                       # the feature bank's sets: cur | prev | map, one of each per slot


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def world():
    """per fuser a room and a short path (computed once, shared, not modified): the scans, the odometry increments, and the
    interest points of every step -- K points fixed in the map frame, seen from the sensor"""
    import torch
    from ndt_feature_graph_amd import synth
    n_steps = 5
    rng = np.random.default_rng(17)
    seeds = np.arange(7100, 7100 + BN)
    poses = np.zeros((n_steps + 1, BN, 3))
    poses[0, :, :2] = rng.uniform(-1.0, 1.0, size=(BN, 2))
    poses[0, :, 2] = rng.uniform(-0.3, 0.3, size=BN)
    for s in range(1, n_steps + 1):
        step = np.stack([rng.uniform(0.15, 0.35, BN), rng.uniform(-0.08, 0.08, BN), rng.uniform(-0.06, 0.06, BN)], axis=1)
        for k in range(BN):
            c, sn = math.cos(poses[s - 1, k, 2]), math.sin(poses[s - 1, k, 2])
            poses[s, k, 0] = poses[s - 1, k, 0] + c * step[k, 0] - sn * step[k, 1]
            poses[s, k, 1] = poses[s - 1, k, 1] + sn * step[k, 0] + c * step[k, 1]
            poses[s, k, 2] = poses[s - 1, k, 2] + step[k, 2]
    scans = [synth.scan_2d(torch.as_tensor(seeds), torch.as_tensor(poses[s]), NPTS, noise_stream=s).numpy() for s in range(n_steps + 1)]
    Tm = np.zeros((n_steps, BN, 4, 4))
    for s in range(n_steps):
        for k in range(BN):
            true = np.linalg.inv(pose2d(*poses[s, k])) @ pose2d(*poses[s + 1, k])
            Tm[s, k] = true @ pose2d(rng.normal(0, 0.03), rng.normal(0, 0.02), rng.normal(0, 0.01))
    feats, descs = [], []
    for k in range(BN):
        w, _, desc, _ = M.hand_made_pair(K, 40 + k)
        w[:, :2] += [1.0, -1.6]                                          # (in front of the robot)
        descs.append(desc)
        per_step = []
        for s in range(n_steps + 1):
            Tmap = init_pose(k) @ np.linalg.inv(pose2d(*poses[0, k])) @ pose2d(*poses[s, k]) @ SENSOR
            Ti = np.linalg.inv(Tmap)
            yaw = math.atan2(Tmap[1, 0], Tmap[0, 0])
            p = np.zeros((K, 3))
            p[:, 0] = Ti[0, 0] * w[:, 0] + Ti[0, 1] * w[:, 1] + Ti[0, 3]
            p[:, 1] = Ti[1, 0] * w[:, 0] + Ti[1, 1] * w[:, 1] + Ti[1, 3]
            p[:, :2] += rng.uniform(-1e-3, 1e-3, size=(K, 2))
            p[:, 2] = np.arctan2(np.sin(w[:, 2] - yaw), np.cos(w[:, 2] - yaw))
            per_step.append(p)
        feats.append(per_step)
    return dict(n_steps=n_steps, scans=scans, Tm=Tm, feats=feats, descs=descs)


def fuser_fields(**more):
    f = dict(resolution=RES, map_size_x=NODE_SIZE[0], map_size_y=NODE_SIZE[1], map_size_z=NODE_SIZE[2], sensor_range=RANGE, neighbours=2,
             delta_score=1e-6, max_cells=4096, sensor_pose=SENSOR)
    f.update(more)
    return f


class Rig:
    """a fuser bank with a feature bank attached: sets [0, n) cur, [n, 2n) prev, [2n, 3n) map"""

    def __init__(self, N, n=BN, max_points=MP, fields=None, **feat_params):
        self.N, self.n = N, n
        self.prm = N.fuser_params(**fuser_fields(**(fields or {})))
        self.bank = N.FuserBank(self.prm, n)
        self.fm = N.FeatureMatcher(3 * n, max_points, 48)
        self.bank.attach_features(self.fm, n, 2 * n, **feat_params)
        self.fprm = self.bank.feat_params

    def stage(self, world, s, slots=None):
        for k in (range(self.n) if slots is None else slots):
            self.fm.set(k, world["feats"][k][s], world["descs"][k])

    def close(self):
        self.bank.close()
        self.fm.close()


def cloud(world, s, lo=0, hi=BN):
    import torch
    return torch.as_tensor(world["scans"][s][lo:hi], device="cuda").contiguous()


def ransac_by_hand(N, fm, ref_sets, mov_sets, **params):
    """FeatureMatcher.match_device -> (records, T16 [n, 16], corr [n, max_points, 2])"""
    import torch
    from ndt_feature_graph_amd import binding
    n = len(ref_sets)
    ri = torch.as_tensor(np.asarray(ref_sets, dtype=np.int32), device="cuda")
    mi = torch.as_tensor(np.asarray(mov_sets, dtype=np.int32), device="cuda")
    res = torch.zeros(n * ctypes.sizeof(binding.FeatMatchResult), dtype=torch.uint8, device="cuda")
    T16 = torch.zeros((n, 16), dtype=torch.float64, device="cuda")
    corr = torch.zeros((n, fm.max_points, 2), dtype=torch.int32, device="cuda")
    fm.match_device(ri, mi, res, T16, corr, **params)
    torch.cuda.synchronize()
    return (np.frombuffer(res.cpu().numpy().tobytes(), dtype=binding.FEATMATCH_RESULT_DTYPE), T16.cpu().numpy(),
            corr.cpu().numpy().view(np.uint32))


def check_state(rig, world, s, T_move, rec, n_map_want, moved=True):
    """prev holds cur's descriptors bit for bit and the model's move of its positions; the counts are the sets'"""
    for k in range(rig.n):
        cur_p, cur_d = rig.fm.get(CUR0 + k)
        prev_p, prev_d = rig.fm.get(PREV0 + k)
        map_p, map_d = rig.fm.get(MAP0 + k)
        assert np.array_equal(cur_p, world["feats"][k][s]) and np.array_equal(cur_d, world["descs"][k]), "cur is read only"
        assert np.array_equal(prev_d, cur_d), (s, k)
        want = M.move(T_move[k], cur_p) if moved else cur_p
        assert np.array_equal(prev_p[:, :2], want[:, :2]), (s, k)
        d = np.abs(prev_p[:, 2] - want[:, 2])
        assert float(np.max(np.minimum(d, 2 * math.pi - d))) <= 1e-12, (s, k)
        assert int(rec["n_prev"][k]) == prev_p.shape[0] == K
        assert int(rec["n_map"][k]) == map_p.shape[0] == n_map_want, (s, k, int(rec["n_map"][k]), map_p.shape[0], n_map_want)
        if int(rec["map_appended"][k]):
            a = int(rec["map_appended"][k])
            assert np.array_equal(map_p[-a:], prev_p[:a]) and np.array_equal(map_d[-a:], prev_d[:a])


@pytest.mark.parametrize("prev_in_map_frame", [0, 1])
def test_feature_path_equals_the_calls_it_replaces(N, world, prev_in_map_frame):
    import torch
    from ndt_feature_graph_amd import binding
    rig = Rig(N, prev_in_map_frame=prev_in_map_frame)
    prm, bank, fm = rig.prm, rig.bank, rig.fm
    nodes, scan_maps = bank.mapsets()
    ref_nodes = N.MapSet(RES, [0, 0, 0], NODE_SIZE, n_maps=BN, max_cells=4096)
    ref_nodes.enable_occupancy()
    local = RANGE + 3 * RES
    ref_scans = N.MapSet(RES, [0, 0, 0], [local, local, NODE_SIZE[2]], n_maps=BN, max_cells=4096)
    Tnow = [init_pose(k) for k in range(BN)]
    rig.stage(world, 0)
    bank.initialize(np.stack(Tnow), cloud(world, 0), cur_sets=np.arange(BN))
    rec = bank.feat_results()
    moved = np.stack([move_cloud(Tnow[k], move_cloud(SENSOR, world["scans"][0][k])) for k in range(BN)])
    for k in range(BN):
        ref_nodes.set_centre(k, [Tnow[k][0, 3], Tnow[k][1, 3], 0.0])
    ref_nodes.add_cloud(torch.as_tensor(moved, device="cuda").contiguous(), np.stack([mm(Tnow[k], SENSOR)[:3, 3] for k in range(BN)]),
                        maxz=100.0, sensor_noise=0.1)
    torch.cuda.synchronize()
    for k in range(BN):
        cells_bits_equal(nodes.export_cells(k), ref_nodes.export_cells(k), "node map %d after initialize" % k)
    check_state(rig, world, 0, [mm(Tnow[k], SENSOR) for k in range(BN)], rec, K)
    assert all(int(rec["map_appended"][k]) == K and int(rec["ransac_run"][k]) == 0 for k in range(BN))
    n_map = K
    ok_records = 0
    for s in range(world["n_steps"]):
        upd = s + 1
        rig.stage(world, upd)
        # -- the RANSAC by hand on (prev, cur) BEFORE the call replaces prev, and the inputs of the cells
        r_h, T16_h, corr_h = ransac_by_hand(N, fm, [PREV0 + k for k in range(BN)], [CUR0 + k for k in range(BN)])
        prev_before = [fm.get(PREV0 + k)[0] for k in range(BN)]
        bank.update(world["Tm"][s], cloud(world, upd), cur_sets=np.arange(BN))
        T_b, r_b = bank.poses()
        rec = bank.feat_results()
        cells = bank.feat_cells()
        feat = []
        for k in range(BN):
            what = "update %d, fuser %d" % (upd, k)
            assert rec["ransac"][k].tobytes() == r_h[k].tobytes(), what
            assert int(rec["ransac_run"][k]) == 1
            n_in = int(r_h["n_inliers"][k])
            # Tfeat = T16 * sensor_pose^-1 and the cells: ndtgpu_fuser_feat_prepare on the read-back inputs
            rec_h, cells_h = N.fuser_feat_prepare(prm, rig.fprm, Tnow[k], world["Tm"][s, k], r_h[k], corr_h[k, :n_in], world["feats"][k][upd],
                                                  prev_before[k], prev_moved=True)
            T_h = T16_h[k].reshape(4, 4).T
            assert np.array_equal(T_h, M.T_of_record(r_h[k])), what                   # (T16 is the 4x4 of (c, s, x, y))
            assert np.array_equal(rec["Tfeat"][k], rec_h["Tfeat"][0]), what
            for f in ("consistent", "n_feat_cells", "n_odom_cells", "truncated"):
                assert int(rec[f][k]) == int(rec_h[f][0]), (what, f)
            assert cells[k].shape == cells_h.shape and np.array_equal(cells[k], cells_h), what
            ok_records += int(r_h["status"][k] == 0 and n_in == K)
            feat.append((cells[k][:, 0:3], cells[k][:, 3:9], cells[k][:, 9:12], cells[k][:, 12:18]))
        # -- matchFusion by hand with those cells and the inputs of ndtgpu_fuser_prepare (tests/test_gpu_fuser_bank.py's method)
        pps = [N.fuser_prepare(prm, Tnow[k], world["Tm"][s, k], node_centres(BN)[k]) for k in range(BN)]
        in_node = np.stack([move_cloud(np.array(pps[k]["Tscan"]).reshape(4, 4).T, world["scans"][upd][k]) for k in range(BN)])
        for k in range(BN):
            ref_scans.set_centre(k, pps[k]["scan_centre"])
        ref_scans.build(torch.as_tensor(in_node, device="cuda").contiguous(), range_limit=RANGE,
                        range_origins=np.stack([pps[k]["range_origin"] for k in range(BN)]))
        idx = np.arange(BN)
        Tcov = np.stack([pps[k]["Tcov"].reshape(6, 6) for k in range(BN)])
        T_est, r = binding.match_fusion_feat_batch(ref_nodes, idx, ref_scans, idx, world["Tm"][s], Tcov, feat, use_soft_constraints=True,
                                                   tikhonov=True, step_control_fusion=True, n_neighbours=2, itr_max=30, delta_score=1e-6,
                                                   step_control=1)
        spose = []
        for k in range(BN):
            what = "update %d, fuser %d" % (upd, k)
            assert np.array_equal(r_b["Tmotion_est"][k].reshape(4, 4).T, T_est[k]), what
            for f in DET_FIELDS:
                assert r_b["match"][f][k] == r[f][k], (what, f)
            Tn = mm(Tnow[k], T_est[k]) if r["converged"][k] else mm(Tnow[k], world["Tm"][s, k])
            assert np.array_equal(T_b[k], Tn), what
            spose.append(mm(Tn, SENSOR))
            assert np.array_equal(r_b["spose"][k].reshape(4, 4).T, spose[k]), what
            Tnow[k] = Tn
        fused = np.stack([move_cloud(spose[k], world["scans"][upd][k]) for k in range(BN)])
        ref_nodes.add_cloud(torch.as_tensor(fused, device="cuda").contiguous(), np.stack([sp[:3, 3] for sp in spose]), maxz=25.0, sensor_noise=0.06)
        torch.cuda.synchronize()
        for k in range(BN):
            cells_bits_equal(nodes.export_cells(k), ref_nodes.export_cells(k), "node map, update %d, fuser %d" % (upd, k))
        # -- the state: map grows at initialize and at update 4 only
        if upd == 4:
            n_map += K
        check_state(rig, world, upd, spose, rec, n_map)
        assert all(int(rec["map_appended"][k]) == (K if upd == 4 else 0) and int(rec["map_overflow"][k]) == 0 for k in range(BN))
    print("prev_in_map_frame %d: %d of %d RANSAC records OK with %d inliers; cells per slot %s" %
          (prev_in_map_frame, ok_records, BN * world["n_steps"], K, [c.shape[0] for c in cells]))
    assert ok_records == BN * world["n_steps"], "the fixture was meant to give K inliers at every update"
    assert all(c.shape[0] == 64 for c in cells)
    rig.close()


def test_update_feature_map_off_and_the_plain_entries(N, world):
    """update_feature_map = 0 leaves prev unmoved and the counter still; a plain update on an attached bank leaves prev and map
    untouched"""
    rig = Rig(N)
    bank, fm = rig.bank, rig.fm
    rig.stage(world, 0)
    bank.initialize(np.stack([init_pose(k) for k in range(BN)]), cloud(world, 0), cur_sets=np.arange(BN))
    rig.stage(world, 1)
    bank.update(world["Tm"][0], cloud(world, 1), cur_sets=np.arange(BN), update_feature_map=False)
    rec = bank.feat_results()
    check_state(rig, world, 1, None, rec, K, moved=False)
    assert all(int(rec["map_appended"][k]) == 0 for k in range(BN))
    # four updates with the map: the counter stood at 1, so the append comes with the fourth
    for j, s in enumerate((2, 3, 4, 5)):
        rig.stage(world, s)
        bank.update(world["Tm"][s - 1], cloud(world, s), cur_sets=np.arange(BN))
        _, r_b = bank.poses()
        rec = bank.feat_results()
        want = K if j == 3 else 0
        assert [int(x) for x in rec["map_appended"]] == [want] * BN, (j, rec["map_appended"])
        check_state(rig, world, s, [r_b["spose"][k].reshape(4, 4).T for k in range(BN)], rec, 2 * K if j == 3 else K)
    # a plain update: the feature state stays, and there are no feature records
    before = [(fm.get(PREV0 + k), fm.get(MAP0 + k)) for k in range(BN)]
    bank.update(world["Tm"][4], cloud(world, 5))
    bank.poses()
    for k in range(BN):
        (pp, pd), (mp, md) = before[k]
        p2, m2 = fm.get(PREV0 + k), fm.get(MAP0 + k)
        assert np.array_equal(p2[0], pp) and np.array_equal(p2[1], pd) and np.array_equal(m2[0], mp) and np.array_equal(m2[1], md)
    assert not bank.feat_results().tobytes().strip(b"\0")
    assert [c.shape[0] for c in bank.feat_cells()] == [40] * BN           # (the plain entry's own odometry cells)
    rig.close()


def test_map_overflow(N, world):
    """max_points = 32, K = 24: the second append keeps 8 points, sets map_overflow, and leaves the neighbouring sets alone"""
    n = 1
    prm = N.fuser_params(**fuser_fields())
    bank = N.FuserBank(prm, n)
    fm = N.FeatureMatcher(5, 32, 48)                    # 0 cur | 1 prev | 2 guard | 3 map | 4 guard
    rng = np.random.default_rng(3)
    guards = {g: (rng.uniform(-5, 5, (32, 3)), rng.uniform(0.1, 1.0, (32, 48))) for g in (2, 4)}
    for g, (p, d) in guards.items():
        fm.set(g, p, d)
    bank.attach_features(fm, 1, 3)
    fm.set(0, world["feats"][0][0], world["descs"][0])
    bank.initialize(init_pose(0)[None], cloud(world, 0, 0, 1), cur_sets=[0])
    first = fm.get(3)
    assert first[0].shape[0] == K
    for s in range(1, 5):
        fm.set(0, world["feats"][0][s], world["descs"][0])
        bank.update(world["Tm"][s - 1][:1], cloud(world, s, 0, 1), cur_sets=[0])
        rec = bank.feat_results()
        assert int(rec["map_overflow"][0]) == (1 if s == 4 else 0)
    assert int(rec["map_appended"][0]) == 8 and int(rec["n_map"][0]) == 32 and int(rec["n_prev"][0]) == K
    mp, md = fm.get(3)
    pp, pd = fm.get(1)
    assert mp.shape[0] == 32
    assert np.array_equal(mp[:K], first[0]) and np.array_equal(md[:K], first[1])
    assert np.array_equal(mp[K:], pp[:8]) and np.array_equal(md[K:], pd[:8])          # the first points that fit
    for g, (p, d) in guards.items():
        gp, gd = fm.get(g)
        assert np.array_equal(gp, p) and np.array_equal(gd, d), "set %d next to the map set changed" % g
    # a fifth update appends nothing more (the counter is 5) and reports no overflow
    fm.set(0, world["feats"][0][5], world["descs"][0])
    bank.update(world["Tm"][4][:1], cloud(world, 5, 0, 1), cur_sets=[0])
    rec = bank.feat_results()
    assert int(rec["map_appended"][0]) == 0 and int(rec["map_overflow"][0]) == 0 and int(rec["n_map"][0]) == 32
    # arguments: a cur index inside the prev / map ranges or outside the bank; ranges that overlap or leave the bank
    for bad in ([1], [3], [5]):
        with pytest.raises(N.NdtGpuError) as e:
            bank.update(world["Tm"][0][:1], cloud(world, 1, 0, 1), cur_sets=bad)
        assert e.value.status == -1
    for prev_first, map_first in ((1, 1), (5, 0), (0, 5)):
        with pytest.raises(N.NdtGpuError):
            bank.attach_features(fm, prev_first, map_first)
    plain = N.FuserBank(prm, 1)
    with pytest.raises(N.NdtGpuError):                  # no feature bank attached
        plain.initialize(init_pose(0)[None], cloud(world, 0, 0, 1), cur_sets=[0])
    plain.close()
    bank.close()
    fm.close()


def snapshot(rig, k):
    T, r = rig.bank.poses(k, 1)
    rec = rig.bank.feat_results(k, 1)
    cells = rig.bank.feat_cells(k, 1)[0]
    nodes, _ = rig.bank.mapsets()
    return dict(T=T[0], r={f: r[f][0] for f in ("Tnow", "Tmotion_est", "spose", "match_ok", "registration_failure", "posecov")},
                det=[r["match"][f][0] for f in DET_FIELDS], rec=rec.tobytes(), cells=cells, node=nodes.export_cells(k),
                prev=rig.fm.get(PREV0 + k), map=rig.fm.get(MAP0 + k))


def same(a, b, what):
    assert np.array_equal(a["T"], b["T"]), what
    for f in a["r"]:
        assert np.array_equal(a["r"][f], b["r"][f]), (what, f)
    assert a["det"] == b["det"] and a["rec"] == b["rec"], what
    assert np.array_equal(a["cells"], b["cells"]), what
    cells_bits_equal(a["node"], b["node"], what)
    for s in ("prev", "map"):
        assert np.array_equal(a[s][0], b[s][0]) and np.array_equal(a[s][1], b[s][1]), (what, s)


def test_a_slot_does_not_depend_on_its_batch(N, world):
    """a slot run alone (count = 1, first = k) gives the bits it gives in the batch of 3"""
    batch, alone = Rig(N), Rig(N)
    T0 = np.stack([init_pose(k) for k in range(BN)])
    for rig in (batch, alone):
        rig.stage(world, 0)
    batch.bank.initialize(T0, cloud(world, 0), cur_sets=np.arange(BN))
    for k in (2, 0, 1):
        alone.bank.initialize(T0[k:k + 1], cloud(world, 0, k, k + 1), first=k, cur_sets=[k])
    for s in (1, 2):
        for rig in (batch, alone):
            rig.stage(world, s)
        batch.bank.update(world["Tm"][s - 1], cloud(world, s), cur_sets=np.arange(BN))
        snaps = [snapshot(batch, k) for k in range(BN)]
        for k in (1, 2, 0):
            alone.bank.update(world["Tm"][s - 1][k:k + 1], cloud(world, s, k, k + 1), first=k, cur_sets=[k])
            same(snapshot(alone, k), snaps[k], "update %d, slot %d" % (s, k))
    batch.close()
    alone.close()


@pytest.mark.parametrize("use_odom", [1, 0])
def test_without_features_the_feat_entries_are_the_plain_ones(N, world, use_odom):
    """empty cur sets: poses, results and node-map cells of the _feat entries are the plain entries' bits"""
    feat = Rig(N, fields=dict(use_odom=use_odom))
    plain = N.FuserBank(feat.prm, BN)
    T0 = np.stack([init_pose(k) for k in range(BN)])
    feat.bank.initialize(T0, cloud(world, 0), cur_sets=np.arange(BN))          # (every set of the bank starts empty)
    plain.initialize(T0, cloud(world, 0))
    for s in (1, 2):
        feat.bank.update(world["Tm"][s - 1], cloud(world, s), cur_sets=np.arange(BN))
        plain.update(world["Tm"][s - 1], cloud(world, s))
        Ta, ra = feat.bank.poses()
        Tb, rb = plain.poses()
        assert np.array_equal(Ta, Tb)
        for f in ("Tnow", "Tmotion_est", "spose", "match_ok", "registration_failure", "cov_singular", "posecov_mean", "posecov"):
            assert np.array_equal(ra[f], rb[f]), (s, f)
        for f in DET_FIELDS:
            assert np.array_equal(ra["match"][f], rb["match"][f]), (s, f)
        na, _ = feat.bank.mapsets()
        nb, _ = plain.mapsets()
        for k in range(BN):
            cells_bits_equal(na.export_cells(k), nb.export_cells(k), "node map %d, update %d" % (k, s))
        rec = feat.bank.feat_results()
        assert all(int(x) == 1 for x in rec["ransac"]["status"]) and not rec["consistent"].any()      # TOO_FEW: an empty set
        assert [int(x) for x in rec["n_odom_cells"]] == [40 * use_odom] * BN and not rec["n_feat_cells"].any()
        ca, cb = feat.bank.feat_cells(), plain.feat_cells()
        for k in range(BN):
            assert np.array_equal(ca[k], cb[k]) and ca[k].shape[0] == 40 * use_odom
    feat.close()
    plain.close()


def test_extract_and_update_chained_on_one_stream(N, world):
    """extract_device -> update_batch_feat on one stream with no host synchronisation equals the same calls with one in between.
    Real scans carry too few points for the default inlier_probability: the records are TOO_FEW, which is the case's point"""
    import torch
    from ndt_feature_graph_amd import binding
    import flirt_fixtures as X
    rows = [X.hall(21 + 7 * s + k, 360) for s in range(3) for k in range(BN)]
    a0, inc = rows[0][1], rows[0][2]
    ranges = [torch.as_tensor(np.stack([rows[s * BN + k][0] for k in range(BN)]), device="cuda").contiguous() for s in range(3)]
    sets = torch.as_tensor(np.arange(BN, dtype=np.int32), device="cuda")
    T0 = np.stack([init_pose(k) for k in range(BN)])
    clouds = [cloud(world, s) for s in range(3)]
    out = []
    for sync in (True, False):
        rig = Rig(N)
        st = torch.cuda.Stream()
        res = torch.zeros(BN * ctypes.sizeof(binding.FeatExtractResult), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for s in range(3):
            rig.fm.extract_device(sets, ranges[s], a0, inc, res, stream=st)
            if sync:
                torch.cuda.synchronize()
            if s == 0:
                rig.bank.initialize(T0, clouds[0], cur_sets=np.arange(BN), stream=st)
            else:
                rig.bank.update(world["Tm"][s - 1], clouds[s], cur_sets=np.arange(BN), stream=st)
            if sync:
                torch.cuda.synchronize()
        T, r = rig.bank.poses()
        rec = rig.bank.feat_results()
        out.append(dict(T=T, est=r["Tmotion_est"].copy(), rec=rec.tobytes(), status=[int(x) for x in rec["ransac"]["status"]],
                        n_prev=[int(x) for x in rec["n_prev"]], sets=[rig.fm.get(j) for j in range(3 * BN)]))
        rig.close()
    a, b = out
    assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["est"], b["est"]) and a["rec"] == b["rec"]
    for (pa, da), (pb, db) in zip(a["sets"], b["sets"]):
        assert np.array_equal(pa, pb) and np.array_equal(da, db)
    print("chained: RANSAC status %s, points per scan %s" % (a["status"], a["n_prev"]))
    assert a["status"] == [1] * BN                      # NDTGPU_FEATMATCH_TOO_FEW
    assert all(1 <= n < 20 for n in a["n_prev"])
