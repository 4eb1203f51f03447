"""The scan simulator on the device (ndtgpu_scansim_*, ScanSimulator) against tests/scansim_model.py, EXACTLY: range bits, n_hits,
flags, poses, indices and counts.  The beam table and the heading tables are inputs of both (made on the host), everything behind
them is integer or fp64 in a fixed order.  No device: these tests fail."""
import math

import numpy as np
import pytest

import scansim_fixtures as F
import scansim_model as M

pytestmark = pytest.mark.gpu

NBS = (1, 2, 63, 64, 65, 255, 256, 257, 1023)
REACHES = (1, 7, 40, 200)


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


@pytest.fixture(scope="module")
def rooms():
    return np.stack([F.room(), F.second_room()]), np.array([F.ROOM_ORIGIN, F.ROOM_ORIGIN])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_scans(got_r, got_rec, want_r, want_rec, what=""):
    assert np.array_equal(got_rec["flags"], want_rec["flags"]), (what, "flags", got_rec["flags"].tolist(), want_rec["flags"].tolist())
    assert np.array_equal(got_rec["n_hits"], want_rec["n_hits"]), (what, "n_hits", np.nonzero(got_rec["n_hits"] != want_rec["n_hits"])[0][:8])
    assert np.array_equal(bits(got_r), bits(want_r)), (what, "ranges", np.argwhere(bits(got_r) != bits(want_r))[:8].tolist())


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def beams_of(nb):
    return (-math.pi / 2, math.pi / (nb - 1) if nb > 1 else 0.0) if nb < 255 else (-math.pi, 2 * math.pi / nb)


def device_scans(N, sim, poses, nb, grid_idx=None, count=None, **prm):
    import torch
    n = poses.shape[0]
    p_t, r_t = dev(poses), torch.full((n, nb), -1.0, dtype=torch.float64, device="cuda")
    res_t = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    g_t = None if grid_idx is None else dev(grid_idx, np.int32)
    c_t = None if count is None else dev(np.array([count, 0], dtype=np.int32))
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sim.simulate_device(p_t, r_t, grid_idx_t=g_t, count_t=c_t, results_t=res_t, stream=st, **prm)
    st.synchronize()
    return r_t.cpu().numpy(), sim.read(res_t, N.SCANSIM_RESULT_DTYPE, n)


# ---- simulate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", REACHES)
@pytest.mark.parametrize("nb", NBS)
def test_simulate_equals_the_model(N, rooms, nb, R):
    """24 poses of every kind in the 65 x 67 room (and its twin as grid 1), host and device forms, unknown_is_obstacle 0 and 1,
    occupied_min 55 and 70 (two of the four combinations a case, all four over the reaches of a beam count).  R = 200 exceeds the
    grid: rays leave the map."""
    grids, origins = rooms
    poses, gi = F.room_poses()
    a0, inc = beams_of(nb)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    rm = R * F.RES + 0.01
    assert M.reach(rm, F.RES) == N.scansim_reach(rm, F.RES) == R
    sim = N.ScanSimulator(2, nb, 24)
    sim.set_beams(nb, a0, inc)
    sim.set_grids(grids, F.RES, origins)
    combos = ((1, 55), (0, 70)) if REACHES.index(R) % 2 == 0 else ((1, 70), (0, 55))
    for unk, om in combos:
        prm = dict(range_max=rm, miss=rm + 1.0, occupied_min=om, unknown_is_obstacle=unk)
        want_r, want_rec = M.simulate(grids, origins, F.RES, poses, cb, sb, gi, **prm)
        F.assert_not_vacuous(want_rec, nb, R)
        got_r, got_rec = sim.simulate(poses, gi, **prm)
        same_scans(got_r, got_rec, want_r, want_rec, ("host", nb, R, unk, om))
        got_r, got_rec = device_scans(N, sim, poses, nb, gi, **prm)
        same_scans(got_r, got_rec, want_r, want_rec, ("device", nb, R, unk, om))
    assert want_rec["flags"].tolist().count(M.OFFMAP) == 3 and want_rec["flags"][-1] == M.BAD_INDEX
    sim.close()


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5)])
def test_simulate_in_tiny_grids(N, h, w):
    rng = np.random.default_rng(h * 10 + w)
    g = F.random_grid(rng, h, w, 0.1)
    g[h - 1, w - 1] = 100
    g[0, 0] = 0
    origin = (0.3, -0.7)
    nb = 65
    cb, sb = N.locmon_beam_table(nb, -math.pi, 2 * math.pi / nb)
    poses = np.array([F.centre(i, j, origin) + (math.cos(t), math.sin(t)) for i in range(w) for j in range(h) for t in (0.0, 2.0)])
    sim = N.ScanSimulator(1, nb, poses.shape[0])
    sim.set_beams(nb, -math.pi, 2 * math.pi / nb)
    sim.set_grids(g[None], F.RES, [origin])
    for R in (1, 7):
        prm = dict(range_max=R * F.RES + 0.01, miss=9.0)
        want_r, want_rec = M.simulate(g[None], [origin], F.RES, poses, cb, sb, **prm)
        assert (want_r == 9.0).any() and (h == 1 or want_rec["n_hits"].sum() > 0)
        same_scans(*sim.simulate(poses, **prm), want_r, want_rec, ("host", h, w, R))
        same_scans(*device_scans(N, sim, poses, nb, **prm), want_r, want_rec, ("device", h, w, R))
    sim.close()


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def test_a_scan_is_the_same_bytes_at_any_row_of_a_batch(N, rooms):
    grids, origins = rooms
    nb = 257
    a0, inc = beams_of(nb)
    rng = np.random.default_rng(5)
    one = np.array([F.centre(20, 40) + (math.cos(0.4), math.sin(0.4))])
    batch = np.array([F.centre(rng.integers(1, 64), rng.integers(1, 66)) + (math.cos(t), math.sin(t)) for t in rng.uniform(-3, 3, 300)])
    rows = (0, 255, 256, 299)
    batch[list(rows)] = one[0]
    sim = N.ScanSimulator(2, nb, 300)
    sim.set_beams(nb, a0, inc)
    sim.set_grids(grids, F.RES, origins)
    prm = dict(range_max=2.0, miss=3.0)
    alone_r, alone_rec = device_scans(N, sim, one, nb, **prm)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    want_r, want_rec = M.simulate(grids, origins, F.RES, one, cb, sb, **prm)
    same_scans(alone_r, alone_rec, want_r, want_rec, "alone")
    assert 0 < want_rec["n_hits"][0] < nb
    got_r, got_rec = device_scans(N, sim, batch, nb, **prm)
    for row in rows:
        assert np.array_equal(bits(got_r[row]), bits(alone_r[0])) and got_rec[row] == alone_rec[0], row
    sim.close()


def test_two_grids_back_to_back_and_a_count_below_n_poses(N, rooms):
    grids, origins = rooms
    origins = np.array([F.ROOM_ORIGIN, (2.0, 1.0)])
    nb = 64
    a0, inc = beams_of(nb)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    rng = np.random.default_rng(9)
    gi = rng.integers(0, 2, 40).astype(np.uint32)
    poses = np.array([F.centre(rng.integers(1, 64), rng.integers(1, 66), origins[g]) + (math.cos(t), math.sin(t))
                      for g, t in zip(gi, rng.uniform(-3, 3, 40))])
    sim = N.ScanSimulator(2, nb, 40)
    sim.set_beams(nb, a0, inc)
    sim.set_grids_device(dev(grids), F.RES, origins)
    prm = dict(range_max=1.5, miss=2.5)
    want_r, want_rec = M.simulate(grids, origins, F.RES, poses, cb, sb, gi, **prm)
    assert (want_rec["n_hits"][gi == 0] > 0).any() and (want_rec["n_hits"][gi == 1] > 0).any() and (want_r == 2.5).any()
    # (the twin differs from the room: the same poses in the other grid give other scans)
    other_r, _ = M.simulate(grids, origins[::-1], F.RES, poses, cb, sb, 1 - gi, **prm)
    assert not np.array_equal(other_r, want_r)
    same_scans(*device_scans(N, sim, poses, nb, gi, **prm), want_r, want_rec, "two grids")
    for count in (0, 1, 17, 40, 1000):
        want_r, want_rec = M.simulate(grids, origins, F.RES, poses, cb, sb, gi, count=count, **prm)
        assert (want_rec["flags"][min(count, 40):] == M.NO_POSE).all() and (want_r[min(count, 40):] == 2.5).all()
        same_scans(*device_scans(N, sim, poses, nb, gi, count=count, **prm), want_r, want_rec, ("count", count))
    sim.close()


# ---- lattice ---------------------------------------------------------------------------------------------------------------------
def free_cells_grid(n_free, w=23, h=37):
    """a grid with exactly n_free free pixels in row-major order, the rest occupied"""
    g = np.full((h, w), 100, dtype=np.int8)
    g.reshape(-1)[np.arange(n_free) * 3 % (w * h)] = 0
    assert (g == 0).sum() == n_free
    return g


LATTICE_CASES = {
    "skip 1": (lambda: F.room(), 1, math.pi / 4, None, None),
    "skip 2": (lambda: F.room(), 2, 2.1, None, None),
    "skip 7 on a 5-wide grid": (lambda: F.random_grid(np.random.default_rng(1), 30, 5, 0.1), 7, 2.1, None, None),
    "255 kept": (lambda: free_cells_grid(255), 1, 7.0, None, None),
    "256 kept": (lambda: free_cells_grid(256), 1, 7.0, None, None),
    "257 kept": (lambda: free_cells_grid(257), 1, 2.1, None, None),
    "all free": (lambda: np.zeros((19, 31), dtype=np.int8), 1, 7.0, None, None),
    "none free": (lambda: np.full((19, 31), -1, dtype=np.int8), 1, 2.1, None, None),
    "a box that cuts": (lambda: F.room(), 1, 7.0, (-0.5, -1.2, 1.1, 0.3), None),
    "capacity below the number that passed": (lambda: F.room(), 2, 2.1, None, 500),
}


@pytest.mark.parametrize("case", sorted(LATTICE_CASES))
def test_lattice_equals_the_model(N, case):
    import torch
    make, skip, angle_step, box, capacity = LATTICE_CASES[case]
    g = make()
    h, w = g.shape
    cs, sn = N.scansim_headings(angle_step)
    wc, ws = M.headings(angle_step)
    assert cs.shape == wc.shape and (np.abs(cs - wc) <= np.spacing(1.0)).all() and (np.abs(sn - ws) <= np.spacing(1.0)).all()
    assert len(cs) == {math.pi / 4: 8, 2.1: 3, 7.0: 1}[angle_step]
    want = M.lattice(g, F.ROOM_ORIGIN, F.RES, skip, cs, sn, box, capacity)
    full = M.lattice(g, F.ROOM_ORIGIN, F.RES, skip, cs, sn, box)
    cap = capacity or max(1, full["passed"]) + 3
    if case.endswith("kept"):
        assert full["passed"] == int(case.split()[0]) * len(cs)
    if case == "none free":
        assert full["passed"] == 0
    if case == "a box that cuts":
        assert 0 < full["passed"] < M.lattice(g, F.ROOM_ORIGIN, F.RES, skip, cs, sn)["passed"]
    if capacity:
        assert want["written"] == capacity < want["passed"] == full["passed"] and capacity % len(cs) != 0
    sim = N.ScanSimulator(1, 8, 16)
    sim.set_grids(g[None], F.RES, [F.ROOM_ORIGIN])
    got = sim.lattice(skip, (cs, sn), cap, box=box)
    assert (got["written"], got["passed"]) == (want["written"], want["passed"]), case
    assert np.array_equal(bits(got["poses"]), bits(want["poses"])) and np.array_equal(got["index"], want["index"])
    # the device form: the rows beyond the count stay as they were
    p_t = torch.full((cap, 4), -7.0, dtype=torch.float64, device="cuda")
    i_t = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    c_t = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sim.lattice_device(skip, (cs, sn), cap, p_t, c_t, index_t=i_t, box=box, stream=st)
    st.synchronize()
    n = want["written"]
    assert c_t.cpu().numpy().view(np.uint32).tolist() == [n, want["passed"]]
    assert np.array_equal(bits(p_t.cpu().numpy()[:n]), bits(want["poses"])) and (p_t.cpu().numpy()[n:] == -7.0).all()
    assert np.array_equal(i_t.cpu().numpy()[:n].view(np.uint32), want["index"]) and (i_t.cpu().numpy()[n:] == -7).all()
    sim.close()


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def test_chain_from_a_grid_to_a_relocalised_pose(N):
    """lattice_device -> simulate_device (the references, then one current scan at lattice pose CHAIN["chosen"]) -> extract_device ->
    match_device on the pairs (reference p, current) -> pick_device -> evaluate_device on ONE stream, no host visit in between.  Each
    stage's output equals what the model or the host form of that stage gives on the previous stage's device output; the pick is the
    chosen pose and its badness is below 0.25 (scansim_fixtures.CHAIN: what the models gave on the CPU)."""
    import torch
    import locmon_model as LM
    c = F.CHAIN
    g = F.chain_grid()
    nb, cap, a0, inc = c["n_beams"], c["capacity"], c["angle_min"], c["angle_increment"]
    cs, sn = N.scansim_headings(c["angle_step"])
    sim = N.ScanSimulator(1, nb, cap + 1)
    fm = N.FeatureMatcher(cap + 1, c["max_points"])
    mon = N.LocalizationMonitor(1, g.size, nb)
    g_t = dev(g[None])
    poses_t = torch.zeros((cap, 4), dtype=torch.float64, device="cuda")
    count_t = torch.zeros(2, dtype=torch.int32, device="cuda")
    ranges_t = torch.zeros((cap + 1, nb), dtype=torch.float64, device="cuda")
    simres_t = torch.zeros(8 * (cap + 1), dtype=torch.uint8, device="cuda")
    sets_t = torch.arange(cap + 1, dtype=torch.int32, device="cuda")
    exres_t = torch.zeros((cap + 1) * N.binding.FEATEXTRACT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ref_t = torch.arange(cap, dtype=torch.int32, device="cuda")
    mov_t = torch.full((cap,), cap, dtype=torch.int32, device="cuda")
    mres_t = torch.zeros(cap * 72, dtype=torch.uint8, device="cuda")
    q_t = torch.zeros(40, dtype=torch.uint8, device="cuda")
    pick_t = torch.zeros(16, dtype=torch.uint8, device="cuda")
    ev_t = torch.zeros(24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    sprm = dict(range_max=c["range_max"], miss=c["miss"])
    sim.set_beams(nb, a0, inc, stream=st)
    sim.set_grids_device(g_t, F.RES, [c["origin"]], stream=st)
    mon.set_beams(nb, a0, inc, stream=st)
    mon.set_grids_device(g_t, F.RES, [c["origin"]], stream=st, max_dist=c["max_dist"])
    sim.lattice_device(c["skip"], (cs, sn), cap, poses_t, count_t, stream=st)
    sim.simulate_device(poses_t, ranges_t[:cap], count_t=count_t, results_t=simres_t, stream=st, **sprm)
    sim.simulate_device(poses_t[c["chosen"]:c["chosen"] + 1], ranges_t[cap:], results_t=simres_t[8 * cap:], stream=st, **sprm)
    fm.extract_device(sets_t, ranges_t, a0, inc, exres_t, stream=st, **c["extract"])
    fm.match_device(ref_t, mov_t, mres_t, stream=st, **c["match"])
    mon.pick_device(mres_t, poses_t, cap, cap, 0, q_t, pick_t, stream=st, post_x=0.0, post_y=0.0)
    mon.evaluate_device(ranges_t, q_t, ev_t, n_queries=1, stream=st, r_min=c["extract"]["r_min"], r_max=c["extract"]["r_max"])
    st.synchronize()
    # the lattice
    want = M.lattice(g, c["origin"], F.RES, c["skip"], cs, sn, capacity=cap)
    n = want["written"]
    assert count_t.cpu().numpy().tolist() == [n, n] and n == c["n_passed"] < cap
    poses = poses_t.cpu().numpy()
    assert np.array_equal(bits(poses[:n]), bits(want["poses"])) and np.abs(poses[c["chosen"]] - c["chosen_pose"]).max() < 1e-12
    # the scans: of the device's poses
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    ranges = ranges_t.cpu().numpy()
    all_poses = np.concatenate([poses, poses[c["chosen"]:c["chosen"] + 1]])
    want_r, want_rec = M.simulate(g[None], [c["origin"]], F.RES, all_poses[:n], cb, sb, **sprm)
    got_rec = sim.read(simres_t, N.SCANSIM_RESULT_DTYPE, cap + 1)
    same_scans(ranges[:n], got_rec[:n], want_r, want_rec, "references")
    assert (got_rec["flags"][n:cap] == M.NO_POSE).all() and (ranges[n:cap] == c["miss"]).all()
    assert np.array_equal(bits(ranges[cap]), bits(ranges[c["chosen"]])) and got_rec[cap] == got_rec[c["chosen"]]
    # the extraction: the host form on the device's ranges
    fm2 = N.FeatureMatcher(cap + 1, c["max_points"])
    ex2, _ = fm2.extract(np.arange(cap + 1), ranges, a0, inc, **c["extract"])
    ex = sim.read(exres_t, N.binding.FEATEXTRACT_RESULT_DTYPE, cap + 1)
    assert np.array_equal(ex, ex2)
    assert ex["n_stored"][c["chosen"]] == ex["n_stored"][cap] == c["n_stored"] and (ex["n_stored"][n:cap] == 0).all()
    for k in (0, c["chosen"], n - 1, n, cap):
        for a, b in zip(fm.get(k), fm2.get(k)):
            assert np.array_equal(bits(a), bits(b)), k
    # the match: the host form on the same banks
    m2, _, _ = fm2.match(np.arange(cap), np.full(cap, cap), **c["match"])
    m = sim.read(mres_t, N.binding.FEATMATCH_RESULT_DTYPE, cap)
    assert m.tobytes() == m2.tobytes()
    ok = m["status"] == 0
    print("chain: stored features %s, inliers of the OK pairs %s" % (ex["n_stored"].tolist(), dict(zip(np.nonzero(ok)[0].tolist(), m["n_inliers"][ok].tolist()))))
    assert m["n_inliers"][c["chosen"]] == c["n_inliers"] and ok[c["chosen"]]
    assert (m["n_inliers"][np.arange(cap) != c["chosen"]] < c["n_inliers"]).all()              # no other pose ties
    # the pick and its badness: the models on the device's match records
    wq, wp = LM.pick(m["status"], m["n_inliers"], np.stack([m["x"], m["y"], m["c"], m["s"]], axis=1), poses, cap, 0, post=(0.0, 0.0))
    gp, gq = sim.read(pick_t, N.LOCMON_PICK_DTYPE)[0], sim.read(q_t, N.LOCMON_QUERY_DTYPE)[0]
    assert (int(gp["pair"]), int(gp["n_inliers"]), int(gp["flags"])) == (wp["pair"], wp["n_inliers"], wp["flags"]) == (c["chosen"], c["n_inliers"], 0)
    assert np.array_equal(bits([gq["x"], gq["y"], gq["c"], gq["s"]]), bits([wq["x"], wq["y"], wq["c"], wq["s"]])) and int(gq["scan"]) == cap
    assert abs(gq["x"] - c["chosen_pose"][0]) < 1e-9 and abs(gq["y"] - c["chosen_pose"][1]) < 1e-9 and abs(gq["c"] - 1.0) < 1e-9
    fld = LM.field(g, LM.radius(c["max_dist"], F.RES))
    wq_rec = np.zeros(1, dtype=N.LOCMON_QUERY_DTYPE)
    for k, v in wq.items():
        wq_rec[k] = v
    want_ev = LM.evaluate([fld], [c["origin"]], F.RES, c["max_dist"], cb, sb, ranges, wq_rec, c["extract"]["r_min"], c["extract"]["r_max"])
    ev = sim.read(ev_t, N.LOCMON_RESULT_DTYPE)
    for f in ("key", "n_kept", "n_offmap", "flags"):
        assert ev[f][0] == want_ev[f][0], f
    assert np.array_equal(bits(ev["badness"]), bits(want_ev["badness"]))
    print("chain: picked pair %d with %d inliers, key %d, badness %.3f" % (gp["pair"], gp["n_inliers"], ev["key"][0], ev["badness"][0]))
    assert ev["key"][0] == c["key"] and ev["badness"][0] < c["badness_below"]
    for hnd in (sim, fm, fm2, mon):
        hnd.close()


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------
def test_live_resources_return_after_close(N, rooms):
    from ndt_feature_graph_amd.binding import live_resources
    import torch
    grids, origins = rooms
    torch.cuda.synchronize()
    before = live_resources()
    sim = N.ScanSimulator(2, 64, 30)
    assert live_resources() != before
    sim.set_beams(64, -1.0, 0.03)
    sim.set_grids(grids, F.RES, origins)
    poses, gi = F.room_poses()
    sim.simulate(poses, gi)
    sim.lattice(3, N.scansim_headings(2.1), 2000)
    for call, status in ((lambda: sim.set_grids(np.zeros((3, 4, 4), dtype=np.int8), F.RES, np.zeros((3, 2))), -4),
                         (lambda: sim.set_beams(65, 0.0, 0.1), -4),
                         (lambda: sim.simulate(np.tile(poses, (2, 1))), -4),
                         (lambda: sim.simulate(poses, range_max=1000.0), -1),
                         (lambda: sim.lattice(0, N.scansim_headings(2.1), 10), -1),
                         (lambda: sim.lattice(3, N.scansim_headings(2.1), 10, grid=2), -1)):
        with pytest.raises(N.NdtGpuError) as e:
            call()
        assert e.value.status == status
    sim.close()
    assert live_resources() == before
    empty = N.ScanSimulator(1, 8, 8)
    with pytest.raises(N.NdtGpuError) as e:                  # nothing installed yet
        empty.n_beams = 8
        empty.simulate(poses[:1])
    assert e.value.status == -1
    empty.close()
    assert live_resources() == before
