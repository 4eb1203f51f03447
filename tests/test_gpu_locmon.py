"""The localisation monitor on the device (ndtgpu_locmon_*, LocalizationMonitor) against tests/locmon_model.py, EXACTLY: field bytes,
keys, counts, flags, indices, and the badness bit for bit.  The beam table is an input of both (the library makes it on the host with
its C library; ndtgpu_locmon_beam_table returns the same entries), everything behind it is integer or fp64 in a fixed order.
No device: these tests fail."""
import math

import numpy as np
import pytest

import locmon_fixtures as F
import locmon_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_records(got, want, what=""):
    for f in ("key", "n_kept", "n_offmap", "flags"):
        assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:8])
    assert np.array_equal(bits(got["badness"]), bits(want["badness"])), (what, "badness")


def dev_bytes(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


# ---- the field -------------------------------------------------------------------------------------------------------------------
def field_grids(rng, h, w):
    """random with unknown and free pixels (sparse, dense), a single corner obstacle, empty, all obstacle"""
    corner = np.zeros((h, w), dtype=np.int8)
    corner[h - 1, 0] = 100
    return [F.random_grid(rng, h, w, 0.003), corner, F.random_grid(rng, h, w, 0.1), np.zeros((h, w), dtype=np.int8),
            np.full((h, w), 100, dtype=np.int8), np.full((h, w), -1, dtype=np.int8)]


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (65, 67), (130, 259)])
def test_field_equals_the_model(N, h, w):
    """R 1, 2, 7, 20 (7 and 20 exceed the width of the 5 x 3 grid), occupied_min 55 and 70, one grid and three back to back (an odd
    width * height leaves the second one unaligned), host form and device form"""
    import torch
    rng = np.random.default_rng(h * 1000 + w)
    grids = field_grids(rng, h, w)
    mon = N.LocalizationMonitor(3, 3 * h * w, 16)
    for R in (1, 2, 7, 20):
        for occ_min in (55, 70):
            for pick in ((0,), (1, 2, 4), (2, 3, 5)):
                if occ_min == 70 and pick != (1, 2, 4):
                    continue
                stack = np.stack([grids[k] for k in pick])
                origins = np.zeros((len(pick), 2))
                if pick == (1, 2, 4):
                    mon.set_grids_device(torch.from_numpy(stack).cuda(), 1.0, origins, max_dist=R + 0.5, occupied_min=occ_min)
                else:
                    mon.set_grids(stack, 1.0, origins, max_dist=R + 0.5, occupied_min=occ_min)
                for g, k in enumerate(pick):
                    got, want = mon.field(g), M.field(grids[k], R, occ_min)
                    assert got.dtype == np.uint16 and np.array_equal(got, want), (h, w, R, occ_min, k, np.argwhere(got != want)[:4])
    mon.close()


# ---- evaluate ----------------------------------------------------------------------------------------------------------------------
RES, MAXD = 0.05, 0.375
EH, EW = 65, 67
ORIGINS = np.array([[-1.0, -2.0], [0.5, 0.25]])


@pytest.fixture(scope="module")
def world():
    """grid 0: walls and posts with unknown and free pixels; grid 1: all obstacle.  Their model fields (R = 7)."""
    rng = np.random.default_rng(77)
    g0 = F.random_grid(rng, EH, EW, 0.004)
    g0[5, :] = 100
    g0[:, 60] = 70
    g1 = np.full((EH, EW), 100, dtype=np.int8)
    grids = np.stack([g0, g1])
    return grids, [M.field(g0, 7), M.field(g1, 7)]


def eval_inputs(rng, nb, n_scans=6, n_q=40):
    """ranges with NaN, inf, values at and below r_min and at and above r_max; scan 0 all dropped, scan 1 all kept (n_kept = nb), scan 2
    all kept but one; queries inside, at the rim of and outside the grids"""
    r_min, r_max = 0.1, 4.0
    r = rng.uniform(0.11, 3.0, size=(n_scans, nb))
    special = np.array([np.nan, np.inf, -np.inf, 0.1, 0.05, 0.0, -1.0, 4.0, 7.0])
    for s in range(3, n_scans):
        k = rng.integers(0, nb, size=max(1, nb // 4))
        r[s, k] = rng.choice(special, size=k.shape[0])
    r[0, :] = rng.choice(special, size=nb)
    r[1, :] = rng.uniform(0.11, 1.0, size=nb)
    r[2, nb // 2] = np.nan
    q = F.queries(rng.integers(0, n_scans, n_q), rng.integers(0, 2, n_q), rng.uniform(-1.5, 3.0, n_q), rng.uniform(-2.5, 2.0, n_q),
                  rng.uniform(-math.pi, math.pi, n_q))
    q[0]["scan"] = 0                                          # NO_BEAMS
    q[1]["scan"] = n_scans                                    # BAD_INDEX (scan)
    q[2]["grid"] = 2                                          # BAD_INDEX (grid)
    q[3]["scan"] = M.NO_SCAN                                  # NO_QUERY
    q[4] = F.queries(1, 1, 2.175, 1.875, 0.3)[0]                 # all keys equal: every endpoint on an obstacle of grid 1 ...
    q[5] = F.queries(1, 0, 50.0, 50.0, 0.3)[0]                # ... and every endpoint off the map
    q[6] = F.queries(2, 1, 2.0, 1.5, 1.0)[0]                  # n_kept = nb - 1
    q[7] = F.queries(1, 0, 0.5, -0.5, 2.0)[0]                 # n_kept = nb, the sparse grid
    return r, q, r_min, r_max


@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 255, 256, 257, 1023])
def test_evaluate_equals_the_model(N, world, nb):
    grids, fields = world
    rng = np.random.default_rng(nb)
    r, q, r_min, r_max = eval_inputs(rng, nb)
    a0, inc = -2.0, 4.0 / nb
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    want = M.evaluate(fields, ORIGINS, RES, MAXD, cb, sb, r, q, r_min, r_max)
    assert want["flags"][:4].tolist() == [M.NO_BEAMS, M.BAD_INDEX, M.BAD_INDEX, M.NO_QUERY]
    assert want["key"][4] == 0 and want["n_offmap"][4] == 0 and want["key"][5] == M.KEY_OFFMAP and want["n_offmap"][5] == nb
    assert want["n_kept"][6] == nb - 1 and want["n_kept"][7] == nb
    mon = N.LocalizationMonitor(2, 2 * EH * EW, 1023)
    mon.set_beams(nb, a0, inc)
    mon.set_grids(grids, RES, ORIGINS, max_dist=MAXD)
    got = mon.evaluate(r, q, r_min=r_min, r_max=r_max)
    same_records(got, want, nb)
    # the same queries at other batch positions and in other batch sizes: the same bits
    perm = rng.permutation(len(q))
    same_records(mon.evaluate(r, q[perm], r_min=r_min, r_max=r_max), want[perm], "permuted")
    one = mon.evaluate(r, q[7:8], r_min=r_min, r_max=r_max)
    same_records(one, want[7:8], "alone")
    rep = mon.evaluate(r, np.concatenate([q[7:8]] * 5 + [q[10:13]]), r_min=r_min, r_max=r_max)
    same_records(rep[:5], np.concatenate([want[7:8]] * 5), "repeated")
    mon.close()


def test_evaluate_medians_land_on_every_kind_of_key(N, world):
    """over the cases above the median is a near key, far and off the map, and n_kept is even and odd"""
    grids, fields = world
    kinds, parity = set(), set()
    for nb in (63, 64, 257):
        r, q, r_min, r_max = eval_inputs(np.random.default_rng(nb), nb)
        cb, sb = N.locmon_beam_table(nb, -2.0, 4.0 / nb)
        want = M.evaluate(fields, ORIGINS, RES, MAXD, cb, sb, r, q, r_min, r_max)
        ok = want[want["flags"] == 0]
        kinds |= {"near" if 0 < k < M.KEY_FAR else {0: "zero", M.KEY_FAR: "far", M.KEY_OFFMAP: "off"}[int(k)] for k in ok["key"]}
        parity |= {int(n) % 2 for n in ok["n_kept"]}
    assert kinds == {"near", "zero", "far", "off"} and parity == {0, 1}


def test_evaluate_device_on_a_stream(N, world):
    import torch
    grids, fields = world
    nb = 257
    r, q, r_min, r_max = eval_inputs(np.random.default_rng(nb), nb)
    cb, sb = N.locmon_beam_table(nb, -2.0, 4.0 / nb)
    want = M.evaluate(fields, ORIGINS, RES, MAXD, cb, sb, r, q, r_min, r_max)
    mon = N.LocalizationMonitor(2, 2 * EH * EW, 512)
    st = torch.cuda.Stream()
    mon.set_beams(nb, -2.0, 4.0 / nb, stream=st)
    g_t, r_t, q_t = torch.from_numpy(grids).cuda(), torch.from_numpy(r).cuda(), dev_bytes(q)
    res_t = torch.zeros(len(q) * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mon.set_grids_device(g_t, RES, ORIGINS, stream=st, max_dist=MAXD)
    mon.evaluate_device(r_t, q_t, res_t, stream=st, r_min=r_min, r_max=r_max)
    st.synchronize()
    same_records(mon.read(res_t, N.LOCMON_RESULT_DTYPE, len(q)), want, "device form")
    mon.close()


# ---- adjust ------------------------------------------------------------------------------------------------------------------------
def lattice(nx, ny, nyaw, x0=0.3, y0=-0.6, step=0.07):
    yaws = -3.0 + 6.0 * np.arange(nyaw) / max(nyaw, 1)
    return dict(xs=x0 + step * np.arange(nx), ys=y0 + step * np.arange(ny), cs=np.cos(yaws), sn=np.sin(yaws))


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 17), (4, 4, 16), (1, 1, 257)])
def test_adjust_equals_the_model(N, world, shape):
    """1, 255, 256 and 257 candidates: the whole volume, the winner (ties to the lowest index), host and device form"""
    import torch
    grids, fields = world
    nb = 65
    rng = np.random.default_rng(sum(shape))
    r = rng.uniform(0.2, 2.0, size=(2, nb))
    r[0] = rng.uniform(0.2, 1.2, size=nb)
    r[1, ::7] = np.nan
    cb, sb = N.locmon_beam_table(nb, -1.5, 3.0 / nb)
    lat = lattice(*shape)
    want = M.adjust(fields[0], ORIGINS[0], RES, MAXD, cb, sb, r[1], lat)
    mon = N.LocalizationMonitor(2, 2 * EH * EW, nb, 257)
    mon.set_beams(nb, -1.5, 3.0 / nb)
    mon.set_grids(grids, RES, ORIGINS, max_dist=MAXD)
    got = mon.adjust(r, 1, 0, lat, want_volume=True)
    assert np.array_equal(got["volume"], want["volume"])
    assert (got["index"], got["key"], got["flags"]) == (want["index"], want["key"], want["flags"])
    assert bits(got["badness"]) == bits(want["badness"])
    assert (want["volume"].reshape(-1)[:want["index"]] > want["key"]).all()            # the first of equals
    res_t = torch.zeros(24, dtype=torch.uint8, device="cuda")
    vol_t = torch.zeros(int(np.prod(shape)), dtype=torch.int32, device="cuda")
    mon.adjust_device(torch.from_numpy(r).cuda(), 1, 0, lat, res_t, vol_t)
    torch.cuda.synchronize()
    rec = mon.read(res_t, N.LOCMON_ADJUST_DTYPE)[0]
    assert (int(rec["index"]), int(rec["key"]), int(rec["flags"])) == (want["index"], want["key"], want["flags"])
    assert bits(rec["badness"]) == bits(want["badness"])
    assert np.array_equal(vol_t.cpu().numpy().view(np.uint32).reshape(shape), want["volume"])
    # every candidate ties on the all-obstacle grid: the lowest index wins
    tie = mon.adjust(r, 0, 1, lattice(*shape, x0=2.1, y0=1.8, step=0.01), want_volume=True)
    assert tie["index"] == 0 and tie["key"] == 0 and tie["flags"] == 0 and (tie["volume"] == 0).all()
    # an all-off-map lattice: NO_RESULT
    off = mon.adjust(r, 0, 0, lattice(*shape, x0=100.0, y0=100.0), want_volume=True)
    assert off["flags"] == N.LOCMON_NO_RESULT and off["index"] == 0 and off["key"] == M.KEY_OFFMAP and off["badness"] == 1e9
    assert (off["volume"] == M.KEY_OFFMAP).all()
    mon.close()


def test_adjust_in_two_chunks(N, world):
    """a handle made for 8192 beams works through a lattice in chunks of 1024 candidates: 7 x 7 x 23 = 1127 candidates, two chunks;
    the winner planted in the second"""
    grids, fields = world
    nb = 33
    rng = np.random.default_rng(3)
    r = rng.uniform(0.2, 0.8, size=(1, nb))
    cb, sb = N.locmon_beam_table(nb, -1.5, 3.0 / nb)
    lat = lattice(7, 7, 23)
    want = M.adjust(fields[0], ORIGINS[0], RES, MAXD, cb, sb, r[0], lat)
    mon = N.LocalizationMonitor(2, 2 * EH * EW, 8192, 1127)
    mon.set_beams(nb, -1.5, 3.0 / nb)
    mon.set_grids(grids, RES, ORIGINS, max_dist=MAXD)
    got = mon.adjust(r, 0, 0, lat, want_volume=True)
    assert np.array_equal(got["volume"], want["volume"]) and (got["index"], got["key"]) == (want["index"], want["key"])
    # the winner planted in the second chunk: the all-obstacle grid from a lattice whose first 6 x nodes are off the map
    lat2 = dict(lat, xs=np.concatenate([np.full(6, 100.0) + np.arange(6), [1.5]]), ys=1.0 + 0.07 * np.arange(7))
    got2 = mon.adjust(r, 0, 1, lat2, want_volume=True)
    want2 = M.adjust(fields[1], ORIGINS[1], RES, MAXD, cb, sb, r[0], lat2)
    assert want2["index"] == 6 * 7 * 23 >= 966 and want2["key"] == 0
    assert np.array_equal(got2["volume"], want2["volume"]) and (got2["index"], got2["key"], got2["flags"]) == (want2["index"], 0, 0)
    with pytest.raises(N.NdtGpuError) as e:
        mon.adjust(r, 0, 0, lattice(7, 7, 24))
    assert e.value.status == -4
    mon.close()


# ---- pick --------------------------------------------------------------------------------------------------------------------------
def match_records(status, n_inliers, poses):
    from ndt_feature_graph_amd import binding
    m = np.zeros(len(status), dtype=binding.FEATMATCH_RESULT_DTYPE)
    m["status"], m["n_inliers"] = status, n_inliers
    m["x"], m["y"], m["c"], m["s"] = poses[:, 0], poses[:, 1], np.cos(poses[:, 2]), np.sin(poses[:, 2])
    m["theta"] = poses[:, 2]
    return m


PICK_CASES = {
    "no qualifying pair": ([0, 0, 1], [3, 8, 50]),
    "ties": ([0, 0, 0, 0], [9, 14, 14, 12]),
    "equal to min_num_matches": ([0], [8]),
    "non-OK status": ([2, 0, 3, 1], [60, 10, 70, 80]),
    "many pairs": ([0] * 700, list(9 + (np.arange(700) * 37) % 90)),
}


@pytest.mark.parametrize("case", sorted(PICK_CASES))
def test_pick_then_evaluate(N, world, case):
    """the pick record and the written query equal the model; evaluate on the written query, on the same stream, equals the model's
    evaluation of the model's query (NO_QUERY where no pair qualifies)"""
    import torch
    grids, fields = world
    status, n_in = PICK_CASES[case]
    n = len(status)
    rng = np.random.default_rng(n)
    mp = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-1, 1, n)], axis=1)
    m = match_records(status, n_in, mp)
    refs = F.queries(0, 0, rng.uniform(0.0, 2.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-3, 3, n))
    ref4 = np.stack([refs["x"], refs["y"], refs["c"], refs["s"]], axis=1)
    nb = 64
    r = rng.uniform(0.2, 2.0, size=(2, nb))
    cb, sb = N.locmon_beam_table(nb, -1.5, 3.0 / nb)
    wq, wp = M.pick(m["status"], m["n_inliers"], np.stack([m["x"], m["y"], m["c"], m["s"]], axis=1), ref4, 1, 0)
    wq_rec = np.zeros(1, dtype=F.QUERY_DTYPE)
    for k, v in wq.items():
        wq_rec[k] = v
    want = M.evaluate(fields, ORIGINS, RES, MAXD, cb, sb, r, wq_rec)
    mon = N.LocalizationMonitor(2, 2 * EH * EW, nb)
    mon.set_beams(nb, -1.5, 3.0 / nb)
    mon.set_grids(grids, RES, ORIGINS, max_dist=MAXD)
    q_t = torch.zeros(40, dtype=torch.uint8, device="cuda")
    p_t = torch.zeros(16, dtype=torch.uint8, device="cuda")
    res_t = torch.zeros(24, dtype=torch.uint8, device="cuda")
    m_t, ref_t, r_t = dev_bytes(m), torch.from_numpy(ref4).cuda(), torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    mon.pick_device(m_t, ref_t, n, 1, 0, q_t, p_t, stream=st)
    mon.evaluate_device(r_t, q_t, res_t, n_queries=1, stream=st)
    st.synchronize()
    gp, gq = mon.read(p_t, N.LOCMON_PICK_DTYPE)[0], mon.read(q_t, N.LOCMON_QUERY_DTYPE)[0]
    assert (int(gp["pair"]), int(gp["n_inliers"]), int(gp["flags"])) == (wp["pair"], wp["n_inliers"], wp["flags"]), case
    assert int(gq["scan"]) == wq["scan"] and int(gq["grid"]) == wq["grid"]
    assert np.array_equal(bits([gq["x"], gq["y"], gq["c"], gq["s"]]), bits([wq["x"], wq["y"], wq["c"], wq["s"]]))
    same_records(mon.read(res_t, N.LOCMON_RESULT_DTYPE), want, case)
    if case in ("no qualifying pair", "equal to min_num_matches"):
        assert wp["pair"] == -1 and want["flags"][0] == M.NO_QUERY
    if case == "ties":
        assert wp["pair"] == 1
    if case == "non-OK status":
        assert wp["pair"] == 1
    mon.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def test_chain_from_ranges_to_a_verdict(N):
    """synth.scan_2d_ranges -> ScanProjector -> MapSet.build -> occupancy_grid (device) -> set_grids_device -> evaluate_device on ONE
    stream.  The device's result equals the model run on the device's own grid; the true pose is "localised" (badness < 0.25) and
    the pose 3 m away is not.  The scene was chosen on the CPU (locmon_fixtures.CHAIN: model keys 0 and 0x10000)."""
    import torch
    from ndt_feature_graph_amd import synth
    c = F.CHAIN
    nb = c["n_beams"]
    r, a0, inc = synth.scan_2d_ranges([c["seed"]], torch.tensor([[0.0, 0.0, 0.0]]), nb, noise_sigma=c["noise_sigma"])
    r_t = torch.as_tensor(r.numpy(), device="cuda").contiguous()
    w, h, origin = N.occupancy_grid_dims(c["map_res"], c["cells"], [0.0, 0.0, 0.0], c["pixel"])
    st = torch.cuda.Stream()
    proj = N.ScanProjector(1, nb)
    ms = N.MapSet(c["map_res"], (0.0, 0.0, 0.0), c["size_m"], n_maps=1)
    assert ms.info()["cells_per_axis"] == list(c["cells"])
    mon = N.LocalizationMonitor(1, w * h, nb)
    mon.set_beams(nb, a0, inc, stream=st)
    cloud = torch.empty((1, nb, 4), dtype=torch.float32, device="cuda")
    grid_t = torch.zeros(h * w, dtype=torch.int8, device="cuda")
    q = F.queries(0, 0, [0.0, c["displaced"][0]], [0.0, c["displaced"][1]], 0.0)
    q_t, res_t = dev_bytes(q), torch.zeros(2 * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    proj.project_device(r_t, cloud, a0, inc, stream=st, r_min=c["r_min"], r_max=c["r_max"])
    ms.build(cloud, stream=st)
    g_t, _ = ms.occupancy_grid(0, 1, c["pixel"], out=grid_t, stream=st)
    mon.set_grids_device(g_t, c["pixel"], [origin[:2]], stream=st, max_dist=c["max_dist"])
    mon.evaluate_device(r_t, q_t, res_t, stream=st, r_min=c["r_min"], r_max=c["r_max"])
    st.synchronize()
    got = mon.read(res_t, N.LOCMON_RESULT_DTYPE, 2)
    grid = g_t.cpu().numpy()[0]
    fld = M.field(grid, M.radius(c["max_dist"], c["pixel"]))
    assert np.array_equal(mon.field(0), fld)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    want = M.evaluate([fld], [origin[:2]], c["pixel"], c["max_dist"], cb, sb, r.numpy(), q, c["r_min"], c["r_max"])
    same_records(got, want, "chain")
    keys = M.beam_keys(fld, (0.0, 0.0, 1.0, 0.0), cb, sb, r.numpy()[0], origin[:2], c["pixel"], c["r_min"], c["r_max"])
    print("chain: %d obstacle pixels, %.3f of the endpoints on them, keys %s, badness %s" % ((grid >= 55).sum(), (keys == 0).mean(),
                                                                                         got["key"].tolist(), got["badness"].tolist()))
    assert (keys == 0).mean() >= c["min_on_obstacle"]
    assert got["key"].tolist() == [c["key_true"], c["key_displaced"]]
    assert got["badness"][0] < 0.25 and not got["badness"][1] < 0.25
    mon.close()
    ms.close()
    proj.close()


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------
def test_live_resources_return_after_destroy(N, world):
    from ndt_feature_graph_amd.binding import live_resources
    import torch
    grids, _ = world
    torch.cuda.synchronize()
    before = live_resources()
    mon = N.LocalizationMonitor(2, 2 * EH * EW, 64, 300)
    assert live_resources() != before
    mon.set_beams(64, -1.0, 0.03)
    mon.set_grids(grids, RES, ORIGINS)
    r = np.full((1, 64), 1.0)
    mon.evaluate(r, F.queries(0, 0, 0.5, 0.0, 0.0))
    mon.adjust(r, 0, 0, lattice(3, 3, 3), want_volume=True)
    mon.field(1)
    with pytest.raises(N.NdtGpuError) as e:
        mon.set_grids(np.zeros((3, 4, 4), dtype=np.int8), RES, np.zeros((3, 2)))
    assert e.value.status == -4
    with pytest.raises(N.NdtGpuError) as e:
        mon.set_beams(65, 0.0, 0.1)
    assert e.value.status == -4
    mon.close()
    assert live_resources() == before
