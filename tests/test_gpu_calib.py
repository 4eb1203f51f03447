"""ndtgpu_calib_search*: the brute-force search over sensor offsets on the device (-m gpu).

Against tests/calib_model.py's contract form, which prunes nothing: every score of the volume, the winner's score, index and flags
and the count of skipped rows are EXACT -- the scores bit for bit.  Shapes: the smallest at which the kernels can go wrong -- clouds
of 0, 1, 2, a wave and its neighbours and 257 kept rows in front of NaN pads, candidate counts around the tile of 256, one to three
pairs, and a handle whose scratch makes the lattice take two chunks."""
import math

import numpy as np
import pytest

import calib_fixtures as X
import calib_model as M

pytestmark = pytest.mark.gpu

TILE = 256
NP = 260                                           # rows of a scan's block in the banks below


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    assert N.CALIB_TILE == TILE == N.lib().ndtgpu_calib_tile()
    return N


@pytest.fixture(scope="module")
def cal(N):
    c = N.Calibrator(4, NP, 4096)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def scene(seed, rows, poses, ts=(0.2, 0.05, 0.03), n_points=NP, noise=0.02, bad_row=None):
    """scans of one random scene from base poses (x, y, yaw) with the laser at ts: xyz float32 [n, n_points, 3] with rows[k] kept
    rows in front of NaN pads, n_kept, poses4.  bad_row = (scan, row, value): a non-finite coordinate inside the kept rows"""
    rng = np.random.default_rng(seed)
    world = np.concatenate([rng.uniform(-4, 4, size=(max(max(rows), 1), 2)), rng.uniform(0.0, 0.02, size=(max(max(rows), 1), 1))], axis=1)
    xyz = np.full((len(rows), n_points, 3), np.nan, dtype=np.float32)
    for k, (n, (x, y, t)) in enumerate(zip(rows, X.sensor_poses(poses, ts))):
        c, s = math.cos(t), math.sin(t)
        dx, dy = world[:n, 0] - x, world[:n, 1] - y
        xyz[k, :n, 0] = c * dx + s * dy + rng.normal(0, noise, n)
        xyz[k, :n, 1] = c * dy - s * dx + rng.normal(0, noise, n)
        xyz[k, :n, 2] = world[:n, 2]
    if bad_row is not None:
        xyz[bad_row[0], bad_row[1], bad_row[2] % 3] = bad_row[3]
    return xyz, np.array(rows, dtype=np.uint32), M.poses4(poses)


def line_lattice(n, yaw=0.02, span=0.1):
    """n candidates on a line of x: nyaw = 1"""
    return dict(xs=0.2 + span * (np.arange(n) / max(n - 1, 1) - 0.5), ys=np.array([0.05]), cs=np.array([math.cos(yaw)]), sn=np.array([math.sin(yaw)]))


def device_search(N, cal, xyz, n_kept, poses4, pairs, lat, want_volume=True, stream=None, **prm):
    """search_device on fresh tensors -> dict like Calibrator.search's"""
    import torch
    dev = torch.device("cuda", 0)
    xt = torch.as_tensor(np.ascontiguousarray(xyz), device=dev)
    kt = torch.as_tensor(np.asarray(n_kept, dtype=np.uint32).view(np.int32), device=dev)
    pt = torch.as_tensor(np.ascontiguousarray(poses4, dtype=np.float64), device=dev)
    rt = torch.as_tensor(np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2).view(np.int32), device=dev)
    res = torch.full((6,), -1, dtype=torch.int32, device=dev)
    nc = len(lat["xs"]) * len(lat["ys"]) * len(lat["cs"])
    vt = torch.full((nc,), float("nan"), dtype=torch.float64, device=dev) if want_volume else None
    cal.search_device(xt, kt, pt, rt, lat, res, volume_t=vt, stream=stream, **prm)
    torch.cuda.synchronize()
    r = N.Calibrator.read_result(res)
    return dict(index=int(r["index"]), score=float(r["score"]), flags=int(r["flags"]), n_skipped=int(r["n_skipped"]),
                volume=None if vt is None else vt.cpu().numpy().reshape(len(lat["xs"]), len(lat["ys"]), len(lat["cs"])))


def same(got, want, what=""):
    if got["volume"] is not None:
        assert np.array_equal(bits(got["volume"]), bits(want["volume"])), (what, "volume", float(np.abs(got["volume"] - want["volume"]).max()))
    assert bits(got["score"]) == bits(want["score"]), (what, got["score"], want["score"])
    assert (got["index"], got["flags"], got["n_skipped"]) == (want["index"], want["flags"], want["n_skipped"]), what


POSES3 = ((0.5, -0.3, 0.1), (0.7, -0.1, 0.7), (0.4, 0.0, 1.4))
SMALL = M.lattice(0.2, 0.05, 0.03, 0.03, 0.03, 0.04, 0.02, 0.04)          # 3 x 3 x 2


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_cloud_sizes_against_the_model(N, cal, n):
    """three pairs over three scans of n, n + 3 and 65 kept rows in front of NaN pads; from n = 2 on a row inside the kept rows of
    the second scan has an infinite coordinate: it is skipped and counted (once per pair that names the scan).  n = 0: pairs with an
    empty cloud1, and with an empty cloud2, contribute 0.0"""
    xyz, kept, p4 = scene(100 + n, [n, n + 3, 65], POSES3, bad_row=(1, n // 2 + 1, n, np.inf if n % 2 else np.nan) if n >= 2 else None)
    pairs = [(0, 1), (1, 0), (2, 1)]
    want = M.search(xyz, kept, p4, pairs, SMALL)
    assert want["n_skipped"] == (3 if n >= 2 else 0)
    got = device_search(N, cal, xyz, kept, p4, pairs, SMALL)
    same(got, want, n)
    host = cal.search(xyz, kept, p4, pairs, SMALL, want_volume=True)
    same(host, want, (n, "host form"))
    if n == 0:
        only = M.search(xyz, kept, p4, [(2, 1)], SMALL)
        assert np.array_equal(bits(want["volume"]), bits(only["volume"]))


@pytest.mark.parametrize("n_pairs", [1, 2])
@pytest.mark.parametrize("n_cand", [1, TILE - 1, TILE, TILE + 1])
def test_candidate_counts_around_the_tile(N, cal, n_cand, n_pairs):
    """nyaw = 1 = ny: the candidates are a line of x"""
    xyz, kept, p4 = scene(7, [33, 40, 36], POSES3)
    pairs = [(0, 1), (1, 2)][:n_pairs]
    lat = line_lattice(n_cand)
    want = M.search(xyz, kept, p4, pairs, lat)
    same(device_search(N, cal, xyz, kept, p4, pairs, lat), want, (n_cand, n_pairs))


def test_threshold_is_strict(N, cal):
    """max_dist = 0.125, D = I: a point at exactly 0.125 from its neighbour has d2 == th2 and contributes d2; its float neighbours
    on either side contribute d2 (below) and th2 (above)"""
    th = 0.125
    lo, hi = np.nextafter(np.float32(th), np.float32(0)), np.nextafter(np.float32(th), np.float32(1))
    xyz = np.full((2, NP, 3), np.nan, dtype=np.float32)
    xyz[0, 0] = (0, 0, 0)
    xyz[1, :3] = [(th, 0, 0), (0, lo, 0), (0, 0, hi)]
    kept = np.array([1, 3], dtype=np.uint32)
    p4 = M.poses4([(1.0, 2.0, 0.0), (1.0, 2.0, 0.0)])
    lat = dict(xs=np.array([0.3]), ys=np.array([-0.1]), cs=np.array([1.0]), sn=np.array([0.0]))
    want = M.search(xyz, kept, p4, [(0, 1)], lat, max_dist=th)
    terms = [th * th, float(lo) * float(lo), th * th]
    assert float(hi) * float(hi) > th * th > terms[1] and want["score"] == (terms[0] + terms[1]) + terms[2]
    same(device_search(N, cal, xyz, kept, p4, [(0, 1)], lat, max_dist=th), want)
    for k in range(3):
        one = xyz.copy()
        one[1, 0] = xyz[1, k]
        got = device_search(N, cal, one, np.array([1, 1], dtype=np.uint32), p4, [(0, 1)], lat, max_dist=th)
        assert got["score"] == terms[k], k


def test_far_points_count_th2_each(N, cal):
    xyz, kept, p4 = scene(9, [40, 57], POSES3[:2])
    xyz[1, :, 0] += 50.0
    want = M.search(xyz, kept, p4, [(0, 1)], SMALL)
    acc = 0.0
    for _ in range(57):
        acc += 0.1 * 0.1
    assert (want["volume"] == acc).all() and want["index"] == 0
    same(device_search(N, cal, xyz, kept, p4, [(0, 1)], SMALL), want)


def test_translations_that_span_several_max_dist(N, cal):
    """x and y from -0.3 to 0.3 around the truth: which neighbours are within reach changes across the lattice"""
    xyz, kept, p4 = scene(21, [65, 70, 64], POSES3, noise=0.01)
    lat = M.lattice(0.2, 0.05, 0.03, 0.3, 0.3, 0.3, 0.05, 0.3)
    assert (len(lat["xs"]), len(lat["ys"]), len(lat["yaws"])) in ((12, 12, 2), (13, 13, 2), (12, 13, 2), (13, 12, 2))
    pairs = [(0, 1), (1, 2), (0, 2)]
    want = M.search(xyz, kept, p4, pairs, lat)
    v = want["volume"]
    assert v.min() < 0.5 * v.max() and (v == v.max()).sum() < v.size // 2, "the lattice must leave and enter reach, or it checks nothing"
    same(device_search(N, cal, xyz, kept, p4, pairs, lat), want)


def test_equal_winners_lowest_index(N, cal):
    """D = I: every candidate has the same score; and two candidates with the same table entries, far apart in the index"""
    xyz, kept, _ = scene(5, [30, 25], ((0, 0, 0), (0, 0, 0)), ts=(0, 0, 0))
    p4 = M.poses4([(1.5, -2.0, 0.0), (1.5, -2.0, 0.0)])
    lat = M.lattice(0.0, 0.0, 0.0, 0.3, 0.3, 0.2, 0.1, 0.1)
    want = M.search(xyz, kept, p4, [(0, 1)], lat)
    assert want["index"] == 0 and (want["volume"] == want["score"]).all() and want["score"] > 0
    same(device_search(N, cal, xyz, kept, p4, [(0, 1)], lat), want)
    xyz, kept, p4 = scene(7, [33, 40], POSES3[:2])
    lat = line_lattice(600, span=0.4)
    full = M.search(xyz, kept, p4, [(0, 1)], lat)
    twin = (full["index"] + 300) % 600                         # a twin of the winner in another tile
    lat["xs"][twin] = lat["xs"][full["index"]]
    want = M.search(xyz, kept, p4, [(0, 1)], lat)
    assert want["index"] == min(full["index"], twin) and want["volume"].reshape(-1)[max(full["index"], twin)] == want["score"]
    same(device_search(N, cal, xyz, kept, p4, [(0, 1)], lat), want)


def test_two_chunks_of_candidates(N):
    """a handle made for 1024 pairs holds the sums of 4096 candidates at once: 4500 candidates take two chunks"""
    xyz, kept, p4 = scene(31, [5, 6, 4], POSES3, n_points=8)
    lat = line_lattice(4500, span=0.5)
    pairs = [(0, 1), (1, 2), (2, 0)]
    want = M.search(xyz, kept, p4, pairs, lat)
    c = N.Calibrator(1024, 8, 5000)
    try:
        same(device_search(N, c, xyz, kept, p4, pairs, lat), want)
        assert want["index"] < 4096
        lat["xs"] = lat["xs"] + (lat["xs"][want["index"]] - lat["xs"][4300])      # the winner now lies in the second chunk
        want2 = M.search(xyz, kept, p4, pairs, lat)
        assert want2["index"] >= 4096
        same(device_search(N, c, xyz, kept, p4, pairs, lat), want2)
    finally:
        c.close()


def test_batch_invariance(N, cal):
    """the same bits for a pair set alone, inside a larger bank at other slots, with and without the volume, on a side stream and
    on a second run"""
    import torch
    xyz, kept, p4 = scene(41, [64, 70, 61], POSES3)
    pairs = [(0, 1), (1, 2)]
    lat = M.lattice(0.2, 0.05, 0.03, 0.05, 0.05, 0.06, 0.02, 0.04)
    want = M.search(xyz, kept, p4, pairs, lat)
    first = device_search(N, cal, xyz, kept, p4, pairs, lat)
    same(first, want, "alone")
    other, okept, op4 = scene(42, [100, 3, 80, 9], ((3, 3, 0.0), (1, 1, 1.0), (0, 2, 2.0), (5, 5, 0.3)))
    bank = np.concatenate([other[:2], xyz[2:3], other[2:], xyz[0:2]])
    bkept = np.concatenate([okept[:2], kept[2:3], okept[2:], kept[0:2]])
    bp4 = np.concatenate([op4[:2], p4[2:3], op4[2:], p4[0:2]])
    same(device_search(N, cal, bank, bkept, bp4, [(5, 6), (6, 2)], lat), want, "inside a larger bank")
    no_vol = device_search(N, cal, xyz, kept, p4, pairs, lat, want_volume=False)
    same(no_vol, want, "without the volume")
    side = torch.cuda.Stream()
    same(device_search(N, cal, xyz, kept, p4, pairs, lat, stream=side), want, "side stream")
    same(device_search(N, cal, xyz, kept, p4, pairs, lat), want, "second run")
    big = N.Calibrator(7, NP + 5, 9000)                         # another handle: other scratch strides
    try:
        same(device_search(N, big, xyz, kept, p4, pairs, lat), want, "another handle")
    finally:
        big.close()


def test_a_pair_that_names_no_scan_is_flagged(N, cal):
    xyz, kept, p4 = scene(41, [64, 70, 61], POSES3)
    want = M.search(xyz, kept, p4, [(0, 1)], SMALL)
    got = device_search(N, cal, xyz, kept, p4, [(0, 1), (1, 3)], SMALL)
    assert got["flags"] == N.CALIB_BAD_PAIR and np.array_equal(bits(got["volume"]), bits(want["volume"]))
    with pytest.raises(N.NdtGpuError) as e:
        cal.search(xyz, kept, p4, [(0, 1), (1, 3)], SMALL)
    assert e.value.status == -1


def test_planted_offset_at_181_beams(N):
    """the host form on the fixture's clouds: the model's volume bit for bit, and the planted node wins"""
    f = X.planted()
    want = X.planted_model()
    c = N.Calibrator(8, 181, 512)
    try:
        got = c.search(f["xyz"], f["n_kept"], f["poses4"], f["pairs"], f["lattice"], want_volume=True)
    finally:
        c.close()
    same(got, want)
    assert (got["ix"], got["iy"], got["iyaw"]) == X.PLANTED_NODE


def test_projector_output_feeds_the_search_on_the_device(N):
    """ScanProjector.project_device -> Calibrator.search_device with no host visit in between: the ranges of the planted fixture.
    The model takes the clouds the device projected (their x and y may differ from the NumPy projection's by one float32 ulp)"""
    import torch
    f = X.planted()
    dev = torch.device("cuda", 0)
    n, nb = f["ranges"].shape
    sp = N.ScanProjector(n, nb)
    c = N.Calibrator(8, nb, 512)
    try:
        rt = torch.as_tensor(f["ranges"], device=dev)
        xyz = torch.zeros((n, nb, 4), dtype=torch.float32, device=dev)
        kept = torch.zeros(n, dtype=torch.int32, device=dev)
        res = torch.zeros(6, dtype=torch.int32, device=dev)
        vol = torch.zeros(11 * 10 * 4, dtype=torch.float64, device=dev)
        poses = torch.as_tensor(f["poses4"], device=dev)
        pairs = torch.as_tensor(f["pairs"].view(np.int32), device=dev)
        sp.project_device(rt, xyz, f["angle_min"], f["angle_increment"], n_kept_t=kept, r_min=0.3, r_max=20.0)
        c.search_device(xyz, kept, poses, pairs, f["lattice"], res, volume_t=vol)
        torch.cuda.synchronize()
        r = N.Calibrator.read_result(res)
        clouds, nk = xyz.cpu().numpy()[:, :, :3], kept.cpu().numpy().view(np.uint32)
    finally:
        c.close()
        sp.close()
    assert nk.tolist() == f["n_kept"].tolist()
    want = M.search(clouds, nk, f["poses4"], f["pairs"], f["lattice"])
    assert np.array_equal(bits(vol.cpu().numpy()), bits(want["volume"].reshape(-1)))
    assert bits(r["score"]) == bits(want["score"]) and int(r["index"]) == want["index"] and int(r["flags"]) == 0
    assert np.unravel_index(int(r["index"]), (11, 10, 4)) == X.PLANTED_NODE


def test_close_returns_every_resource(N):
    start = N.binding.live_resources()
    c = N.Calibrator(3, 64, 300)
    xyz, kept, p4 = scene(3, [20, 22], POSES3[:2], n_points=64)
    c.search(xyz, kept, p4, [(0, 1)], SMALL)
    assert N.binding.live_resources() != start
    c.close()
    assert N.binding.live_resources() == start
    with pytest.raises(N.NdtGpuError) as e:
        cal = N.Calibrator(2, 16, 10)
        try:
            cal.search(np.zeros((2, 16, 3), dtype=np.float32), [1, 1], M.poses4(POSES3[:2]), [(0, 1)], SMALL)
        finally:
            cal.close()
    assert e.value.status == -4 and N.binding.live_resources() == start
