"""ndtgpu_scanproj_project*: a batch of laser scans to the clouds the fuser bank and the registrar take, on the device (-m gpu).

Against tests/scanproject_model.py with the tolerances tests/test_scanproject_model.py derives: the kept set, the order, n_kept, z
and the pads are EXACT; x and y are within one float32 unit in the last place of the model's value (two fp64 cosine / sine
libraries, one rounding to float each).  Shapes: the smallest at which the kernels can go wrong -- one beam, a wave and its
neighbours, a tile (T = 1024 beams) and its neighbours, three tiles the last of which holds one beam."""
import numpy as np
import pytest

import flirt_fixtures as X
import scanproject_model as M

pytestmark = pytest.mark.gpu

T = 1024
A0, INC = -2.1, 0.0031
SENTINEL = 0x5A5A5A5A
ONE = int(np.float32(1.0).view(np.uint32))


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    assert N.SCANPROJECT_TILE == T == N.lib().ndtgpu_scanproj_tile()
    return N


@pytest.fixture(scope="module")
def sp(N):
    p = N.ScanProjector(8, 4 * T)
    yield p
    p.close()


def mixed_ranges(n, nb, seed):
    """kept and dropped beams interleaved in runs of every length: NaN, infinities, too near, too far, the gates themselves"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.6, 29.0, size=(n, nb))
    kind = rng.integers(0, 12, size=(n, nb))
    r[kind == 0] = np.nan
    r[kind == 1] = rng.uniform(0.0, 0.5, size=int((kind == 1).sum()))
    r[kind == 2] = rng.uniform(30.0, 50.0, size=int((kind == 2).sum()))
    r[kind == 3] = np.inf
    flat = r.reshape(-1)
    flat[rng.integers(0, flat.shape[0], size=8)] = [0.5, 30.0, np.nextafter(0.5, 1.0), np.nextafter(30.0, 0.0), -np.inf, 0.0, -3.0, 30.0]
    if nb > 600:
        r[0, 100:100 + 300] = np.nan                 # a run of dropped beams longer than a workgroup
    return r


def device_project(N, sp, ranges, a0=A0, inc=INC, ids=None, words=3, with_kept=True, stream=None, **prm):
    """project_device into fresh tensors -> (xyz uint32 [n, nb, words] bits, n_kept or None)"""
    import torch
    dev = torch.device("cuda", 0)
    n, nb = ranges.shape
    rt = torch.as_tensor(np.ascontiguousarray(ranges), device=dev)
    xyz = torch.full((n, nb, words), SENTINEL, dtype=torch.int32, device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev) if with_kept else None
    idt = None if ids is None else torch.as_tensor(np.asarray(ids, dtype=np.uint64).view(np.int64), device=dev)
    sp.project_device(rt, xyz.view(torch.float32), a0, inc, scan_ids_t=idt, n_kept_t=kept, stream=stream, **prm)
    torch.cuda.synchronize()
    return xyz.cpu().numpy().view(np.uint32), None if kept is None else kept.cpu().numpy().view(np.uint32)


def check_against_model(bits, n_kept, ranges, a0, inc, ids=None, what="", **prm):
    """bits uint32 [n, nb, >= 3]: the first three words of every row against the model"""
    want, want_kept = M.project(ranges, a0, inc, scan_ids=ids, **prm)
    if n_kept is not None:
        assert n_kept.tolist() == want_kept.tolist(), what
    got = np.ascontiguousarray(bits[:, :, :3]).view(np.float32)
    worst = 0.0
    for b in range(ranges.shape[0]):
        m = int(want_kept[b])
        assert np.array_equal(bits[b, m:, :3], np.full((ranges.shape[1] - m, 3), 0x7FC00000, dtype=np.uint32)), (what, b, "pads")
        assert not np.isnan(got[b, :m]).any(), (what, b, "a NaN among the kept rows: the kept set differs")
        assert np.array_equal(got[b, :m, 2].view(np.uint32), want[b, :m, 2].view(np.uint32)), (what, b, "z: the order or the draws differ")
        d = np.abs(got[b, :m, :2].astype(np.float64) - want[b, :m, :2].astype(np.float64))
        ulp = np.spacing(np.abs(want[b, :m, :2])).astype(np.float64)
        assert (d <= ulp).all(), (what, b, "x / y beyond one float32 ulp", float((d / ulp).max()))
        if m:
            worst = max(worst, float((d / ulp).max()))
    return worst


@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_against_the_model(N, sp, n_beams):
    """three scans: every beam kept, none kept, only the last beam kept"""
    rng = np.random.default_rng(n_beams)
    r = np.empty((3, n_beams))
    r[0] = rng.uniform(0.6, 29.0, size=n_beams)
    r[1] = np.where(np.arange(n_beams) % 3 == 0, np.nan, np.where(np.arange(n_beams) % 3 == 1, 0.2, 31.0))
    r[2] = 0.3
    r[2, -1] = 4.0
    bits, n_kept = device_project(N, sp, r, seed=3)
    assert n_kept.tolist() == [n_beams, 0, 1]
    worst = check_against_model(bits, n_kept, r, A0, INC, seed=3, what="%d beams" % n_beams)
    print("%d beams: worst |dx| %.0f float32 ulp" % (n_beams, worst))


@pytest.mark.parametrize("words", [3, 4, 8])
def test_strides_and_untouched_bytes(N, sp, words):
    """records of 12, 16 and 32 bytes, scans map_stride_bytes apart with a gap that is no multiple of a record, guard regions in
    front and behind: every byte the specification does not name keeps its sentinel, the fourth float is 1.0f from 16 bytes on,
    and n_kept_dev = NULL works"""
    import torch
    dev = torch.device("cuda", 0)
    n, nb, guard = 3, T + 5, 4096
    ms = nb * words + 5                              # words between the scans' blocks
    r = mixed_ranges(n, nb, 21)
    r[1] = 31.0                                      # a scan of pads only
    buf = torch.full((guard + n * ms + guard,), SENTINEL, dtype=torch.int32, device=dev)
    view = torch.as_strided(buf.view(torch.float32), (n, nb, words), (ms, words, 1), storage_offset=guard)
    rt = torch.as_tensor(r, device=dev)
    sp.project_device(rt, view, A0, INC, n_kept_t=None, seed=1)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().view(np.uint32)
    assert (raw[:guard] == SENTINEL).all() and (raw[guard + n * ms:] == SENTINEL).all(), "a guard region was written"
    named = min(words, 4)
    rows = np.empty((n, nb, words), dtype=np.uint32)
    for b in range(n):
        blk = raw[guard + b * ms: guard + (b + 1) * ms]
        rows[b] = blk[:nb * words].reshape(nb, words)
        assert (blk[nb * words:] == SENTINEL).all(), "the gap behind scan %d was written" % b
    assert (rows[:, :, named:] == SENTINEL).all(), "bytes behind a record's named floats were written"
    if words >= 4:
        assert (rows[:, :, 3] == ONE).all(), "the fourth float of every row, pads included, is 1.0f"
    check_against_model(rows, None, r, A0, INC, seed=1, what="%d words" % words)
    # the same rows as the packed call gives them
    packed, n_kept = device_project(N, sp, r, seed=1)
    assert np.array_equal(packed, rows[:, :, :3]) and n_kept.tolist() == M.project(r, A0, INC, seed=1)[1].tolist()


def test_same_bits_alone_and_in_any_batch(N, sp):
    """five scans with explicit ids: each equals the call that projects it alone and a call with the scans in another order; two
    runs of one call give the same bytes; scan_id_dev = NULL is ids 0 .. n - 1"""
    nb = 2 * T + 1
    ids = [7, 3, (1 << 40) + 1, 0, (1 << 64) - 2]
    r = mixed_ranges(5, nb, 33)
    prm = dict(seed=11, varz=0.05)
    allb, kept = device_project(N, sp, r, ids=ids, **prm)
    check_against_model(allb, kept, r, A0, INC, ids=ids, what="five scans", **prm)
    again, kept2 = device_project(N, sp, r, ids=ids, **prm)
    assert np.array_equal(allb, again) and np.array_equal(kept, kept2)
    for b in range(5):
        alone, k1 = device_project(N, sp, r[b:b + 1], ids=[ids[b]], **prm)
        assert np.array_equal(alone[0], allb[b]) and k1[0] == kept[b], "scan %d alone" % b
    perm = [3, 0, 4, 2, 1]
    pb, pk = device_project(N, sp, r[perm], ids=[ids[k] for k in perm], **prm)
    for j, k in enumerate(perm):
        assert np.array_equal(pb[j], allb[k]) and pk[j] == kept[k], "scan %d at position %d" % (k, j)
    null_ids, nk = device_project(N, sp, r, ids=None, **prm)
    explicit, ek = device_project(N, sp, r, ids=[0, 1, 2, 3, 4], **prm)
    assert np.array_equal(null_ids, explicit) and np.array_equal(nk, ek)
    assert not np.array_equal(null_ids[..., 2], allb[..., 2])            # (the ids do matter)


@pytest.mark.parametrize("stride", [12, 16])
def test_host_form_equals_device_form(N, sp, stride):
    nb = T + 65
    r = mixed_ranges(4, nb, 44)
    ids = [5, 6, 9, 1]
    xyz, kept = sp.project(r, A0, INC, scan_ids=ids, stride=stride, r_min=1.0, r_max=25.0, seed=2)
    bits, dk = device_project(N, sp, r, ids=ids, words=stride // 4, r_min=1.0, r_max=25.0, seed=2)
    assert xyz.dtype == np.float32 and xyz.shape == (4, nb, stride // 4)
    assert np.array_equal(xyz.view(np.uint32), bits) and np.array_equal(kept, dk)
    check_against_model(bits, dk, r, A0, INC, ids=ids, r_min=1.0, r_max=25.0, seed=2, what="host form")
    # no upper gate: r_max = +inf keeps every finite range above r_min
    xyz, kept = sp.project(r, A0, INC, stride=stride, r_max=float("inf"))
    assert kept.tolist() == [int((np.isfinite(r[b]) & (r[b] > 0.5)).sum()) for b in range(4)]


def test_n_kept_is_the_feature_extraction_s_n_valid(N, sp):
    """on the hall scans of the feature tests (720 beams) with some beams knocked out, n_kept equals ndtgpu_featbank_extract's
    n_valid for the same r_min / r_max: one ranges buffer serves both calls"""
    scans = [X.hall(s, 720) for s in (1, 2, 3, 4)]
    a0, inc = scans[0][1], scans[0][2]
    r = np.stack([s[0] for s in scans])
    r[0, 10:40] = np.nan
    r[1, ::9] = 0.3
    r[2, 700:] = np.inf
    r[3, 5] = 30.0
    fm = N.FeatureMatcher(4, 64)
    for gates in (dict(r_min=0.5, r_max=30.0), dict(r_min=2.0, r_max=9.0)):
        res, _ = fm.extract([0, 1, 2, 3], r, a0, inc, **gates)
        _, kept = sp.project(r, a0, inc, **gates)
        assert kept.tolist() == [int(x) for x in res["n_valid"]], gates
        assert kept.tolist() == [int(M.kept(r[b], **gates).sum()) for b in range(4)]
    assert kept[0] < 690
    fm.close()


def pose2d(x, y, yaw):
    Tm = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    Tm[:2, :2] = [[c, -s], [s, c]]
    Tm[0, 3], Tm[1, 3] = x, y
    return Tm


def test_one_stream_no_host_visit(N):
    """3 fusers, 1440 beams, the node maps of tests/test_gpu_fuser_bank.py.  Run A: project_device -> FuserBank.initialize, then
    project_device -> FuserBank.update twice, all on ONE stream with no synchronisation in between.  Run B: project, synchronise,
    copy the cloud to a fresh tensor, feed that.  The same pose bits and the same node-map cell bits."""
    import torch
    from ndt_feature_graph_amd import synth
    dev = torch.device("cuda", 0)
    Bn, nb, steps = 3, 1440, 2
    seeds = torch.as_tensor(np.arange(4100, 4100 + Bn))
    path = [np.array([[0.1 * k + 0.25 * s, -0.2 * k + 0.03 * s, 0.05 * k + 0.02 * s] for k in range(Bn)]) for s in range(steps + 1)]
    ranges, a0, inc = [], None, None
    for s in range(steps + 1):
        r, a0, inc = synth.scan_2d_ranges(seeds, torch.as_tensor(path[s]), nb, noise_stream=s)
        ranges.append(torch.as_tensor(r.numpy(), device=dev).contiguous())
    assert all(int(torch.isnan(r).sum()) < nb // 2 for r in ranges)
    Tm = [np.stack([np.linalg.inv(pose2d(*path[s][k])) @ pose2d(*path[s + 1][k]) @ pose2d(0.02, -0.01, 0.005) for k in range(Bn)])
          for s in range(steps)]
    T0 = np.stack([pose2d(*path[0][k]) for k in range(Bn)])
    prm = N.fuser_params(resolution=0.5, map_size_x=100.0, map_size_y=100.0, map_size_z=1.0, sensor_range=30.0, neighbours=2,
                         delta_score=1e-6, max_cells=4096, sensor_pose=pose2d(0.25, -0.05, 0.02))
    proj = N.ScanProjector(Bn, nb)
    out = {}
    for run in ("A", "B"):
        bank = N.FuserBank(prm, Bn)
        nodes, _ = bank.mapsets()
        clouds = [torch.empty((Bn, nb, 4), dtype=torch.float32, device=dev) for _ in range(steps + 1)]
        kept = [torch.zeros(Bn, dtype=torch.int32, device=dev) for _ in range(steps + 1)]
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        for s in range(steps + 1):
            proj.project_device(ranges[s], clouds[s], a0, inc, n_kept_t=kept[s], stream=st, seed=s)
            cloud = clouds[s]
            if run == "B":
                st.synchronize()
                cloud = clouds[s].clone()
                torch.cuda.synchronize()
            if s == 0:
                bank.initialize(T0, cloud, stream=st)
            else:
                bank.update(Tm[s - 1], cloud, stream=st)
        st.synchronize()
        Tn, res = bank.poses()
        cells = [nodes.export_cells(k) for k in range(Bn)]
        occ = [nodes.occupancy(k) for k in range(Bn)]
        out[run] = (Tn, res, cells, occ, [k.cpu().numpy() for k in kept])
        bank.close()
    proj.close()
    (Ta, ra, ca, oa, ka), (Tb, rb, cb, ob, kb) = out["A"], out["B"]
    assert all(np.array_equal(x, y) for x, y in zip(ka, kb)) and all((x > nb // 2).all() for x in ka)
    assert np.array_equal(Ta, Tb), "poses differ"
    for f in ("converged", "iterations", "fevals", "exit_code", "score", "n_source", "n_target"):         # (not the cycle counters)
        assert np.array_equal(ra["match"][f], rb["match"][f]), f
    assert np.array_equal(ra["Tmotion_est"], rb["Tmotion_est"]) and np.array_equal(ra["spose"], rb["spose"])
    assert ra["match"]["n_source"].min() > 10, "the registration had nothing to work on"
    for k in range(Bn):
        for x, y, name in zip(ca[k], cb[k], ("mean", "cov", "idx", "n")):
            assert np.array_equal(x, y), "node map %d: %s differs" % (k, name)
        assert len(ca[k][2]) > 20 and np.array_equal(oa[k], ob[k])


def test_lifecycle_and_capacity(N):
    from ndt_feature_graph_amd.binding import live_resources
    import torch
    torch.cuda.synchronize()
    before = live_resources()
    p = N.ScanProjector(2, 100)
    during = live_resources()
    assert during[0] == before[0] + 1 and during[2] == before[2] + 1 and during[3] == before[3] + 1       # tile counts, fence, stream
    r = np.full((2, 100), 3.0)
    xyz, kept = p.project(r, 0.0, 0.01)
    assert kept.tolist() == [100, 100]
    staged = live_resources()
    assert staged[0] == during[0] + 1 and staged[1] == during[1] + 1                                      # the host form's staging
    for bad in (np.full((3, 100), 3.0), np.full((1, 101), 3.0)):
        with pytest.raises(N.NdtGpuError) as e:
            p.project(bad, 0.0, 0.01)
        assert e.value.status == -4
    xyz0, kept0 = p.project(np.zeros((0, 100)), 0.0, 0.01)                                                # no scans: a no-op
    assert xyz0.shape == (0, 100, 3) and kept0.shape == (0,)
    p.close()
    assert live_resources() == before
    p.close()                                                                                             # (idempotent)
