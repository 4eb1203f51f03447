"""Every handle gives back what it took (-m gpu): ndtgpu_live_resources counts the device buffers, pinned buffers, events and
streams the library owns, and after create / use / destroy the four counts are those from before -- exactly, they are integers.

Per case: one warm-up cycle (the grid-barrier matcher's per-device ordering event and the like are made once and stay), the
baseline, three more cycles.  The "use" step reaches every lazily created member of the handle and grows each grow-only buffer
once (the same call with the larger cloud or more pairs).  While the handle is alive at least one resource of every kind the
subsystem uses must be counted: a subsystem that went around the owning types would otherwise pass trivially.

Shapes: 0.5 m cells on a 20 m x 20 m x 1 m grid, 2 to 4 maps, clouds of 256 points and 1024 for the grow step.  The handles
without a map set (link gate, feature bank, scan projector, calibrator, localisation monitor) take the smallest shapes that reach
every lazily created member: a few scans of 64 to 180 beams, lattices of 3 x 3 x 2 and 5 x 5 x 4 nodes."""
import ctypes as C

import numpy as np
import pytest

import calib_fixtures
import flirt_fixtures
import linkgate_fixtures
import locmon_fixtures

pytestmark = pytest.mark.gpu

RES, SIZE = 0.5, [20.0, 20.0, 1.0]
SMALL, LARGE = 256, 1024
DEVICE, PINNED, EVENTS, STREAMS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def live():
    from ndt_feature_graph_amd import binding
    return binding.live_resources


def room_scan(n_points, seed, pose=(0.0, 0.0, 0.0)):
    """n_points on the walls of a 16 m x 12 m room, seen from `pose` (x, y, yaw): float32 [n_points, 3]"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 4.0, n_points)
    side, u = t.astype(np.int64), t - np.floor(t)
    hx, hy = 8.0, 6.0
    x = np.choose(side, [-hx + 2 * hx * u, np.full(n_points, hx), hx - 2 * hx * u, np.full(n_points, -hx)])
    y = np.choose(side, [np.full(n_points, -hy), -hy + 2 * hy * u, np.full(n_points, hy), hy - 2 * hy * u])
    p = np.stack([x, y], axis=1) + rng.normal(0.0, 0.02, (n_points, 2))
    c, s = np.cos(pose[2]), np.sin(pose[2])
    q = (p - np.array(pose[:2])) @ np.array([[c, -s], [s, c]])
    return np.concatenate([q, rng.normal(0.0, 0.005, (n_points, 1))], axis=1).astype(np.float32)


def clouds(count, n_points, seed=1, moved=False):
    pose = (0.2, -0.1, 0.03) if moved else (0.0, 0.0, 0.0)
    return np.stack([room_scan(n_points, seed + 17 * k, pose) for k in range(count)])


def eye(n):
    return np.tile(np.eye(4), (n, 1, 1))


def check_cycles(live, cycle, kinds):
    """cycle(): read the counts, create, use, read the counts, destroy -> (the counts just before the create -- with whatever
    the case itself needs beside the handle, a borrowed map set, already made --, the counts while the handle was alive)"""
    cycle()
    base = live()
    for _ in range(3):
        before, alive = cycle()
        assert live() == base
        for k in kinds:
            assert alive[k] > before[k], (k, alive, before)


def test_mapset(N, live, monkeypatch):
    import torch
    dev = torch.device("cuda:0")

    def cycle():
        st = torch.cuda.Stream(device=dev)
        before = live()
        ms = N.MapSet(RES, [0, 0, 0], SIZE, n_maps=4)
        ms.profiling(True)
        for n_maps, n_points, host_pairs, dev_pairs in ((2, SMALL, 1, 8), (4, LARGE, 2, 16)):
            pts = clouds(n_maps, n_points)
            pts_dev = torch.from_numpy(pts).to(dev)
            torch.cuda.synchronize()
            ms.build(pts_dev, range_limit=15.0, range_origins=np.zeros((n_maps, 3)), stream=st)       # device build, range origins
            monkeypatch.setenv("NDTGPU_HOST_PIPE", "0")
            ms.build(pts, range_limit=15.0)                                                          # host build, a single copy
            monkeypatch.setenv("NDTGPU_HOST_PIPE", "1")
            ms.build(pts, range_limit=15.0)                                                          # ... through the pinned ring
            monkeypatch.delenv("NDTGPU_HOST_PIPE")
            assert ms.last_kernel_ms(0) > 0.0
            idx = np.arange(host_pairs) % n_maps
            pinned = live()[PINNED]                                                                  # (the host ring is counted already)
            N.match_batch(ms, idx, ms, (idx + 1) % n_maps, eye(host_pairs))                          # grid-barrier area, pinned block
            assert live()[PINNED] == pinned + (1 if n_points == SMALL else 0)                        # ... made once, regrown in place
            k = torch.arange(dev_pairs, device=dev, dtype=torch.int32)
            ti, si = (k % n_maps).contiguous(), ((k + 1) % n_maps).contiguous()
            T16 = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).repeat(dev_pairs, 1).contiguous()
            res = torch.zeros((dev_pairs, 64), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            from ndt_feature_graph_amd import binding
            binding.match_batch_device(ms, ti, ms, si, T16, res, dev_pairs, stream=st)               # persistent work area
            st.synchronize()
            assert ms.last_kernel_ms(1) > 0.0
        ms.enable_occupancy()
        assert ms.occupied_cells_max() == 0
        alive = live()
        ms.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


@pytest.mark.parametrize("form", ["per_batch", "stream_fed"])
def test_registrar(N, live, form):
    import torch
    from ndt_feature_graph_amd import binding
    dev = torch.device("cuda:0")
    matcher_form = binding.MATCHER_PER_BATCH if form == "per_batch" else binding.MATCHER_STREAM_FED

    def cycle():
        before = live()
        reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=8, depth=2, matcher_form=matcher_form)
        assert reg.info()["matcher_form"] == matcher_form
        tg, sc = clouds(8, SMALL), clouds(8, SMALL, moved=True)
        tg_dev, sc_dev = torch.from_numpy(tg).to(dev), torch.from_numpy(sc).to(dev)
        T16 = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).repeat(8, 1).contiguous()
        res = torch.zeros((8, 64), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        reg.submit(tg_dev, sc_dev, T16, res, range_limit=15.0)                                       # the device entry
        reg.sync()
        _, r = reg.register_host(tg, sc, eye(8), range_limit=15.0)                                   # the host entry
        assert (r["n_source"] > 0).all() and (r["n_target"] > 0).all() and (r["iterations"] > 0).all()
        # ... and with the covariance, two sub-batches of larger clouds: every staging area grows
        _, r, cov, _ = reg.register_host(clouds(16, LARGE), clouds(16, LARGE, moved=True), eye(16), range_limit=15.0, covariance_mode=0)
        assert (r["n_source"] > 0).all() and np.isfinite(cov).all()
        reg.sync()
        assert (res.cpu().numpy().view(binding.RESULT_DTYPE)["n_source"] > 0).all()                  # (the device entry's)
        assert reg.info()["submitted"] == 4
        alive = live()
        reg.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, EVENTS, STREAMS) + ((PINNED,) if form == "stream_fed" else ()))


def test_registrar_failing_create(N, live):
    """the stream-fed form needs depth >= 2: the create fails after its map set was made, and leaves nothing behind"""
    from ndt_feature_graph_amd import binding

    def cycle():
        with pytest.raises(N.NdtGpuError) as e:
            N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=8, depth=1, matcher_form=binding.MATCHER_STREAM_FED)
        assert e.value.status == -1          # NDTGPU_ERR_INVALID
        return live(), live()

    check_cycles(live, cycle, ())


@pytest.mark.parametrize("nodes", ["own", "borrowed"])
def test_fuser_bank(N, live, nodes):
    import torch
    dev = torch.device("cuda:0")

    def cycle():
        node_maps = N.MapSet(RES, [0, 0, 0], SIZE, n_maps=2) if nodes == "borrowed" else None
        prm = N.fuser_params(resolution=RES, map_size_x=SIZE[0], map_size_y=SIZE[1], map_size_z=SIZE[2], sensor_range=15.0)
        before = live()
        bank = N.FuserBank(prm, 2, node_maps)
        step = eye(2)
        step[:, 0, 3] = 0.1
        bank.initialize(eye(2), torch.from_numpy(clouds(2, SMALL)).to(dev))
        bank.update(step, torch.from_numpy(clouds(2, SMALL, moved=True)).to(dev))
        bank.update(step, torch.from_numpy(clouds(2, LARGE, moved=True)).to(dev))                    # larger clouds
        bank.poses()
        pts = clouds(2, LARGE, seed=5, moved=True)                                                   # one *_host entry
        T = np.ascontiguousarray(np.transpose(step, (0, 2, 1))).reshape(2, 16)
        rc = N.lib().ndtgpu_fuser_update_batch_host(bank.h, C.c_size_t(0), C.c_size_t(2), T.ctypes.data_as(C.POINTER(C.c_double)),
                                                    C.c_void_p(pts.ctypes.data), C.c_size_t(LARGE), C.c_size_t(12), C.c_size_t(12 * LARGE),
                                                    C.c_int(1))
        assert rc == 0, N.lib().ndtgpu_last_error()
        T_now, r = bank.poses()
        assert np.isfinite(T_now).all() and (r["match"]["n_source"] > 0).all()
        alive = live()
        bank.close()
        if node_maps is not None:
            node_maps.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


def test_multires(N, live):
    import torch
    dev = torch.device("cuda:0")

    def cycle():
        before = live()
        mr = N.MultiRes([0, 0, 0], SIZE, resolutions=(0.5, 1.0), pairs_per_batch=2)                  # 3 pairs per call: two sub-batches
        tg_dev, sc_dev = torch.from_numpy(clouds(3, SMALL)).to(dev), torch.from_numpy(clouds(3, SMALL, moved=True)).to(dev)
        T16 = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).repeat(3, 1).contiguous()
        res = torch.zeros((3, 2 * 64), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        mr.register_device(tg_dev, sc_dev, T16, res, range_limit=15.0)
        torch.cuda.synchronize()
        _, r = mr.register_host(clouds(3, LARGE), clouds(3, LARGE, moved=True), eye(3), range_limit=15.0)   # larger clouds
        assert (r["n_source"] > 0).all()
        assert mr.info()["levels_fused"] + mr.info()["levels_unfused"] == 8
        alive = live()
        mr.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, EVENTS, STREAMS))


def test_mcl(N, live):
    import torch
    dev = torch.device("cuda:0")

    def cycle():
        ms = N.MapSet(RES, [0, 0, 0], SIZE, n_maps=2)
        ms.build(clouds(2, LARGE))
        before = live()
        mcl = N.MCL(ms, [0, 1], 64, scan_size=SIZE, seed=7)                                          # 2 filters x 64 particles
        mcl.initialize(np.zeros((2, 6)), np.full((2, 6), 0.05))
        mcl.update(eye(2), clouds(2, SMALL, moved=True))
        mcl.update(eye(2), clouds(2, LARGE, moved=True))                                             # larger clouds
        mcl.update(eye(2), torch.from_numpy(clouds(2, SMALL, moved=True)).to(dev))
        assert (mcl.mean()[1]["n_scan_cells"] > 0).all()
        assert np.isfinite(mcl.particles()[1]).all()
        alive = live()
        mcl.close()
        ms.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


def test_pgo(N, live):
    square = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, np.pi / 2], [1.0, 1.0, np.pi], [0.0, 1.0, -np.pi / 2]])
    ref, mov = [0, 1, 2, 3], [1, 2, 3, 0]
    meas = np.tile([1.0, 0.0, np.pi / 2], (4, 1))                                                    # every link: one side, a left turn

    def cycle():
        before = live()
        bank = N.PGO(2, 4, 4)                                                                        # 2 graphs of 4 nodes and 4 links
        for g in range(2):
            bank.set_graph(g, square + 0.05 * (g + 1) * np.array([[0, 0, 0], [1, -1, 1], [-1, 1, -1], [1, 1, 1]]), ref, mov, meas)
        bank.optimize()
        for g in range(2):
            assert bank.poses(g)[1]["iterations"] > 0
        alive = live()
        bank.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, EVENTS, STREAMS))


def lattice(nx, ny, nyaw, x0=0.2, y0=0.05, yaw0=0.02):
    """nx x ny x nyaw nodes around (x0, y0, yaw0): the tables Calibrator.search and LocalizationMonitor.adjust take"""
    yaws = yaw0 + 0.04 * (np.arange(nyaw) - (nyaw - 1) / 2)
    return dict(xs=x0 + 0.02 * (np.arange(nx) - (nx - 1) / 2), ys=y0 + 0.02 * (np.arange(ny) - (ny - 1) / 2), cs=np.cos(yaws), sn=np.sin(yaws))


def test_linkgate(N, live):
    _, node_T = linkgate_fixtures.walk(8, seed=3)

    def cycle():
        before = live()
        gate = N.LinkGate(8, 32)                                                                     # 8 nodes, 32 links
        gate.set_nodes(node_T)                                                                       # from the host
        ref, mov, T16 = gate.candidates(32, min_idx_dist=1, max_dist=100.0, max_angle=4.0, clip_cosine=1)
        count, overflow = gate.count()
        assert count == 28 and not overflow                                                          # every pair i < j of 8 nodes
        alive = live()
        gate.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, EVENTS, STREAMS))


def test_featbank(N, live):
    halls = {nb: np.stack([flirt_fixtures.hall(4100 + k, nb)[0] for k in range(4)]) for nb in (90, 180)}
    geometry = {nb: flirt_fixtures.hall(4100, nb)[1:] for nb in (90, 180)}

    def cycle():
        before = live()
        fm = N.FeatureMatcher(4, 64, 48)                                                             # 4 sets x 64 points x 48 values
        for n, nb in ((2, 90), (4, 180)):                                                            # ... then more, larger scans
            res, per_scan = fm.extract(np.arange(n), halls[nb][:n], *geometry[nb])
            assert res.shape == (n,) and len(per_scan) == n and (res["n_valid"] > 0).all()
            res, T, corr = fm.match(np.arange(n), (np.arange(n) + 1) % n)                            # n pairs
            assert res.shape == (n,) and T.shape == (n, 4, 4) and len(corr) == n
        alive = live()
        fm.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


def test_scanproj(N, live):
    rng = np.random.default_rng(11)

    def cycle():
        before = live()
        sp = N.ScanProjector(4, 128)
        for n, nb in ((2, 64), (4, 128)):                                                            # the host form; its staging grows
            xyz, kept = sp.project(rng.uniform(1.0, 20.0, (n, nb)), -1.0, 2.0 / nb)
            assert xyz.shape == (n, nb, 3) and (kept == nb).all()
        alive = live()
        sp.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


def test_calib(N, live):
    f = calib_fixtures.planted(n_beams=64)
    pairs = f["pairs"][:2]                                                                           # 2 pairs of 64-point scans
    assert len(pairs) == 2 and f["xyz"].shape[1] == 64

    def cycle():
        before = live()
        cal = N.Calibrator(2, 64, 100)
        r = cal.search(f["xyz"], f["n_kept"], f["poses4"], pairs, lattice(3, 3, 2))                   # the host form
        assert 0 <= r["index"] < 18 and r["volume"] is None
        r = cal.search(f["xyz"], f["n_kept"], f["poses4"], pairs, lattice(5, 5, 4), want_volume=True)  # staging and tables grow
        assert 0 <= r["index"] < 100 and r["volume"].shape == (5, 5, 4)
        alive = live()
        cal.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))


def test_locmon(N, live):
    rng = np.random.default_rng(13)
    grid = locmon_fixtures.random_grid(rng, 32, 32, 0.05)[None]                                      # one 32 x 32 grid
    ranges = rng.uniform(0.5, 3.0, (2, 64))                                                          # 64 beams
    q = locmon_fixtures.queries(rng.integers(0, 2, 16), 0, rng.uniform(0.5, 2.5, 16), rng.uniform(0.5, 2.5, 16), rng.uniform(-3.0, 3.0, 16))

    def cycle():
        before = live()
        mon = N.LocalizationMonitor(1, 32 * 32, 64, 18)
        mon.set_beams(64, -1.5, 3.0 / 64)
        mon.set_grids(grid, 0.1, [[0.0, 0.0]])                                                       # the host form: the device block
        for n in (4, 16):                                                                            # ... and the pinned block, grown
            assert mon.evaluate(ranges, q[:n]).shape == (n,)
        r = mon.adjust(ranges, 1, 0, lattice(3, 3, 2, x0=1.6, y0=1.6), want_volume=True)             # the lattice tables
        assert 0 <= r["index"] < 18 and r["volume"].shape == (3, 3, 2)
        alive = live()
        mon.close()
        return before, alive

    check_cycles(live, cycle, (DEVICE, PINNED, EVENTS, STREAMS))
