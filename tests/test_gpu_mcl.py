"""The NDT Monte Carlo localisation bank on the device (ndtgpu_mcl_*, include/ndtgpu.h) against its NumPy restatement
(tests/mcl_model.py): likelihoods, batch independence, prediction, normalisation / SIR / mean, localisation and a full-size bank."""
import math

import numpy as np
import pytest
import torch

import mcl_model as M

pytestmark = pytest.mark.gpu

RES = 0.5
SCAN = [60.0, 60.0, 1.0]
CAP = 4096


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    if N.device_count() < 1:
        pytest.fail("no HIP device")
    return N


def chunk_of(cap):
    per = (cap + 15) // 16
    return max(1, (per + 255) // 256) * 256


def scans(poses, n_points, seed=1, noise_stream=0):
    from ndt_feature_graph_amd import synth
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    return synth.scan_2d([seed] * poses.shape[0], torch.tensor(poses), n_points, noise_stream=noise_stream).numpy()


def T2(x, y, yaw):
    return M.pose([x, y, 0.0], np.float64(0.0), np.float64(0.0), np.float64(yaw))


@pytest.fixture(scope="module")
def room(N):
    """map 0: the room seen from the origin (40 k points); map 1: the same cells with their covariances negated (set_cells)"""
    ms = N.MapSet(RES, [0, 0, 0], [60, 60, 1], n_maps=2, max_cells=CAP)
    pts = scans([[0.0, 0.0, 0.0]], 40000, noise_stream=5)
    ms.build(pts[:1], first=0)
    mean, cov, idx, _ = ms.export_cells(0)
    return dict(ms=ms, mean=mean, cov=cov, idx=idx, info=ms.info())


def map_model(room, i=0):
    mean, cov, idx, _ = room["ms"].export_cells(i)
    return M.MapModel(RES, [0, 0, 0], room["info"]["cells_per_axis"], mean, cov, idx)


def scan_cells(N, pts):
    sm = N.MapSet(RES, [0, 0, 0], SCAN, n_maps=1, max_cells=CAP)
    sm.build(pts[None])
    mean, cov, _, _ = sm.export_cells(0)
    return mean, M.sym6(cov)


QUIET = dict(motion_model=np.zeros(36), motion_model_offset=np.zeros(6), sir_varp_threshold=1e9, sir_max_iters_wo_resampling=1 << 30)


def bank(N, room, n_filters, n_particles, map_idx=0, **kw):
    prm = dict(scan_size=SCAN, max_scan_cells=CAP, seed=7)
    prm.update(kw)
    return N.MCL(room["ms"], [map_idx] * n_filters, n_particles, **prm)


def test_likelihoods_against_the_model(N, room):
    pts = scans([[0.3, -0.2, 0.1]], 12000, noise_stream=1)[0]
    smean, scov = scan_cells(N, pts)
    truth = T2(0.3, -0.2, 0.1)
    rng = np.random.default_rng(2)
    Ts = [truth, T2(100.0, 0.0, 0.0), T2(29.0, 0.0, 0.0)]                 # at the truth, outside the grid, half outside
    low = truth.copy()
    low[2, 3] = -0.2                  # every cell at z ~ -0.2: inside the grid, on the map's Gaussians, below zfilt_min -0.1 only
    Ts.append(low)
    for _ in range(60):
        Ts.append(T2(0.3 + rng.normal(0, 0.4), -0.2 + rng.normal(0, 0.4), 0.1 + rng.normal(0, 0.1)))
    Ts.append(M.pose([0.3, -0.2, 0.0], np.float64(0.2), np.float64(-0.1), np.float64(0.1)))   # tilted: many cells without a Gaussian
    Ts = np.stack(Ts)
    n = Ts.shape[0]
    f = bank(N, room, 1, n, **QUIET)
    f.set_particles(Ts[None])
    f.update(np.eye(4)[None], pts[None])
    _, _, lik = f.particles()
    ref, terms = M.likelihood(Ts, smean, scov, np.ones(smean.shape[0], bool), map_model(room), -5.0, chunk_of(CAP))
    assert np.allclose(lik[0], ref, rtol=1e-12, atol=0)
    assert lik[0][1] == 0.0 and lik[0][3] > 0.0 and 0 < lik[0][2] < lik[0][0]
    assert lik[0][0] == lik[0].max()
    _, res = f.mean()
    assert res["terms"][0] == terms and res["n_scan_cells"][0] == smean.shape[0] and res["overflow"][0] == 0

    # zfilt_min -0.1: the lowered particle loses every term to the z filter alone
    fz = bank(N, room, 1, n, zfilt_min=-0.1, **QUIET)
    fz.set_particles(Ts[None])
    fz.update(np.eye(4)[None], pts[None])
    _, _, likz = fz.particles()
    refz, termsz = M.likelihood(Ts, smean, scov, np.ones(smean.shape[0], bool), map_model(room), -0.1, chunk_of(CAP))
    assert np.allclose(likz[0], refz, rtol=1e-12, atol=0)
    assert likz[0][3] == 0.0 and likz[0][0] == lik[0][0]
    assert fz.mean()[1]["terms"][0] == termsz

    # subsample_level 0.5: the cells the model's draws keep, and nothing else
    fs = bank(N, room, 1, n, **QUIET)
    fs.set_particles(Ts[None])
    fs.update(np.eye(4)[None], pts[None], subsample_level=0.5)
    _, _, liks = fs.particles()
    keep = M.subsample_mask(7, 0, 0, smean.shape[0], 0.5)
    assert 0.3 < keep.mean() < 0.7
    refs, termss = M.likelihood(Ts, smean, scov, keep, map_model(room), -5.0, chunk_of(CAP))
    assert np.allclose(liks[0], refs, rtol=1e-12, atol=0)
    assert fs.mean()[1]["terms"][0] == termss and termss < terms

    # a singular combined covariance: map 1 holds the scan's own cells with negated covariances; at the identity C + c = 0
    cov33 = np.zeros((smean.shape[0], 3, 3))
    for k, c in enumerate(scov):
        cov33[k] = -np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    room["ms"].set_cells(1, smean, cov33)
    g = bank(N, room, 1, n, map_idx=1, **QUIET)
    Ts[0] = np.eye(4)
    g.set_particles(Ts[None])
    g.update(np.eye(4)[None], pts[None])
    _, _, lik1 = g.particles()
    ref1, _ = M.likelihood(Ts, smean, scov, np.ones(smean.shape[0], bool), map_model(room, 1), -5.0, chunk_of(CAP))
    assert lik1[0][0] == 0.0
    assert np.allclose(lik1[0], ref1, rtol=1e-12, atol=0)
    room["ms"].build(scans([[0.0, 0.0, 0.0]], 40000, noise_stream=5), first=1)


def _run_bank(N, room, n_filters, pieces, clouds, Tm):
    f = bank(N, room, n_filters, 256, motion_model=np.eye(6).ravel() * 0.2, motion_model_offset=np.full(6, 0.01) * [1, 1, 0, 0, 0, 1])
    f.initialize(np.tile([0.2, 0.1, 0, 0, 0, 0.05], (n_filters, 1)), np.tile([0.3, 0.3, 0, 0, 0, 0.05], (n_filters, 1)))
    for step in range(3):
        for first, count in pieces:
            f.update(Tm[first:first + count], torch.from_numpy(clouds[step, first:first + count]).cuda(), first=first,
                     subsample_level=0.7 if step == 1 else 1.0)
    torch.cuda.synchronize()
    return f.particles(), f.mean()


def test_batch_independence(N, room):
    n_f = 64
    clouds = np.stack([scans(np.tile([0.1 * s, 0.0, 0.02 * s], (n_f, 1)), 6000, noise_stream=10 + s) for s in range(3)])
    Tm = np.tile(T2(0.1, 0.0, 0.02), (n_f, 1, 1))
    (Ta, wa, la), (Ma, ra) = _run_bank(N, room, n_f, [(0, n_f)], clouds, Tm)
    (Tb, wb, lb), (Mb, rb) = _run_bank(N, room, n_f, [(0, 1), (1, 20), (21, 43)], clouds, Tm)
    (Tc, wc, lc), (Mc, rc) = _run_bank(N, room, 1, [(0, 1)], clouds[:, :1], Tm[:1])
    assert np.array_equal(Ta, Tb) and np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(Ma, Mb)
    assert np.array_equal(Ta[:1], Tc) and np.array_equal(wa[:1], wc) and np.array_equal(la[:1], lc) and np.array_equal(Ma[:1], Mc)
    assert np.array_equal(ra, rb) and np.array_equal(ra[:1], rc)
    assert not np.array_equal(Ta[0], Ta[1])                  # (the filters' draws differ)


def test_predict_against_the_models_generator(N, room):
    n = 2000
    mm = np.diag([0.2, 0.3, 0.1, 0.05, 0.05, 0.2]).ravel()
    off = np.array([0.01, 0.02, 0.003, 0.001, 0.002, 0.004])
    f = bank(N, room, 2, n, motion_model=mm, motion_model_offset=off, sir_varp_threshold=1e9, sir_max_iters_wo_resampling=1 << 30)
    pose6 = np.array([[0.5, -0.3, 0.0, 0.0, 0.0, 0.4], [1.0, 1.0, 0.0, 0.01, -0.02, -2.5]])
    sig6 = np.array([[0.5, 0.5, 0.1, 0.03, 0.03, 0.03], [0.2, 0.1, 0.0, 0.0, 0.0, 0.5]])
    f.initialize(pose6, sig6)
    T0, w0, _ = f.particles()
    for k in range(2):
        assert np.allclose(T0[k], M.initialize(7, k, 0, n, pose6[k], sig6[k]), rtol=0, atol=1e-12)
    assert np.all(w0 == 1.0 / n)
    Tm = np.stack([M.pose([0.4, -0.1, 0.0], np.float64(0.0), np.float64(0.0), np.float64(-0.3)),
                   M.pose([0.2, 0.05, 0.01], np.float64(0.02), np.float64(-0.01), np.float64(0.25))])
    f.update(Tm, scans([[0.0, 0.0, 0.0], [0.2, 0.0, 0.1]], 4000))
    T1, _, _ = f.particles()
    for k in range(2):
        tr, rot, sigma = M.motion(Tm[k], mm, off)
        ref = M.predict(7, k, 1, T0[k], tr, rot, sigma)
        assert np.allclose(T1[k], ref, rtol=0, atol=1e-12)
        inc = np.linalg.inv(T0[k]) @ T1[k]
        z = (inc[:, :3, 3] - tr) / sigma[:3]
        assert np.all(np.abs(z.mean(axis=0)) < 4.0 / math.sqrt(n))
        assert np.all(np.abs(z.std(axis=0) - 1.0) < 0.1)


def _model_sequence(N, room, n, steps, force_sir=False, threshold=0.006, max_iters=25, far=False):
    rng = np.random.default_rng(11)
    truth = T2(0.3, -0.2, 0.1)
    Ts = np.stack([T2(0.3 + rng.normal(0, 0.3) + (200.0 if far else 0.0), -0.2 + rng.normal(0, 0.3), 0.1 + rng.normal(0, 0.08))
                   for _ in range(n)])
    pts = scans([[0.3, -0.2, 0.1]], 8000, noise_stream=3)[0]
    smean, scov = scan_cells(N, pts)
    mp = map_model(room)
    f = bank(N, room, 1, n, motion_model=np.zeros(36), motion_model_offset=np.zeros(6), force_sir=int(force_sir),
             sir_varp_threshold=threshold, sir_max_iters_wo_resampling=max_iters)
    f.set_particles(Ts[None])
    w = np.full(n, 1.0 / n)
    since = 0
    seen = set()
    for c in range(steps):
        f.update(np.eye(4)[None], pts[None])
        Td, wd, ld = f.particles()
        Md, rd = f.mean()
        lik, _ = M.likelihood(Ts, smean, scov, np.ones(smean.shape[0], bool), mp, -5.0, chunk_of(CAP))
        assert np.allclose(ld[0], lik, rtol=1e-12, atol=0)
        w, S = M.normalise(w, lik)
        vp = M.var_p(w)
        sir, since = M.sir_decision(vp, since, force_sir, threshold, max_iters)
        assert abs(rd["var_p"][0] - vp) <= 1e-12 * max(vp, 1e-3)
        assert bool(rd["resampled"][0]) == sir and rd["since_sir"][0] == since and rd["draws"][0] == c + 1
        if sir:
            u0 = M.sir_offset(7, 0, c)
            thr = M.thresholds(u0, n)
            cum = M.cumulative_fx(w).astype(np.float64)
            gap = np.min(np.abs(thr[:, None] - cum[None, :])) / 2.0 ** M.FX_SHIFT
            assert gap > 1e-9, "a threshold lies within 1e-9 of a cumulative sum"
            j = M.systematic_resample(w, u0)
            Ts = Ts[j]
            w = np.full(n, 1.0 / n)
            assert np.array_equal(Td[0], Ts)
        else:
            assert np.allclose(Td[0], Ts, rtol=0, atol=0)
        assert np.allclose(wd[0], w, rtol=1e-12, atol=1e-15)
        assert np.allclose(Md[0], M.mean(Ts, w), rtol=0, atol=1e-9)
        seen.add(sir)
    return seen


def test_normalise_sir_and_mean_against_the_model(N, room):
    assert True in _model_sequence(N, room, 300, 4)
    assert _model_sequence(N, room, 300, 5, threshold=1e9, max_iters=2) == {False, True}     # sinceSIR > 2 forces the 4th


def test_force_sir_and_all_zero_likelihoods(N, room):
    assert _model_sequence(N, room, 200, 3, force_sir=True) == {True}
    # every particle far outside the map: lik 0, weights fall back to 1/N, varP 0
    assert _model_sequence(N, room, 200, 3, far=True, threshold=0.006, max_iters=25) == {False}
    assert _model_sequence(N, room, 200, 2, far=True, force_sir=True) == {True}


def _angle(T):
    return math.atan2(T[1, 0], T[0, 0])


def test_tracking_converges(N, room):
    """16 filters x 1000 particles follow 30 steps of noisy odometry.  Motion model: sigma = diag(0.1, 0.1, 0, 0, 0, 0.1) |incr| +
    (0.02, 0.02, 0, 0, 0, 0.01)."""
    n_f, n, steps = 16, 1000, 30
    mm = np.diag([0.1, 0.1, 0.0, 0.0, 0.0, 0.1]).ravel()
    off = np.array([0.02, 0.02, 0.0, 0.0, 0.0, 0.01])
    f = bank(N, room, n_f, n, motion_model=mm, motion_model_offset=off)
    truth = [(0.05 * s, 0.03 * s, 0.01 * s) for s in range(steps + 1)]
    p0 = truth[0]
    f.initialize(np.tile([p0[0] + 0.35, p0[1] - 0.35, 0, 0, 0, p0[2] + math.radians(5)], (n_f, 1)),
                 np.tile([0.5, 0.5, 0, 0, 0, math.radians(5)], (n_f, 1)))
    rng = np.random.default_rng(5)
    for s in range(1, steps + 1):
        inc = np.linalg.inv(T2(*truth[s - 1])) @ T2(*truth[s])
        odo = inc @ T2(rng.normal(0, 0.01), rng.normal(0, 0.01), rng.normal(0, math.radians(0.2)))
        pts = scans(np.tile(truth[s], (n_f, 1)), 8000, noise_stream=20 + s)
        f.update(np.tile(odo, (n_f, 1, 1)), torch.from_numpy(pts).cuda())
    Mn, res = f.mean()
    Tt = T2(*truth[-1])
    for k in range(n_f):
        dt = np.linalg.norm(Mn[k][:2, 3] - Tt[:2, 3])
        da = abs(math.remainder(_angle(Mn[k]) - _angle(Tt), 2 * math.pi))
        assert dt < 0.1 and da < math.radians(1.0), (k, dt, math.degrees(da))
    assert np.all(res["overflow"] == 0)


def test_global_localisation(N, room):
    """20 000 particles spread over 6 m x 6 m x 360 degrees converge within 0.2 m / 2 degrees."""
    truth = (0.7, -0.4, 0.6)
    pts = scans([truth], 12000, noise_stream=40)
    # the scene has no near-symmetric pose: on a grid of poses, every pose 1 m / 20 degrees from the truth scores well below it
    xs = np.arange(-3.0, 3.01, 0.25)
    ys = np.arange(-3.0, 3.01, 0.25)
    yaws = np.radians(np.arange(0, 360, 5))
    G = np.array([(x, y, a) for x in xs for y in ys for a in yaws])
    g = bank(N, room, 1, G.shape[0] + 1, **QUIET)
    Ts = np.stack([T2(*p) for p in G] + [T2(*truth)])
    g.set_particles(Ts[None])
    g.update(np.eye(4)[None], pts)
    _, _, lik = g.particles()
    far = (np.hypot(G[:, 0] - truth[0], G[:, 1] - truth[1]) > 1.0) | \
        (np.abs(np.remainder(G[:, 2] - truth[2] + np.pi, 2 * np.pi) - np.pi) > math.radians(20))
    assert lik[0][:-1][far].max() < 0.8 * lik[0][-1]

    n = 20000
    rng = np.random.default_rng(9)
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-math.pi, math.pi, n)], axis=1)
    f = bank(N, room, 1, n, motion_model=np.diag([0.1, 0.1, 0, 0, 0, 0.1]).ravel(), motion_model_offset=[0.02, 0.02, 0, 0, 0, 0.01])
    f.set_particles(np.stack([T2(*p) for p in P])[None])
    for s in range(15):
        f.update(np.eye(4)[None], scans([truth], 12000, noise_stream=41 + s))
    Mn, _ = f.mean()
    Tt = T2(*truth)
    dt = np.linalg.norm(Mn[0][:2, 3] - Tt[:2, 3])
    da = abs(math.remainder(_angle(Mn[0]) - _angle(Tt), 2 * math.pi))
    assert dt < 0.2 and da < math.radians(2.0), (dt, math.degrees(da))


def test_full_size_bank(N, room):
    """64 x 4096 particles x 20 k-point scans: no overflow, and the same bits as per-filter calls."""
    n_f, n = 64, 4096
    pts = torch.from_numpy(scans(np.tile([0.2, 0.1, 0.05], (n_f, 1)), 20000, noise_stream=60)).cuda()
    Tm = np.tile(T2(0.05, 0.0, 0.01), (n_f, 1, 1))
    out = []
    for per_filter in (False, True):
        f = bank(N, room, n_f, n)
        f.initialize(np.tile([0.15, 0.1, 0, 0, 0, 0.04], (n_f, 1)), np.tile([0.3, 0.3, 0, 0, 0, 0.05], (n_f, 1)))
        for _ in range(2):
            if per_filter:
                for k in range(n_f):
                    f.update(Tm[k:k + 1], pts[k:k + 1], first=k)
            else:
                f.update(Tm, pts)
        torch.cuda.synchronize()
        out.append((f.particles(), f.mean()))
    (Ta, wa, la), (Ma, ra) = out[0]
    (Tb, wb, lb), (Mb, rb) = out[1]
    assert np.all(ra["overflow"] == 0) and np.all(ra["n_scan_cells"] > 100)
    assert np.array_equal(Ta, Tb) and np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(Ma, Mb)
    assert np.array_equal(ra, rb)


def test_likelihoods_in_a_fused_node_map(N, room):
    """an occupancy-enabled node map after a ray-traced insert (its cells live in the second cell array) against the model"""
    node = N.MapSet(RES, [0, 0, 0], [60, 60, 1], n_maps=1, max_cells=CAP)
    node.enable_occupancy()
    node.add_cloud(scans([[0.0, 0.0, 0.0]], 20000, noise_stream=6), np.zeros((1, 3)))
    mean, cov, idx, _ = node.export_cells(0)
    assert mean.shape[0] > 100
    mp = M.MapModel(RES, [0, 0, 0], node.info()["cells_per_axis"], mean, cov, idx)
    pts = scans([[0.3, -0.2, 0.1]], 12000, noise_stream=1)[0]
    smean, scov = scan_cells(N, pts)
    rng = np.random.default_rng(4)
    Ts = np.stack([T2(0.3, -0.2, 0.1)] + [T2(0.3 + rng.normal(0, 0.3), -0.2 + rng.normal(0, 0.3), 0.1 + rng.normal(0, 0.1))
                                          for _ in range(40)])
    f = N.MCL(node, [0], Ts.shape[0], scan_size=SCAN, max_scan_cells=CAP, seed=7, **QUIET)
    f.set_particles(Ts[None])
    f.update(np.eye(4)[None], pts[None])
    _, _, lik = f.particles()
    ref, terms = M.likelihood(Ts, smean, scov, np.ones(smean.shape[0], bool), mp, -5.0, chunk_of(CAP))
    assert np.allclose(lik[0], ref, rtol=1e-12, atol=0) and terms > 0
    assert f.mean()[1]["terms"][0] == terms


def test_bad_arguments_on_a_real_handle(N, room):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    p = binding.mcl_params(map_res=0.25)
    idx = (binding.C.c_uint32 * 1)(0)
    h = binding.C.c_void_p()
    assert L.ndtgpu_mcl_create(room["ms"].h, idx, binding.C.byref(p), 1, 10, binding.C.byref(h)) == -1      # resolution mismatch
    assert b"differs" in L.ndtgpu_last_error()
    idx[0] = 2                                                                                               # map index out of range
    assert L.ndtgpu_mcl_create(room["ms"].h, idx, binding.C.byref(binding.mcl_params()), 1, 10, binding.C.byref(h)) == -1
    f = bank(N, room, 4, 10)
    d = np.zeros(4 * 16)
    six = np.zeros(6)
    for first, count in ((0, 0), (4, 1), (3, 2), (5, 1)):
        assert L.ndtgpu_mcl_initialize(f.h, first, count, binding._dp(six), binding._dp(six)) == -1
        assert L.ndtgpu_mcl_update_host(f.h, first, count, binding._dp(d), 1.0, None, 0, 12, 0) == -1
        assert L.ndtgpu_mcl_particles(f.h, first, count, None, None, None) == -1
        assert L.ndtgpu_mcl_mean(f.h, first, count, None, None) == -1
        assert L.ndtgpu_mcl_set_particles(f.h, first, count, binding._dp(d), None) == -1
    with pytest.raises(ValueError):
        f.set_particles(np.tile(np.eye(4), (15, 1, 1)))          # not a whole set of 10
    with pytest.raises(ValueError):
        f.set_particles(np.tile(np.eye(4), (10, 1, 1)), weights=np.ones(9))
