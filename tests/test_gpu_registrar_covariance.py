"""ndtgpu_register_batch_cov_device / _host: the registrar returns each pair's D2D covariance, computed in the matcher (-m gpu).

The reference's link update produces, per link, the registered pose (NDTMatcherD2D::match, graph.cpp:273) and the link covariance
(NDTMatcherD2D::covariance, graph.cpp:283-310).  The covariance entries must leave the plain registrar's poses and results as
they are (bit for bit), agree with ndtgpu_covariance_batch at the registered poses to rounding (only the order of the sums
differs) and with the CPU oracle, give the same bits in every form and split of the registrar, and describe pairs that did not
run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DET_FIELDS = ["converged", "iterations", "fevals", "exit_code", "score", "n_source", "n_target", "pair_terms_g", "pair_terms_h"]
RES, SIZE, RNG = 0.5, [100.0, 100.0, 1.0], 30.0


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def scene(N):
    """96 scan pairs of 20 k points in HBM"""
    import torch
    from ndt_feature_graph_amd import synth
    dev = torch.device("cuda", 0)
    B, NP = 96, 20000
    pr = synth.pair_2d(torch.arange(9001, 9001 + B, dtype=torch.int64, device=dev), NP, device=dev)
    both = torch.cat([pr["fixed"], pr["moving"]]).contiguous()
    T0 = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
    torch.cuda.synchronize()
    return {"B": B, "both": both, "T0": T0, "dev": dev}


def run(N, scene, reg, mode=None, stream=None, **params):
    """one call on `reg` -> (T16 [B, 16], results, cov [B, 36] or None, flags [B] or None), synchronised"""
    import torch
    from ndt_feature_graph_amd import binding
    B, both, dev = scene["B"], scene["both"], scene["dev"]
    T16 = scene["T0"].clone()
    res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev) if mode is not None else None
    flg = torch.full((B,), 99, dtype=torch.int32, device=dev) if mode is not None else None
    torch.cuda.synchronize()
    reg.submit(both[:B], both[B:], T16, res, range_limit=RNG, stream=stream, covariance_mode=mode, cov36_dev=cov, cov_flags_dev=flg,
               **params)
    reg.sync()
    r = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B)
    return (T16.cpu().numpy(), r, None if cov is None else cov.cpu().numpy(), None if flg is None else flg.cpu().numpy())


def assert_same_match(a, b):
    assert np.array_equal(a[0], b[0])
    for f in DET_FIELDS:
        assert np.array_equal(a[1][f], b[1][f]), f


def unchanged_on_host(T_in, T_out):
    return np.all(T_in.view(np.uint64) == T_out.view(np.uint64), axis=1)


def check_against_covariance_batch(N, scene, reg_set, out, mode, **params):
    """cov / SINGULAR / POSE_UNCHANGED of one call against ndtgpu_covariance_batch on the maps it built, at its poses"""
    from ndt_feature_graph_amd import binding
    B = scene["B"]
    T16, r, cov, flags = out
    T = T16.reshape(B, 4, 4).transpose(0, 2, 1)
    cref, sing = N.covariance(reg_set, np.arange(B), reg_set, np.arange(B) + B, T, mode=mode, **params)
    cov = cov.reshape(B, 6, 6)
    for b in range(B):
        scale = np.abs(cref[b]).max()
        assert np.max(np.abs(cov[b] - cref[b])) <= 1e-8 * scale, (b, np.max(np.abs(cov[b] - cref[b])), scale)
    assert np.array_equal((flags & binding.COV_SINGULAR) != 0, sing != 0)
    assert np.array_equal((flags & binding.COV_POSE_UNCHANGED) != 0, unchanged_on_host(scene["T0"].cpu().numpy(), T16))
    assert not (flags & binding.COV_NOT_COMPUTED).any()
    return cref


@pytest.mark.parametrize("mode", [0, 1])
def test_plain_path_unchanged_and_covariance_batch_parity(N, scene, mode):
    """poses and deterministic fields are those of ndtgpu_register_batch_device; cov agrees with ndtgpu_covariance_batch"""
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=scene["B"], depth=1, max_cells=4096)
    plain = run(N, scene, reg)
    withc = run(N, scene, reg, mode=mode)
    assert_same_match(plain, withc)
    assert plain[1]["converged"].mean() > 0.8
    check_against_covariance_batch(N, scene, reg.mapset(0), withc, mode)
    reg.close()


def test_same_bits_in_every_form_and_split(N, scene):
    """per-batch form and stream-fed form (2 / 3 slots, 96 / 176 matcher workgroups, depth 2 / 8), sub-batches of 32 and 96"""
    for per in (32, 96):
        ref_reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=per, depth=1, max_cells=4096)
        ref = run(N, scene, ref_reg, mode=0)
        plain_ref = run(N, scene, ref_reg)
        ref_reg.close()
        assert_same_match(plain_ref, ref)
        configs = [dict(depth=2, matcher_form=1), dict(depth=2, matcher_form=2, matcher_slots=2, matcher_groups=96),
                   dict(depth=8, matcher_form=2, matcher_slots=3, matcher_groups=176),
                   dict(depth=8, matcher_form=2, matcher_slots=2, matcher_groups=176), dict(depth=2, matcher_slots=3)]
        for cfg in configs:
            reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=per, max_cells=4096, **cfg)
            for _ in range(2):                          # (the second call runs on a registrar past its calibration)
                out = run(N, scene, reg, mode=0)
                assert_same_match(ref, out)
                assert np.array_equal(out[2], ref[2]), cfg
                assert np.array_equal(out[3], ref[3]), cfg
            reg.close()


def test_calls_in_flight_on_two_streams(N, scene):
    import torch
    B, both, dev = scene["B"], scene["both"], scene["dev"]
    ref_reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=48, depth=1, max_cells=4096)
    ref = run(N, scene, ref_reg, mode=1)
    ref_reg.close()
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=48, depth=3, max_cells=4096)
    sa, sb, sc = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    outs = []
    for st in (sa, sb, sa, sb):
        with torch.cuda.stream(st):
            T16 = scene["T0"].clone()
            res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
            cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev)
            flg = torch.full((B,), 99, dtype=torch.int32, device=dev)
            reg.submit(both[:B], both[B:], T16, res, range_limit=RNG, stream=st, covariance_mode=1, cov36_dev=cov, cov_flags_dev=flg)
            outs.append((T16, res, cov, flg))
    reg.wait_stream(sc)
    with torch.cuda.stream(sc):
        copies = [(o[0].clone(), o[2].clone(), o[3].clone()) for o in outs]
    sc.synchronize()
    for T16, cov, flg in copies:
        assert np.array_equal(T16.cpu().numpy(), ref[0])
        assert np.array_equal(cov.cpu().numpy(), ref[2])
        assert np.array_equal(flg.cpu().numpy(), ref[3])
    reg.sync()
    reg.close()


def test_against_the_oracle(N, scene):
    """8 pairs, the longest registrations among them, against oracle.covariance at the registered pose; symmetric, PSD"""
    import oracle as O
    B, both = scene["B"], scene["both"]
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=B, depth=1, max_cells=4096)
    for mode in (0, 1):
        T16, r, cov, flags = run(N, scene, reg, mode=mode)
        T = T16.reshape(B, 4, 4).transpose(0, 2, 1)
        cov = cov.reshape(B, 6, 6)
        longest = np.argsort(-r["iterations"], kind="stable")[:4]
        picks = sorted(set(longest.tolist()) | set(np.linspace(0, B - 1, 8).astype(int).tolist()))
        assert len(picks) >= 8
        for b in picks:
            ot = O.OracleMap(RES, [0, 0, 0], SIZE); ot.load_points(both[b].cpu().numpy(), RNG); ot.compute_cells()
            os_ = O.OracleMap(RES, [0, 0, 0], SIZE); os_.load_points(both[B + b].cpu().numpy(), RNG); os_.compute_cells()
            co = O.covariance(ot, os_, T[b], mode=mode)
            scale = np.abs(co).max()
            assert scale > 0
            assert np.max(np.abs(cov[b] - co)) < 1e-7 * scale, (mode, b, np.max(np.abs(cov[b] - co)) / scale)
            assert np.max(np.abs(cov[b] - cov[b].T)) < 1e-9 * scale
            assert np.linalg.eigvalsh(0.5 * (cov[b] + cov[b].T)).min() > -1e-9 * scale
    reg.close()


def test_overflowed_maps_are_not_computed(N, scene):
    from ndt_feature_graph_amd import binding
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=scene["B"], depth=1, max_cells=128)
    plain = run(N, scene, reg)
    T16, r, cov, flags = out = run(N, scene, reg, mode=0)
    assert_same_match(plain, out)
    bad = r["exit_code"] == -3
    assert bad.any()
    assert np.array_equal((flags & binding.COV_NOT_COMPUTED) != 0, bad)
    assert np.all(flags[bad] == binding.COV_NOT_COMPUTED)
    assert np.all(cov[bad] == 0.0)
    reg.close()


def test_planar_dof_mask_gives_the_full_covariance(N, scene):
    """NDTMatcherD2D_2D (dof_mask 0x23): the registration is planar, the covariance the full 6x6 of ndtgpu_covariance_batch"""
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=scene["B"], depth=1, max_cells=4096)
    plain = run(N, scene, reg, dof_mask=0x23)
    out = run(N, scene, reg, mode=0, dof_mask=0x23)
    assert_same_match(plain, out)
    cref = check_against_covariance_batch(N, scene, reg.mapset(0), out, 0, dof_mask=0x23)
    c = out[2].reshape(-1, 6, 6)
    assert np.abs(c[:, 2:5, 2:5]).max() > 0 and np.abs(cref[:, 2:5, 2:5]).max() > 0      # z / roll / pitch are there
    reg.close()


def test_bad_mode_refused(N, scene):
    import torch
    B, both, dev = scene["B"], scene["both"], scene["dev"]
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=B, depth=2, max_cells=4096)
    T16 = scene["T0"].clone()
    res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    cov = torch.zeros((B, 36), dtype=torch.float64, device=dev)
    flg = torch.zeros((B,), dtype=torch.int32, device=dev)
    for mode in (2, -1):
        with pytest.raises(N.NdtGpuError):
            reg.submit(both[:B], both[B:], T16, res, range_limit=RNG, covariance_mode=mode, cov36_dev=cov, cov_flags_dev=flg)
    with pytest.raises(N.NdtGpuError):
        reg.register_host(both[:4].cpu().numpy(), both[B:B + 4].cpu().numpy(), np.tile(np.eye(4), (4, 1, 1)), covariance_mode=2)
    reg.sync()
    reg.close()


def test_calls_with_and_without_covariance_alternate(N, scene):
    """one stream-fed registrar, plain and covariance calls in turn: each gives its own bits, and wait_stream on a caller stream
    orders reading cov after the call"""
    import torch
    B, both, dev = scene["B"], scene["both"], scene["dev"]
    ref_reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=48, depth=1, max_cells=4096)
    ref_plain = run(N, scene, ref_reg)
    ref_cov = run(N, scene, ref_reg, mode=0)
    ref_reg.close()
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=48, depth=4, max_cells=4096)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    outs, keep = [], []
    for k in range(6):
        with_cov = k % 2 == 1
        T16 = scene["T0"].clone()
        res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
        cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev) if with_cov else None
        flg = torch.full((B,), 99, dtype=torch.int32, device=dev) if with_cov else None
        torch.cuda.current_stream().synchronize()
        t = reg.submit(both[:B], both[B:], T16, res, range_limit=RNG, covariance_mode=0 if with_cov else None, cov36_dev=cov,
                       cov_flags_dev=flg)
        keep.append((T16, res, cov, flg))                 # (the call writes them until it is complete)
        reg.wait_stream(side, ticket=t)
        with torch.cuda.stream(side):
            outs.append((with_cov, T16.clone(), res.clone(), None if cov is None else cov.clone(), None if flg is None else flg.clone()))
    side.synchronize()
    from ndt_feature_graph_amd import binding
    for with_cov, T16, res, cov, flg in outs:
        r = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B)
        assert_same_match(ref_cov if with_cov else ref_plain, (T16.cpu().numpy(), r))
        if with_cov:
            assert np.array_equal(cov.cpu().numpy(), ref_cov[2])
            assert np.array_equal(flg.cpu().numpy(), ref_cov[3])
    reg.sync()
    reg.close()


def test_grid_barrier_sub_batches(N, scene):
    """sets with room for >= 16384 cells per map and sub-batches of at most half as many pairs as CUs go to the grid-barrier /
    pool matcher: their covariance comes from a follow-on ndtgpu_covariance_batch launch -- its bits, its flags"""
    B = scene["B"]
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=B, depth=1, max_cells=16384)
    plain = run(N, scene, reg)
    out = run(N, scene, reg, mode=1)
    assert_same_match(plain, out)
    check_against_covariance_batch(N, scene, reg.mapset(0), out, 1)
    reg.close()


def test_host_form_equals_device_form(N, scene):
    """the host form against the device form on buffers laid out like the host form's staging (sources behind targets: ONE
    build launch per sub-batch of 40 pairs, the launches the host form makes)"""
    import torch
    from ndt_feature_graph_amd import binding
    B, both, dev = scene["B"], scene["both"], scene["dev"]
    per = 40
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=per, depth=2, max_cells=4096)
    T16 = scene["T0"].clone()
    res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev)
    flg = torch.full((B,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for off in range(0, B, per):
        p = min(per, B - off)
        pack = torch.cat([both[off:off + p], both[B + off:B + off + p]]).contiguous()
        reg.submit(pack[:p], pack[p:], T16[off:off + p], res[off:off + p], range_limit=RNG, covariance_mode=0,
                   cov36_dev=cov[off:off + p], cov_flags_dev=flg[off:off + p])
        reg.sync()
    r_ref = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B)
    reg.close()
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=per, depth=2, max_cells=4096)
    scans = both.cpu().numpy()
    T_init = scene["T0"].cpu().numpy().reshape(B, 4, 4).transpose(0, 2, 1)
    for _ in range(2):                                            # (again: the staging areas are reused)
        T, r, c, f = reg.register_host(scans[:B], scans[B:], T_init, range_limit=RNG, covariance_mode=0)
        assert np.array_equal(T.transpose(0, 2, 1).reshape(B, 16), T16.cpu().numpy())
        for fld in DET_FIELDS:
            assert np.array_equal(r[fld], r_ref[fld]), fld
        assert c.shape == (B, 6, 6) and np.array_equal(c.reshape(B, 36), cov.cpu().numpy())
        assert np.array_equal(f, flg.cpu().numpy())
    reg.close()


def test_full_size_against_covariance_batch(N):
    """two calls of the bench's workload (1024 pairs x 100 k points) through a default registrar; 32 sampled pairs, the 8 longest
    among them, against ndtgpu_covariance_batch on the same scans at the registered poses"""
    import torch
    from ndt_feature_graph_amd import binding, synth
    dev = torch.device("cuda", 0)
    B, NP = 1024, 100000
    pr = synth.pair_2d(torch.arange(1, B + 1, dtype=torch.int64, device=dev), NP, device=dev, chunk_bytes=2 << 30)
    both = torch.cat([pr["fixed"], pr["moving"]]).contiguous()
    T0 = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=B, depth=8, max_cells=4096)
    outs = []
    torch.cuda.synchronize()
    for _ in range(2):
        T16 = T0.clone()
        res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
        cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev)
        flg = torch.full((B,), 99, dtype=torch.int32, device=dev)
        reg.submit(both[:B], both[B:], T16, res, range_limit=RNG, covariance_mode=0, cov36_dev=cov, cov_flags_dev=flg)
        outs.append((T16, res, cov, flg))
    reg.sync()
    T16, res, cov, flg = [x.cpu().numpy() for x in outs[-1]]
    for o in outs[:-1]:
        assert np.array_equal(o[2].cpu().numpy(), cov) and np.array_equal(o[3].cpu().numpy(), flg)
    r = res.view(binding.RESULT_DTYPE).reshape(B)
    assert r["converged"].mean() > 0.8 and not (flg & binding.COV_NOT_COMPUTED).any()
    longest = np.argsort(-r["iterations"], kind="stable")[:8]
    picks = np.unique(np.concatenate([longest, np.linspace(0, B - 1, 24).astype(int)]))
    k = len(picks)
    # (the second call was the registrar's second sub-batch: its maps are in internal map set 1)
    ms = reg.mapset(1)
    T = T16.reshape(B, 4, 4).transpose(0, 2, 1)[picks]
    cref, sing = N.covariance(ms, picks, ms, picks + B, T, mode=0)
    c = cov.reshape(B, 6, 6)[picks]
    for i in range(k):
        scale = np.abs(cref[i]).max()
        assert np.max(np.abs(c[i] - cref[i])) <= 1e-8 * scale, (picks[i], np.max(np.abs(c[i] - cref[i])) / scale)
    assert np.array_equal((flg[picks] & binding.COV_SINGULAR) != 0, sing != 0)
    reg.close()
