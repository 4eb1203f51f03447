"""ndtgpu_register_multires_device / _host: coarse-to-fine D2D registration of raw scan pairs (-m gpu).

NDTMatcherD2D(irregular, useDefaultGridResolutions, resolutions).match(target_pc, source_pc, T, useInitialGuess)
(ndt_odom_debug.cpp:159-165, ndt_feature_pcl_eval.cpp:620-642).  What the entry returns must be, bit for bit, the chain of the
existing entries it replaces -- clouds moved on the host, ndtgpu_mapset_build and ndtgpu_match_batch_device per level, poses
composed on the host -- on grids and lists whose source builds go through the general build after a separate move (the default
list and {0.5, 1, 2, 4} at max_cells 0 on 100 x 100 x 1 m) and through the flat kernel that moves on load and hands the moved
cloud to the next level (FLAT: 64 x 64 x 2 m at max_cells 4096, where 0.5 m and 1 m are flat-grid levels and 2 m is not), and
within the contract's tolerance of the CPU oracle's composition of the same steps."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DET_FIELDS = ["converged", "iterations", "fevals", "exit_code", "score", "n_source", "n_target", "pair_terms_g", "pair_terms_h"]
SIZE, RNG = [100.0, 100.0, 1.0], 30.0
LISTS = [(0.2, 0.5, 1.0, 2.0), (0.5, 1.0, 2.0, 4.0)]


def _composition():
    spec = importlib.util.spec_from_file_location("multires_oracle_composition", os.path.join(HERE, "test_multires_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MO = _composition()


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def O():
    import oracle
    return oracle


@pytest.fixture(scope="module")
def scene(N):
    """24 scan pairs of 20 k points, initial guesses off by 0.3 m / 2 degrees"""
    import torch
    from ndt_feature_graph_amd import synth
    dev = torch.device("cuda", 0)
    B, NP = 24, 20000
    pr = synth.pair_2d(torch.arange(8101, 8101 + B, dtype=torch.int64), NP)
    T_gt = pr["T_gt"].numpy()
    T_init = np.stack([MO.pose_mul(T_gt[k], MO.T2d(0.3, -0.2, np.radians(2.0))) for k in range(B)])
    return {"B": B, "NP": NP, "fixed": pr["fixed"].numpy(), "moving": pr["moving"].numpy(), "T_init": T_init, "T_gt": T_gt,
            "fixed_dev": pr["fixed"].to(dev).contiguous(), "moving_dev": pr["moving"].to(dev).contiguous(), "dev": dev}


def T16_of(T):
    return np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64), (0, 2, 1))).reshape(-1, 16)


def T_of(T16):
    return np.transpose(np.asarray(T16).reshape(-1, 4, 4), (0, 2, 1)).copy()


def run_multires(N, sc, resolutions, T_init, use_initial_guess=1, pairs_per_batch=None, max_cells=0, n=None, size=SIZE, info=None,
                 rng=RNG):
    import torch
    from ndt_feature_graph_amd import binding
    n = sc["B"] if n is None else n
    mr = N.MultiRes([0, 0, 0], size, resolutions, pairs_per_batch=pairs_per_batch or n, max_cells=max_cells)
    T16 = torch.tensor(T16_of(T_init[:n]), dtype=torch.float64, device=sc["dev"])
    res = torch.zeros((n, 64 * len(resolutions)), dtype=torch.uint8, device=sc["dev"])
    mr.register_device(sc["fixed_dev"][:n], sc["moving_dev"][:n], T16, res, use_initial_guess=use_initial_guess, range_limit=rng)
    torch.cuda.synchronize()
    if info is not None:
        info.update(mr.info())
    mr.close()
    return T16.cpu().numpy(), res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(n, len(resolutions))


def run_chain(N, sc, resolutions, T_init, use_initial_guess=1, max_cells=0, size=SIZE, rng=RNG):
    """the same registration through the existing entries: host-moved clouds, MapSet.build + match_batch_device per level"""
    import torch
    from ndt_feature_graph_amd import binding
    B, dev = sc["B"], sc["dev"]
    src = [MO.range_filter(sc["moving"][k], rng) for k in range(B)]
    Tinit = [T_init[k] if use_initial_guess else np.eye(4) for k in range(B)]
    if use_initial_guess:
        src = [MO.move_cloud(T_init[k], src[k]) for k in range(B)]
    T = [np.eye(4) for _ in range(B)]
    results = np.zeros((B, len(resolutions)), dtype=binding.RESULT_DTYPE)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    for j in range(len(resolutions) - 1, -1, -1):
        ts = N.MapSet(resolutions[j], [0, 0, 0], size, n_maps=B, max_cells=max_cells)
        ss = N.MapSet(resolutions[j], [0, 0, 0], size, n_maps=B, max_cells=max_cells)
        ts.build(sc["fixed_dev"], range_limit=rng)
        ss.build(torch.tensor(np.stack(src), device=dev).contiguous())
        T16 = torch.tensor(T16_of(np.stack([np.eye(4)] * B)), dtype=torch.float64, device=dev)
        res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
        binding.match_batch_device(ts, idx, ss, idx, T16, res, B, use_initial_guess=0)
        torch.cuda.synchronize()
        Temp = T_of(T16.cpu().numpy())
        results[:, j] = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B)
        for k in range(B):
            src[k] = MO.move_cloud(Temp[k], src[k])
            T[k] = MO.pose_mul(Temp[k], T[k])
        ts.close()
        ss.close()
    return T16_of(np.stack([MO.pose_mul(T[k], Tinit[k]) for k in range(B)])), results


def same_results(r, r_ref):
    for f in DET_FIELDS:
        assert np.array_equal(r[f], r_ref[f]), f


@pytest.mark.parametrize("resolutions", LISTS)
def test_multires_equals_the_chain_of_existing_entries(N, scene, resolutions):
    T16, r = run_multires(N, scene, resolutions, scene["T_init"])
    T16_ref, r_ref = run_chain(N, scene, resolutions, scene["T_init"])
    assert np.array_equal(T16, T16_ref)
    same_results(r, r_ref)
    assert (r["exit_code"] >= 0).all() and (r["n_source"] > 0).all()


# a grid and a list on which the flat kernel takes the 1 m and 0.5 m source builds (even cell counts, fp32 cell centres,
# max_cells <= 4096): 2 m (32 x 32 x 1: odd) goes through the separate move, 1 m moves on load and writes the moved cloud for
# 0.5 m, which moves it on load again.  A batch of fewer than 256 maps goes to the flat kernel only with NDTGPU_FLAT=2 -- in
# ndtgpu_mapset_build and in the multi-resolution entry alike.
FLAT = dict(size=[64.0, 64.0, 2.0], max_cells=4096, lists=[(0.5, 1.0, 2.0), (0.5, 1.0)])


def test_small_batches_follow_the_build_choice_of_the_existing_entry(N, scene):
    """without NDTGPU_FLAT=2, 24 maps per build go to the general kernel: so does every source build of the entry"""
    info = {}
    T16, r = run_multires(N, scene, FLAT["lists"][1], scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"], info=info)
    assert info["levels_fused"] == 0 and info["levels_unfused"] == 2, info
    T16_ref, r_ref = run_chain(N, scene, FLAT["lists"][1], scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"])
    assert np.array_equal(T16, T16_ref)
    same_results(r, r_ref)


@pytest.mark.parametrize("resolutions", FLAT["lists"])
def test_fused_source_builds_equal_the_chain_of_existing_entries(N, scene, resolutions, monkeypatch):
    monkeypatch.setenv("NDTGPU_FLAT", "2")
    info = {}
    T16, r = run_multires(N, scene, resolutions, scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"], info=info)
    flat_levels = sum(1 for x in resolutions if x < 2.0)
    assert info["levels_fused"] == flat_levels and info["levels_unfused"] == len(resolutions) - flat_levels, info
    T16_ref, r_ref = run_chain(N, scene, resolutions, scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"])
    assert np.array_equal(T16, T16_ref)
    same_results(r, r_ref)
    assert (r["exit_code"] >= 0).all() and (r["n_source"] > 0).all()


def test_fused_source_builds_from_pcl_records_and_sub_batches(N, scene, monkeypatch):
    """the first fused level reading 16-byte records (pcl::PointXYZ) straight from the caller; sub-batches of 10 + 10 + 4"""
    import torch
    monkeypatch.setenv("NDTGPU_FLAT", "2")
    from ndt_feature_graph_amd import binding
    B, dev, lst = scene["B"], scene["dev"], FLAT["lists"][1]
    pad = lambda c: torch.cat([c, torch.ones_like(c[..., :1])], dim=-1).contiguous()
    T16_ref, r_ref = run_chain(N, scene, lst, scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"], rng=-1.0)
    for per in (B, 10):
        mr = N.MultiRes([0, 0, 0], FLAT["size"], lst, pairs_per_batch=per, max_cells=FLAT["max_cells"])
        T16 = torch.tensor(T16_of(scene["T_init"]), dtype=torch.float64, device=dev)
        res = torch.zeros((B, 64 * len(lst)), dtype=torch.uint8, device=dev)
        mr.register_device(pad(scene["fixed_dev"]), pad(scene["moving_dev"]), T16, res, use_initial_guess=True, range_limit=-1.0)
        torch.cuda.synchronize()
        info = mr.info()
        mr.close()
        assert info["levels_fused"] == 2 * ((B + per - 1) // per) and info["levels_unfused"] == 0, info
        r = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B, len(lst))
        if per == B:
            first = (T16.cpu().numpy(), r)
        else:
            assert np.array_equal(T16.cpu().numpy(), first[0])
            same_results(r, first[1])
    # (no range filter: the first level reads the caller's records themselves)
    assert np.array_equal(first[0], T16_ref)
    same_results(first[1], r_ref)


def test_multires_without_initial_guess_equals_the_chain(N, scene):
    T16, r = run_multires(N, scene, LISTS[1], scene["T_init"], use_initial_guess=0)
    T16_ref, r_ref = run_chain(N, scene, LISTS[1], scene["T_init"], use_initial_guess=0)
    assert np.array_equal(T16, T16_ref)
    same_results(r, r_ref)


def test_fused_and_unfused_source_builds_give_the_same_bits(N, scene, monkeypatch):
    monkeypatch.setenv("NDTGPU_FLAT", "2")
    lst = FLAT["lists"][0]
    info, info_u = {}, {}
    T16, r = run_multires(N, scene, lst, scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"], info=info)
    monkeypatch.setenv("NDTGPU_MR_FUSED", "0")
    T16_u, r_u = run_multires(N, scene, lst, scene["T_init"], max_cells=FLAT["max_cells"], size=FLAT["size"], info=info_u)
    assert info["levels_fused"] == 2 and info_u["levels_fused"] == 0 and info_u["levels_unfused"] == 3, (info, info_u)
    assert np.array_equal(T16, T16_u)
    same_results(r, r_u)


def test_sub_batches_give_the_bits_of_one_batch(N, scene):
    T16, r = run_multires(N, scene, LISTS[1], scene["T_init"])
    T16_s, r_s = run_multires(N, scene, LISTS[1], scene["T_init"], pairs_per_batch=12)
    assert np.array_equal(T16, T16_s)
    same_results(r, r_s)


def test_host_entry_equals_the_device_entry(N, scene):
    T16, r = run_multires(N, scene, LISTS[0], scene["T_init"])
    mr = N.MultiRes([0, 0, 0], SIZE, LISTS[0], pairs_per_batch=12)
    T, rh = mr.register_host(scene["fixed"], scene["moving"], scene["T_init"], use_initial_guess=True, range_limit=RNG)
    mr.close()
    assert np.array_equal(T16_of(T), T16)
    same_results(rh, r)


def test_multires_against_the_oracle(N, O, scene):
    """8 pairs against the oracle's composition: pose within 1e-4 m / 1e-4 rad, the same iterations at every level"""
    for resolutions in LISTS:
        T16, r = run_multires(N, scene, resolutions, scene["T_init"])
        T = T_of(T16)
        for k in np.linspace(0, scene["B"] - 1, 4).astype(int):
            To, ro = MO.multires_match(O, scene["fixed"][k], scene["moving"][k], scene["T_init"][k], resolutions, 1, RNG)
            dt, dr = MO.pose_error(T[k], To)
            assert dt <= 1e-4 and dr <= 1e-4, (resolutions, k, dt, dr)
            assert [int(x) for x in r["iterations"][k]] == [x["iterations"] for x in ro], (resolutions, k)


def test_overflow_stops_the_pair_at_that_level(N, scene):
    """max_cells that the 4 m maps fit and the 0.5 m maps do not: with the list {0.5, 4} the 0.5 m level reports -3 and is not
    run, the pose is that of the 4 m level times Tinit -- the pose of the list {4}"""
    lst = (0.5, 4.0)
    _, r = run_multires(N, scene, lst, scene["T_init"])
    coarse = int(max(r["n_source"][:, 1].max(), r["n_target"][:, 1].max()))
    fine = int(min(r["n_source"][:, 0].min(), r["n_target"][:, 0].min()))
    # (max_cells counts every cell a build touches, Gaussian or not: room above the coarse maps' Gaussian cells, below the
    #  fine maps' Gaussian cells)
    cap = (coarse + fine) // 2
    assert 3 * coarse < 2 * cap, (coarse, fine)
    T16, r_o = run_multires(N, scene, lst, scene["T_init"], max_cells=cap)
    T16_c, r_c = run_multires(N, scene, lst[1:], scene["T_init"], max_cells=cap)
    assert (r_o["exit_code"][:, 1] >= 0).all() and (r_c["exit_code"] >= 0).all()
    assert (r_o["exit_code"][:, 0] == -3).all() and (r_o["iterations"][:, 0] == 0).all()
    same_results(r_o[:, 1:], r_c)
    assert np.array_equal(T16, T16_c)


def test_full_size_batch_oracle_sampled(N, O):
    """1024 pairs x 100 k points through the device entry; 2 of them against the oracle's composition"""
    import torch
    from ndt_feature_graph_amd import binding, synth
    dev = torch.device("cuda", 0)
    B, NP = 1024, 100000
    pr = synth.pair_2d(torch.arange(5001, 5001 + B, dtype=torch.int64, device=dev), NP, device=dev)
    T16 = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
    mr = N.MultiRes([0, 0, 0], SIZE, LISTS[1], pairs_per_batch=B)
    res = torch.zeros((B, 64 * 4), dtype=torch.uint8, device=dev)
    mr.register_device(pr["fixed"].contiguous(), pr["moving"].contiguous(), T16, res, use_initial_guess=True, range_limit=RNG)
    torch.cuda.synchronize()
    mr.close()
    T = T_of(T16.cpu().numpy())
    r = res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B, 4)
    assert (r["exit_code"] >= 0).all()
    T_init = pr["T_init"].cpu().numpy()
    for k in (0, B - 1):
        f, m = pr["fixed"][k].cpu().numpy(), pr["moving"][k].cpu().numpy()
        To, ro = MO.multires_match(O, f, m, T_init[k], LISTS[1], 1, RNG)
        dt, dr = MO.pose_error(T[k], To)
        assert dt <= 1e-4 and dr <= 1e-4, (k, dt, dr)


# Pairs of the bench's 2D scenes whose initial guess is off by 1.0 m / -0.7 m / 5 degrees.  Over seeds 9001-9024 the oracle's single
# 0.5 m match ends more than 0.1 m from T_gt on 9001, 9002, 9012, 9018 and 9023, and {0.5, 1, 2, 4} ends within 2.1 mm / 1e-4 rad on
# all 24 (tests/test_multires_oracle.py checks the five on the CPU).
BASIN_SEEDS = tuple(range(9001, 9025))
BASIN_FAR = (9001, 9002, 9012, 9018, 9023)


def test_basin_coarse_to_fine_converges_where_the_single_resolution_registrar_does_not(N):
    import torch
    from ndt_feature_graph_amd import binding, synth
    dev = torch.device("cuda", 0)
    B = len(BASIN_SEEDS)
    pr = synth.pair_2d(torch.tensor(BASIN_SEEDS, dtype=torch.int64), MO.BASIN_POINTS)
    T_gt = pr["T_gt"].numpy()
    T0 = np.stack([MO.pose_mul(T_gt[k], MO.T2d(*MO.BASIN_PERTURB)) for k in range(B)])
    fixed, moving = pr["fixed"].to(dev).contiguous(), pr["moving"].to(dev).contiguous()
    mr = N.MultiRes([0, 0, 0], SIZE, MO.BASIN_RESOLUTIONS, pairs_per_batch=B)
    T16 = torch.tensor(T16_of(T0), dtype=torch.float64, device=dev)
    res = torch.zeros((B, 64 * 4), dtype=torch.uint8, device=dev)
    mr.register_device(fixed, moving, T16, res, use_initial_guess=True, range_limit=RNG)
    reg = N.Registrar(0.5, [0, 0, 0], SIZE, pairs_per_batch=B, depth=1, max_cells=4096)
    T16s = torch.tensor(T16_of(T0), dtype=torch.float64, device=dev)
    res_s = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    reg.submit(fixed, moving, T16s, res_s, range_limit=RNG)
    reg.sync()
    torch.cuda.synchronize()
    mr.close()
    reg.close()
    T, Ts = T_of(T16.cpu().numpy()), T_of(T16s.cpu().numpy())
    for k in range(B):
        dt, dr = MO.pose_error(T[k], T_gt[k])
        assert dt <= 0.02 and dr <= 0.005, (BASIN_SEEDS[k], dt, dr)
    far = [BASIN_SEEDS[k] for k in range(B) if MO.pose_error(Ts[k], T_gt[k])[0] > 0.1]
    assert set(far) == set(BASIN_FAR), far
