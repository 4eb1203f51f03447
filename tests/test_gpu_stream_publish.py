"""The stream-fed matcher's hand-overs (-m gpu): how a finished registration's outputs reach memory, and which shares of an
evaluation are handed out.

(a) Visibility.  A finished registration's pose, result record and covariance entries are written through by the wave that
finished it and counted in the batch's done counter afterwards; the maps of a ring entry are rebuilt every `depth` batches and
read through caches that are invalidated once per workgroup and batch.  A small registrar (8 matcher workgroups, two map sets,
sub-batches of 32 pairs) is fed two different sets of scans in alternation, so every ring entry holds other maps and every
output buffer other results from call to call: a stale map line or an output that was counted before it was in memory shows up
as other bits than the two-call path's (ndtgpu_mapset_build + ndtgpu_match_batch_device).  The outputs are read the three ways a
caller can: after sync(), on a second stream behind wait_stream, and as the host form's return values.

(b) Share classes.  Sources of at most 256 cells are dealt to all eight shares, sources of 257..448 cells to five to seven; only
shares that hold cells get a ticket.  Both classes through the stream-fed form with three and with two registrations per
workgroup and through ndt_match_kernel (ndtgpu_match_batch_device): the same bits, and the oracle's poses within the contract."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DET_FIELDS = ["converged", "iterations", "fevals", "exit_code", "score", "n_source", "n_target", "pair_terms_g", "pair_terms_h"]
RES, SIZE, RNG = 0.5, [100.0, 100.0, 1.0], 30.0
PER, NP = 32, 4096              # pairs per sub-batch; points per scan (the flat build's cloud size)


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


def two_call(N, targets, sources, T0, per, packed=False, range_limit=RNG):
    """ndtgpu_mapset_build + ndtgpu_match_batch_device in the launches the registrar makes for sub-batches of `per` pairs: one
    build launch for the targets and one for the sources (device form), or ONE for both (packed: the host form stages a
    sub-batch's sources behind its targets).  -> (T16 [n, 16], result records [n])"""
    import torch
    from ndt_feature_graph_amd import binding
    n, dev = int(targets.shape[0]), targets.device
    st = torch.cuda.current_stream()
    T16 = T0.clone()
    res = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    for off in range(0, n, per):
        p = min(per, n - off)
        ms = N.MapSet(RES, [0, 0, 0], SIZE, n_maps=2 * p, max_cells=4096)
        if packed:
            ms.build(torch.cat([targets[off:off + p], sources[off:off + p]]).contiguous(), range_limit=range_limit, first=0, stream=st)
        else:
            ms.build(targets[off:off + p], range_limit=range_limit, first=0, stream=st)
            ms.build(sources[off:off + p], range_limit=range_limit, first=p, stream=st)
        idx = torch.arange(p, dtype=torch.int32, device=dev)
        binding.match_batch_device(ms, idx, ms, idx + p, T16[off:off + p], res[off:off + p], p, stream=st)
        torch.cuda.synchronize()
    return T16.cpu().numpy(), res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(n)


def assert_same_match(T16, r, ref, what):
    assert np.array_equal(T16, ref[0]), what
    for f in DET_FIELDS:
        assert np.array_equal(r[f], ref[1][f]), (what, f)


@pytest.fixture(scope="module")
def scene_sets(N):
    """two sets of 64 scan pairs of 4096 points, each with: the two-call reference for the device form and for the host form,
    and the covariance entries of the per-batch form of the registrar (one map set, one matcher launch per sub-batch)"""
    import torch
    from ndt_feature_graph_amd import binding, synth
    dev = torch.device("cuda", 0)
    B = 2 * PER
    sets = []
    for seed in (11001, 12001):
        pr = synth.pair_2d(torch.arange(seed, seed + B, dtype=torch.int64, device=dev), NP, device=dev)
        tg, sc = pr["fixed"].contiguous(), pr["moving"].contiguous()
        T0 = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
        s = {"tg": tg, "sc": sc, "T0": T0, "T_init": pr["T_init"].cpu().numpy(),
             "ref": two_call(N, tg, sc, T0, PER), "ref_host": two_call(N, tg, sc, T0, PER, packed=True)}
        reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=PER, depth=1, max_cells=4096, matcher_form=binding.MATCHER_PER_BATCH)
        T16, res = T0.clone(), torch.zeros((B, 64), dtype=torch.uint8, device=dev)
        cov = torch.full((B, 36), 7.0, dtype=torch.float64, device=dev)
        flg = torch.full((B,), 99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        reg.submit(tg, sc, T16, res, range_limit=RNG, covariance_mode=0, cov36_dev=cov, cov_flags_dev=flg)
        reg.sync()
        assert_same_match(T16.cpu().numpy(), res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(B), s["ref"], "per-batch form")
        s["cov"], s["flags"] = cov.cpu().numpy(), flg.cpu().numpy()
        assert not (s["flags"] & binding.COV_NOT_COMPUTED).any()
        reg.close()
        sets.append(s)
    assert not np.array_equal(sets[0]["ref"][0], sets[1]["ref"][0])
    assert sets[0]["ref"][1]["converged"].mean() > 0.8 and sets[1]["ref"][1]["converged"].mean() > 0.8
    return {"B": B, "dev": dev, "sets": sets}


@pytest.mark.parametrize("with_cov", [False, True])
def test_outputs_visible_every_way_they_are_read(N, scene_sets, with_cov):
    import torch
    from ndt_feature_graph_amd import binding
    B, dev, sets = scene_sets["B"], scene_sets["dev"], scene_sets["sets"]
    reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=PER, depth=2, max_cells=4096, matcher_form=binding.MATCHER_STREAM_FED,
                      matcher_groups=8)
    assert reg.info()["matcher_form"] == binding.MATCHER_STREAM_FED
    caller, side = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    mode = 0 if with_cov else None
    # ONE set of output buffers for all the device calls: every call overwrites what the call before it left there
    T16 = torch.empty((B, 16), dtype=torch.float64, device=dev)
    res = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
    cov = torch.empty((B, 36), dtype=torch.float64, device=dev) if with_cov else None
    flg = torch.empty((B,), dtype=torch.int32, device=dev) if with_cov else None
    scans_host = [(s["tg"].cpu().numpy(), s["sc"].cpu().numpy()) for s in sets]
    torch.cuda.synchronize()
    for k in range(24):
        s = sets[k % 2]
        way = ("sync", "wait_stream", "host")[k % 3]
        what = (k, way)
        if way == "host":
            out = reg.register_host(scans_host[k % 2][0], scans_host[k % 2][1], s["T_init"], range_limit=RNG, covariance_mode=mode)
            T_out = np.ascontiguousarray(out[0].transpose(0, 2, 1)).reshape(B, 16)
            assert_same_match(T_out, out[1], s["ref_host"], what)
            if with_cov:
                assert np.array_equal(out[2].reshape(B, 36), s["cov"]), what
                assert np.array_equal(out[3], s["flags"]), what
            continue
        with torch.cuda.stream(caller):
            T16.copy_(s["T0"])
            res.zero_()
            if with_cov:
                cov.fill_(7.0)
                flg.fill_(99)
            t = reg.submit(s["tg"], s["sc"], T16, res, range_limit=RNG, stream=caller, covariance_mode=mode, cov36_dev=cov,
                           cov_flags_dev=flg)
        if way == "sync":
            reg.sync()
            got = [T16.cpu(), res.cpu()] + ([cov.cpu(), flg.cpu()] if with_cov else [])
        else:
            reg.wait_stream(side, ticket=t)
            with torch.cuda.stream(side):
                got = [T16.clone(), res.clone()] + ([cov.clone(), flg.clone()] if with_cov else [])
            side.synchronize()
            caller.wait_stream(side)                      # (the next call's refill of the buffers comes after these copies)
        assert_same_match(got[0].cpu().numpy(), got[1].cpu().numpy().view(binding.RESULT_DTYPE).reshape(B), s["ref"], what)
        if with_cov:
            assert np.array_equal(got[2].cpu().numpy(), s["cov"]), what
            assert np.array_equal(got[3].cpu().numpy(), s["flags"]), what
    reg.sync()
    reg.close()


@pytest.fixture(scope="module")
def share_classes(N):
    """A pool of 48 scan pairs of 4096 points built at several range limits; per class of source cell counts the first range
    limit at which eight pairs of the pool have a source map in the class (and a target map worth matching against)."""
    import torch
    from ndt_feature_graph_amd import synth
    dev = torch.device("cuda", 0)
    P = 48
    pr = synth.pair_2d(torch.arange(13001, 13001 + P, dtype=torch.int64, device=dev), NP, device=dev)
    tg, sc = pr["fixed"].contiguous(), pr["moving"].contiguous()
    T0 = pr["T_init"].transpose(1, 2).contiguous().reshape(P, 16)
    counts = {}
    for rl in (30.0, 20.0, 14.0, 10.0, 7.0):
        ms = N.MapSet(RES, [0, 0, 0], SIZE, n_maps=2 * P, max_cells=4096)
        ms.build(tg, range_limit=rl, first=0)
        ms.build(sc, range_limit=rl, first=P)
        torch.cuda.synchronize()
        counts[rl] = ms.num_cells_all()
    classes = {}
    for name, lo, hi in (("eight shares", 64, 256), ("five to seven shares", 257, 448)):
        for rl, c in counts.items():
            pick = np.nonzero((c[P:] >= lo) & (c[P:] <= hi) & (c[:P] >= 64))[0]
            if len(pick) >= 8 and name not in classes:
                sel = torch.as_tensor(pick[:8], device=dev)
                classes[name] = {"rl": rl, "lo": lo, "hi": hi, "tg": tg[sel].contiguous(), "sc": sc[sel].contiguous(),
                                 "T0": T0[sel].contiguous(), "T_init": pr["T_init"][sel].cpu().numpy(), "n_source": c[P:][pick[:8]]}
    missing = [n for n in ("eight shares", "five to seven shares") if n not in classes]
    assert not missing, ("no eight pairs of the pool in class", missing, {rl: np.sort(c[P:]).tolist() for rl, c in counts.items()})
    return classes


@pytest.mark.parametrize("name", ["eight shares", "five to seven shares"])
def test_share_classes_same_bits_in_every_form(N, share_classes, name):
    import torch
    import oracle as O
    from ndt_feature_graph_amd import binding
    c = share_classes[name]
    tg, sc, T0, rl = c["tg"], c["sc"], c["T0"], c["rl"]
    n, dev = int(tg.shape[0]), tg.device
    ref = two_call(N, tg, sc, T0, n, range_limit=rl)                       # ndt_match_kernel
    assert np.array_equal(ref[1]["n_source"], c["n_source"])
    assert np.all((ref[1]["n_source"] >= c["lo"]) & (ref[1]["n_source"] <= c["hi"]))
    assert np.all(ref[1]["exit_code"] >= 0) and ref[1]["converged"].sum() >= n // 2
    for slots in (3, 2):
        reg = N.Registrar(RES, [0, 0, 0], SIZE, pairs_per_batch=n, depth=2, max_cells=4096, matcher_form=binding.MATCHER_STREAM_FED,
                          matcher_slots=slots)
        for call in range(2):                                              # (the second call: past the registrar's first sub-batch)
            T16, res = T0.clone(), torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            reg.submit(tg, sc, T16, res, range_limit=rl)
            reg.sync()
            assert_same_match(T16.cpu().numpy(), res.cpu().numpy().view(binding.RESULT_DTYPE).reshape(n), ref, (name, slots, call))
        assert reg.info()["matcher_slots"] == slots
        reg.close()
    T = ref[0].reshape(n, 4, 4).transpose(0, 2, 1)
    for b in range(n):
        ot = O.OracleMap(RES, [0, 0, 0], SIZE); ot.load_points(tg[b].cpu().numpy(), rl); ot.compute_cells()
        os_ = O.OracleMap(RES, [0, 0, 0], SIZE); os_.load_points(sc[b].cpu().numpy(), rl); os_.compute_cells()
        assert os_.num_cells() == ref[1]["n_source"][b] and ot.num_cells() == ref[1]["n_target"][b]
        To, ro = O.match_d2d(ot, os_, c["T_init"][b])
        dt = np.linalg.norm(T[b][:3, 3] - To[:3, 3])
        dr = 2.0 * np.arcsin(min(1.0, np.linalg.norm(T[b][:3, :3] - To[:3, :3]) / (2.0 * np.sqrt(2.0))))
        assert dt <= 1e-4 and dr <= 1e-4, (name, b, dt, dr)               # the tolerance BASELINE.json's north_star states
