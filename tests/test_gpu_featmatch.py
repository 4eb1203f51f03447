"""ndtgpu_featbank_*: batched feature-set RANSAC matching on the device (-m gpu) against tests/featmatch_model.py.

The integer outputs (status, candidates, hypotheses tested, best hypothesis, inliers, correspondence lists) must EQUAL the model's;
score, c, s, x, y and theta must be within 1e-9 absolute of it (the project's HIP-vs-oracle tolerance for fp64 sums,
test_gpu_parity.py).  Integer equality is a fair demand only where the model's own decisions are not within rounding of a threshold,
so every comparison first asserts ON THE MODEL that the fixture's margins are above 1e-6 (featmatch_model.match: the relative gap
between the best and the next distinct hypothesis score, the smallest |d - threshold| of the descriptor test and of the
acceptance test).  A fixture that fails that is a bug of this file, not a reason to skip."""
import math

import numpy as np
import pytest

import featmatch_model as M

pytestmark = pytest.mark.gpu
T_PLANTED = (0.3, -0.2, 0.4)
TOL = 1e-9
MARGIN = 1e-6
INT_FIELDS = ("status", "n_candidates", "n_hypotheses", "n_tested", "best_hypothesis", "n_inliers")
F64_FIELDS = ("score", "c", "s", "x", "y", "theta")
# the fields of ndtgpu_match_result that do not hold clock readings
MATCH_DET_FIELDS = ("converged", "iterations", "fevals", "exit_code", "score", "n_source", "n_target", "pair_terms_g", "pair_terms_h")


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


def sets(seed, n_ref, n_mov, n_common, T=T_PLANTED, **kw):
    from ndt_feature_graph_amd import synth
    f = synth.feature_sets(seed, n_ref, n_mov, n_common, T, **kw)
    return [f[k].numpy() for k in ("ref_pos", "ref_desc", "mov_pos", "mov_desc")]


def bank_of(N, pairs, max_points=None):
    """a bank with sets 2p (ref) and 2p + 1 (mov) of pair p"""
    mp = max_points or max(max(a[0].shape[0], a[2].shape[0], 1) for a in pairs)
    fm = N.FeatureMatcher(2 * len(pairs), mp, 48)
    for p, a in enumerate(pairs):
        fm.set(2 * p, a[0], a[1])
        fm.set(2 * p + 1, a[2], a[3])
    return fm


def assert_margins(m):
    assert m["status"] == M.OK
    for k in ("descriptor", "score", "acceptance"):
        assert m["margins"][k] > MARGIN, (k, m["margins"])


def assert_equals_model(r, T, corr, m):
    for f in INT_FIELDS:
        assert int(r[f]) == m[f], (f, int(r[f]), m[f])
    assert np.array_equal(corr, m["corr"])
    for f in F64_FIELDS:
        print("%-6s device %.17g model %.17g diff %.3e" % (f, r[f], m[f], abs(r[f] - m[f])))
        assert abs(r[f] - m[f]) <= TOL, f
    # T16 is built from (c, s, x, y) without trigonometry
    want = np.eye(4)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1], want[0, 3], want[1, 3] = r["c"], -r["s"], r["s"], r["c"], r["x"], r["y"]
    assert np.array_equal(T, want)


def assert_failed(r, T, corr, status, n_c=None):
    assert int(r["status"]) == status and r["score"] == 1e17 and int(r["n_inliers"]) == 0 and len(corr) == 0
    assert (r["c"], r["s"], r["x"], r["y"], r["theta"]) == (1.0, 0.0, 0.0, 0.0, 0.0) and int(r["best_hypothesis"]) == -1
    assert np.array_equal(T, np.eye(4))
    if n_c is not None:
        assert int(r["n_candidates"]) == n_c


@pytest.fixture(scope="module")
def three(N):
    """the three fixtures of the comparison (sizes off every multiple of 64 and 256), the model's results, and the device's for
    them in ONE batch: computed once, shared, not modified"""
    pairs = [sets(11, 32, 28, 24), sets(12, 64, 64, 40), sets(13, 257, 130, 70)]
    model = [M.match(*a) for a in pairs]
    fm = bank_of(N, pairs)
    out = fm.match([0, 2, 4], [1, 3, 5])
    yield dict(pairs=pairs, model=model, fm=fm, out=out)
    fm.close()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_against_the_model(three, k):
    m = three["model"][k]
    assert_margins(m)
    res, T, corr = three["out"]
    assert_equals_model(res[k], T[k], corr[k], m)
    assert abs(m["x"] - 0.3) < 0.03 and abs(m["y"] + 0.2) < 0.03 and abs(m["theta"] - 0.4) < 0.01      # (and the pose is the planted one)


def test_ties_go_to_the_lowest_ref_index(N):
    ref_pos, ref_desc, mov_pos, mov_desc = sets(11, 32, 28, 24)
    # every ref point twice: descriptor j + 32 equals descriptor j, position j + 32 equals position j
    a = [np.concatenate([ref_pos, ref_pos]), np.concatenate([ref_desc, ref_desc]), mov_pos, mov_desc]
    m = M.match(*a)
    assert_margins(m)
    assert all(j < 32 for _, j in m["candidates"]) and np.all(m["corr"][:, 1] < 32)
    fm = bank_of(N, [a])
    res, T, corr = fm.match([0], [1])
    fm.close()
    assert_equals_model(res[0], T[0], corr[0], m)
    assert np.all(corr[0][:, 1] < 32)


def test_edges_in_one_batch(N, three):
    e19, e20, rigid = sets(16, 24, 19, 19), sets(17, 24, 20, 20), sets(14, 24, 24, 24)
    rigid[0] = rigid[0].copy()
    rigid[0][:, :2] *= 3.0                                  # no sample is rigid
    m19, m20, mr = M.match(*e19), M.match(*e20), M.match(*rigid)
    assert m19["status"] == M.TOO_FEW and m19["n_candidates"] == 19 and mr["status"] == M.NO_HYPOTHESIS
    assert_margins(m20)
    assert m20["n_candidates"] == 20
    fm = bank_of(N, [e19, e20, rigid, three["pairs"][0]], max_points=33)
    empty = np.zeros((0, 3)), np.zeros((0, 48))
    fm.set(6, *empty)                                       # set 6: empty (it was pair 3's ref); 7 stays pair 3's mov
    ref = [0, 2, 4, 6, 3, 2, 99, 2, 2]
    mov = [1, 3, 5, 7, 6, 3, 3, 2 ** 32 - 1, 3]
    res, T, corr = fm.match(ref, mov)
    assert_failed(res[0], T[0], corr[0], M.TOO_FEW, 19)
    assert_equals_model(res[1], T[1], corr[1], m20)
    assert_failed(res[2], T[2], corr[2], M.NO_HYPOTHESIS, 24)
    assert_failed(res[3], T[3], corr[3], M.TOO_FEW, 0)      # empty ref
    assert_failed(res[4], T[4], corr[4], M.TOO_FEW, 0)      # empty mov
    # out-of-range indices: BAD_INDEX, and the neighbours in the batch are what they are without it
    assert_failed(res[6], T[6], corr[6], M.BAD_INDEX, 0)
    assert_failed(res[7], T[7], corr[7], M.BAD_INDEX, 0)
    for k in (5, 8):
        assert res[k].tobytes() == res[1].tobytes() and np.array_equal(T[k], T[1]) and np.array_equal(corr[k], corr[1])
    # a set that is emptied and set again
    fm.set(6, three["pairs"][0][0], three["pairs"][0][1])
    res, T, corr = fm.match([6], [7])
    fm.close()
    assert res[0].tobytes() == three["out"][0][0].tobytes() and np.array_equal(corr[0], three["out"][2][0])


def test_full_size_sets(N):
    """n = max_points = 1024 on both sides, once; 69 hypotheses (success_probability 0.5) keep the model's run short"""
    a = sets(21, 1024, 1024, 600)
    m = M.match(*a, success_probability=0.5)
    assert_margins(m)
    assert m["n_hypotheses"] == 69
    fm = bank_of(N, [a])
    assert fm.max_points == 1024
    res, T, corr = fm.match([0], [1], success_probability=0.5)
    fm.close()
    assert_equals_model(res[0], T[0], corr[0], m)


def test_a_pair_does_not_depend_on_its_batch(N, three):
    import torch
    from ndt_feature_graph_amd import binding
    others = [sets(31, 40, 30, 19), sets(32, 24, 24, 24), sets(33, 70, 90, 50)]
    fm = bank_of(N, [three["pairs"][2]] + others)
    alone = fm.match([0], [1], seed=5)
    ref = [0] + [2 + 2 * (k % 3) for k in range(298)] + [0]
    mov = [1] + [3 + 2 * (k % 3) for k in range(298)] + [1]
    res, T, corr = fm.match(ref, mov, seed=5)
    for k in (0, 299):
        assert res[k].tobytes() == alone[0][0].tobytes() and np.array_equal(T[k], alone[1][0]) and np.array_equal(corr[k], alone[2][0])
    assert int(res[0]["status"]) == M.OK and all(int(s) == M.OK for s in res["status"])
    assert res[1].tobytes() == res[4].tobytes() and res[1].tobytes() != res[2].tobytes()
    # another seed draws other samples; the device entry gives the host entry's bits
    assert alone[0][0].tobytes() != three["out"][0][2].tobytes()
    dev = torch.device("cuda", 0)
    n = len(ref)
    rd, md = torch.tensor(ref, dtype=torch.int32, device=dev), torch.tensor(mov, dtype=torch.int32, device=dev)
    out = torch.zeros((n, binding.FEATMATCH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    T16 = torch.zeros((n, 16), dtype=torch.float64, device=dev)
    cd = torch.zeros((n, fm.max_points, 2), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    fm.match_device(rd, md, out, T16, cd, stream=st, seed=5)
    st.synchronize()
    fm.close()
    assert out.cpu().numpy().tobytes() == res.tobytes()
    assert np.array_equal(T16.cpu().numpy().reshape(n, 4, 4).transpose(0, 2, 1), T)
    c = cd.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(c[k, :len(corr[k])], corr[k]) for k in range(n))


def test_T16_chains_into_the_ndt_matcher(N):
    """T16_dev of match_device is ndtgpu_match_batch_device's initial guess as it stands: the registration it seeds gives the bits of
    the one seeded with the same poses fetched and uploaded by hand"""
    import torch
    from ndt_feature_graph_amd import binding, synth
    dev = torch.device("cuda", 0)
    pr = synth.pair_2d([1], 10000)
    ms = N.MapSet(1.0, [0, 0, 0], [100, 100, 1], n_maps=2)
    ms.build(np.stack([pr["fixed"][0].numpy(), pr["moving"][0].numpy()]), range_limit=30.0)
    guess = (synth.PAIR_OFFSET_2D[0] + 0.1, synth.PAIR_OFFSET_2D[1] - 0.05, synth.PAIR_OFFSET_2D[2] + math.radians(1.0))
    fm = bank_of(N, [sets(41, 32, 28, 24, T=guess)])
    st = torch.cuda.current_stream()
    i0, i1 = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    size = binding.FEATMATCH_RESULT_DTYPE.itemsize

    def seed_poses():
        out = torch.zeros((1, size), dtype=torch.uint8, device=dev)
        T16 = torch.zeros((1, 16), dtype=torch.float64, device=dev)
        fm.match_device(i0, i1, out, T16, None, stream=st)
        return out, T16

    out, T16 = seed_poses()
    torch.cuda.synchronize()
    r = out.cpu().numpy().view(binding.FEATMATCH_RESULT_DTYPE).reshape(-1)[0]
    assert int(r["status"]) == M.OK and abs(r["x"] - guess[0]) < 0.03 and abs(r["theta"] - guess[2]) < 0.01
    by_hand = torch.tensor(T16.cpu().numpy().copy(), dtype=torch.float64, device=dev)
    res_hand = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
    binding.match_batch_device(ms, i0, ms, i1, by_hand, res_hand, 1, stream=st)
    out, T16 = seed_poses()
    res = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
    binding.match_batch_device(ms, i0, ms, i1, T16, res, 1, stream=st)          # no host visit between the two calls
    torch.cuda.synchronize()
    fm.close()
    ms.close()
    assert np.array_equal(T16.cpu().numpy(), by_hand.cpu().numpy())
    ra, rb = (x.cpu().numpy().view(binding.RESULT_DTYPE).reshape(-1)[0] for x in (res, res_hand))
    for f in MATCH_DET_FIELDS:
        assert ra[f] == rb[f], f
    assert int(ra["converged"]) == 1
    Tm = T16.cpu().numpy().reshape(4, 4).T
    assert np.linalg.norm(Tm[:2, 3] - np.array(synth.PAIR_OFFSET_2D[:2])) < 0.05       # the seeded registration finds the pair's offset


def test_lifecycle_returns_every_resource(N):
    from ndt_feature_graph_amd.binding import live_resources
    before = live_resources()
    fm = bank_of(N, [sets(11, 32, 28, 24)])
    during = live_resources()
    assert during[0] > before[0] and during[3] > before[3]
    fm.match([0], [1])
    fm.match([0, 0, 0], [1, 1, 1])                          # (the result buffers grow)
    fm.close()
    assert live_resources() == before
    with pytest.raises(N.NdtGpuError):
        N.FeatureMatcher(1, 2000)
