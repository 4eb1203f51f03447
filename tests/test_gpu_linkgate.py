"""The link gate on the device (ndtgpu_linkgate_*, binding.LinkGate, binding.optimize_gated) against the NumPy model
(tests/linkgate_model.py), distributed.valid_links and the existing PGO entries.

Device and model evaluate the same expressions in the same order, but a link is left out of an equality check where the model
shows it to lie in the band |dist - max_dist| < 1e-9, |ang - max_angle| < 1e-9 or (clip_cosine = 0) |r00| > 1 - 1e-12; at most
0.1 % of a case may be left out, asserted from the model alone.  The exact cases (tests/linkgate_fixtures.py) have no band."""
import numpy as np
import pytest

import linkgate_fixtures as F
import linkgate_model as M
from ndt_feature_graph_amd import distributed as D

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def cm(T):
    """[m, 4, 4] -> [m, 16] column-major"""
    return np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4), (0, 2, 1))).reshape(-1, 16)


def dev_candidates(N, torch, node_T, capacity, with_T=True, **prm):
    """-> (count, overflow, ref, mov, T [capacity, 4, 4] or None): whole arrays, filled with SENTINEL beforehand"""
    gate = N.LinkGate(max(len(node_T), 1), 1)
    gate.set_nodes(node_T)
    ref = torch.full((capacity + 3,), SENTINEL, dtype=torch.int32, device="cuda")
    mov = torch.full((capacity + 3,), SENTINEL, dtype=torch.int32, device="cuda")
    T16 = torch.full((capacity + 3, 16), float(SENTINEL), dtype=torch.float64, device="cuda") if with_T else None
    gate.candidates_into(ref, mov, T16, capacity, **prm)
    count, overflow = gate.count()
    gate.close()
    T = None if T16 is None else np.transpose(T16.cpu().numpy().reshape(-1, 4, 4), (0, 2, 1))
    return count, overflow, ref.cpu().numpy().astype(np.int64), mov.cpu().numpy().astype(np.int64), T


def dev_valid(N, node_T, ref, mov, T, score=None, **prm):
    gate = N.LinkGate(len(node_T), max(len(ref), 1))
    gate.set_nodes(node_T)
    gate.valid(ref, mov, T, score, **prm)
    count, overflow = gate.count()
    keep = gate.keep()
    gate.close()
    assert count == len(keep) and not overflow
    return keep


def assert_same_outside_band(got_idx, model, total):
    got = np.zeros(total, dtype=bool)
    got[got_idx] = True
    mask, band = model["mask"] if "mask" in model else model["keep"], model["band"]
    assert band.mean() <= 1e-3 if total else True                          # (from the model alone)
    assert np.array_equal(got[~band], mask[~band])
    return int(band.sum())


# ---- candidates -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_nodes", [1, 2, 3, 65, 257, 1000])
def test_candidates_against_the_model(N, torch, n_nodes):
    _, node_T = F.walk(n_nodes, 100 + n_nodes)
    node_T[:, :2, 3] += 300.0                                              # coordinates up to 10^3 m
    for prm in (dict(max_dist=6.0, max_angle=0.6), dict(max_dist=6.0, max_angle=float("inf"), clip_cosine=1),
                dict(max_dist=6.0, max_angle=0.6, min_idx_dist=0), dict(max_dist=14.0, max_angle=0.6, min_idx_dist=7)):
        want = M.candidates(node_T, **prm)
        n_band = int(want["band"].sum())
        assert n_band <= 1e-3 * max(len(want["keep"]), 1)
        cap = len(want["ref"]) + n_band + 8
        count, overflow, ref, mov, T = dev_candidates(N, torch, node_T, cap, **prm)
        print("n_nodes %d %s: %d kept (model %d, %d in the band)" % (n_nodes, prm, count, len(want["ref"]), n_band))
        assert not overflow
        if n_band == 0:
            assert count == len(want["ref"])
            assert np.array_equal(ref[:count], want["ref"]) and np.array_equal(mov[:count], want["mov"])      # indices and order
        else:
            i, j = M.all_pairs(n_nodes)
            code = {(a, b): k for k, (a, b) in enumerate(zip(i.tolist(), j.tolist()))}
            got = np.asarray([code[(a, b)] for a, b in zip(ref[:count].tolist(), mov[:count].tolist())], dtype=np.int64)
            assert np.all(np.diff(got) > 0)
            assert_same_outside_band(got, want, len(i))
        assert np.all(ref[count:] == SENTINEL) and np.all(mov[count:] == SENTINEL) and np.all(T[count:] == SENTINEL)
        if count:
            exact = np.linalg.inv(node_T[ref[:count]]) @ node_T[mov[:count]]
            err = np.max(np.abs(T[:count] - exact)) / np.max(np.abs(exact))
            print("  T16 against inv(T_i) @ T_j: %.3g of the largest entry (allowed 1e-12)" % err)
            assert err <= 1e-12
            if n_band == 0:
                assert np.array_equal(T[:count], want["T"])               # the header's operation order: the model's bits


def test_candidates_past_2_24_pairs(N, torch):
    """6000 nodes: 17 997 000 pairs, past 2^24 -- indices only"""
    _, node_T = F.walk(6000, 11)
    prm = dict(max_dist=6.0, max_angle=1.0)
    want = M.candidates(node_T, with_T=False, **prm)
    assert int(want["band"].sum()) == 0 and len(want["ref"]) > 10000
    count, overflow, ref, mov, _ = dev_candidates(N, torch, node_T, len(want["ref"]) + 8, with_T=False, **prm)
    assert count == len(want["ref"]) and not overflow
    assert np.array_equal(ref[:count], want["ref"]) and np.array_equal(mov[:count], want["mov"])
    assert mov[count - 1] - ref[count - 1] >= 2 and ref[count - 1] > 5900  # (the last rows are reached)


@pytest.mark.parametrize("case", F.exact_candidate_cases(), ids=lambda c: c[0])
def test_exact_candidate_cases(N, torch, case):
    _, node_T, prm, expected = case
    count, overflow, ref, mov, T = dev_candidates(N, torch, node_T, 16, **prm)
    assert count == len(expected) and not overflow
    assert list(zip(ref[:count].tolist(), mov[:count].tolist())) == expected
    assert np.array_equal(T[:count], np.stack([M.relative(node_T[i], node_T[j]) for i, j in expected]))


def test_random_candidates_counts(N, torch):
    node_T = F.random_case()["node_T"]
    for max_angle, n_keep in ((0.2, 256), (1.0, 619), (float("inf"), 664)):
        want = M.candidates(node_T, max_dist=6.0, max_angle=max_angle, clip_cosine=1)
        assert int(want["band"].sum()) == 0
        count, overflow, ref, mov, _ = dev_candidates(N, torch, node_T, 700, max_dist=6.0, max_angle=max_angle, clip_cosine=1)
        assert count == n_keep and not overflow
        assert np.array_equal(ref[:count], want["ref"]) and np.array_equal(mov[:count], want["mov"])


# ---- valid ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_links", [0, 1, 63, 64, 65, 1023, 1024, 1025, 44850])
def test_valid_against_the_model_and_distributed(N, n_links):
    c = F.random_case()
    # a spread of the case's links: every stride-th one, so that short cases also hold far pairs
    pick = np.arange(n_links) * (44850 // max(n_links, 1)) if n_links < 44850 else np.arange(44850)
    ref, mov, T, score = c["ref"][pick], c["mov"][pick], c["T"][pick], c["score"][pick]
    edges = np.stack([ref, mov], axis=1)
    for sc in (score, None):
        want = M.valid(ref, mov, T, c["node_T"], sc)
        keep = dev_valid(N, c["node_T"], ref, mov, T, sc)
        n_band = assert_same_outside_band(keep, want, n_links)
        ref_keep = D.valid_links(edges, T, c["node_T"], scores=sc) if n_links else np.zeros(0, dtype=np.int64)
        got = np.zeros(n_links, dtype=bool)
        got[keep] = True
        d = np.zeros(n_links, dtype=bool)
        d[ref_keep] = True
        assert np.array_equal(got[~want["band"]], d[~want["band"]])
        print("n_links %d, scores %s: %d kept (model %d, distributed.valid_links %d, %d in the band)"
              % (n_links, sc is not None, len(keep), len(want["keep"]), len(ref_keep), n_band))
        assert np.all(np.diff(keep) > 0)
        if n_links == 44850 and sc is not None:
            assert len(keep) == 13702 and n_band == 0


@pytest.mark.parametrize("case", F.exact_cases(), ids=lambda c: c[0])
def test_exact_link_cases(N, case):
    _, node_T, links, prm, expected = case
    ref, mov, T, score = F.links_arrays(links)
    assert np.array_equal(dev_valid(N, node_T, ref, mov, T, score, **prm), np.nonzero(expected)[0])


def test_consistent_graph_with_the_clipped_cosine(N):
    c = F.random_case()
    want = M.valid(c["ref"], c["mov"], c["rel"], c["node_T"], clip_cosine=1)
    keep = dev_valid(N, c["node_T"], c["ref"], c["mov"], c["rel"], clip_cosine=1)
    assert_same_outside_band(keep, want, 44850)
    far = (c["mov"] - c["ref"]) >= 2
    got = np.zeros(44850, dtype=bool)
    got[keep] = True
    assert np.array_equal(got[~want["band"]], far[~want["band"]])          # every link with index distance >= 2
    # upstream's rule loses links here; what it keeps is what the model keeps (same expressions, same order), band left out
    d = M.valid(c["ref"], c["mov"], c["rel"], c["node_T"], clip_cosine=0)
    keep0 = dev_valid(N, c["node_T"], c["ref"], c["mov"], c["rel"], clip_cosine=0)
    assert len(keep0) < len(keep) and np.array_equal(keep0, d["keep"])


# ---- gather, overflow, determinism -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_bytes", [4, 128, 288])
@pytest.mark.parametrize("dst_first_row", [0, 5])
def test_gather(N, torch, row_bytes, dst_first_row):
    c = F.random_case()
    m = 1025
    gate = N.LinkGate(300, m)
    gate.set_nodes(c["node_T"])
    gate.valid(c["ref"][:m], c["mov"][:m], c["T"][:m], c["score"][:m], max_dist=3.0, max_angle=0.6, max_score=0.15)
    keep = gate.keep()
    assert 64 < len(keep) < m
    words = row_bytes // 4
    g = torch.Generator().manual_seed(row_bytes)
    src = torch.randint(0, 2**31 - 1, (m, words), dtype=torch.int32, generator=g)
    dst = torch.full((dst_first_row + len(keep) + 7, words), SENTINEL, dtype=torch.int32, device="cuda")
    src_dev = src.cuda()
    gate.gather(src_dev, dst, dst_first_row=dst_first_row)
    gate.count()                                                           # (waits for the handle)
    out = dst.cpu().numpy()
    gate.close()
    a, b = dst_first_row, dst_first_row + len(keep)
    assert np.array_equal(out[a:b], src.numpy()[keep])
    assert np.all(out[:a] == SENTINEL) and np.all(out[b:] == SENTINEL)     # rows in front and behind are untouched


def test_gather_takes_typed_rows(N, torch):
    """T16 (float64 x 16) and flags (int32) through the tensors' own row size"""
    c = F.random_case()
    m = 300
    gate = N.LinkGate(300, m)
    gate.set_nodes(c["node_T"])
    gate.valid(c["ref"][:m], c["mov"][:m], c["T"][:m], None, max_dist=3.0, max_angle=0.6)
    keep = gate.keep()
    T16 = torch.tensor(cm(c["T"][:m]), device="cuda")
    flags = torch.arange(m, dtype=torch.int32, device="cuda")
    T_out = torch.zeros((len(keep) + 2, 16), dtype=torch.float64, device="cuda")
    f_out = torch.full((len(keep) + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    gate.gather(T16, T_out, dst_first_row=2)
    gate.gather(flags, f_out, dst_first_row=2)
    gate.count()
    gate.close()
    assert np.array_equal(T_out.cpu().numpy()[2:], cm(c["T"][:m])[keep]) and np.array_equal(f_out.cpu().numpy()[2:], keep)
    assert np.all(f_out.cpu().numpy()[:2] == SENTINEL)


def test_overflow_reports_the_true_count(N, torch):
    c = F.random_case()
    want = M.candidates(c["node_T"], max_dist=6.0, max_angle=1.0)
    n = len(want["ref"])
    count, overflow, ref, mov, T = dev_candidates(N, torch, c["node_T"], 100, max_dist=6.0, max_angle=1.0)
    assert n == 619 and count == n and overflow
    assert np.array_equal(ref[:100], want["ref"][:100]) and np.array_equal(mov[:100], want["mov"][:100])
    assert np.all(ref[100:] == SENTINEL) and np.all(mov[100:] == SENTINEL) and np.all(T[100:] == SENTINEL)   # nothing behind the capacity
    # valid: keep_dev of 50 entries; the handle's own keep list is complete
    gate = N.LinkGate(300, 44850)
    gate.set_nodes(c["node_T"])
    keep_dev = torch.full((60,), SENTINEL, dtype=torch.int32, device="cuda")
    gate.valid(c["ref"], c["mov"], c["T"], c["score"], keep_dev=keep_dev, capacity=50)
    count, overflow = gate.count()
    keep = gate.keep()
    gate.close()
    assert count == 13702 and overflow and len(keep) == 13702
    k = keep_dev.cpu().numpy()
    assert np.array_equal(k[:50], keep[:50]) and np.all(k[50:] == SENTINEL)


def test_determinism_and_batch_independence(N, torch):
    c = F.random_case()
    runs = [dev_candidates(N, torch, c["node_T"], 700, max_dist=6.0, max_angle=1.0) for _ in range(2)]
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][2:], runs[1][2:]):
        assert a.tobytes() == b.tobytes()
    whole = dev_valid(N, c["node_T"], c["ref"], c["mov"], c["T"], c["score"])
    assert whole.tobytes() == dev_valid(N, c["node_T"], c["ref"], c["mov"], c["T"], c["score"]).tobytes()
    for a, b in ((0, 1000), (1000, 1024), (1023, 3072), (5001, 44850)):    # a link's fate does not depend on its batch
        part = dev_valid(N, c["node_T"], c["ref"][a:b], c["mov"][a:b], c["T"][a:b], c["score"][a:b])
        assert np.array_equal(part + a, whole[(whole >= a) & (whole < b)])


# ---- the chain into the optimiser ---------------------------------------------------------------------------------------------------

def _made_up_cov(m, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.05, (m, 6, 6))
    cov = A @ np.transpose(A, (0, 2, 1)) + 0.01 * np.eye(6)
    flags = np.where(rng.random(m) < 0.1, 2, 0).astype(np.int32)
    return cov.reshape(m, 36), flags


def test_chain_into_set_links_device(N, torch):
    """valid -> gather -> pgo.set_links_device -> optimize on the 30-node graph: the pose bytes of set_links_device on the same
    links filtered on the host"""
    g = F.loop_graph()
    n, k, m = len(g["start"]), len(g["incr_ref"]), len(g["ref"])
    cov, flags = _made_up_cov(m, 1)
    T16_dev, cov_dev, flags_dev = torch.tensor(cm(g["T"]), device="cuda"), torch.tensor(cov, device="cuda"), torch.tensor(flags, device="cuda")
    node_T = M.pose_T(g["start"])
    gate = N.LinkGate(n, m)
    gate.set_nodes(node_T)
    gate.valid(g["ref"], g["mov"], T16_dev, g["score"])
    T_all = torch.zeros((k + m, 16), dtype=torch.float64, device="cuda")
    cov_all = torch.zeros((k + m, 36), dtype=torch.float64, device="cuda")
    flags_all = torch.full((k + m,), 4, dtype=torch.int32, device="cuda")
    T_all[:k] = torch.tensor(cm(g["incr_T"]), device="cuda")
    gate.gather(T16_dev, T_all, dst_first_row=k)
    gate.gather(cov_dev, cov_all, dst_first_row=k)
    gate.gather(flags_dev, flags_all, dst_first_row=k)
    keep = gate.keep()
    gate.close()
    want = D.valid_links(np.stack([g["ref"], g["mov"]], axis=1), g["T"], node_T, scores=g["score"])
    assert np.array_equal(keep, want) and 20 < len(keep) < m
    torch.cuda.synchronize()
    ref_all, mov_all = np.concatenate([g["incr_ref"], g["ref"][keep]]), np.concatenate([g["incr_mov"], g["mov"][keep]])
    # the same links filtered on the host
    T_h = torch.tensor(np.concatenate([cm(g["incr_T"]), cm(g["T"])[want]]), device="cuda")
    cov_h = torch.tensor(np.concatenate([np.zeros((k, 36)), cov[want]]), device="cuda")
    flags_h = torch.tensor(np.concatenate([np.full(k, 4, dtype=np.int32), flags[want]]), device="cuda")
    bank = N.PGO(2, n, k + m)
    bank.set_links_device(0, g["start"], ref_all, mov_all, T_all, cov_all, flags_all)
    bank.set_links_device(1, g["start"], ref_all, mov_all, T_h, cov_h, flags_h)
    bank.optimize()
    (p0, r0), (p1, r1) = bank.poses(0), bank.poses(1)
    bank.close()
    assert r0["exit_code"] == 0 and r0 == r1 and p0.tobytes() == p1.tobytes()
    assert r0["n_edges"] == k + len(keep) and r0["cost_final"] < r0["cost_initial"]


def test_optimize_gated_against_the_host_loop(N, torch):
    """optimize_gated keeps the same set in every round as the model loop composed from distributed.valid_links and the existing
    PGO entries, and ends at the same poses"""
    g = F.loop_graph()
    n, k, m = len(g["start"]), len(g["incr_ref"]), len(g["ref"])
    cov, flags = _made_up_cov(m, 2)
    T16 = cm(g["T"])
    T16_dev, cov_dev, flags_dev = torch.tensor(T16, device="cuda"), torch.tensor(cov, device="cuda"), torch.tensor(flags, device="cuda")
    score_dev = torch.tensor(g["score"], device="cuda")
    incr_dev = torch.tensor(cm(g["incr_T"]), device="cuda")
    gate, bank = N.LinkGate(n, m), N.PGO(2, n, k + m)
    rounds, poses = N.optimize_gated(bank, 0, gate, g["start"], g["incr_ref"], g["incr_mov"], incr_dev, g["ref"], g["mov"], T16_dev, score_dev,
                                     cov_dev, flags_dev, max_rounds=8)
    gate.close()
    edges = np.stack([g["ref"], g["mov"]], axis=1)

    def host_gate(ref, mov, T, node_T, scores, **kw):
        return D.valid_links(edges, T, node_T, scores=scores)

    def host_optimise(p, kept):
        T_h = torch.tensor(np.concatenate([cm(g["incr_T"]), T16[kept]]), device="cuda")
        cov_h = torch.tensor(np.concatenate([np.zeros((k, 36)), cov[kept]]), device="cuda")
        flags_h = torch.tensor(np.concatenate([np.full(k, 4, dtype=np.int32), flags[kept]]), device="cuda")
        bank.set_links_device(1, p, np.concatenate([g["incr_ref"], g["ref"][kept]]), np.concatenate([g["incr_mov"], g["mov"][kept]]), T_h, cov_h, flags_h)
        bank.optimize(1, 1)
        return bank.poses(1)[0]

    want_rounds, want_poses = M.gated_loop(host_optimise, g["start"], g["ref"], g["mov"], g["T"], g["score"], max_rounds=8, gate=host_gate)
    bank.close()
    print("rounds kept: device %s, host loop %s" % ([len(r) for r in rounds], [len(r) for r in want_rounds]))
    assert len(rounds) == len(want_rounds) >= 2
    for a, b in zip(rounds, want_rounds):
        assert np.array_equal(a, b)
    assert poses.tobytes() == want_poses.tobytes()
    assert len(rounds) < 8 and len(rounds[-1]) == len(rounds[-2])          # (it stopped because the count repeated)
    # nothing kept: one round, the start poses
    gate = N.LinkGate(n, m)
    bank = N.PGO(1, n, k + m)
    r, p = N.optimize_gated(bank, 0, gate, g["start"], g["incr_ref"], g["incr_mov"], incr_dev, g["ref"], g["mov"], T16_dev, score_dev,
                            max_score=-1.0)
    gate.close()
    bank.close()
    assert len(r) == 1 and r[0].size == 0 and np.array_equal(p, g["start"])


def test_lifecycle(N, torch):
    base = N.binding.live_resources()
    c = F.random_case()
    gate = N.LinkGate(300, 1000)
    assert N.binding.live_resources() != base
    gate.set_nodes(c["node_T"])
    ref, mov, T16 = gate.candidates(700, max_dist=6.0)
    gate.valid(c["ref"][:1000], c["mov"][:1000], c["T"][:1000], c["score"][:1000])
    assert gate.count()[0] == len(gate.keep())
    gate.set_nodes(torch.tensor(cm(c["node_T"][:100]), device="cuda"))     # the device form, fewer nodes: links to the others are rejected
    gate.valid(c["ref"][:1000], c["mov"][:1000], c["T"][:1000], None)
    keep = gate.keep()
    want = M.valid(c["ref"][:1000], c["mov"][:1000], c["T"][:1000], c["node_T"][:100])
    assert np.array_equal(keep, want["keep"]) or want["band"].any()
    gate.close()
    gate.close()                                                           # (closing twice is harmless)
    assert N.binding.live_resources() == base
