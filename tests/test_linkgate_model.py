"""The NumPy model of the link gate (tests/linkgate_model.py) on the CPU: its vector forms equal its scalar forms bit for bit, its
pair decoding is computeAllPossibleLinks' order, the exact cases have the expectations of tests/linkgate_fixtures.py, and on the
random graphs it keeps what distributed.valid_links and the NumPy gate over distributed.all_pairs keep outside a band that the
model itself shows to be (nearly) empty."""
import numpy as np
import pytest

import linkgate_fixtures as F
import linkgate_model as M
import pgo_model
from ndt_feature_graph_amd import distributed as D


def test_vector_acos_is_the_scalar_one():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1, 1, 4000), 1.0 - 10.0 ** -rng.uniform(1, 16, 1000), -1.0 + 10.0 ** -rng.uniform(1, 16, 1000),
                        [1.0, -1.0, 0.0, 0.5, -0.5, 1 - 2.0 ** -53, 1e-20, np.nan]])
    assert np.array_equal(M.acos_vec(x), np.array([pgo_model.acos_fd(v) for v in x]), equal_nan=True)
    assert np.nanmax(np.abs(M.acos_vec(x) - np.arccos(x))) < 1e-15         # ... and libm's within two ulps


def test_pair_decoding_is_all_pairs_order():
    for n in (2, 3, 65, 257):
        pairs = D.all_pairs(n)
        assert [M.decode_pair(p, n) for p in range(len(pairs))] == [tuple(int(v) for v in r) for r in pairs]
        i, j = M.all_pairs(n)
        assert np.array_equal(np.stack([i, j], axis=1), pairs)
    for n in (5000, 6000, 65536):                                          # 12.5 M, 18 M (past 2^24) and 2^31 pairs: the ends of rows
        for i in (0, 1, n // 3, 4095, n - 3, n - 2):
            first = M.pairs_before(i, n)
            assert M.decode_pair(first, n) == (i, i + 1)
            assert M.decode_pair(first + (n - i - 2), n) == (i, n - 1)
    assert M.decode_pair(65536 * 65535 // 2 - 1, 65536) == (65534, 65535)


def test_vector_forms_equal_the_scalar_forms():
    rng, node_T = F.walk(40, 3)
    i, j = M.all_pairs(40)
    for kw in (dict(max_dist=6.0), dict(max_dist=6.0, max_angle=float("inf"), clip_cosine=1, min_idx_dist=0), dict(max_dist=20.0, max_angle=1.0, min_idx_dist=7)):
        c = M.candidates(node_T, **kw)
        ref, mov, T = M.candidates_scalar(node_T, **kw)
        assert len(ref) > 0 and np.array_equal(c["ref"], ref) and np.array_equal(c["mov"], mov) and np.array_equal(c["T"], T)
    rel = M.relative_vec(node_T[i], node_T[j])
    T = rel @ F.se2(rng.normal(0, 0.6, len(i)), rng.normal(0, 0.6, len(i)), rng.normal(0, 0.15, len(i)))
    score = rng.uniform(0, 0.2, len(i))
    for sc in (None, score):
        v = M.valid(i, j, T, node_T, sc)
        assert 0 < len(v["keep"]) < len(i) and np.array_equal(v["keep"], M.valid_scalar(i, j, T, node_T, sc))
    assert np.array_equal(M.valid(j, i, np.linalg.inv(T), node_T)["keep"], M.valid_scalar(j, i, np.linalg.inv(T), node_T))


@pytest.mark.parametrize("case", F.exact_cases(), ids=lambda c: c[0])
def test_exact_link_cases(case):
    _, node_T, links, prm, expected = case
    ref, mov, T, score = F.links_arrays(links)
    v = M.valid(ref, mov, T, node_T, score, **prm)
    assert np.array_equal(v["mask"], expected)
    assert np.array_equal(M.valid_scalar(ref, mov, T, node_T, score, **prm), np.nonzero(expected)[0])


@pytest.mark.parametrize("case", F.exact_candidate_cases(), ids=lambda c: c[0])
def test_exact_candidate_cases(case):
    _, node_T, prm, expected = case
    c = M.candidates(node_T, **prm)
    assert list(zip(c["ref"].tolist(), c["mov"].tolist())) == expected
    assert np.array_equal(c["T"], np.stack([M.relative(node_T[i], node_T[j]) for i, j in expected]))


def test_random_case_against_distributed_valid_links():
    c = F.random_case()
    edges = np.stack([c["ref"], c["mov"]], axis=1)
    v = M.valid(c["ref"], c["mov"], c["T"], c["node_T"], c["score"])
    assert v["band"].mean() <= 1e-3                                        # (0 of 44 850 on this case)
    want = np.zeros(len(edges), dtype=bool)
    want[D.valid_links(edges, c["T"], c["node_T"], scores=c["score"])] = True
    out = ~v["band"]
    assert np.array_equal(v["mask"][out], want[out])
    assert len(edges) == 44850 and int(want.sum()) == 13702 and len(v["keep"]) == 13702
    # without scores
    v = M.valid(c["ref"], c["mov"], c["T"], c["node_T"])
    want[:] = False
    want[D.valid_links(edges, c["T"], c["node_T"])] = True
    assert np.array_equal(v["mask"][~v["band"]], want[~v["band"]]) and want.sum() > 13702


def test_consistent_graph_needs_the_clipped_cosine():
    c = F.random_case()
    edges = np.stack([c["ref"], c["mov"]], axis=1)
    far = (c["mov"] - c["ref"]) >= 2
    # upstream's rule: about one link in six is lost to acos(1 + ulp)
    lost = int(far.sum()) - len(D.valid_links(edges, c["rel"], c["node_T"]))
    pred = np.einsum("eij,ejk->eik", c["node_T"][c["ref"]], c["rel"])
    above = np.einsum("ej,ej->e", c["node_T"][c["mov"], :3, 0], pred[:, :3, 0]) > 1.0
    # (7 021 of the 44 850 links have a cosine above 1; 6 980 of them are among the 44 551 with index distance >= 2)
    assert int(far.sum()) == 44551 and int(above.sum()) == 7021 and lost == int((above & far).sum()) == 6980
    v = M.valid(c["ref"], c["mov"], c["rel"], c["node_T"], clip_cosine=1)
    assert v["band"].mean() <= 1e-3
    assert np.array_equal(v["mask"][~v["band"]], far[~v["band"]])           # every link 2 apart: dist and angle are roundings of 0
    d = M.valid(c["ref"], c["mov"], c["rel"], c["node_T"], clip_cosine=0)   # the default keeps strictly fewer
    assert len(d["keep"]) < len(v["keep"])


def test_random_candidates_against_the_numpy_gate():
    c = F.random_case()
    node_T = c["node_T"]
    edges = D.all_pairs(len(node_T))
    d2 = np.linalg.norm(node_T[edges[:, 0], :3, 3] - node_T[edges[:, 1], :3, 3], axis=1)
    rc = np.einsum("ej,ej->e", node_T[edges[:, 0], :3, 0], node_T[edges[:, 1], :3, 0])
    ac = np.abs(np.arccos(np.clip(rc, -1, 1)))
    for max_angle, n_keep in ((0.2, 256), (1.0, 619), (float("inf"), 664)):
        got = M.candidates(node_T, max_dist=6.0, max_angle=max_angle, clip_cosine=1)
        assert got["band"].mean() <= 1e-3
        want = (d2 < 6.0) & (ac < max_angle) & ((edges[:, 1] - edges[:, 0]) >= 2)
        out = ~got["band"]
        assert np.array_equal(got["keep"][out], want[out]) and int(want.sum()) == n_keep == len(got["ref"])
        T = np.linalg.inv(node_T[got["ref"]]) @ node_T[got["mov"]]
        assert np.max(np.abs(got["T"] - T)) <= 1e-12 * np.max(np.abs(T))


def test_gather_and_loop():
    src = np.arange(40, dtype=np.float64).reshape(10, 4)
    dst = np.full((12, 4), -1.0)
    M.gather([1, 4, 9], src, dst, dst_first_row=5)
    assert np.array_equal(dst[5:8], src[[1, 4, 9]]) and np.all(dst[:5] == -1) and np.all(dst[8:] == -1)
    # the loop: stops when the count repeats, when nothing is kept, and at max_rounds
    g = F.loop_graph()
    calls = []

    def optimise(poses, kept):
        calls.append(len(kept))
        return g["truth"]                                                  # (a perfect optimiser: the second gate sees the truth)
    rounds, poses = M.gated_loop(optimise, g["start"], g["ref"], g["mov"], g["T"], g["score"])
    assert len(rounds) >= 2 and len(rounds) == len(calls) and len(rounds[-1]) == len(rounds[-2]) and np.array_equal(poses, g["truth"])
    rounds, poses = M.gated_loop(optimise, g["start"], g["ref"], g["mov"], g["T"], g["score"], max_score=-1.0)
    assert len(rounds) == 1 and rounds[0].size == 0 and np.array_equal(poses, g["start"])
    flip = [0]

    def oscillate(poses, kept):
        flip[0] ^= 1
        return g["truth"] if flip[0] else g["start"] + [3.0, 0, 0] * (np.arange(len(poses))[:, None] % 2)
    rounds, _ = M.gated_loop(oscillate, g["start"], g["ref"], g["mov"], g["T"], g["score"], max_rounds=4)
    assert len(rounds) <= 4
