"""csrc/ndt_linkgate.h on the host (tests/native/linkgate_checks.hip, compiled by hipcc, no GPU): the distance, the two rigid
products, the link test and the decoding of a pair index are the model's (tests/linkgate_model.py) bit for bit -- doubles travel as
hexadecimal floats -- and the decoding is exact at 12.5 M pairs, past 2^24 and at the 2^31 pairs of the largest handle."""
import os
import subprocess

import numpy as np
import pytest

import linkgate_fixtures as F
import linkgate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path_factory.mktemp("linkgate") / "linkgate_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "linkgate_checks.hip"),
                           "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.splitlines()
    return run


def cmh(T):
    """a [4, 4] pose as 16 hexadecimal floats, column-major"""
    return " ".join(float(v).hex() for v in np.asarray(T, dtype=np.float64).T.reshape(-1))


def doubles(line):
    return [float.fromhex(v) for v in line.split()]


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_distance_and_products_are_the_models_bits(ask):
    rng, node_T = F.walk(40, 5)
    node_T[:, 2, 3] = rng.normal(0, 0.3, 40)                               # (dz takes part)
    up = np.eye(4)
    up[0, 0] = 1.0 + 2.0 ** -30
    pairs = [(node_T[i], node_T[j]) for i, j in rng.integers(0, 40, (200, 2))] + [(np.eye(4), up), (np.eye(4), np.eye(4)), (up, up)]
    lines, want = [], []
    for a, b in pairs:
        for clip in (0, 1):
            lines.append("D %d %s %s" % (clip, cmh(a), cmh(b)))
            want.append(M.distance(a, b, clip)[:2])
    got = ask(lines)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert same(doubles(g), w), (g, w)
    assert np.isnan(doubles(got[2 * 200])[1]) and doubles(got[2 * 200 + 1])[1] == 0.0       # the NaN rule and its switch
    lines = ["C %s %s" % (cmh(a), cmh(b)) for a, b in pairs[:50]] + ["R %s %s" % (cmh(a), cmh(b)) for a, b in pairs[:50]]
    got = ask(lines)
    for k, (a, b) in enumerate(pairs[:50]):
        assert same(np.array(doubles(got[k])).reshape(4, 4).T, M.compose(a, b))
        assert same(np.array(doubles(got[50 + k])).reshape(4, 4).T, M.relative(a, b))
        assert same(M.compose_vec(a, b), M.compose(a, b)) and same(M.relative_vec(a, b), M.relative(a, b))


def test_pair_decoding_is_exact(ask):
    cases = []
    for n in (2, 3, 65, 257):
        cases += [(p, n) for p in range(n * (n - 1) // 2)]
    rng = np.random.default_rng(9)
    for n in (5000, 6000, 65536):
        total = n * (n - 1) // 2
        rows = [0, 1, 2, n // 3, 4095, 4096, n - 4, n - 3, n - 2] + [int(v) for v in rng.integers(0, n - 1, 300)]
        for i in rows:                                                     # the first and the last pair of a row, and its neighbours
            first = M.pairs_before(i, n)
            cases += [(p, n) for p in (first - 1, first, first + 1, first + (n - i - 2)) if 0 <= p < total]
        cases += [(int(p), n) for p in rng.integers(0, total, 2000)] + [(total - 1, n)]
    got = ask(["P %d %d" % c for c in cases])
    for (p, n), line in zip(cases, got):
        i, j = (int(v) for v in line.split())
        assert i < j < n and M.pairs_before(i, n) + (j - i - 1) == p, (p, n, i, j)       # the definition of the enumeration
        assert (i, j) == M.decode_pair(p, n)


@pytest.mark.parametrize("case", F.exact_cases(), ids=lambda c: c[0])
def test_exact_link_cases_on_the_host(ask, case):
    _, node_T, links, prm, expected = case
    p = M.params(**prm)
    nodes = " ".join(cmh(T) for T in node_T)
    lines = ["V %d %s %d %d %s 1 %s %s %s %s %d %d" % (len(node_T), nodes, ref, mov, cmh(T), float(score).hex(), float(p["max_score"]).hex(),
                                                       float(p["max_dist"]).hex(), float(p["max_angle"]).hex(), p["min_idx_dist"], p["clip_cosine"])
             for ref, mov, T, score in links]
    assert [int(v) for v in ask(lines)] == [int(v) for v in expected]


def test_random_links_on_the_host(ask):
    c = F.random_case()
    pick = np.arange(0, 44850, 97)
    nodes = " ".join(cmh(T) for T in c["node_T"])
    p = M.params()
    lines = ["V 300 %s %d %d %s 1 %s %s %s %s %d %d" % (nodes, c["ref"][k], c["mov"][k], cmh(c["T"][k]), float(c["score"][k]).hex(),
                                                        float(p["max_score"]).hex(), float(p["max_dist"]).hex(), float(p["max_angle"]).hex(),
                                                        p["min_idx_dist"], p["clip_cosine"]) for k in pick]
    want = M.valid(c["ref"][pick], c["mov"][pick], c["T"][pick], c["node_T"], c["score"][pick])
    got = np.array([int(v) for v in ask(lines)], dtype=bool)
    assert np.array_equal(got, want["mask"]) and 50 < got.sum() < len(pick)        # (the same expressions: no band is needed)
