"""Cases of the link-gate tests (tests/test_linkgate_model.py on the CPU, tests/test_gpu_linkgate.py on the device): the exact
cases, whose expectations are stated here once for both, and the random graphs."""
import functools

import numpy as np


def se2(x, y, t):
    """[n, 4, 4] planar poses"""
    x, y, t = np.atleast_1d(x).astype(np.float64), np.atleast_1d(y).astype(np.float64), np.atleast_1d(t).astype(np.float64)
    T = np.tile(np.eye(4), (len(x), 1, 1))
    c, s = np.cos(t), np.sin(t)
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 0, 3], T[:, 1, 3] = c, -s, s, c, x, y
    return T


def quarter(x, y, turns):
    """a pose with a rotation by turns * 90 degrees and an integer translation: every product and sum with it is exact"""
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][turns % 4]
    return np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)


def exact_cases():
    """-> list of (name, node_T [n, 4, 4], links [(ref, mov, T, score)], params, expected kept mask).  Rotations by 0 or 90 degrees
    and small integers only, so nothing is rounded before the comparison with the threshold."""
    I = np.eye(4)
    line = np.stack([quarter(3 * k, 0, 0) for k in range(6)])                 # six nodes 3 m apart on a line
    step = lambda d: quarter(d, 0, 0)                                         # a link d metres ahead
    half_pi = float(np.arccos(0.0))
    up = I.copy()
    up[0, 0] = 1.0 + 2.0 ** -30                                               # a cosine a rounding above 1
    cases = []
    # strictness of the distance: the prediction lands 2 m / 1 m from the node; max_dist 2 rejects the first (dist == max_dist)
    cases.append(("dist_strict", line, [(0, 2, step(4), 0.0), (0, 2, step(5), 0.0), (0, 2, step(8), 0.0)],
                  dict(max_dist=2.0), [False, True, False]))
    # strictness of the angle: a 90 degree link at max_angle = acos(0) is rejected, at a larger threshold kept
    turn = quarter(6, 0, 1)
    cases.append(("angle_strict", line, [(0, 2, turn, 0.0), (0, 2, step(6), 0.0)], dict(max_angle=half_pi), [False, True]))
    cases.append(("angle_above", line, [(0, 2, turn, 0.0)], dict(max_angle=np.nextafter(half_pi, 4.0)), [True]))
    # the score is not strict; the index distance is not strict either
    cases.append(("score_equal", line, [(0, 2, step(6), 0.25), (0, 2, step(6), 0.5)], dict(max_score=0.25), [True, False]))
    cases.append(("idx_equal", line, [(0, 3, step(9), 0.0), (0, 2, step(6), 0.0), (4, 1, step(-9), 0.0)], dict(min_idx_dist=3),
                  [True, False, True]))
    # ref > mov is an ordinary link
    cases.append(("ref_above_mov", line, [(5, 1, step(-12), 0.0), (5, 1, step(12), 0.0)], dict(), [True, False]))
    # an index >= n_nodes is rejected
    cases.append(("index_range", line, [(0, 6, step(18), 0.0), (7, 2, step(0), 0.0), (0, 5, step(15), 0.0)], dict(), [False, False, True]))
    # the NaN rule: own = I, the prediction's (0, 0) entry is 1 + 2^-30
    two = np.stack([I, I, I])
    cases.append(("nan_rule_default", two, [(0, 2, up, 0.0), (0, 2, I, 0.0)], dict(clip_cosine=0), [False, True]))
    cases.append(("nan_rule_clipped", two, [(0, 2, up, 0.0), (0, 2, I, 0.0)], dict(clip_cosine=1), [True, True]))
    return [(name, nT, links, prm, np.asarray(exp, dtype=bool)) for name, nT, links, prm, exp in cases]


def exact_candidate_cases():
    """-> list of (name, node_T, params, expected [(i, j)]) for the candidate gate"""
    line = np.stack([quarter(3 * k, 0, 0) for k in range(5)])
    bent = line.copy()
    bent[2] = quarter(6, 0, 1)                                                # node 2 looks along y
    half_pi = float(np.arccos(0.0))
    I3 = np.stack([np.eye(4)] * 3)
    up = I3.copy()
    up[1, 0, 0] = 1.0 + 2.0 ** -30
    return [
        ("dist_strict", line, dict(max_dist=6.0, min_idx_dist=1), [(0, 1), (1, 2), (2, 3), (3, 4)]),          # 6 m == max_dist is out
        ("dist_above", line, dict(max_dist=6.5, min_idx_dist=1), [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4)]),
        ("idx_equal", line, dict(max_dist=100.0, min_idx_dist=3), [(0, 3), (0, 4), (1, 4)]),
        ("angle_strict", bent, dict(max_dist=4.0, min_idx_dist=1, max_angle=half_pi), [(0, 1), (3, 4)]),      # 90 degrees == max_angle is out
        ("angle_off", bent, dict(max_dist=4.0, min_idx_dist=1, max_angle=float("inf"), clip_cosine=1), [(0, 1), (1, 2), (2, 3), (3, 4)]),
        ("nan_rule_default", up, dict(min_idx_dist=0), [(0, 2)]),
        ("nan_rule_clipped", up, dict(min_idx_dist=0, clip_cosine=1), [(0, 1), (0, 2), (1, 2)]),
    ]


def links_arrays(links):
    ref = np.asarray([l[0] for l in links], dtype=np.int64)
    mov = np.asarray([l[1] for l in links], dtype=np.int64)
    T = np.stack([l[2] for l in links]).astype(np.float64)
    score = np.asarray([l[3] for l in links], dtype=np.float64)
    return ref, mov, T, score


def walk(n, seed, step=2.0, yaw_sigma=0.25):
    """n nodes on a walk of `step` metre steps with yaw steps N(0, yaw_sigma) -> (rng, node_T)"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.normal(0, yaw_sigma, n))
    return rng, se2(np.cumsum(step * np.cos(t)), np.cumsum(step * np.sin(t)), t)


@functools.lru_cache(maxsize=None)
def random_case(n=300, seed=7):
    """The 300-node case: links are all pairs, T = T_i^-1 T_j times a perturbation (xy N(0, 0.6 m), yaw N(0, 0.15 rad)), scores
    U(0, 0.2) -> dict(node_T, ref, mov, T (perturbed), rel (exact T_i^-1 T_j: the consistent graph), score).  Read-only."""
    rng, node_T = walk(n, seed)
    i, j = np.triu_indices(n, k=1)
    rel = np.einsum("eij,ejk->eik", np.linalg.inv(node_T)[i], node_T[j])
    m = len(i)
    noise = se2(rng.normal(0, 0.6, m), rng.normal(0, 0.6, m), rng.normal(0, 0.15, m))
    T = np.einsum("eij,ejk->eik", rel, noise)
    score = rng.uniform(0, 0.2, m)
    out = dict(node_T=node_T, ref=i.astype(np.int64), mov=j.astype(np.int64), T=T, rel=rel, score=score)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def loop_graph(n=30, seed=5):
    """A 30-node loop for the chain tests: truth on an ellipse, start poses drifted, incremental links i -> i + 1 and matched
    links between all pairs at least 2 apart, some of them wrong by metres -> dict(truth, start [n, 3], incr_ref, incr_mov, incr_T,
    ref, mov, T, score).  Read-only."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    truth = np.stack([6.0 * np.cos(a), 4.0 * np.sin(a), a + np.pi / 2], axis=1)
    tT = se2(truth[:, 0], truth[:, 1], truth[:, 2])
    start = truth + np.concatenate([np.zeros((1, 3)), np.cumsum(rng.normal(0, [0.03, 0.03, 0.01], (n - 1, 3)), axis=0)])
    inv = np.linalg.inv(tT)
    ir, im = np.arange(n - 1), np.arange(1, n)
    incr_T = inv[ir] @ tT[im]
    i, j = np.triu_indices(n, k=2)
    m = len(i)
    noise = se2(rng.normal(0, 0.02, m), rng.normal(0, 0.02, m), rng.normal(0, 0.01, m))
    wrong = rng.random(m) < 0.3
    noise[wrong] = se2(rng.normal(0, 1.5, wrong.sum()), rng.normal(0, 1.5, wrong.sum()), rng.normal(0, 0.5, wrong.sum()))
    T = inv[i] @ tT[j] @ noise
    score = rng.uniform(0, 0.12, m)
    out = dict(truth=truth, start=start, incr_ref=ir.astype(np.int64), incr_mov=im.astype(np.int64), incr_T=incr_T,
               ref=i.astype(np.int64), mov=j.astype(np.int64), T=T, score=score)
    for v in out.values():
        v.setflags(write=False)
    return out
