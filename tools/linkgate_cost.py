#!/usr/bin/env python3
"""Times the link gate on the device (HIP events around the calls on torch's stream, the first repeat warms up, median over the
rest) against the NumPy path the tests use today, on the same box:
  - candidates for 500 and 5000 nodes (124 750 and 12 497 500 pairs; the latter is the replay's) at the replay's gate -- nodes within
    6 m, at least 2 indices apart, the angle gate off -- against distributed.all_pairs + the vectorised gate of
    tests/test_gpu_replay.py:394-402 + the initial guesses T_i^-1 T_j of its line 402;
  - valid + the gather of T16, cov36 and flags for 44 486 and 12 497 500 registered links against distributed.valid_links + the
    three fancy-index copies.
The nodes are a lawn-mower walk of 1 m steps in rows 2 m apart; the links are T_i^-1 T_j times a perturbation (xy N(0, 0.6 m), yaw
N(0, 0.15 rad)) with scores U(0, 0.2).  Prints one JSON line per case.
usage: python tools/linkgate_cost.py [--repeats R] [--skip-large]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402
from ndt_feature_graph_amd import distributed as D  # noqa: E402


def se2(x, y, t):
    T = np.tile(np.eye(4), (len(x), 1, 1))
    c, s = np.cos(t), np.sin(t)
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 0, 3], T[:, 1, 3] = c, -s, s, c, x, y
    return T


def lawn(n, cols=100, seed=1):
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    r, c = k // cols, k % cols
    c = np.where(r % 2 == 0, c, cols - 1 - c)
    t = np.where(r % 2 == 0, 0.0, np.pi) + rng.normal(0, 0.02, n)
    return se2(1.0 * c + rng.normal(0, 0.05, n), 2.0 * r + rng.normal(0, 0.05, n), t)


def cm(T):
    return np.ascontiguousarray(np.transpose(T, (0, 2, 1))).reshape(-1, 16)


def timed(fn, repeats, st):
    import torch
    ms = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(ms[1:])), ms_min=float(np.min(ms[1:])), ms_max=float(np.max(ms[1:])))


def candidates_case(n, repeats):
    import torch
    st = torch.cuda.current_stream()
    node_T = lawn(n)
    prm = dict(max_dist=6.0, max_angle=float("inf"), clip_cosine=1, min_idx_dist=2)
    t0 = time.perf_counter()
    edges_all = D.all_pairs(n)
    d = np.linalg.norm(node_T[edges_all[:, 0], :2, 3] - node_T[edges_all[:, 1], :2, 3], axis=1)
    edges = edges_all[np.nonzero((d < 6.0) & ((edges_all[:, 1] - edges_all[:, 0]) >= 2))[0]]
    T0 = np.einsum("eij,ejk->eik", np.linalg.inv(node_T)[edges[:, 0]], node_T[edges[:, 1]])
    numpy_s = time.perf_counter() - t0
    cap = len(edges) + 1024
    gate = N.LinkGate(n, 1)
    gate.set_nodes(node_T)
    ref = torch.empty(cap, dtype=torch.int32, device="cuda")
    mov = torch.empty(cap, dtype=torch.int32, device="cuda")
    T16 = torch.empty((cap, 16), dtype=torch.float64, device="cuda")
    t = timed(lambda: gate.candidates_into(ref, mov, T16, cap, stream=st, **prm), repeats, st)
    count, overflow = gate.count()
    same = count == len(edges) and np.array_equal(ref[:count].cpu().numpy(), edges[:, 0]) and np.array_equal(mov[:count].cpu().numpy(), edges[:, 1])
    err = float(np.max(np.abs(T16[:count].cpu().numpy() - cm(T0[:count])))) if same else None
    gate.close()
    return dict(case="candidates", nodes=n, pairs=len(edges_all), kept=count, overflow=overflow, numpy_ms=1e3 * numpy_s,
                same_pairs_as_numpy=bool(same), T16_max_abs_difference=err, **t)


def valid_case(n_nodes, n_links, repeats, seed=3):
    import torch
    st = torch.cuda.current_stream()
    rng = np.random.default_rng(seed)
    node_T = lawn(n_nodes)
    if n_links == n_nodes * (n_nodes - 1) // 2:
        edges = D.all_pairs(n_nodes)
    else:                                                # the gated pairs of the candidates case, cut or repeated to n_links
        e = D.all_pairs(n_nodes)
        d = np.linalg.norm(node_T[e[:, 0], :2, 3] - node_T[e[:, 1], :2, 3], axis=1)
        e = e[np.nonzero((d < 6.0) & ((e[:, 1] - e[:, 0]) >= 2))[0]]
        edges = e[np.arange(n_links) % len(e)]
    m = len(edges)
    inv = np.linalg.inv(node_T)
    T = np.empty((m, 4, 4))
    for a in range(0, m, 1 << 20):                       # (chunks: 12.5 M 4x4 products)
        s = slice(a, a + (1 << 20))
        k = len(edges[s])
        T[s] = inv[edges[s, 0]] @ node_T[edges[s, 1]] @ se2(rng.normal(0, 0.6, k), rng.normal(0, 0.6, k), rng.normal(0, 0.15, k))
    score = rng.uniform(0, 0.2, m)
    cov = rng.normal(0, 1, (m, 36))
    flags = rng.integers(0, 4, m).astype(np.int32)
    T16 = cm(T)
    t0 = time.perf_counter()
    keep = D.valid_links(edges, T, node_T, scores=score)
    numpy_gate_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    packed = (T16[keep], cov[keep], flags[keep])
    numpy_gather_s = time.perf_counter() - t0
    ref_dev = torch.tensor(edges[:, 0].astype(np.int32), device="cuda")
    mov_dev = torch.tensor(edges[:, 1].astype(np.int32), device="cuda")
    T_dev, s_dev = torch.tensor(T16, device="cuda"), torch.tensor(score, device="cuda")
    cov_dev, f_dev = torch.tensor(cov, device="cuda"), torch.tensor(flags, device="cuda")
    rows = m                                             # (room for every link: the count is the device's)
    T_out = torch.empty((rows, 16), dtype=torch.float64, device="cuda")
    cov_out = torch.empty((rows, 36), dtype=torch.float64, device="cuda")
    f_out = torch.empty(rows, dtype=torch.int32, device="cuda")
    gate = N.LinkGate(n_nodes, m)
    gate.set_nodes(node_T)
    tv = timed(lambda: gate.valid(ref_dev, mov_dev, T_dev, s_dev, stream=st), repeats, st)

    def both():
        gate.valid(ref_dev, mov_dev, T_dev, s_dev, stream=st)
        gate.gather(T_dev, T_out, stream=st)
        gate.gather(cov_dev, cov_out, stream=st)
        gate.gather(f_dev, f_out, stream=st)
    tb = timed(both, repeats, st)
    got = gate.keep()
    differ = int(len(np.setxor1d(got, keep)))
    same_rows = differ == 0 and np.array_equal(T_out[:len(got)].cpu().numpy(), packed[0]) and np.array_equal(cov_out[:len(got)].cpu().numpy(), packed[1]) \
        and np.array_equal(f_out[:len(got)].cpu().numpy(), packed[2])
    gate.close()
    return dict(case="valid + gather", nodes=n_nodes, links=m, kept=len(got), links_decided_differently_from_numpy=differ,
                gathered_rows_equal_numpy=bool(same_rows), numpy_valid_links_ms=1e3 * numpy_gate_s, numpy_gather_ms=1e3 * numpy_gather_s,
                valid_ms_median=tv["ms_median"], valid_ms_min=tv["ms_min"], valid_ms_max=tv["ms_max"],
                valid_gather_ms_median=tb["ms_median"], valid_gather_ms_min=tb["ms_min"], valid_gather_ms_max=tb["ms_max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 12.5 M-link valid case (it needs about 8 GB of host memory)")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("linkgate_cost: no HIP device (nothing to measure)")
    version = N.lib().ndtgpu_version().decode()
    for n in (500, 5000):
        print(json.dumps(dict(version=version, **candidates_case(n, a.repeats))), flush=True)
    print(json.dumps(dict(version=version, **valid_case(5000, 44486, a.repeats))), flush=True)
    if not a.skip_large:
        print(json.dumps(dict(version=version, **valid_case(5000, 12497500, a.repeats))), flush=True)


if __name__ == "__main__":
    main()
