#!/usr/bin/env python3
"""Times ndtgpu_pgo_marginals_device / ndtgpu_pgo3_marginals_device (HIP events around the asynchronous call into device
buffers, median of 7 after a warm-up) on the grid-world graphs of tools/pgo_cost.py (SE(3): lifted by tools/pgo3_cost.py), optimised
first, at the default parameters:
  - ALL marginals of the 500-node / 1886-link graph (500 queries: 1500 columns, SE(3) 3000),
  - the last node of each of 256 such graphs in one call,
and reports the inner iterations of the columns and the exit codes, against numpy.linalg.inv of the model's dense H
(tests/pgo_marginals_model.py) of the 500-node graph on the same box, with the largest relative block difference between the two.
usage: python tools/pgo_marginals_cost.py [--repeats R] [--skip-model] [--skip-bank]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ndt_feature_graph_amd as N  # noqa: E402
import pgo_marginals_model as MM  # noqa: E402
import pgo_cost  # noqa: E402
import pgo3_cost  # noqa: E402


def timed(dof, graphs, gi, qi, repeats):
    """-> (ms per repeat, cov [n, dof, dof], result records, the bank's poses of graph 0)"""
    import torch
    bank = (N.PGO if dof == 3 else N.PGO3)(len(graphs), max(G.n_nodes for G in graphs), max(G.n_edges for G in graphs))
    for k, G in enumerate(graphs):
        bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
    st = torch.cuda.current_stream()
    bank.optimize(stream=st)
    n = len(qi)
    cov = torch.zeros(n * dof * dof, dtype=torch.float64, device="cuda")
    res = torch.zeros(n * N.PGO_MARGINAL_RESULT.itemsize, dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up, and allocates the workspace)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        bank.marginals_device(gi, qi, None, cov, None, res, stream=st)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    P = bank.poses(0)[0]
    bank.close()
    return times[1:], cov.cpu().numpy().reshape(n, dof, dof), res.cpu().numpy().view(N.PGO_MARGINAL_RESULT), P


def report(case, dof, G, n_graphs, n_queries, t, res, **more):
    slot, slots, launches = N.pgo_marginal_plan(G.n_nodes, G.n_edges, n_queries, dof)
    print(json.dumps(dict(case=case, bank="SE(2)" if dof == 3 else "SE(3)", graphs=n_graphs, nodes=G.n_nodes, links=G.n_edges, queries=n_queries,
                          columns=n_queries * dof, slot_bytes=slot, slots=slots, solve_launches=launches, ms_median=float(np.median(t)),
                          ms_min=float(np.min(t)), ms_max=float(np.max(t)), repeats=len(t),
                          column_iterations_max=int(res["max_column_iterations"].max()), inner_iterations=int(res["linear_iterations"].sum()),
                          exit_codes=sorted({int(c) for c in res["exit_code"]}), asymmetry_max=float(res["asymmetry"].max()),
                          version=N.lib().ndtgpu_version().decode(), **more)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-bank", action="store_true", help="leave out the 256-graph case")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("pgo_marginals_cost: no HIP device (nothing to measure)")
    for dof in (3, 6):
        make = (lambda seed: pgo_cost.grid(20, 25, (1,), seed)) if dof == 3 else (lambda seed: pgo3_cost.lift(pgo_cost.grid(20, 25, (1,), seed), seed))
        G = make(1)
        q = np.arange(G.n_nodes)
        t, cov, res, P = timed(dof, [G], 0, q, a.repeats)
        more = {}
        if not a.skip_model:
            w = time.perf_counter()
            S = MM.system(G, P)
            Hi = MM.dense_inverse(S)
            more["numpy_inv_seconds"] = time.perf_counter() - w
            more["largest_relative_block_difference"] = max(MM.block_diff(cov[i], Hi[i, i]) for i in q)
        report("all marginals of one graph", dof, G, 1, len(q), t, res, **more)
        if not a.skip_bank:
            graphs = [make(100 + k) for k in range(256)]
            t, cov, res, _ = timed(dof, graphs, np.arange(256), np.full(256, G.n_nodes - 1), a.repeats)
            report("the last node of each of 256 graphs", dof, G, 256, 256, t, res)


if __name__ == "__main__":
    main()
