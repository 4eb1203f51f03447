#!/usr/bin/env python3
"""Times ndtgpu_pgo_optimize (device events around the call; the graph is set again before every repeat, median over repeats) and
reports the Gauss-Newton and conjugate-gradient iterations, at the default parameters, for
  - one grid-world graph of 500 nodes,
  - one of the replay's size: 5000 nodes and about 44 k links,
  - 256 graphs of 500 nodes in one launch,
and the NumPy model's time (tests/pgo_model.py, dense solve) at 500 nodes on one core for comparison.  The graphs are lawn-mower
trajectories over a grid of 0.5 m cells with noisy links to the nodes within `reach` columns in the next rows, started 0.2 m and
0.1 rad off.
--wide instead times, in one run, one graph of 500 nodes, one of about 1500 and one of the replay's size in BOTH forms: the
one-workgroup form (ndtgpu_pgo_optimize, device events around the asynchronous call) and the chip-wide form
(ndtgpu_pgo_optimize_wide at check_every 8, 32 and 128; HOST WALL TIME around the call, which returns when the graph is done) --
per case and form the median of the repeats after a warm-up, the Gauss-Newton updates, the inner iterations, microseconds per
inner iteration and the exit code.  The one-workgroup form of the same run is the yardstick.
usage: python tools/pgo_cost.py [--repeats R] [--skip-model] [--wide]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ndt_feature_graph_amd as N  # noqa: E402
import pgo_model as M  # noqa: E402


def grid(rows, cols, reach, seed, cell=0.5):
    """reach = (columns either side in the next row, ... in the row after)"""
    rng = np.random.default_rng(seed)
    truth, idx = [], {}
    for r in range(rows):
        for c in (range(cols) if r % 2 == 0 else range(cols - 1, -1, -1)):
            idx[(r, c)] = len(truth)
            truth.append([cell * c, cell * r, 0.0 if r % 2 == 0 else np.pi])
    truth = np.array(truth)
    n = truth.shape[0]
    ref, mov = list(range(n - 1)), list(range(1, n))
    for dr, w in enumerate(reach, start=1):
        for r in range(rows - dr):
            for c in range(cols):
                for d in range(-w, w + 1):
                    if 0 <= c + d < cols:
                        ref.append(idx[(r, c)]); mov.append(idx[(r + dr, c + d)])
    z = M._measure(truth, ref, mov, rng, 0.01, 0.005)
    return M.Graph(M._perturbed(truth, rng), ref, mov, z, truth=truth)


def timed(graphs, repeats):
    import torch
    bank = N.PGO(len(graphs), max(G.n_nodes for G in graphs), max(G.n_edges for G in graphs))
    st = torch.cuda.current_stream()
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up)
        for k, G in enumerate(graphs):
            bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        bank.optimize(stream=st)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    res = [bank.poses(k)[1] for k in range(len(graphs))]
    err = max(float(np.max(np.abs((bank.poses(k)[0] - G.truth)[:, :2]))) for k, G in enumerate(graphs[:4]))
    bank.close()
    t = times[1:]
    return dict(graphs=len(graphs), nodes=graphs[0].n_nodes, links=graphs[0].n_edges, ms_median=float(np.median(t)), ms_min=float(np.min(t)),
                ms_max=float(np.max(t)), iterations=sorted({r["iterations"] for r in res}), linear_iterations_max=max(r["linear_iterations"] for r in res),
                exit_codes=sorted({r["exit_code"] for r in res}), cost_initial=res[0]["cost_initial"], cost_final=res[0]["cost_final"],
                worst_xy_error_m=err)


def timed_wide(G, repeats, check_every):
    """the chip-wide form of one graph: host wall time round the synchronous call, the device idle before it"""
    import torch
    bank = N.PGO(1, G.n_nodes, G.n_edges)
    st = torch.cuda.current_stream()
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up)
        bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
        torch.cuda.synchronize()
        t = time.perf_counter()
        bank.optimize_wide(0, stream=st, check_every=check_every)
        times.append(1e3 * (time.perf_counter() - t))
    p, r = bank.poses(0)
    bank.close()
    return times[1:], r, float(np.max(np.abs((p - G.truth)[:, :2])))


def report(case, form, clock, G, ms, repeats, r, err, **more):
    """ms: (median, min, max)"""
    print(json.dumps(dict(case=case, form=form, clock=clock, nodes=G.n_nodes, links=G.n_edges, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2],
                          repeats=repeats, iterations=r["iterations"], linear_iterations=r["linear_iterations"],
                          us_per_inner_iteration=1e3 * ms[0] / max(r["linear_iterations"], 1), exit_code=r["exit_code"],
                          cost_final=r["cost_final"], worst_xy_error_m=err, **more)), flush=True)


def wide_leg(repeats):
    version = N.lib().ndtgpu_version().decode()
    for case, G in (("500 nodes", grid(20, 25, (1,), 1)), ("1500 nodes", grid(30, 50, (2,), 3)), ("replay size", grid(50, 100, (2, 1), 2))):
        one = timed([G], repeats)
        r1 = dict(iterations=one["iterations"][0], linear_iterations=one["linear_iterations_max"], exit_code=one["exit_codes"][0],
                  cost_final=one["cost_final"])
        report(case, "one workgroup", "device events", G, (one["ms_median"], one["ms_min"], one["ms_max"]), repeats, r1, one["worst_xy_error_m"],
               version=version)
        for every in (8, 32, 128):
            t, r, err = timed_wide(G, repeats, every)
            ms = (float(np.median(t)), float(np.min(t)), float(np.max(t)))
            report(case, "wide", "host wall time", G, ms, repeats, r, err, check_every=every, ratio_to_one_workgroup=one["ms_median"] / ms[0],
                   version=version)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--wide", action="store_true", help="both forms on one graph of 500, 1500 and 5000 nodes")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("pgo_cost: no HIP device (nothing to measure)")
    if a.wide:
        wide_leg(a.repeats)
        return
    small = grid(20, 25, (1,), 1)
    print(json.dumps(dict(case="one graph of 500 nodes", **timed([small], a.repeats))), flush=True)
    print(json.dumps(dict(case="256 graphs of 500 nodes", **timed([grid(20, 25, (1,), 100 + k) for k in range(256)], a.repeats))), flush=True)
    print(json.dumps(dict(case="replay size", **timed([grid(50, 100, (2, 1), 2)], max(1, a.repeats // 2)))), flush=True)
    if not a.skip_model:
        try:
            from threadpoolctl import threadpool_limits
            limit = threadpool_limits(limits=1)
        except ImportError:
            limit = None                                       # (run with OMP_NUM_THREADS=1 for the one-core figure)
        t = time.perf_counter()
        _, r = M.optimize(small)
        print(json.dumps(dict(case="NumPy model, dense, 500 nodes", seconds=time.perf_counter() - t, iterations=r["iterations"],
                              blas_limited_to_one_thread=limit is not None or os.environ.get("OMP_NUM_THREADS") == "1")), flush=True)


if __name__ == "__main__":
    main()
