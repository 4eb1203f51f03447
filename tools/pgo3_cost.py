#!/usr/bin/env python3
"""Times ndtgpu_pgo3_optimize (device events around the call; the graphs are set again before every repeat, median over the
repeats after a warm-up) and reports the Gauss-Newton and conjugate-gradient iterations, at the default parameters, for
  - one graph of 500 nodes,
  - 256 such graphs in one call,
  - one graph of the replay's size: 5000 nodes and about 44 k links,
beside the SE(2) bank (ndtgpu_pgo_optimize, timed the same way in the same run) on graphs of the same nodes and links, and the
NumPy model's time (tests/pgo3_model.py, dense solve) at 500 nodes on the same box.  The graphs are those of tools/pgo_cost.py --
lawn-mower trajectories over a grid of 0.5 m cells with noisy links to the nodes in the next rows -- lifted to 3D: a height that
undulates by 0.3 m and roll and pitch of +-0.1 rad, started 0.2 m and 0.1 rad off in every component.  Every line carries the
library's version.  Figures, not pass / fail.
--wide: the chip-wide form (ndtgpu_pgo3_optimize_wide; host wall time round the synchronous call, the device idle before it) at
check_every 8, 32 and 128 against the one-workgroup form (device events) in the same run, on one graph of 500, 1500 and 5000
nodes: updates, inner iterations and us per inner iteration of both, and the ratio.
usage: python tools/pgo3_cost.py [--repeats R] [--skip-model] [--skip-replay] [--wide]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ndt_feature_graph_amd as N  # noqa: E402
import pgo3_model as M  # noqa: E402
import pgo_cost  # noqa: E402


def lift(G2, seed):
    """the SE(2) graph's nodes and links in 3D"""
    rng = np.random.default_rng(seed)
    truth = np.stack([M.euler_T(x, y, 0.3 * math.sin(0.7 * x) * math.cos(0.5 * y), 0.1 if k % 2 else -0.1, -0.1 if (k // 2) % 2 else 0.1, t)
                      for k, (x, y, t) in enumerate(G2.truth)])
    return M.Graph(M._perturbed(truth, rng), G2.ref, G2.mov, M._measure(truth, G2.ref, G2.mov, rng, 0.01, 0.005), truth=truth)


def timed(graphs, repeats):
    import torch
    bank = N.PGO3(len(graphs), max(G.n_nodes for G in graphs), max(G.n_edges for G in graphs))
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
    err = max(float(np.max(np.abs((bank.poses(k)[0] - G.truth)[:, :3, 3]))) for k, G in enumerate(graphs[:4]))
    bank.close()
    t = times[1:]
    return dict(graphs=len(graphs), nodes=graphs[0].n_nodes, links=graphs[0].n_edges, ms_median=float(np.median(t)), ms_min=float(np.min(t)),
                ms_max=float(np.max(t)), repeats=repeats, iterations=sorted({r["iterations"] for r in res}),
                linear_iterations_max=max(r["linear_iterations"] for r in res), exit_codes=sorted({r["exit_code"] for r in res}),
                cost_initial=res[0]["cost_initial"], cost_final=res[0]["cost_final"], worst_position_error_m=err)


def timed_wide(G, repeats, check_every):
    """the chip-wide form of one graph: host wall time round the synchronous call, the device idle before it"""
    import torch
    bank = N.PGO3(1, G.n_nodes, G.n_edges)
    st = torch.cuda.current_stream()
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up)
        bank.set_graph(0, G.poses, G.ref, G.mov, G.meas, G.info)
        torch.cuda.synchronize()
        t = time.perf_counter()
        bank.optimize_wide(0, stream=st, check_every=check_every)
        times.append(1e3 * (time.perf_counter() - t))
    T, r = bank.poses(0)
    bank.close()
    return times[1:], r, float(np.max(np.abs((T - G.truth)[:, :3, 3])))


def report(case, form, clock, G, ms, repeats, r, err, **more):
    """ms: (median, min, max)"""
    print(json.dumps(dict(case=case, form=form, clock=clock, nodes=G.n_nodes, links=G.n_edges, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2],
                          repeats=repeats, iterations=r["iterations"], linear_iterations=r["linear_iterations"],
                          us_per_inner_iteration=1e3 * ms[0] / max(r["linear_iterations"], 1), exit_code=r["exit_code"],
                          cost_final=r["cost_final"], worst_position_error_m=err, **more)), flush=True)


def wide_leg(repeats, skip_replay):
    version = N.lib().ndtgpu_version().decode()
    cases = [("500 nodes", pgo_cost.grid(20, 25, (1,), 1), repeats), ("1500 nodes", pgo_cost.grid(30, 50, (2,), 3), repeats)]
    if not skip_replay:
        cases.append(("replay size", pgo_cost.grid(50, 100, (2, 1), 2), max(1, repeats // 2)))
    for k, (case, G2, reps) in enumerate(cases):
        G = lift(G2, 7 + k)
        one = timed([G], reps)
        r1 = dict(iterations=one["iterations"][0], linear_iterations=one["linear_iterations_max"], exit_code=one["exit_codes"][0],
                  cost_final=one["cost_final"])
        report(case, "one workgroup", "device events", G, (one["ms_median"], one["ms_min"], one["ms_max"]), reps, r1,
               one["worst_position_error_m"], version=version)
        for every in (8, 32, 128):
            t, r, err = timed_wide(G, repeats, every)
            ms = (float(np.median(t)), float(np.min(t)), float(np.max(t)))
            report(case, "wide", "host wall time", G, ms, repeats, r, err, check_every=every, ratio_to_one_workgroup=one["ms_median"] / ms[0],
                   version=version)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--wide", action="store_true", help="both forms on one graph of 500, 1500 and 5000 nodes")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("pgo3_cost: no HIP device (nothing to measure)")
    if a.wide:
        wide_leg(a.repeats, a.skip_replay)
        return
    version = N.lib().ndtgpu_version().decode()
    cases = [("one graph of 500 nodes", [pgo_cost.grid(20, 25, (1,), 1)], a.repeats),
             ("256 graphs of 500 nodes", [pgo_cost.grid(20, 25, (1,), 100 + k) for k in range(256)], a.repeats)]
    if not a.skip_replay:
        cases.append(("replay size", [pgo_cost.grid(50, 100, (2, 1), 2)], max(1, a.repeats // 2)))
    for case, flat, repeats in cases:
        se3 = timed([lift(G2, 7 + k) for k, G2 in enumerate(flat)], repeats)
        se2 = pgo_cost.timed(flat, repeats)
        print(json.dumps(dict(case=case, form="SE(3)", version=version, **se3)), flush=True)
        print(json.dumps(dict(case=case, form="SE(2)", version=version, ratio_se3_to_se2=se3["ms_median"] / se2["ms_median"], **se2)), flush=True)
    if not a.skip_model:
        G = lift(pgo_cost.grid(20, 25, (1,), 1), 7)
        t = time.perf_counter()
        _, r = M.optimize(G)
        print(json.dumps(dict(case="NumPy model, dense, 500 nodes", version=version, seconds=time.perf_counter() - t, iterations=r["iterations"],
                              threads=os.environ.get("OMP_NUM_THREADS", "all"))), flush=True)


if __name__ == "__main__":
    main()
