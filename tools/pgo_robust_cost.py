#!/usr/bin/env python3
"""Times the robust pose-graph optimisation (ndtgpu_pgo_optimize_robust, ndtgpu_pgo3_optimize_robust: DCS, Phi = 1, the defaults)
against the plain optimiser on the same graphs with FALSE LOOP CLOSURES, and reports how far each ends from the optimum of the
graph without them: the grid world of tools/pgo_cost.py at 500 nodes with 2 % false closures (links between nodes at least 2 apart
in index and 2 m apart in truth, measured uniformly in +-0.5 m / +-0.3 rad), in SE(2) and lifted to SE(3) as tools/pgo3_cost.py
does, one graph, a bank of 256 such graphs in one call, and the replay's 5000 nodes through the wide form.  Device events round
the call on the caller's stream (the robust call is synchronous towards the host: the events bracket its launches and the
host's looks between the rounds), the graph set again before every repeat, the median of the repeats after a warm-up.
usage: python tools/pgo_robust_cost.py [--repeats R] [--skip-replay] [--skip-se3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ndt_feature_graph_amd as N  # noqa: E402
import pgo3_model as M3  # noqa: E402
import pgo_model as M2  # noqa: E402
import pgo3_cost  # noqa: E402
import pgo_cost  # noqa: E402
import pgo_robust_model as R  # noqa: E402


def with_false_closures(mod, G, fraction, seed):
    """(G with fraction * n_edges false closures behind its links, the mask of the false ones)"""
    rng = np.random.default_rng(seed)
    k = max(1, int(round(fraction * G.n_edges)))
    two = mod is M2
    pairs = R._false_pairs(G.truth[:, :2] if two else G.truth[:, :3, 3], k, rng)
    if two:
        z = rng.uniform(-1.0, 1.0, size=(k, 3)) * [0.5, 0.5, 0.3]
    else:
        z = np.stack([M3.euler_T(*row) for row in rng.uniform(-1.0, 1.0, size=(k, 6)) * [0.5, 0.5, 0.5, 0.3, 0.3, 0.3]])
    ref = np.concatenate([G.ref, [a for a, _ in pairs]])
    mov = np.concatenate([G.mov, [b for _, b in pairs]])
    return mod.Graph(G.poses, ref, mov, np.concatenate([G.meas, z]), truth=G.truth), np.arange(ref.shape[0]) >= G.n_edges


def timed(mod, graphs, repeats, robust, wide=False):
    """-> (times [ms], poses of graph 0, per-graph records)"""
    import torch
    cls = N.PGO if mod is M2 else N.PGO3
    bank = cls(len(graphs), max(G.n_nodes for G in graphs), max(G.n_edges for G in graphs))
    st = torch.cuda.current_stream()
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up)
        for k, G in enumerate(graphs):
            bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        if robust:
            bank.optimize_robust(0, len(graphs), robust={}, wide=wide, stream=st)
        elif wide:
            bank.optimize_wide(0, stream=st)
        else:
            bank.optimize(stream=st)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    poses = [bank.poses(k)[0] for k in range(len(graphs))]
    recs = [bank.robust_links(k) if robust else bank.poses(k)[1] for k in range(len(graphs))]
    bank.close()
    return times[1:], poses, recs


def case(name, mod, cleans, repeats, wide=False):
    dirty = [with_false_closures(mod, G, 0.02, 500 + k) for k, G in enumerate(cleans)]
    graphs = [d[0] for d in dirty]
    _, clean_poses, _ = timed(mod, cleans[:1], 0, False, wide)
    out = dict(case=name, bank="SE(2)" if mod is M2 else "SE(3)", graphs=len(graphs), nodes=graphs[0].n_nodes, links=graphs[0].n_edges,
               false_closures=int(dirty[0][1].sum()), form="wide" if wide else "one workgroup", repeats=repeats,
               version=N.lib().ndtgpu_version().decode())
    t, poses, recs = timed(mod, graphs, repeats, False, wide)
    out.update(plain_ms=float(np.median(t)), plain_distance_m=R.distance(mod, poses[0], clean_poses[0]),
               plain_updates=sorted({r["iterations"] for r in recs}))
    t, poses, recs = timed(mod, graphs, repeats, True, wide)
    false = dirty[0][1]
    w = recs[0][1]
    out.update(robust_ms=float(np.median(t)), robust_ms_min=float(np.min(t)), robust_ms_max=float(np.max(t)),
               robust_distance_m=R.distance(mod, poses[0], clean_poses[0]), rounds=sorted({r[3]["rounds"] for r in recs}),
               inner_iterations_max=max(r[3]["linear_iterations"] for r in recs), exit_codes=sorted({r[3]["exit_code"] for r in recs}),
               false_weight_max=float(w[false].max()), true_weight_min=float(w[~false].min()), outliers=recs[0][3]["outliers"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--skip-se3", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("pgo_robust_cost: no HIP device (nothing to measure)")
    lifts = (lambda G, s: G, pgo3_cost.lift)
    for mod, lift in ((M2, lifts[0]),) + (() if a.skip_se3 else ((M3, lifts[1]),)):
        case("one graph of 500 nodes", mod, [lift(pgo_cost.grid(20, 25, (1,), 1), 7)], a.repeats)
        case("256 graphs of 500 nodes", mod, [lift(pgo_cost.grid(20, 25, (1,), 100 + k), 7 + k) for k in range(256)], a.repeats)
        if not a.skip_replay:
            case("replay size, wide", mod, [lift(pgo_cost.grid(50, 100, (2, 1), 2), 9)], max(1, a.repeats // 2), wide=True)


if __name__ == "__main__":
    main()
