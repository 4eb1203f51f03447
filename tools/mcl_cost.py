#!/usr/bin/env python3
"""Times ndtgpu_mcl_update (device events around the call, after warm-up; median and spread over repeats) for the node's default
1 x 100 particles, 1 x 50 000 and 64 x 1 024, with 20 k-point planar scans of the synth room at 0.5 m; and, from a rocprofv3
kernel trace of the same run (--kernel-stats CSV), the likelihood kernel's time and its share of the fp64 vector peak.  The
operations are the terms scored (ndtgpu_mcl_result.terms) times OPS_PER_TERM, an ESTIMATE of the fp64 operations per term read off
the source (not counted from the ISA or by counters): transform 18, float cast and three cell indices 15, R C R^T 45 + 6 adds,
the 3 x 3 inverse 30 and a division, the quadratic form 15, the term 3 and exp ~20.
usage: python tools/mcl_cost.py [--repeats R] [--only K]    (under rocprofv3 --kernel-trace --stats for the kernel figures)
       python tools/mcl_cost.py --only K --stats <that run's kernel_stats.csv> --terms T"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ndt_feature_graph_amd as N  # noqa: E402
from ndt_feature_graph_amd import synth  # noqa: E402

FP64_PEAK = 78.6e12        # MI355X fp64 vector peak (spec)
OPS_PER_TERM = 160         # estimate, see above
# (filters, particles, max_scan_cells).  The likelihood kernel cuts a filter's scan cells into at most 16 chunks of a multiple
# of 256 cells, one workgroup per (particle tile, chunk): with max_scan_cells 4096 the ~340 cells of these scans are two
# 256-cell chunks; with 8192 they are one 512-cell chunk, so 1 x 100 runs on a single workgroup -- the single-workgroup form the
# split is compared against.
SHAPES = [(1, 100, 4096), (1, 100, 8192), (1, 50000, 4096), (64, 1024, 4096)]


def run(n_filters, n_particles, cap, repeats, ms):
    pts = synth.scan_2d([1] * n_filters, torch.tensor([[0.2, 0.1, 0.05]] * n_filters, dtype=torch.float64), 20000).cuda()
    f = N.MCL(ms, [0] * n_filters, n_particles, scan_size=[60.0, 60.0, 1.0], max_scan_cells=cap)
    f.initialize(np.tile([0.2, 0.1, 0, 0, 0, 0.05], (n_filters, 1)), np.tile([0.3, 0.3, 0, 0, 0, 0.05], (n_filters, 1)))
    Tm = np.tile(np.eye(4), (n_filters, 1, 1))
    st = torch.cuda.current_stream()
    for _ in range(3):
        f.update(Tm, pts)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        f.update(Tm, pts)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    _, res = f.mean()
    terms = int(res["terms"].sum())
    f.close()
    return dict(filters=n_filters, particles=n_particles, max_scan_cells=cap, update_ms_median=float(np.median(times)), update_ms_min=float(np.min(times)),
                update_ms_max=float(np.max(times)), scan_cells=int(res["n_scan_cells"][0]), terms_per_update=terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--only", type=int, help="one shape of SHAPES (its index)")
    ap.add_argument("--stats", help="rocprofv3 kernel-stats CSV of a run of this tool with --only: the likelihood kernel's share of peak")
    ap.add_argument("--terms", type=int, help="terms per update that run printed")
    a = ap.parse_args()
    if a.stats:
        with open(a.stats) as fh:
            for r in csv.DictReader(fh):
                if "ndt_mcl_likelihood_kernel" in r["Name"]:
                    s = float(r["AverageNs"]) * 1e-9
                    ops = a.terms * OPS_PER_TERM
                    print(json.dumps(dict(shape=SHAPES[a.only], kernel="ndt_mcl_likelihood_kernel", calls=int(r["Calls"]),
                                          average_ms=s * 1e3, fp64_tflops=ops / s / 1e12, share_of_fp64_peak=ops / s / FP64_PEAK)))
        return
    if N.device_count() < 1:
        raise SystemExit("mcl_cost: no HIP device (nothing to measure)")
    ms = N.MapSet(0.5, [0, 0, 0], [60, 60, 1], n_maps=1, max_cells=4096)
    ms.build(synth.scan_2d([1], torch.tensor([[0.0, 0.0, 0.0]], dtype=torch.float64), 40000).numpy())
    shapes = SHAPES if a.only is None else [SHAPES[a.only]]
    rows = [run(nf, npart, cap, a.repeats, ms) for nf, npart, cap in shapes]
    for r in rows:
        r["fp64_ops_per_update"] = r["terms_per_update"] * OPS_PER_TERM
        print(json.dumps(r))


if __name__ == "__main__":
    main()
