#!/usr/bin/env python3
"""Times ndtgpu_featbank_match_device (device events around the call, one warm-up, median over repeats) at the default parameters
(230 hypotheses) for
  - 1024 pairs of sets of 64, 256 and 1024 points,
  - the replay's 44 486 gated edges at 128 points per set,
and reports how many hypotheses a pair tested on average (a hypothesis the rigidity test skips costs nothing).  The pairs cycle
through `--distinct` seeded (ref, mov) pairs of synth.feature_sets with 60 % of the points in common, so every workgroup does
the work of a real loop-closure candidate.  There is no baseline to compare with: flirtlib is not in the reference tree, and
tests/featmatch_model.py is a checker.
usage: python tools/featmatch_cost.py [--repeats R] [--distinct P] [--only POINTS]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402
from ndt_feature_graph_amd import binding, synth  # noqa: E402


def timed(points, n_pairs, distinct, repeats):
    import torch
    dev = torch.device("cuda", 0)
    fm = N.FeatureMatcher(2 * distinct, points, 48)
    for p in range(distinct):
        f = synth.feature_sets(1000 + p, points, points, (6 * points) // 10, (0.3, -0.2, 0.4))
        fm.set(2 * p, f["ref_pos"].numpy(), f["ref_desc"].numpy())
        fm.set(2 * p + 1, f["mov_pos"].numpy(), f["mov_desc"].numpy())
    k = torch.arange(n_pairs, dtype=torch.int32, device=dev) % distinct
    ref, mov = (2 * k).contiguous(), (2 * k + 1).contiguous()
    out = torch.zeros((n_pairs, binding.FEATMATCH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    T16 = torch.zeros((n_pairs, 16), dtype=torch.float64, device=dev)
    corr = torch.zeros((n_pairs, points, 2), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    times = []
    for _ in range(repeats + 1):                   # (the first run warms up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fm.match_device(ref, mov, out, T16, corr, stream=st)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    r = out.cpu().numpy().view(binding.FEATMATCH_RESULT_DTYPE).reshape(-1)
    fm.close()
    t = times[1:]
    return dict(points=points, pairs=n_pairs, distinct_pairs=distinct, ms_median=float(np.median(t)), ms_min=float(np.min(t)),
                ms_max=float(np.max(t)), us_per_pair=1e3 * float(np.median(t)) / n_pairs, statuses=sorted({int(s) for s in r["status"]}),
                n_tested_mean=float(np.mean(r["n_tested"])), n_candidates_mean=float(np.mean(r["n_candidates"])),
                n_inliers_mean=float(np.mean(r["n_inliers"])), worst_xy_error_m=float(np.max(np.hypot(r["x"] - 0.3, r["y"] + 0.2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("featmatch_cost: no HIP device (nothing to measure)")
    for points, n_pairs, what in ((64, 1024, "1024 pairs"), (256, 1024, "1024 pairs"), (1024, 1024, "1024 pairs"),
                                  (128, 44486, "the replay's gated edges")):
        if a.only and a.only != points:
            continue
        print(json.dumps(dict(case="%s at %d points per set" % (what, points), **timed(points, n_pairs, a.distinct, a.repeats))), flush=True)


if __name__ == "__main__":
    main()
