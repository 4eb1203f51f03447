#!/usr/bin/env python3
"""Times ndtgpu_featbank_extract_device (device events around the call, one warm-up, median over repeats) at the default
parameters for 1024 scans of 360, 720 and 1440 beams:
  - the extraction alone,
  - the extraction followed by ndtgpu_featbank_match_device of consecutive scans (scan b against scan b + 1: 1023 pairs,
    inlier_probability 0.5 and success_probability 0.99, 17 hypotheses -- a hall has too few corners for the default 0.1).
The scans cycle through `--distinct` seeded halls of synth.scan_2d_ranges (range noise 0.005 m), each seen from (0, 0, 0) and from
(0.3, -0.2, 0.1) in turn, so every workgroup does the work of a real scan and every pair that of a real link.  There is no baseline
to compare with: flirtlib is not in the reference tree, and tests/flirt_model.py is a checker.
usage: python tools/featextract_cost.py [--repeats R] [--distinct P] [--only BEAMS] [--scans N]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402
from ndt_feature_graph_amd import binding, synth  # noqa: E402

MAX_POINTS = 64


def timed(n_beams, n_scans, distinct, repeats):
    import torch
    dev = torch.device("cuda", 0)
    seeds = [1 + (k // 2) for k in range(2 * distinct)]
    poses = [(0.0, 0.0, 0.0) if k % 2 == 0 else (0.3, -0.2, 0.1) for k in range(2 * distinct)]
    rr, a0, inc = synth.scan_2d_ranges(seeds, poses, n_beams, noise_sigma=0.005)
    ranges = rr[torch.arange(n_scans) % (2 * distinct)].contiguous().to(dev)
    fm = N.FeatureMatcher(n_scans, MAX_POINTS, 48)
    idx = torch.arange(n_scans, dtype=torch.int32, device=dev)
    ref, mov = idx[:-1].contiguous(), idx[1:].contiguous()
    recs = torch.zeros((n_scans, binding.FEATEXTRACT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    out = torch.zeros((n_scans - 1, binding.FEATMATCH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    T16 = torch.zeros((n_scans - 1, 16), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream()
    t_extract, t_both = [], []
    for _ in range(repeats + 1):                   # (the first run warms up)
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record(st)
        fm.extract_device(idx, ranges, a0, inc, recs, stream=st)
        b.record(st)
        fm.match_device(ref, mov, out, T16, None, stream=st, inlier_probability=0.5, success_probability=0.99)
        c.record(st)
        c.synchronize()
        t_extract.append(a.elapsed_time(b))
        t_both.append(a.elapsed_time(c))
    r = recs.cpu().numpy().view(binding.FEATEXTRACT_RESULT_DTYPE).reshape(-1)
    m = out.cpu().numpy().view(binding.FEATMATCH_RESULT_DTYPE).reshape(-1)
    fm.close()
    ok = m["status"] == 0
    # scan b + 1 into scan b: the planted pose where b is even, its inverse where b is odd (within one hall)
    same_hall = (np.arange(n_scans - 1) % 2 == 0) & ok
    err = np.hypot(m["x"] - 0.3, m["y"] + 0.2)[same_hall]
    te, tb = t_extract[1:], t_both[1:]
    return dict(beams=n_beams, scans=n_scans, distinct_scans=2 * distinct, lds_bytes=2560 + ((n_beams + 7) // 8 * 8) * 48,
                extract_ms_median=float(np.median(te)), extract_ms_min=float(np.min(te)), extract_ms_max=float(np.max(te)),
                extract_us_per_scan=1e3 * float(np.median(te)) / n_scans,
                extract_and_match_ms_median=float(np.median(tb)), extract_and_match_ms_min=float(np.min(tb)),
                extract_and_match_ms_max=float(np.max(tb)), statuses=sorted({int(s) for s in r["status"]}),
                n_valid_mean=float(np.mean(r["n_valid"])), n_found_mean=float(np.mean(r["n_found"])), n_found_max=int(np.max(r["n_found"])),
                match_ok=int(np.sum(ok)), same_hall_pairs_ok=int(np.sum(same_hall)),
                same_hall_median_xy_error_m=float(np.median(err)) if err.size else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--scans", type=int, default=1024)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("featextract_cost: no HIP device (nothing to measure)")
    for n_beams in (360, 720, 1440):
        if a.only and a.only != n_beams:
            continue
        print(json.dumps(dict(case="%d scans of %d beams" % (a.scans, n_beams), **timed(n_beams, a.scans, a.distinct, a.repeats))), flush=True)


if __name__ == "__main__":
    main()
