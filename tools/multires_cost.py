#!/usr/bin/env python3
"""Cost of the coarse-to-fine registrar (ndtgpu_register_multires_device) on the bench's 2D scenes: registrations/s for the
default list and for {0.5, 1, 2, 4}, per-level build and match milliseconds (the same levels through ndtgpu_mapset_build +
ndtgpu_match_batch_device, timed with events), and the A/B of the fused source build (move on load) against a separate move
plus build (NDTGPU_MR_FUSED=0).  usage: python tools/multires_cost.py [--pairs 1024] [--points 100000] [--reps 5] [--max-cells 4096]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ndt_feature_graph_amd as N                       # noqa: E402
from ndt_feature_graph_amd import binding, synth      # noqa: E402

SIZE, RNG = [100.0, 100.0, 1.0], 30.0


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-cells", type=int, default=4096)   # (the bench registrar's; 0: the library's min(slots, 16384))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = a.pairs
    pr = synth.pair_2d(torch.arange(5001, 5001 + B, dtype=torch.int64, device=dev), a.points, device=dev)
    tg, sc = pr["fixed"].contiguous(), pr["moving"].contiguous()
    T0 = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
    out = {"pairs": B, "points": a.points, "max_cells": a.max_cells}
    for name, lst in (("default", (0.2, 0.5, 1.0, 2.0)), ("0.5-4", (0.5, 1.0, 2.0, 4.0))):
        mr = N.MultiRes([0, 0, 0], SIZE, lst, pairs_per_batch=B, max_cells=a.max_cells)
        res = torch.zeros((B, 64 * len(lst)), dtype=torch.uint8, device=dev)
        row = {}
        for fused in ("1", "0"):
            os.environ["NDTGPU_MR_FUSED"] = fused
            T16 = T0.clone()
            ms = timed(lambda: (T16.copy_(T0), mr.register_device(tg, sc, T16, res, use_initial_guess=True, range_limit=RNG)), a.reps)
            row["fused" if fused == "1" else "move+build"] = {"ms_per_call": ms, "registrations_per_s": B / ms * 1e3}
        os.environ.pop("NDTGPU_MR_FUSED", None)
        mr.close()
        # per level: the existing entries on the same clouds (source as given: the cost of a build and a match at that cell size)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        levels = {}
        for r in lst:
            ts = N.MapSet(r, [0, 0, 0], SIZE, n_maps=B, max_cells=a.max_cells)
            ss = N.MapSet(r, [0, 0, 0], SIZE, n_maps=B, max_cells=a.max_cells)
            b_ms = timed(lambda: ss.build(sc, range_limit=RNG), a.reps)
            ts.build(tg, range_limit=RNG)
            T16 = T0.clone()
            rr = torch.zeros((B, 64), dtype=torch.uint8, device=dev)
            m_ms = timed(lambda: (T16.copy_(T0), binding.match_batch_device(ts, idx, ss, idx, T16, rr, B)), a.reps)
            levels[str(r)] = {"build_ms": b_ms, "match_ms": m_ms}
            ts.close()
            ss.close()
        row["levels"] = levels
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
