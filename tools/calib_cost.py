#!/usr/bin/env python3
"""What the extrinsic calibration's search costs (ndtgpu_calib_search_device, include/ndtgpu.h "extrinsic calibration"), at the
shape of the reference's launch files -- 16 pairs of 720-beam scans, x and y +- 0.05 by 0.001 and yaw +- 0.01 by 0.001 (about
100 x 100 x 20 candidates) -- and at the program's own defaults, +- 0.05 by 0.01 and +- 2 degrees by 0.05 degrees (about
10 x 10 x 80):
  search    the launches of one call: a HIP event before the call and one behind it on the call's stream; the MEDIAN of --reps
            intervals after a warm-up, min and max beside it;
  ckdtree   the literal form on the same box's host: per candidate and pair both clouds moved into the world frame, a SciPy cKDTree
            of cloud1 and one 1-NN query per point of cloud2 (what scoreICP does with PCL's kd-tree), timed over --sample
            candidates spread evenly over the lattice and SCALED to the lattice's size -- the figure is an extrapolation and the
            line says so.
One JSON line per lattice.  usage: python tools/calib_cost.py [--reps 7] [--sample 48] [--beams 720] [--pairs 16]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402

PLANTED = (0.023, 0.012, 0.004)
LATTICES = {"launch files": (0.0, 0.0, 0.0, 0.05, 0.05, 0.01, 0.001, 0.001),
            "program defaults": (0.0, 0.0, 0.0, 0.05, 0.05, 2.0 * math.pi / 180.0, 0.01, 0.05 * math.pi / 180.0)}


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), reps=len(ms))


def ckdtree_seconds_per_candidate(clouds, base, pairs, lat, sample):
    from scipy.spatial import cKDTree
    nx, ny, nyaw = len(lat["xs"]), len(lat["ys"]), len(lat["yaws"])
    picks = np.linspace(0, nx * ny * nyaw - 1, sample).astype(np.int64)
    t0 = time.perf_counter()
    best = None
    for idx in picks:
        ix, iy, iw = idx // (ny * nyaw), (idx // nyaw) % ny, idx % nyaw
        ts = (lat["xs"][ix], lat["ys"][iy], lat["yaws"][iw])
        e = 0.0
        for i1, i2 in pairs:
            w = []
            for i in (i1, i2):
                x, y, t = base[i]
                c, s = math.cos(t), math.sin(t)
                sx, sy, st = x + c * ts[0] - s * ts[1], y + s * ts[0] + c * ts[1], t + ts[2]
                c, s = math.cos(st), math.sin(st)
                p = clouds[i]
                w.append(np.stack([sx + c * p[:, 0] - s * p[:, 1], sy + s * p[:, 0] + c * p[:, 1], p[:, 2]], axis=1).astype(np.float32))
            d, _ = cKDTree(w[0]).query(w[1], k=1)
            e += float(np.minimum(d.astype(np.float64) ** 2, 0.01).sum())
        best = e if best is None else min(best, e)
    return (time.perf_counter() - t0) / sample, best


def main():
    import torch
    from ndt_feature_graph_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=48)
    ap.add_argument("--beams", type=int, default=720)
    ap.add_argument("--pairs", type=int, default=16)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("calib_cost: no HIP device (nothing to measure)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    version = N.lib().ndtgpu_version().decode()

    # a base that turns by 30 degrees a step within a few centimetres, 1.5 m inside a corner of hall 5; the laser at PLANTED on it
    seed, n = 5, a.pairs + 1
    half, _ = synth.room_2d([seed])
    hx, hy = half[0].tolist()
    base = [(hx - 1.5 + 0.1 * math.cos(0.7 * k), hy - 1.5 + 0.1 * math.sin(0.9 * k), math.radians(30.0) * k) for k in range(n)]
    sens = []
    for x, y, t in base:
        c, s = math.cos(t), math.sin(t)
        sens.append((x + c * PLANTED[0] - s * PLANTED[1], y + s * PLANTED[0] + c * PLANTED[1], t + PLANTED[2]))
    ranges, a0, inc = synth.scan_2d_ranges([seed] * n, sens, a.beams, noise_sigma=0.005)
    rt = ranges.to(dev).contiguous()
    poses4 = np.array([[x, y, math.cos(t), math.sin(t)] for x, y, t in base])
    pairs = N.calib_select_pairs(poses4)
    assert len(pairs) == a.pairs, "the base must give one pair per step"

    proj = N.ScanProjector(n, a.beams)
    xyz = torch.zeros((n, a.beams, 4), dtype=torch.float32, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    proj.project_device(rt, xyz, a0, inc, n_kept_t=kept, r_min=0.3, r_max=20.0)
    torch.cuda.synchronize()
    proj.close()
    nk = kept.cpu().numpy()
    clouds = [xyz[k, :nk[k], :3].cpu().numpy().astype(np.float64) for k in range(n)]
    pt = torch.as_tensor(poses4, device=dev)
    prt = torch.as_tensor(pairs.view(np.int32), device=dev)
    res = torch.zeros(6, dtype=torch.int32, device=dev)

    for name, args in LATTICES.items():
        lat = N.calib_lattice(*args)
        nx, ny, nyaw = len(lat["xs"]), len(lat["ys"]), len(lat["yaws"])
        nc = nx * ny * nyaw
        cal = N.Calibrator(a.pairs, a.beams, nc)
        cal.search_device(xyz, kept, pt, prt, lat, res)                   # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            cal.search_device(xyz, kept, pt, prt, lat, res)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        r = N.Calibrator.read_result(res)
        cal.close()
        idx = int(r["index"])
        win = (float(lat["xs"][idx // (ny * nyaw)]), float(lat["ys"][(idx // nyaw) % ny]), float(lat["yaws"][idx % nyaw]))
        per, _ = ckdtree_seconds_per_candidate(clouds, base, pairs, lat, a.sample)
        line = dict(case=name, library=version, pairs=int(a.pairs), beams=int(a.beams), kept_mean=float(nk.mean()), lattice=[nx, ny, nyaw],
                    candidates=nc, search=stats(ms), winner=win, planted=PLANTED, score=float(r["score"]), flags=int(r["flags"]),
                    point_pairs=float(nc) * float(sum(int(nk[i]) * int(nk[j]) for i, j in pairs)),
                    ckdtree=dict(sampled_candidates=a.sample, ms_per_candidate=1e3 * per, ms_scaled_to_lattice=1e3 * per * nc,
                                 note="extrapolated from the sample"))
        line["ratio_ckdtree_over_search"] = line["ckdtree"]["ms_scaled_to_lattice"] / line["search"]["ms_median"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
