#!/usr/bin/env python3
"""What the feature path adds to a fuser-bank update: ndtgpu_fuser_update_batch_feat against the plain ndtgpu_fuser_update_batch of
the same process, on the `fuser_update` leg's shape of bench.py (64 fusers x 100 k points per scan, 0.5 m cells, 100 x 100 x 1 m
node maps, the fuser's default Params()), with cur sets of 24 and of 256 interest points per scan.

Timing: a HIP event before the call and one behind it on the call's stream (the call is asynchronous; the interval covers the
host's staging of the call and all its device work), one interval per scan step, the MEDIAN over the steps after a warm-up step;
min and max beside it.  The interest points are fixed in the map frame and seen from every pose with 1e-3 m of noise, descriptors
equal at every step, so that the RANSAC ends OK and the FLIRT cells are really built (24 points: 24 cells + 40 odometry cells; 256
points: truncated to 24).  Staging the cur sets (ndtgpu_featbank_set) is outside the interval: on the device path they come from
ndtgpu_featbank_extract_device.
usage: python tools/fuser_feat_cost.py [--fusers 64] [--points 100000] [--steps 9]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402

RES, RANGE, SIZE = 0.5, 30.0, [100.0, 100.0, 1.0]


def T2(p):
    T = np.tile(np.eye(4), (p.shape[0], 1, 1))
    T[:, 0, 0] = np.cos(p[:, 2]); T[:, 0, 1] = -np.sin(p[:, 2]); T[:, 1, 0] = np.sin(p[:, 2]); T[:, 1, 1] = np.cos(p[:, 2])
    T[:, 0, 3], T[:, 1, 3] = p[:, 0], p[:, 1]
    return T


def seen(world, pose, rng):
    """world points [K, 3] from the 2D pose (x, y, yaw), 1e-3 m of noise"""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = world[:, 0] - pose[0], world[:, 1] - pose[1]
    out = np.zeros_like(world)
    out[:, 0] = c * dx + s * dy
    out[:, 1] = -s * dx + c * dy
    out[:, :2] += rng.uniform(-1e-3, 1e-3, size=(world.shape[0], 2))
    out[:, 2] = np.arctan2(np.sin(world[:, 2] - pose[2]), np.cos(world[:, 2] - pose[2]))
    return out


def main():
    import torch
    from ndt_feature_graph_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--fusers", type=int, default=64)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=9)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("fuser_feat_cost: no HIP device (nothing to measure)")
    dev = torch.device("cuda")
    B, n_steps = a.fusers, a.steps
    prm = N.fuser_params(resolution=RES, map_size_x=SIZE[0], map_size_y=SIZE[1], map_size_z=SIZE[2], sensor_range=RANGE, neighbours=2,
                         itr_max=30, delta_score=1e-6, max_cells=4096)
    gen = np.random.default_rng(11)
    seeds = torch.arange(9001, 9001 + B, dtype=torch.int64, device=dev)
    poses = np.zeros((n_steps + 1, B, 3))
    for s in range(1, n_steps + 1):
        step = np.stack([gen.uniform(0.15, 0.3, B), gen.uniform(-0.05, 0.05, B), gen.uniform(-0.04, 0.04, B)], axis=1)
        c, sn = np.cos(poses[s - 1, :, 2]), np.sin(poses[s - 1, :, 2])
        poses[s, :, 0] = poses[s - 1, :, 0] + c * step[:, 0] - sn * step[:, 1]
        poses[s, :, 1] = poses[s - 1, :, 1] + sn * step[:, 0] + c * step[:, 1]
        poses[s, :, 2] = poses[s - 1, :, 2] + step[:, 2]
    scans = [synth.scan_2d(seeds, torch.as_tensor(poses[s], device=dev), a.points, noise_stream=s).contiguous() for s in range(n_steps + 1)]
    Tm = []
    for s in range(n_steps):
        true = np.linalg.inv(T2(poses[s])) @ T2(poses[s + 1])
        noise = T2(np.stack([gen.normal(0, 0.01, B), gen.normal(0, 0.01, B), gen.normal(0, 0.003, B)], axis=1))
        Tm.append(true @ noise)
    st = torch.cuda.current_stream()
    version = N.lib().ndtgpu_version().decode()

    def run(K):
        """K: interest points per scan; None: the plain entries -> per-step milliseconds (the warm-up step dropped), records"""
        bank = N.FuserBank(prm, B)
        fm = None
        if K is not None:
            side = int(math.ceil(math.sqrt(K)))
            fm = N.FeatureMatcher(3 * B, max(64, 4 * K), 48)
            bank.attach_features(fm, B, 2 * B)
            worlds, descs = [], []
            for k in range(B):
                w = np.zeros((K, 3))
                w[:, 0] = 1.0 + 0.8 * (np.arange(K) % side) + gen.uniform(-0.1, 0.1, K)
                w[:, 1] = -0.4 * side + 0.8 * (np.arange(K) // side) + gen.uniform(-0.1, 0.1, K)
                w[:, 2] = gen.uniform(-1, 1, K)
                worlds.append(w)
                descs.append(gen.uniform(0.1, 1.0, (K, 48)))

            def stage(s):
                for k in range(B):
                    fm.set(k, seen(worlds[k], poses[s, k], gen), descs[k])
            stage(0)
        cur = None if K is None else np.arange(B)
        bank.initialize(T2(poses[0]), scans[0], stream=st, cur_sets=cur)
        ms, rec = [], None
        for s in range(n_steps):
            if K is not None:
                stage(s + 1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            bank.update(Tm[s], scans[s + 1], stream=st, cur_sets=cur)
            e1.record(st)
            T, r = bank.poses()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            if K is not None:
                rec = bank.feat_results()
        bank.close()
        if fm is not None:
            fm.close()
        return ms[1:], T, rec

    plain_ms, T_plain, _ = run(None)
    base = float(np.median(plain_ms))
    print(json.dumps(dict(case="plain update", fusers=B, points=a.points, steps_timed=len(plain_ms), ms_median=base, ms_min=min(plain_ms),
                          ms_max=max(plain_ms), version=version)), flush=True)
    for K in (24, 256):
        ms, T, rec = run(K)
        med = float(np.median(ms))
        print(json.dumps(dict(case="update with features", cur_points=K, fusers=B, points=a.points, steps_timed=len(ms), ms_median=med,
                              ms_min=min(ms), ms_max=max(ms), added_ms=med - base, added_percent=100.0 * (med - base) / base,
                              ransac_ok=int((rec["ransac"]["status"] == 0).sum()), feat_cells=[int(rec["n_feat_cells"].min()),
                                                                                               int(rec["n_feat_cells"].max())],
                              truncated=int(rec["truncated"].sum()), version=version)), flush=True)


if __name__ == "__main__":
    main()
