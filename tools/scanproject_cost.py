#!/usr/bin/env python3
"""What the laser-scan projection costs (ndtgpu_scanproj_project_device, include/ndtgpu.h "laser-scan projection"), at 1024 scans of
1440 beams and at 64 scans of 100 000 beams:
  projection     the two launches alone: a HIP event before the call and one behind it on the call's stream;
  numpy+upload   the path it replaces on the same box: the projection in NumPy on the host (cosine, sine, the counter-based z draw,
                 the compaction per scan) and the upload of the float32 cloud, a host clock around work that ends in a device
                 synchronise;
  fuser update   at 64 x 100 000 only: the fuser bank's plain update (the `fuser_update` shape of bench.py: 0.5 m cells,
                 100 x 100 x 1 m node maps, default Params()) alone and with the projection of its scan in front of it on the same
                 stream, events around both; the two banks walk the same sequence on the same clouds.
Every figure is the MEDIAN of --reps (>= 8) intervals after a warm-up; min and max beside it.  One JSON line per case.
usage: python tools/scanproject_cost.py [--reps 9] [--skip-fuser]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ndt_feature_graph_amd as N  # noqa: E402

RES, RANGE, SIZE = 0.5, 30.0, [100.0, 100.0, 1.0]
R_MIN, R_MAX, VARZ = 0.5, 30.0, 0.02


def T2(p):
    T = np.tile(np.eye(4), (p.shape[0], 1, 1))
    T[:, 0, 0] = np.cos(p[:, 2]); T[:, 0, 1] = -np.sin(p[:, 2]); T[:, 1, 0] = np.sin(p[:, 2]); T[:, 1, 1] = np.cos(p[:, 2])
    T[:, 0, 3], T[:, 1, 3] = p[:, 0], p[:, 1]
    return T


def numpy_project(ranges, a0, inc, seed=0):
    """the projection on the host: float32 [n, n_beams, 3], the kept points first, NaN rows behind them"""
    import torch
    from ndt_feature_graph_amd import synth
    n, nb = ranges.shape
    i = np.arange(nb)
    a = a0 + i * inc
    c, s = np.cos(a), np.sin(a)
    idx = torch.as_tensor(i.astype(np.int64))
    out = np.full((n, nb, 3), np.nan, dtype=np.float32)
    for b in range(n):
        r = ranges[b]
        with np.errstate(invalid="ignore"):
            k = np.isfinite(r) & (r > R_MIN) & (r < R_MAX)
        m = int(k.sum())
        out[b, :m, 0] = (r[k] * c[k]).astype(np.float32)
        out[b, :m, 1] = (r[k] * s[k]).astype(np.float32)
        out[b, :m, 2] = (VARZ * synth.hash_uniform(seed, b, idx).numpy()[k]).astype(np.float32)
    return out


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), reps=len(ms))


def main():
    import torch
    from ndt_feature_graph_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-fuser", action="store_true")
    a = ap.parse_args()
    if a.reps < 8:
        raise SystemExit("scanproject_cost: at least 8 repetitions")
    if N.device_count() < 1:
        raise SystemExit("scanproject_cost: no HIP device (nothing to measure)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    version = N.lib().ndtgpu_version().decode()

    for n_scans, n_beams in ((1024, 1440), (64, 100000)):
        seeds = torch.arange(9001, 9001 + n_scans, dtype=torch.int64, device=dev)
        poses = torch.zeros((n_scans, 3), dtype=torch.float64, device=dev)
        ranges, a0, inc = synth.scan_2d_ranges(seeds, poses, n_beams)
        ranges = ranges.contiguous()
        sp = N.ScanProjector(n_scans, n_beams)
        cloud = torch.empty((n_scans, n_beams, 3), dtype=torch.float32, device=dev)
        kept = torch.zeros(n_scans, dtype=torch.int32, device=dev)
        ms = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            sp.project_device(ranges, cloud, a0, inc, n_kept_t=kept, stream=st)
            e1.record(st)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        n_kept = int(kept.sum())
        # bytes the two launches need: the ranges twice (the second time from the cache at best), a row per beam, the counts
        moved = n_scans * n_beams * (8 + 8 + 12)
        med = float(np.median(ms[1:]))
        print(json.dumps(dict(case="projection", scans=n_scans, beams=n_beams, kept_share=n_kept / (n_scans * n_beams), **stats(ms[1:]),
                              us_per_scan=1e3 * med / n_scans, gbytes_per_s=moved / (med * 1e-3) / 1e9, version=version)), flush=True)
        host_ranges = ranges.cpu().numpy()
        gpu_bits = cloud.cpu().numpy()
        ms_model, ms_upload = [], []
        up = None
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            xyz = numpy_project(host_ranges, a0, inc)
            t1 = time.perf_counter()
            up = torch.as_tensor(xyz, device=dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ms_model.append(1e3 * (t1 - t0))
            ms_upload.append(1e3 * (t2 - t1))
        both = [x + y for x, y in zip(ms_model[1:], ms_upload[1:])]
        same_kept = bool(np.array_equal(np.isnan(xyz), np.isnan(gpu_bits)))
        print(json.dumps(dict(case="numpy+upload", scans=n_scans, beams=n_beams, **stats(both), model_ms_median=float(np.median(ms_model[1:])),
                              upload_ms_median=float(np.median(ms_upload[1:])), same_kept_rows_as_device=same_kept,
                              times_the_projection=float(np.median(both)) / med, version=version)), flush=True)
        del up
        sp.close()

    if a.skip_fuser:
        return
    B, nb, n_steps = 64, 100000, a.reps + 1
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
    ranges, a0, inc = [], None, None
    for s in range(n_steps + 1):
        r, a0, inc = synth.scan_2d_ranges(seeds, torch.as_tensor(poses[s], device=dev), nb, noise_stream=s)
        ranges.append(r.contiguous())
    Tm = []
    for s in range(n_steps):
        true = np.linalg.inv(T2(poses[s])) @ T2(poses[s + 1])
        noise = T2(np.stack([gen.normal(0, 0.01, B), gen.normal(0, 0.01, B), gen.normal(0, 0.003, B)], axis=1))
        Tm.append(true @ noise)
    sp = N.ScanProjector(B, nb)
    clouds = [torch.empty((B, nb, 3), dtype=torch.float32, device=dev) for _ in range(n_steps + 1)]
    for s in range(n_steps + 1):
        sp.project_device(ranges[s], clouds[s], a0, inc, stream=st, seed=s)
    torch.cuda.synchronize()

    def run(project):
        bank = N.FuserBank(prm, B)
        scratch = torch.empty((B, nb, 3), dtype=torch.float32, device=dev)
        bank.initialize(T2(poses[0]), clouds[0], stream=st)
        ms = []
        for s in range(n_steps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            if project:
                sp.project_device(ranges[s + 1], scratch, a0, inc, stream=st, seed=s + 1)
                bank.update(Tm[s], scratch, stream=st)
            else:
                bank.update(Tm[s], clouds[s + 1], stream=st)
            e1.record(st)
            T, _ = bank.poses()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        bank.close()
        return ms[1:], T

    plain, T_plain = run(False)
    withp, T_with = run(True)
    base, med = float(np.median(plain)), float(np.median(withp))
    print(json.dumps(dict(case="fuser update alone", fusers=B, beams=nb, **stats(plain), version=version)), flush=True)
    print(json.dumps(dict(case="projection + fuser update", fusers=B, beams=nb, **stats(withp), added_ms=med - base,
                          added_percent=100.0 * (med - base) / base, same_poses=bool(np.array_equal(T_plain, T_with)), version=version)),
          flush=True)
    sp.close()


if __name__ == "__main__":
    main()
