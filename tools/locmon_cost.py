#!/usr/bin/env python3
"""What the localisation monitor costs (ndtgpu_locmon_*, include/ndtgpu.h "localisation monitor"):
  field          the distance field of the replay's world (tools/occgrid_cost.py: all node maps of the replay's shape assembled into
                 one map of 1360 x 1200 x 2 cells of 0.5 m) rasterised at 0.05 m (13600 x 12000 pixels), R = 7: set_grids_device;
  evaluate       1024 queries of 1440-beam scans in that field: evaluate_device;
  adjust         adjustPose of one scan over a 20 x 20 x 315 lattice (pos_range 0.5, dpos 0.05, dtheta 0.02): adjust_device;
  evaluate+fuser 64 queries in front of the fuser bank's plain update (64 fusers x 1440 beams) on one stream, against the update alone.
Each is timed with HIP events around the call, the MEDIAN of --reps (7) intervals after a warm-up, min and max beside it.
Baselines on the same box: SciPy's distance_transform_edt (one core) on a crop of --crop x --crop pixels of the same grid, SCALED to
the whole grid by the pixel count (an extrapolation, said so in the record); the NumPy evaluator of tests/locmon_model.py on --model-queries
of the queries, scaled to all of them; for adjust the same evaluator scaled from --model-queries candidates.  One JSON line per case.
usage: python tools/locmon_cost.py [--reps 7] [--nodes 5000] [--skip-fuser]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ndt_feature_graph_amd as N  # noqa: E402
import locmon_model as M  # noqa: E402
import world_cost as WC  # noqa: E402
import world_model as W  # noqa: E402

PIXEL, MAX_DIST = 0.05, 0.375


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), reps=len(ms))


def timed(call, reps, st):
    import torch
    ms = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[1:]


def T2(p):
    T = np.tile(np.eye(4), (p.shape[0], 1, 1))
    T[:, 0, 0] = np.cos(p[:, 2]); T[:, 0, 1] = -np.sin(p[:, 2]); T[:, 1, 0] = np.sin(p[:, 2]); T[:, 1, 1] = np.cos(p[:, 2])
    T[:, 0, 3], T[:, 1, 3] = p[:, 0], p[:, 1]
    return T


def main():
    import torch
    from ndt_feature_graph_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--node-points", type=int, default=20000)
    ap.add_argument("--crop", type=int, default=3000)
    ap.add_argument("--model-queries", type=int, default=32)
    ap.add_argument("--skip-fuser", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("locmon_cost: no HIP device (nothing to measure)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    version = N.lib().ndtgpu_version().decode()

    # ---- the replay's world and its grid
    pool, T_local, T_world, room = WC.replay_nodes(a.nodes, a.node_points)
    n_rooms = int(room.max()) + 1
    cols, rows = min(n_rooms, 8), (n_rooms + 7) // 8
    centre = [40.0 * (cols - 1), 40.0 * (rows - 1), 0.0]
    size = [80.0 * (cols - 1) + 120.0, 80.0 * (rows - 1) + 120.0, 1.0]
    world = N.MapSet(WC.RES, centre, size, n_maps=1, max_cells=1 << 20)
    N.assemble_world(world, 0, pool, [list(range(a.nodes))], [T_world])
    wcells = W.grid_cells(WC.RES, size)
    w, h, origin = N.occupancy_grid_dims(WC.RES, wcells, centre, PIXEL)
    grid_t = torch.empty(h * w, dtype=torch.int8, device=dev)
    g_t, _ = world.occupancy_grid(0, 1, PIXEL, out=grid_t)
    torch.cuda.synchronize()
    pool.close()
    n_beams = 1440
    mon = N.LocalizationMonitor(1, w * h, n_beams, 22 * 22 * 320)
    R = N.locmon_radius(MAX_DIST, PIXEL)
    ms = timed(lambda: mon.set_grids_device(g_t, PIXEL, [origin[:2]], stream=st, max_dist=MAX_DIST), a.reps, st)
    med = float(np.median(ms))
    n_obst = int((g_t >= 55).sum())
    rec = dict(case="field", width=w, height=h, mpixels=w * h / 1e6, R=R, obstacle_pixels=n_obst, **stats(ms), gpixels_per_s=w * h / (med * 1e-3) / 1e9,
               version=version)
    # the baseline on a crop around the first room, and the device's field of the crop against it where the crop's rim cannot matter
    from scipy.ndimage import distance_transform_edt
    cw = min(a.crop, w, h)
    x0, y0 = min(max(int((0.0 - origin[0]) / PIXEL) - cw // 2, 0), w - cw), min(max(int((0.0 - origin[1]) / PIXEL) - cw // 2, 0), h - cw)
    crop = g_t[0, y0:y0 + cw, x0:x0 + cw].cpu().numpy()
    t0 = time.perf_counter()
    d2 = np.rint(distance_transform_edt(~(crop >= 55)) ** 2).astype(np.int64) if (crop >= 55).any() else np.full(crop.shape, 1 << 40)
    t_edt = 1e3 * (time.perf_counter() - t0)
    want = np.where(d2 <= R * R, d2, M.FIELD_FAR)
    got = mon.field(0)[y0:y0 + cw, x0:x0 + cw]
    inner = (slice(R, cw - R), slice(R, cw - R))
    rec.update(scipy_crop_pixels=cw * cw, scipy_crop_ms=t_edt, scipy_scaled_to_the_grid_ms=t_edt * (w * h) / (cw * cw),
               scipy_scaled_over_device=t_edt * (w * h) / (cw * cw) / med, crop_obstacle_pixels=int((crop >= 55).sum()),
               crop_interior_equals_scipy=bool(np.array_equal(got[inner], want[inner])))
    print(json.dumps(rec), flush=True)

    # ---- evaluate: 1024 queries of 1440-beam scans taken in the first rooms, poses jittered around the truth
    n_q = 1024
    gen = np.random.default_rng(5)
    local = np.stack([gen.uniform(-8, 8, n_q), gen.uniform(-8, 8, n_q), gen.uniform(-np.pi, np.pi, n_q)], axis=1)
    q_room = np.arange(n_q) % max(n_rooms, 1)
    ranges, a0, inc = synth.scan_2d_ranges(torch.as_tensor(4000 + q_room, dtype=torch.int64, device=dev), torch.as_tensor(local, device=dev), n_beams)
    ranges = ranges.contiguous()
    pose = local.copy()
    pose[:, 0] += 80.0 * (q_room % 8) + gen.normal(0, 0.05, n_q)
    pose[:, 1] += 80.0 * (q_room // 8) + gen.normal(0, 0.05, n_q)
    pose[n_q // 2:, 0] += 3.0                                      # half of them 3 m off
    q = N.LocalizationMonitor.queries(np.arange(n_q), 0, pose[:, 0], pose[:, 1], np.cos(pose[:, 2]), np.sin(pose[:, 2]))
    q_t = torch.from_numpy(q.view(np.uint8).copy()).to(dev)
    res_t = torch.zeros(n_q * 24, dtype=torch.uint8, device=dev)
    mon.set_beams(n_beams, a0, inc, stream=st)
    ms = timed(lambda: mon.evaluate_device(ranges, q_t, res_t, stream=st, r_min=0.5, r_max=30.0), a.reps, st)
    med = float(np.median(ms))
    got = mon.read(res_t, N.LOCMON_RESULT_DTYPE, n_q)
    fld = mon.field(0)
    cb, sb = N.locmon_beam_table(n_beams, a0, inc)
    host_r = ranges.cpu().numpy()
    m = min(a.model_queries, n_q)
    t0 = time.perf_counter()
    want = M.evaluate([fld], [origin[:2]], PIXEL, MAX_DIST, cb, sb, host_r, q[:m], 0.5, 30.0)
    t_model = 1e3 * (time.perf_counter() - t0)
    same = all(np.array_equal(got[f][:m], want[f]) for f in ("key", "n_kept", "n_offmap", "flags"))
    print(json.dumps(dict(case="evaluate", queries=n_q, beams=n_beams, **stats(ms), us_per_query=1e3 * med / n_q,
                          localised_true_half=float((got["badness"][:n_q // 2] < 0.25).mean()),
                          localised_displaced_half=float((got["badness"][n_q // 2:] < 0.25).mean()), numpy_queries=m, numpy_ms=t_model,
                          numpy_scaled_ms=t_model * n_q / m, numpy_scaled_over_device=t_model * n_q / m / med, same_as_numpy=bool(same),
                          version=version)), flush=True)

    # ---- adjust: 20 x 20 x 315
    lat = N.calib_lattice(pose[0, 0], pose[0, 1], pose[0, 2], 0.5, 0.5, 3.14, 0.05, 0.02)
    shape = (len(lat["xs"]), len(lat["ys"]), len(lat["cs"]))
    ares_t = torch.zeros(24, dtype=torch.uint8, device=dev)
    ms = timed(lambda: mon.adjust_device(ranges, 0, 0, lat, ares_t, stream=st, r_min=0.5, r_max=30.0), a.reps, st)
    med = float(np.median(ms))
    win = mon.read(ares_t, N.LOCMON_ADJUST_DTYPE)[0]
    nc = int(np.prod(shape))
    sub = dict(xs=lat["xs"][:1], ys=lat["ys"][:1], cs=lat["cs"][:m], sn=lat["sn"][:m])
    t0 = time.perf_counter()
    M.adjust(fld, origin[:2], PIXEL, MAX_DIST, cb, sb, host_r[0], sub, 0.5, 30.0)
    t_model = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(case="adjust", lattice=list(shape), candidates=nc, beams=n_beams, **stats(ms), us_per_candidate=1e3 * med / nc,
                          winner_index=int(win["index"]), winner_key=int(win["key"]), winner_badness=float(win["badness"]), numpy_candidates=m,
                          numpy_ms=t_model, numpy_scaled_ms=t_model * nc / m, numpy_scaled_over_device=t_model * nc / m / med, version=version)),
          flush=True)

    if a.skip_fuser:
        mon.close()
        return
    # ---- 64 queries in front of the fuser bank's plain update on one stream
    B, n_steps = 64, a.reps + 1
    prm = N.fuser_params(resolution=0.5, map_size_x=100.0, map_size_y=100.0, map_size_z=1.0, sensor_range=30.0, neighbours=2, itr_max=30,
                         delta_score=1e-6, max_cells=4096)
    seeds = torch.arange(9001, 9001 + B, dtype=torch.int64, device=dev)
    poses = np.zeros((n_steps + 1, B, 3))
    for s in range(1, n_steps + 1):
        step = np.stack([gen.uniform(0.15, 0.3, B), gen.uniform(-0.05, 0.05, B), gen.uniform(-0.04, 0.04, B)], axis=1)
        c, sn = np.cos(poses[s - 1, :, 2]), np.sin(poses[s - 1, :, 2])
        poses[s, :, 0] = poses[s - 1, :, 0] + c * step[:, 0] - sn * step[:, 1]
        poses[s, :, 1] = poses[s - 1, :, 1] + sn * step[:, 0] + c * step[:, 1]
        poses[s, :, 2] = poses[s - 1, :, 2] + step[:, 2]
    sp = N.ScanProjector(B, n_beams)
    rr, clouds = [], []
    for s in range(n_steps + 1):
        r, a0, inc = synth.scan_2d_ranges(seeds, torch.as_tensor(poses[s], device=dev), n_beams, noise_stream=s)
        rr.append(r.contiguous())
        clouds.append(torch.empty((B, n_beams, 3), dtype=torch.float32, device=dev))
        sp.project_device(rr[s], clouds[s], a0, inc, stream=st, seed=s)
    Tm = [np.linalg.inv(T2(poses[s])) @ T2(poses[s + 1]) for s in range(n_steps)]
    q64_t, r64_t = q_t[:64 * 40].contiguous(), torch.zeros(64 * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run(evaluate):
        bank = N.FuserBank(prm, B)
        bank.initialize(T2(poses[0]), clouds[0], stream=st)
        ms = []
        for s in range(n_steps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            if evaluate:
                mon.evaluate_device(rr[s + 1], q64_t, r64_t, stream=st, r_min=0.5, r_max=30.0)
            bank.update(Tm[s], clouds[s + 1], stream=st)
            e1.record(st)
            T, _ = bank.poses()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        bank.close()
        return ms[1:], T

    plain, T_plain = run(False)
    withe, T_with = run(True)
    base, med = float(np.median(plain)), float(np.median(withe))
    print(json.dumps(dict(case="fuser update alone", fusers=B, beams=n_beams, **stats(plain), version=version)), flush=True)
    print(json.dumps(dict(case="evaluate + fuser update", fusers=B, beams=n_beams, queries=64, **stats(withe), added_ms=med - base,
                          added_percent=100.0 * (med - base) / base, same_poses=bool(np.array_equal(T_plain, T_with)), version=version)),
          flush=True)
    sp.close()
    mon.close()


if __name__ == "__main__":
    main()
