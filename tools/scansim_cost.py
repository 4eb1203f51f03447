#!/usr/bin/env python3
"""What scan simulation costs (ndtgpu_scansim_*, include/ndtgpu.h "scan simulation"), in the replay's world (tools/locmon_cost.py: all
node maps of the replay's shape assembled into one map and rasterised at 0.05 m, 13600 x 12000 pixels):
  simulate       1024 poses on free pixels x 1440 beams over the full circle, range_max 30 (R = 600): simulate_device;
  lattice        generateRefScans' lattice of the whole grid at ref_pos_resolution 1 m (skip 20) and 8 headings: lattice_device;
  refscans       the scans of that lattice in the configuration of place_rec_test, 181 beams over +- pi / 2, range_max 10 (R = 200):
                 simulate_device behind the lattice's count, with the cells walked per second (the cells of a sample of --model-poses
                 poses counted by the model, SCALED to all poses: an extrapolation, said so in the record);
  extract        the FLIRT extraction of the first --extract-scans of those scans on the same stream, alone and with their simulation
                 in front.
Each is timed with HIP events around the call, the MEDIAN of --reps (7) intervals after a warm-up, min and max beside it.  Baseline on
the same box: tests/scansim_model.py on one core on --model-poses poses of each case, SCALED to all of them.  One JSON line per case.
usage: python tools/scansim_cost.py [--reps 7] [--nodes 5000]"""
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
import scansim_model as M  # noqa: E402
import world_cost as WC  # noqa: E402
import world_model as W  # noqa: E402
from locmon_cost import stats, timed  # noqa: E402

PIXEL = 0.05


def model_sample(crop, origin, poses, cb, sb, **prm):
    """the model on a few poses in a crop of the grid that holds their reach: (ms a pose, cells walked a pose, ranges)"""
    t0 = time.perf_counter()
    ranges, _ = M.simulate(crop[None], [origin], PIXEL, poses, cb, sb, **prm)
    ms = 1e3 * (time.perf_counter() - t0) / len(poses)
    # the cells a beam walks: the steps up to its hit, or up to where a miss stops (the reach, the rim of the crop is beyond it)
    R = M.reach(prm["range_max"], PIXEL)
    cells = 0
    for p, row in zip(poses, ranges):
        ex, ey = p[2] * cb - p[3] * sb, p[3] * cb + p[2] * sb
        major = np.maximum(np.abs(ex), np.abs(ey))
        cells += float(np.where(row != prm["miss"], row / PIXEL * major, R * major).sum())
    return ms, cells / len(poses), ranges


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--node-points", type=int, default=20000)
    ap.add_argument("--model-poses", type=int, default=4)
    ap.add_argument("--extract-scans", type=int, default=16384)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("scansim_cost: no HIP device (nothing to measure)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    version = N.lib().ndtgpu_version().decode()

    # ---- the replay's world and its grid (as tools/locmon_cost.py)
    pool, T_local, T_world, room = WC.replay_nodes(a.nodes, a.node_points)
    n_rooms = int(room.max()) + 1
    cols, rows = min(n_rooms, 8), (n_rooms + 7) // 8
    centre = [40.0 * (cols - 1), 40.0 * (rows - 1), 0.0]
    size = [80.0 * (cols - 1) + 120.0, 80.0 * (rows - 1) + 120.0, 1.0]
    world = N.MapSet(WC.RES, centre, size, n_maps=1, max_cells=1 << 20)
    N.assemble_world(world, 0, pool, [list(range(a.nodes))], [T_world])
    w, h, origin = N.occupancy_grid_dims(WC.RES, W.grid_cells(WC.RES, size), centre, PIXEL)
    grid_t = torch.empty(h * w, dtype=torch.int8, device=dev)
    g_t, _ = world.occupancy_grid(0, 1, PIXEL, out=grid_t)
    torch.cuda.synchronize()
    pool.close()
    # the assembled world carries no free-space evidence (its pixels are occupied or unknown): where that is so, the unknown pixels are
    # taken as free, which is what a robot that has driven through the rooms would have recorded
    as_free = int((g_t == 0).sum()) == 0
    if as_free:
        g_t = torch.where(g_t < 0, torch.zeros_like(g_t), g_t).contiguous()
    free = int((g_t == 0).sum())
    base = dict(width=w, height=h, free_pixels=free, unknown_taken_as_free=as_free, obstacle_pixels=int((g_t >= 55).sum()), version=version)

    # a crop around the first room for the model and for choosing poses: 2400 x 2400 pixels (120 m), reach 30 m inside its middle
    cw = min(2400, w, h)
    x0, y0 = min(max(int((0.0 - origin[0]) / PIXEL) - cw // 2, 0), w - cw), min(max(int((0.0 - origin[1]) / PIXEL) - cw // 2, 0), h - cw)
    crop = g_t[0, y0:y0 + cw, x0:x0 + cw].cpu().numpy()
    crop_origin = (origin[0] + x0 * PIXEL, origin[1] + y0 * PIXEL)
    gen = np.random.default_rng(5)
    mid = crop[cw // 2 - 400:cw // 2 + 400, cw // 2 - 400:cw // 2 + 400]
    fj, fi = np.nonzero(mid == 0)
    if fj.shape[0] == 0:
        raise SystemExit("scansim_cost: no free pixel around the first room")

    # ---- simulate: 1024 poses x 1440 beams, range_max 30
    n_p, nb = 1024, 1440
    pick = gen.integers(0, fj.shape[0], n_p)
    th = gen.uniform(-math.pi, math.pi, n_p)
    poses = np.stack([crop_origin[0] + (fi[pick] + cw // 2 - 400 + 0.5) * PIXEL, crop_origin[1] + (fj[pick] + cw // 2 - 400 + 0.5) * PIXEL,
                      np.cos(th), np.sin(th)], axis=1)
    a0, inc = -math.pi, 2 * math.pi / nb
    prm = dict(range_max=30.0, miss=31.0)
    sim = N.ScanSimulator(1, nb, n_p)
    sim.set_beams(nb, a0, inc)
    sim.set_grids_device(g_t, PIXEL, [origin[:2]])
    p_t = torch.as_tensor(poses, device=dev).contiguous()
    r_t = torch.zeros((n_p, nb), dtype=torch.float64, device=dev)
    res_t = torch.zeros(8 * n_p, dtype=torch.uint8, device=dev)
    ms = timed(lambda: sim.simulate_device(p_t, r_t, results_t=res_t, stream=st, **prm), a.reps, st)
    med = float(np.median(ms))
    rec = sim.read(res_t, N.SCANSIM_RESULT_DTYPE, n_p)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    m_ms, m_cells, m_ranges = model_sample(crop, crop_origin, poses[:a.model_poses], cb, sb, **prm)
    same = bool(np.array_equal(r_t[:a.model_poses].cpu().numpy().view(np.uint64), m_ranges.view(np.uint64)))
    print(json.dumps(dict(case="simulate", poses=n_p, beams=nb, R=N.scansim_reach(30.0, PIXEL), **stats(ms), us_per_pose=1e3 * med / n_p,
                          hit_fraction=float(rec["n_hits"].sum()) / (n_p * nb), flagged=int((rec["flags"] != 0).sum()),
                          cells_per_pose_sample=m_cells, gcells_per_s_scaled=m_cells * n_p / (med * 1e-3) / 1e9, model_poses=a.model_poses,
                          model_ms_per_pose=m_ms, model_scaled_ms=m_ms * n_p, model_scaled_over_device=m_ms * n_p / med,
                          sample_equals_model=same, **base)), flush=True)
    sim.close()

    # ---- the lattice of the whole grid: skip 20 (1 m), 8 headings
    nb, a0, inc = 181, -math.pi / 2, math.pi / 180
    prm = dict(range_max=10.0, miss=11.0)
    skip = N.scansim_skip(1.0, PIXEL)
    heads = N.scansim_headings(math.pi / 4)
    nyaw = len(heads[0])
    cap = min(1 << 24, ((w + skip - 1) // skip) * ((h + skip - 1) // skip) * nyaw)
    sim = N.ScanSimulator(1, nb, cap)
    sim.set_beams(nb, a0, inc)
    sim.set_grids_device(g_t, PIXEL, [origin[:2]])
    lp_t = torch.zeros((cap, 4), dtype=torch.float64, device=dev)
    cnt_t = torch.zeros(2, dtype=torch.int32, device=dev)
    ms = timed(lambda: sim.lattice_device(skip, heads, cap, lp_t, cnt_t, stream=st), a.reps, st)
    written, passed = (int(v) for v in cnt_t.cpu().numpy().view(np.uint32))
    print(json.dumps(dict(case="lattice", skip=skip, headings=nyaw, nodes=cap, poses_written=written, poses_passed=passed, **stats(ms),
                          mpositions_per_s=cap / nyaw / (float(np.median(ms)) * 1e-3) / 1e6, **base)), flush=True)
    if written == 0:
        raise SystemExit("scansim_cost: the lattice kept no pose")

    # ---- the reference scans of that lattice
    r_t = torch.zeros((written, nb), dtype=torch.float64, device=dev)
    res_t = torch.zeros(8 * written, dtype=torch.uint8, device=dev)
    ms = timed(lambda: sim.simulate_device(lp_t, r_t, n_poses=written, count_t=cnt_t, results_t=res_t, stream=st, **prm), a.reps, st)
    med = float(np.median(ms))
    rec = sim.read(res_t, N.SCANSIM_RESULT_DTYPE, written)
    cb, sb = N.locmon_beam_table(nb, a0, inc)
    lp = lp_t[:written].cpu().numpy()
    inside = np.nonzero((np.abs(lp[:, 0] - (crop_origin[0] + cw * PIXEL / 2)) < 20.0) & (np.abs(lp[:, 1] - (crop_origin[1] + cw * PIXEL / 2)) < 20.0))[0]
    sample = inside[:a.model_poses]
    m_ms, m_cells, m_ranges = model_sample(crop, crop_origin, lp[sample], cb, sb, **prm)
    same = bool(np.array_equal(r_t[torch.as_tensor(sample, device=dev)].cpu().numpy().view(np.uint64), m_ranges.view(np.uint64)))
    print(json.dumps(dict(case="refscans", poses=written, beams=nb, R=N.scansim_reach(10.0, PIXEL), **stats(ms), us_per_pose=1e3 * med / written,
                          hit_fraction=float(rec["n_hits"].sum()) / (written * nb), flagged=int((rec["flags"] != 0).sum()),
                          cells_per_pose_sample=m_cells, gcells_per_s_scaled=m_cells * written / (med * 1e-3) / 1e9, model_poses=len(sample),
                          model_ms_per_pose=m_ms, model_scaled_ms=m_ms * written, model_scaled_over_device=m_ms * written / med,
                          sample_equals_model=same, **base)), flush=True)

    # ---- the extraction of the first scans, alone and behind their simulation
    # (the lattice poses within 20 m of the first room: the first poses of the lattice lie in the empty rim of the world)
    n_e = min(a.extract_scans, len(inside))
    fm = N.FeatureMatcher(n_e, 64)
    sets_t = torch.arange(n_e, dtype=torch.int32, device=dev)
    ex_t = torch.zeros(n_e * N.binding.FEATEXTRACT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lp_e = lp_t[torch.as_tensor(inside[:n_e], device=dev)].contiguous()
    r_e, res_e = torch.zeros((n_e, nb), dtype=torch.float64, device=dev), res_t[:8 * n_e]
    sim.simulate_device(lp_e, r_e, n_poses=n_e, results_t=res_e, stream=st, **prm)
    eprm = dict(r_min=0.02, r_max=10.5)
    ms_alone = timed(lambda: fm.extract_device(sets_t, r_e, a0, inc, ex_t, stream=st, **eprm), a.reps, st)

    def both():
        sim.simulate_device(lp_e, r_e, n_poses=n_e, results_t=res_e, stream=st, **prm)
        fm.extract_device(sets_t, r_e, a0, inc, ex_t, stream=st, **eprm)

    ms_both = timed(both, a.reps, st)
    ms_sim = timed(lambda: sim.simulate_device(lp_e, r_e, n_poses=n_e, results_t=res_e, stream=st, **prm), a.reps, st)
    ex = sim.read(ex_t, N.binding.FEATEXTRACT_RESULT_DTYPE, n_e)
    print(json.dumps(dict(case="extract", scans=n_e, beams=nb, extract_alone=stats(ms_alone), simulate_then_extract=stats(ms_both),
                          simulate_alone=stats(ms_sim), added_ms=float(np.median(ms_both) - np.median(ms_alone)),
                          features_per_scan=float(ex["n_stored"].mean()), **base)), flush=True)
    fm.close()
    sim.close()
    world.close()


if __name__ == "__main__":
    main()
