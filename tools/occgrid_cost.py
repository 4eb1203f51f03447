#!/usr/bin/env python3
"""Times the occupancy-grid export (ndtgpu_mapset_occupancy_grid*, csrc/ndt_occgrid.hip) on an MI355X:
  - the replay's world (tools/world_cost.py: all node maps of the replay's shape assembled into one map of 1360 x 1200 x 2 cells of
    0.5 m) at 0.05 m (13600 x 12000 = 163 M pixels) and 0.1 m,
  - 64 node maps (100 x 100 m at 0.5 m) at 0.05 m (2000 x 2000 pixels each) in one call.
Device form: HIP-event time around the asynchronous call into a device tensor, median over repeats after a warm-up.  Host form:
wall time around the synchronous call (kernel + one device-to-host copy into pageable memory + the counts).  The output-write
rate is width * height * count bytes over the device form's time, as a fraction of the 6.29 TB/s copy ceiling.  The route without
the call -- ndtgpu_mapset_export_cells + the NumPy rasteriser of tests/occgrid_model.py -- is timed on the same box at 0.1 m
(--baseline-fine adds 0.05 m: ~20 GB of NumPy temporaries), and its grid compared with the device's.
usage: python tools/occgrid_cost.py [--nodes 5000] [--node-points 20000] [--repeats 5] [--skip-baseline] [--baseline-fine]"""
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
import occgrid_model as M  # noqa: E402
import world_cost as WC  # noqa: E402
import world_model as W  # noqa: E402

COPY_CEILING = 6.29e12      # bytes/s


def device_ms(ms, first, count, r, out, repeats):
    import torch
    ms.occupancy_grid(first, count, r, out=out)           # (the first run warms up)
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ms.occupancy_grid(first, count, r, out=out)
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def host_ms(ms, first, count, r, repeats):
    t, grid, info = [], None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        grid, info = ms.occupancy_grid(first, count, r)
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), grid, info


def case(name, ms, first, count, r, cells, centres, repeats, baseline):
    import torch
    w, h, _ = N.occupancy_grid_dims(ms.res, cells, centres[0], r)
    out = torch.empty(count * h * w, dtype=torch.int8, device="cuda")
    d = device_ms(ms, first, count, r, out, repeats)
    hm, grid, info = host_ms(ms, first, count, r, max(2, repeats // 2))
    assert out.cpu().numpy().tobytes() == grid.tobytes()
    nbytes = count * h * w
    rec = dict(case=name, maps=count, r=r, width=w, height=h, mpixels=nbytes / 1e6, device_ms_median=d[0], device_ms_min=d[1], device_ms_max=d[2],
               host_form_ms=hm, write_rate_tb_s=nbytes / (d[0] * 1e-3) / 1e12, fraction_of_copy_ceiling=nbytes / (d[0] * 1e-3) / COPY_CEILING,
               gaussian_cells=int(sum(ms.num_cells(first + k) for k in range(count))),
               n_occupied=int(sum(i["n_occupied"] for i in info)), n_free=int(sum(i["n_free"] for i in info)),
               n_unknown=int(sum(i["n_unknown"] for i in info)))
    if baseline:
        t0 = time.perf_counter()
        differ = left_out = 0
        for k in range(count):
            mean, cov, idx, _ = ms.export_cells(first + k)
            want, v100, face = M.rasterise(ms.res, cells, centres[k], r, mean, cov, idx)
            vb, fb = M.bands(v100, face)
            left_out += int((vb | fb).sum())
            differ += int(np.count_nonzero((grid[k] != want) & ~(vb | fb)))
        rec["baseline_ms"] = 1e3 * (time.perf_counter() - t0)       # (the comparison included: a few per cent of it)
        rec["baseline_over_host_form"] = rec["baseline_ms"] / hm
        rec["pixels_that_differ_outside_the_band"] = differ
        rec["pixels_in_the_band"] = left_out
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--node-points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--baseline-fine", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("occgrid_cost: no HIP device (nothing to measure)")
    pool, T_local, T_world, room = WC.replay_nodes(a.nodes, a.node_points)
    n_rooms = int(room.max()) + 1
    cols, rows = min(n_rooms, 8), (n_rooms + 7) // 8
    centre = [40.0 * (cols - 1), 40.0 * (rows - 1), 0.0]
    size = [80.0 * (cols - 1) + 120.0, 80.0 * (rows - 1) + 120.0, 1.0]
    world = N.MapSet(WC.RES, centre, size, n_maps=1, max_cells=1 << 20)
    wres, = N.assemble_world(world, 0, pool, [list(range(a.nodes))], [T_world])
    wcells = W.grid_cells(WC.RES, size)
    ncells = W.grid_cells(WC.RES, WC.NODE_SIZE)
    print(json.dumps(dict(case="setup", nodes=a.nodes, world_cells_per_axis=wcells, world_gaussian_cells=wres["n_cells"],
                          node_cells_per_axis=ncells, version=N.lib().ndtgpu_version().decode())), flush=True)
    base = not a.skip_baseline
    case("world", world, 0, 1, 0.1, wcells, [centre], a.repeats, base)
    case("world", world, 0, 1, 0.05, wcells, [centre], a.repeats, base and a.baseline_fine)
    n64 = min(64, a.nodes)
    case("node maps in one call", pool, 0, n64, 0.05, ncells, [[0.0, 0.0, 0.0]] * n64, a.repeats, False)
    case("one node map", pool, 0, 1, 0.05, ncells, [[0.0, 0.0, 0.0]], a.repeats, base)


if __name__ == "__main__":
    main()
