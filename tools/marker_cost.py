#!/usr/bin/env python3
"""Times the marker export (ndtgpu_mapset_markers*, ndtgpu_marker_links*, ndtgpu_mcl_markers*, csrc/ndt_marker.hip) on an MI355X:
  - the replay's world (tools/world_cost.py: all node maps of the replay's shape assembled into one map, the layout
    tools/occgrid_cost.py uses) as one map,
  - 64 and --nodes (5000) node maps under their graph poses in one call,
  - the links of a graph of --nodes nodes with --links (44 486, the replay's gated edges) links, a third of them odometry links with a
    negative score, with and without skip_negative (the link LIST is synthetic: random pairs of the replay's nodes),
  - a bank of 64 x 5000 particles.
HIP events around the asynchronous call into device tensors, the median of 7 after a warm-up, min .. max.  The bytes written (48 a
segment, + 8 with src) over the time as a share of the 6.29 TB/s copy ceiling.  What binds: the same call with capacity 0 runs every
launch and every Jacobi and stores nothing -- `no_store_ms`; the difference is what the stores cost.
The route without the call -- ndtgpu_mapset_export_cells per map + numpy.linalg.eigh + the stacking loop of ndt_rviz.h in Python -- is
timed on the same box for every cell case, its loop over at most 20 000 cells and SCALED beyond (--skip-baseline leaves it out).  Links
and particles have no eigen-pairs: their baseline is the copy of the poses to the host and NumPy indexing.
usage: python tools/marker_cost.py [--nodes 5000] [--node-points 20000] [--links 44486] [--repeats 7] [--skip-baseline]"""
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
import world_cost as WC  # noqa: E402
import world_model as W  # noqa: E402

COPY_CEILING = 6.29e12      # bytes/s


def timed(call, repeats):
    import torch
    call()                                                 # (the first run warms up)
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def cm16(T):
    import torch
    return torch.tensor(np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4), (0, 2, 1))).reshape(-1, 16), device="cuda")


def baseline(ms, first, count, poses, min_eval=1e-4, loop_cells=20000):
    """export_cells + eigh + the loop of ndt_rviz.h:1127-1153 in Python.  The loop runs over the first loop_cells cells of the call and its
    time is SCALED to all of them (an extrapolation where the call has more) -> (ms, points of the looped cells [n, 2, 3], cells looped)"""
    t0 = time.perf_counter()
    cells = []
    for k in range(count):
        mean, cov, _, _ = ms.export_cells(first + k)
        w, V = np.linalg.eigh(cov) if mean.shape[0] else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
        cells.append((mean, w, V))
    t_eig = time.perf_counter() - t0
    total = sum(c[0].shape[0] for c in cells)
    t0 = time.perf_counter()
    out, done = [], 0
    for k, (mean, w, V) in enumerate(cells):
        R, t = (None, None) if poses is None else (poses[k][:3, :3], poses[k][:3, 3])
        for i in range(min(mean.shape[0], loop_cells - done)):
            for j in range(3):
                if w[i, j] < min_eval:
                    continue
                o = V[i, :, j] * np.sqrt(w[i, j])
                p1, p2 = mean[i] - o, mean[i] + o
                if R is not None:
                    p1, p2 = R @ p1 + t, R @ p2 + t
                out.append((p1, p2))
        done += min(mean.shape[0], loop_cells - done)
        if done >= loop_cells:
            break
    t_loop = (time.perf_counter() - t0) * (total / max(done, 1))
    return 1e3 * (t_eig + t_loop), np.array(out).reshape(-1, 2, 3), done


def cells_case(name, ms, first, count, poses, repeats, with_baseline):
    import torch
    cells = int(sum(ms.num_cells(first + k) for k in range(count)))
    mk = N.Marker(count, 0)
    T = None if poses is None else cm16(poses)
    cap = 3 * cells
    pts = torch.empty((max(cap, 1), 6), dtype=torch.float64, device="cuda")
    src = torch.empty((max(cap, 1), 2), dtype=torch.int32, device="cuda")
    d = timed(lambda: ms.markers_device(mk, first, count, pts, src_t=src, poses_t=T, capacity=cap), repeats)
    n, overflow, flags = mk.count()
    d0 = timed(lambda: ms.markers_device(mk, first, count, pts, src_t=src, poses_t=T, capacity=0), repeats)
    dn = timed(lambda: ms.markers_device(mk, first, count, pts, src_t=None, poses_t=T, capacity=cap), repeats)
    nbytes = 56 * n
    rec = dict(case=name, maps=count, gaussian_cells=cells, max_cells=ms.info()["max_cells"], segments=n,
               overflow=overflow, flags=flags, device_ms_median=d[0], device_ms_min=d[1], device_ms_max=d[2], no_store_ms=d0[0],
               no_src_ms=dn[0], bytes_written=nbytes, write_rate_tb_s=nbytes / (d[0] * 1e-3) / 1e12,
               fraction_of_copy_ceiling=nbytes / (d[0] * 1e-3) / COPY_CEILING, cells_per_us=cells / (d[0] * 1e3))
    if with_baseline:
        t0 = time.perf_counter()
        host_pts, _, info = ms.markers(first, count, poses=poses, marker=mk, capacity=cap)
        rec["host_form_ms"] = 1e3 * (time.perf_counter() - t0)
        bms, bpts, looped = baseline(ms, first, count, poses)
        rec["baseline_ms"] = bms
        rec["baseline_cells_looped"] = looped
        rec["baseline_is_scaled"] = looped < cells
        rec["baseline_over_device"] = bms / d[0]
        rec["baseline_over_host_form"] = bms / rec["host_form_ms"]
        k = bpts.shape[0]
        if 0 < k <= host_pts.shape[0]:
            # (eigh's signs are its own: a segment may come back with its endpoints exchanged; inside a degenerate eigenspace its
            #  directions are its own too: those segments are far from the library's and show here)
            a = np.abs(host_pts[:k] - bpts).max(axis=(1, 2))
            b = np.abs(host_pts[:k] - bpts[:, ::-1]).max(axis=(1, 2))
            rec["median_distance_to_baseline"] = float(np.median(np.minimum(a, b)))
            rec["max_distance_to_baseline"] = float(np.minimum(a, b).max())
    mk.close()
    print(json.dumps(rec), flush=True)


def links_case(poses, n_links, repeats):
    import torch
    rng = np.random.default_rng(1)
    n_nodes = poses.shape[0]
    ref = rng.integers(0, n_nodes, n_links).astype(np.uint32)
    mov = rng.integers(0, n_nodes, n_links).astype(np.uint32)
    score = rng.uniform(0.0, 0.1, n_links)
    score[::3] = -1.0
    T = cm16(poses)
    r, m = torch.tensor(ref.view(np.int32), device="cuda"), torch.tensor(mov.view(np.int32), device="cuda")
    sc = torch.tensor(score, device="cuda")
    out = torch.empty((n_links, 6), dtype=torch.float64, device="cuda")
    mk = N.Marker(1, n_links)
    for skip in (0, 1):
        d = timed(lambda: mk.links_device(T, r, m, out, score_t=sc, skip_negative=skip), repeats)
        n, overflow, flags = mk.count()
        print(json.dumps(dict(case="links", nodes=n_nodes, links=n_links, skip_negative=skip, segments=n, flags=flags, device_ms_median=d[0],
                              device_ms_min=d[1], device_ms_max=d[2], bytes_written=48 * n,
                              fraction_of_copy_ceiling=48 * n / (d[0] * 1e-3) / COPY_CEILING)), flush=True)
    t0 = time.perf_counter()
    keep = score >= 0
    pts = np.stack([poses[ref[keep], :3, 3], poses[mov[keep], :3, 3]], axis=1)
    print(json.dumps(dict(case="links, NumPy on the host", segments=int(pts.shape[0]), ms=1e3 * (time.perf_counter() - t0))), flush=True)
    mk.close()


def particles_case(pool, n_filters, n_particles, repeats):
    import torch
    bank = N.MCL(pool, [0] * n_filters, n_particles, max_scan_cells=1024)
    bank.initialize(np.tile([1.0, 2.0, 0.0, 0.0, 0.0, 0.3], (n_filters, 1)), np.tile([0.5, 0.5, 0.1, 0.03, 0.03, 0.1], (n_filters, 1)))
    out = torch.empty(n_filters * n_particles * 6, dtype=torch.float64, device="cuda")
    d = timed(lambda: bank.particle_markers(out=out), repeats)
    n = n_filters * n_particles
    t0 = time.perf_counter()
    T = bank.particles()[0]
    host = np.stack([T[..., :3, 3], T[..., :3, 0] * 0.3 + T[..., :3, 3]], axis=2)
    bms = 1e3 * (time.perf_counter() - t0)
    got = out.cpu().numpy().reshape(n_filters, n_particles, 2, 3)
    print(json.dumps(dict(case="particles", filters=n_filters, particles=n_particles, segments=n, device_ms_median=d[0], device_ms_min=d[1],
                          device_ms_max=d[2], bytes_read=96 * n, bytes_written=48 * n,
                          fraction_of_copy_ceiling=144 * n / (d[0] * 1e-3) / COPY_CEILING, baseline_ms=bms, baseline_over_device=bms / d[0],
                          max_distance_to_baseline=float(np.abs(got - host).max()))), flush=True)
    bank.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--node-points", type=int, default=20000)
    ap.add_argument("--links", type=int, default=44486)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("marker_cost: no HIP device (nothing to measure)")
    pool, T_local, T_world, room = WC.replay_nodes(a.nodes, a.node_points)
    n_rooms = int(room.max()) + 1
    cols, rows = min(n_rooms, 8), (n_rooms + 7) // 8
    centre = [40.0 * (cols - 1), 40.0 * (rows - 1), 0.0]
    size = [80.0 * (cols - 1) + 120.0, 80.0 * (rows - 1) + 120.0, 1.0]
    world = N.MapSet(WC.RES, centre, size, n_maps=1, max_cells=1 << 20)
    wres, = N.assemble_world(world, 0, pool, [list(range(a.nodes))], [T_world])
    print(json.dumps(dict(case="setup", nodes=a.nodes, world_cells_per_axis=W.grid_cells(WC.RES, size), world_gaussian_cells=wres["n_cells"],
                          version=N.lib().ndtgpu_version().decode())), flush=True)
    base = not a.skip_baseline
    poses = np.asarray(T_world, dtype=np.float64).reshape(-1, 4, 4)
    cells_case("world", world, 0, 1, None, a.repeats, base)
    n64 = min(64, a.nodes)
    cells_case("node maps in one call", pool, 0, n64, poses[:n64], a.repeats, base)
    cells_case("node maps in one call", pool, 0, a.nodes, poses, a.repeats, base)
    links_case(poses, a.links, a.repeats)
    particles_case(pool, 64, 5000, a.repeats)


if __name__ == "__main__":
    main()
