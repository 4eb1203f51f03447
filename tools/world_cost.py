#!/usr/bin/env python3
"""Times ndtgpu_world_assemble (the call is synchronous: host wall time around it, median over repeats) against the only route to
a world map that exists without it -- ndtgpu_mapset_export_cells per node, the NumPy merge of tests/world_model.py
(baseline_merge: float64 pooling on the host) and ndtgpu_mapset_set_cells -- for
  - 64 / 512 / all node maps of the replay's shape (bench.py --config 4: one node every 2 m on a serpentine path, 100 nodes per
    room, rooms 80 m apart, 100 x 100 x 1 m node grids at 0.5 m) into ONE world,
  - 64 worlds of 64 nodes in one call.
The node maps here are plain builds of one scan each (--node-points points), not the replay's fused maps of ten scans: the
assembly's cost depends on the cells of a node map, not on how they were made.
usage: python tools/world_cost.py [--nodes 5000] [--node-points 20000] [--repeats 3] [--skip-baseline]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ndt_feature_graph_amd as N  # noqa: E402
import world_model as W  # noqa: E402

RES, NODE_SIZE, PER_ROOM, CAP = 0.5, [100.0, 100.0, 1.0], 100, 4096


def replay_nodes(n_nodes, node_points):
    """the node maps (one MapSet), their room-relative poses and their world poses (4 x 4)"""
    import torch
    from ndt_feature_graph_amd import synth
    q, room = np.arange(n_nodes) % PER_ROOM, np.arange(n_nodes) // PER_ROOM
    col, row = q // 10, q % 10
    row = np.where(col % 2 == 1, 9 - row, row)
    lx, ly = -9.0 + 2.0 * col, -9.0 + 2.0 * row
    yaw = np.where(col % 2 == 1, -np.pi / 2, np.pi / 2)
    pool = N.MapSet(RES, [0, 0, 0], NODE_SIZE, n_maps=n_nodes, max_cells=CAP)
    dev = torch.device("cuda")
    for k0 in range(0, n_nodes, 500):
        k1 = min(n_nodes, k0 + 500)
        local = np.stack([lx[k0:k1], ly[k0:k1], yaw[k0:k1]], axis=1)
        sc = synth.scan_2d(torch.as_tensor(4000 + room[k0:k1], dtype=torch.int64, device=dev), torch.as_tensor(local, device=dev),
                           node_points, chunk_bytes=2 << 30).contiguous()
        pool.build(sc, first=k0)
        torch.cuda.synchronize()
    T_local = np.stack([W.pose2d(x, y, a) for x, y, a in zip(lx, ly, yaw)])
    T_world = T_local.copy()
    T_world[:, 0, 3] += 80.0 * (room % 8)
    T_world[:, 1, 3] += 80.0 * (room // 8)
    return pool, T_local, T_world, room


def median_ms(f, repeats):
    f()                                            # (the first run warms up)
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def baseline(pool, nodes, poses, dst, dst_map, centre, cells):
    exported = [pool.export_cells(int(k)) for k in nodes]
    mean, cov = W.baseline_merge([(m, c, n) for m, c, _, n in exported], poses, RES, centre, cells)
    dst.set_cells(dst_map, mean, cov)
    return mean.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--node-points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("world_cost: no HIP device (nothing to measure)")
    pool, T_local, T_world, room = replay_nodes(a.nodes, a.node_points)
    n_rooms = int(room.max()) + 1
    cols, rows = min(n_rooms, 8), (n_rooms + 7) // 8
    centre = [40.0 * (cols - 1), 40.0 * (rows - 1), 0.0]
    size = [80.0 * (cols - 1) + 120.0, 80.0 * (rows - 1) + 120.0, 1.0]
    world = N.MapSet(RES, centre, size, n_maps=1, max_cells=1 << 20)
    cells = W.grid_cells(RES, size)
    print(json.dumps(dict(case="setup", nodes=a.nodes, node_points=a.node_points, node_cells_mean=float(pool.num_cells_all().mean()),
                          world_cells_per_axis=cells, version=N.lib().ndtgpu_version().decode())), flush=True)
    for n in sorted({min(64, a.nodes), min(512, a.nodes), a.nodes}):
        nodes = list(range(n))
        res = {}

        def run():
            res["r"], = N.assemble_world(world, 0, pool, [nodes], [T_world[:n]])
        ms = median_ms(run, a.repeats)
        out = dict(case="one world", nodes=n, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2], **res["r"])
        if not a.skip_baseline:
            t0 = time.perf_counter()
            out["baseline_cells"] = baseline(pool, nodes, T_world[:n], world, 0, centre, cells)
            out["baseline_ms"] = 1e3 * (time.perf_counter() - t0)
            out["ratio"] = out["baseline_ms"] / ms[0]
        print(json.dumps(out), flush=True)
    # 64 worlds of 64 nodes: world w is the first 64 nodes of room w (mod the rooms there are), in the room's own frame
    W64, K = 64, min(64, a.nodes)
    rooms = [w % n_rooms for w in range(W64)]
    lists = [[r * PER_ROOM + k for k in range(K) if r * PER_ROOM + k < a.nodes] for r in rooms]
    Ts = [T_local[l] for l in lists]
    room_size = [120.0, 120.0, 1.0]
    many = N.MapSet(RES, [0, 0, 0], room_size, n_maps=W64, max_cells=32768)
    res = {}

    def run_many():
        res["r"] = N.assemble_world(many, 0, pool, lists, Ts)
    ms = median_ms(run_many, a.repeats)
    out = dict(case="64 worlds in one call", nodes_per_world=K, ms_median=ms[0], ms_min=ms[1], ms_max=ms[2],
               n_cells=[min(r["n_cells"] for r in res["r"]), max(r["n_cells"] for r in res["r"])],
               overflow=max(r["overflow"] for r in res["r"]), n_contributions=sum(r["n_contributions"] for r in res["r"]))
    if not a.skip_baseline:
        t0 = time.perf_counter()
        rc = W.grid_cells(RES, room_size)
        for w in range(W64):
            baseline(pool, lists[w], Ts[w], many, w, [0, 0, 0], rc)
        out["baseline_ms"] = 1e3 * (time.perf_counter() - t0)
        out["ratio"] = out["baseline_ms"] / ms[0]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
