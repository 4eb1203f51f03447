"""The graphs of the chip-wide optimiser's tests (ndtgpu_pgo_optimize_wide; tests/test_pgo_wide_model.py on the CPU,
tests/test_gpu_pgo_wide.py on the device), built from pgo_model's generators, and the floor of each graph's tolerance.

The wide form cuts links and nodes into tiles of 256, so the graphs sit on the tile's edges: random graphs of 255, 256 and 257
nodes, and a hub graph -- one node with more incident links than a tile holds, all of them summed by one lane.

FLOORS.  pgo_model.TOL belongs to the three graphs of pgo_model.model_graphs() and does not carry over: a graph's floor is the
largest pose difference (m or rad) between the model's dense run and its run with the restated conjugate gradients at the
default eps_linear, and it grows with the graph's extent and with how weakly the prior holds its rotation (the random graphs are
wandering chains 45 to 72 m long).  The values below are what tests/test_pgo_wide_model.py::test_pcg_floor measures on the CPU,
rounded up in the last digit shown; COST is the relative difference of cost_final between the same two runs.  The GPU tests allow
ten times a graph's floor, the project's margin for the device's other summation order.  No number here comes from a device."""
import numpy as np

import pgo_model as M

TILE = 256                                           # NDT_PGO_WIDE_TILE (csrc/ndt_pgo_wide.h)

# name -> (pose floor, relative cost floor), measured: 6.39e-14 / 5.74e-15, 1.42e-14 / 7.04e-15, 2.13e-13 / 7.61e-15,
# 1.62e-14 / 1.67e-15, 3.55e-15 / 9.73e-15
FLOORS = {"random_255": (6.4e-14, 5.8e-15), "random_256": (1.43e-14, 7.1e-15), "random_257": (2.2e-13, 7.7e-15),
          "hub": (1.7e-14, 1.7e-15), "weighted_40": (3.6e-15, 9.8e-15)}


def hub_graph():
    """grid_world(17, 34) -- 578 nodes -- whose middle node is linked to every second node as well: 1586 links, the hub has 293,
    more than a tile"""
    G = M.grid_world(17, 34)
    n = G.n_nodes
    h = n // 2
    others = [i for i in range(0, n, 2) if i != h]
    rng = np.random.default_rng(21)
    z = np.vstack([G.meas, M._measure(G.truth, [h] * len(others), others, rng, 0.01, 0.005)])
    return M.Graph(G.poses, np.concatenate([G.ref, np.full(len(others), h)]), np.concatenate([G.mov, others]), z, truth=G.truth)


def wide_graphs():
    """the new graphs, by name"""
    return {"random_255": M.random_graph(255, 255), "random_256": M.random_graph(256, 256), "random_257": M.random_graph(257, 257),
            "hub": hub_graph(), "weighted_40": M.random_graph(40, 7, per_link_info=True)}


def measure_floor(G):
    """(pose floor, relative cost floor, dense result, pcg result) of a graph: the model's dense run against its run with the
    restated conjugate gradients, on the CPU"""
    pd, rd = M.optimize(G)
    pp, rp = M.optimize(G, solver="pcg")
    d = pd - pp
    d[:, 2] = M.wrap(d[:, 2])
    return float(np.max(np.abs(d))), abs(rd["cost_final"] - rp["cost_final"]) / rd["cost_final"], rd, rp


def tolerance(name):
    """(pose tolerance, relative cost tolerance) of "compare the device with the model" for a graph by name"""
    if name in FLOORS:
        return 10 * FLOORS[name][0], 10 * FLOORS[name][1]
    assert name in ("ring_inconsistent", "ring_wrap", "grid_world")          # pgo_model.model_graphs()
    return M.TOL, M.COST_RTOL


def tiles(n):
    return (n + TILE - 1) // TILE
