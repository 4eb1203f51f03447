"""The graphs of the SE(3) chip-wide optimiser's tests (ndtgpu_pgo3_optimize_wide; tests/test_pgo3_wide_model.py on the CPU,
tests/test_gpu_pgo3_wide.py on the device), built from pgo3_model's generators, and the floor of each graph's tolerance.

The wide form cuts nodes into tiles of 256 and the links -- with the prior behind them, n_edges + 1 items -- likewise, so the
graphs sit on the tile's edges: random graphs of 255, 256 and 257 nodes; a graph of 255 links, whose 256 items fill exactly one
link tile; the same graph with one more loop closure, whose second link tile holds the prior alone; and a hub graph -- one node
with more incident links than a tile holds, all of them summed by one lane.

FLOORS.  pgo3_model.TOL belongs to the graphs of pgo3_model.model_graphs() and does not carry over: a graph's floor is the largest
entrywise difference of the 4x4 poses between the model's dense run and its run with the restated conjugate gradients at the
default eps_linear, and it grows with the graph's extent and with how weakly the prior holds its rotation (the random graphs are
wandering chains that reach 38 to 93 m from the origin).  The values below are what
tests/test_pgo3_wide_model.py::test_pcg_floor measures on the CPU, rounded up in the last digit shown; COST is the relative difference of cost_final between the same two runs.  The GPU tests allow
ten times a graph's floor, the project's margin for the device's other summation order and its sincos / atan2.  No number here
comes from a device."""
import numpy as np

import pgo3_model as M

TILE = 256                                           # NDT_PGO_WIDE_TILE (csrc/ndt_pgo_wide_core.h)

# name -> (pose floor, relative cost floor), measured: 4.71e-13 / 4.60e-15, 7.46e-12 / 6.53e-15, 4.50e-12 / 5.64e-15,
# 3.13e-13 / 2.25e-14, 4.46e-13 / 6.79e-15, 7.11e-15 / 1.02e-15
FLOORS = {"random_255": (4.8e-13, 4.7e-15), "random_256": (7.5e-12, 6.6e-15), "random_257": (4.6e-12, 5.7e-15),
          "links_255": (3.2e-13, 2.3e-14), "links_256": (4.5e-13, 6.8e-15), "hub": (7.2e-15, 1.1e-15)}


def links_255():
    """171 nodes and 170 + 85 = 255 links: with the prior 256 items, exactly one link tile"""
    return M.random_graph(171, 171)


def links_256():
    """links_255 with one more loop closure, 3 -> n - 5: 256 links, 257 items, the second link tile holds the prior alone"""
    G = links_255()
    rng = np.random.default_rng(22)
    a, b = 3, G.n_nodes - 5
    z = np.concatenate([G.meas, M._measure(G.truth, [a], [b], rng, 0.02, 0.01)])
    return M.Graph(G.poses, np.concatenate([G.ref, [a]]), np.concatenate([G.mov, [b]]), z, truth=G.truth)


def hub_graph():
    """grid3d() -- 588 nodes, 1524 links -- whose middle node is linked to every second node as well: 1817 links, the hub has 300,
    more than a tile"""
    G = M.grid3d()
    n = G.n_nodes
    h = n // 2
    others = [i for i in range(0, n, 2) if i != h]
    rng = np.random.default_rng(21)
    z = np.concatenate([G.meas, M._measure(G.truth, [h] * len(others), others, rng, 0.01, 0.005)])
    return M.Graph(G.poses, np.concatenate([G.ref, np.full(len(others), h)]), np.concatenate([G.mov, others]), z, truth=G.truth)


def wide_graphs():
    """the new graphs, by name"""
    return {"random_255": M.random_graph(255, 255), "random_256": M.random_graph(256, 256), "random_257": M.random_graph(257, 257),
            "links_255": links_255(), "links_256": links_256(), "hub": hub_graph()}


def measure_floor(G):
    """(pose floor, relative cost floor, dense result, pcg result) of a graph: the model's dense run against its run with the
    restated conjugate gradients, on the CPU"""
    Td, rd = M.optimize(G)
    Tp, rp = M.optimize(G, solver="pcg")
    return float(np.max(np.abs(Td - Tp))), abs(rd["cost_final"] - rp["cost_final"]) / rd["cost_final"], rd, rp


def tolerance(name):
    """(pose tolerance, relative cost tolerance) of "compare the device with the model" for a graph by name"""
    if name in FLOORS:
        return 10 * FLOORS[name][0], 10 * FLOORS[name][1]
    assert name in ("helix_ring", "grid3d", "doubled", "weighted")           # pgo3_model.model_graphs()
    return M.TOL, M.COST_RTOL


def tiles(n):
    return (n + TILE - 1) // TILE


def link_tiles(n_edges):
    """the link passes run over n_edges + 1 items: the prior is the link behind the last"""
    return tiles(n_edges + 1)
