"""The graphs of the chip-wide optimiser's tests (tests/pgo_wide_graphs.py) checked on the CPU: they sit on the tile's edges, the
model converges on each (a GPU failure is never the generator's fault), and the floors of their tolerances are the measured
ones: the model's dense run against its run with the restated conjugate gradients, as tests/test_pgo_model.py::test_pcg_floor
does for the graphs of pgo_model.model_graphs()."""
import numpy as np
import pytest

import pgo_model as M
import pgo_wide_graphs as WG


@pytest.fixture(scope="module")
def graphs():
    return WG.wide_graphs()


def test_graphs_sit_on_the_tile_edges(graphs):
    assert WG.TILE == 256
    assert [graphs["random_%d" % n].n_nodes for n in (255, 256, 257)] == [255, 256, 257]
    assert [WG.tiles(graphs["random_%d" % n].n_nodes) for n in (255, 256, 257)] == [1, 1, 2]
    assert all(WG.tiles(graphs["random_%d" % n].n_edges) == 2 for n in (255, 256, 257))
    hub = graphs["hub"]
    degree = np.bincount(np.concatenate([hub.ref, hub.mov]), minlength=hub.n_nodes)
    assert (hub.n_nodes, hub.n_edges) == (578, 1586) and degree.max() == degree[hub.n_nodes // 2] > WG.TILE
    assert WG.tiles(hub.n_nodes) == 3 and WG.tiles(hub.n_edges) == 7
    big = M.grid_world()                                   # 5 node tiles and 11 link tiles, the last of each partial
    assert (WG.tiles(big.n_nodes), WG.tiles(big.n_edges)) == (5, 11) and big.n_nodes % WG.TILE and big.n_edges % WG.TILE
    assert set(WG.FLOORS) == set(graphs)
    assert WG.tolerance("grid_world") == (M.TOL, M.COST_RTOL) and WG.tolerance("hub") == (10 * 1.7e-14, 10 * 1.7e-15)


def test_pcg_floor(graphs):
    """every new graph's floor (pgo_wide_graphs.FLOORS) is the measured value, up to the factor 2 that another BLAS' rounding may
    move numbers this close to the last place"""
    for name, G in graphs.items():
        floor, cost_floor, rd, rp = WG.measure_floor(G)
        assert rd["exit_code"] == M.CONVERGED and rd["iterations"] <= 15, (name, rd)
        assert rp["exit_code"] == M.CONVERGED and rp["iterations"] == rd["iterations"] and rp["linear_iterations"] > 0, (name, rp)
        assert rd["cost_final"] < rd["cost_initial"] and rd["cost_final"] > 1e-3, (name, rd)
        print("%s: %d nodes, %d links, %d updates, %d inner iterations, largest pose difference %.3g, cost %.3g relative"
              % (name, G.n_nodes, G.n_edges, rp["iterations"], rp["linear_iterations"], floor, cost_floor))
        want, want_cost = WG.FLOORS[name]
        assert want / 2 <= floor <= 2 * want, (name, floor)
        assert cost_floor <= 2 * want_cost, (name, cost_floor)
