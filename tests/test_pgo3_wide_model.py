"""The graphs of the SE(3) chip-wide optimiser's tests (tests/pgo3_wide_graphs.py) checked on the CPU: they sit on the tile's
edges -- of the nodes, and of the n_edges + 1 link items, the prior being the link behind the last --, the model converges on each
(a GPU failure is never the generator's fault), and the floors of their tolerances are the measured ones: the model's dense run
against its run with the restated conjugate gradients, as tests/test_pgo3_model.py::test_floor does for the graphs of
pgo3_model.model_graphs()."""
import numpy as np
import pytest

import pgo3_model as M
import pgo3_wide_graphs as WG


@pytest.fixture(scope="module")
def graphs():
    return WG.wide_graphs()


def test_graphs_sit_on_the_tile_edges(graphs):
    assert WG.TILE == 256
    assert [graphs["random_%d" % n].n_nodes for n in (255, 256, 257)] == [255, 256, 257]
    assert [WG.tiles(graphs["random_%d" % n].n_nodes) for n in (255, 256, 257)] == [1, 1, 2]
    assert all(WG.link_tiles(graphs["random_%d" % n].n_edges) == 2 for n in (255, 256, 257))
    a, b = graphs["links_255"], graphs["links_256"]
    assert (a.n_nodes, a.n_edges, b.n_nodes, b.n_edges) == (171, 255, 171, 256)
    assert a.n_edges + 1 == WG.TILE and WG.link_tiles(a.n_edges) == 1      # the links and the prior fill exactly one tile
    assert b.n_edges == WG.TILE and WG.link_tiles(b.n_edges) == 2          # the second tile holds the prior alone
    assert (int(b.ref[-1]), int(b.mov[-1])) == (3, 166) and np.array_equal(b.meas[:-1], a.meas) and np.array_equal(b.poses, a.poses)
    hub = graphs["hub"]
    degree = np.bincount(np.concatenate([hub.ref, hub.mov]), minlength=hub.n_nodes)
    assert (hub.n_nodes, hub.n_edges) == (588, 1817) and degree.max() == degree[hub.n_nodes // 2] == 300 > WG.TILE
    assert WG.tiles(hub.n_nodes) == 3 and WG.link_tiles(hub.n_edges) == 8
    assert WG.link_tiles(0) == 1                                          # a graph without links still has the prior's tile
    big = M.grid3d()                                       # 3 node tiles and 6 link tiles, the last of each partial
    assert (WG.tiles(big.n_nodes), WG.link_tiles(big.n_edges)) == (3, 6) and big.n_nodes % WG.TILE and (big.n_edges + 1) % WG.TILE
    assert set(WG.FLOORS) == set(graphs)
    assert WG.tolerance("grid3d") == (M.TOL, M.COST_RTOL) and WG.tolerance("hub") == (10 * 7.2e-15, 10 * 1.1e-15)


def test_pcg_floor(graphs):
    """every new graph's floor (pgo3_wide_graphs.FLOORS) is the measured value, up to the factor 2 that another BLAS' rounding may
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
