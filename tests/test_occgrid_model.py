"""The NumPy model of the occupancy-grid export (tests/occgrid_model.py) on hand-built cells, one case per value, and the count of
pixels that the comparison band of tests/test_gpu_occgrid.py leaves out of the inputs that test uses."""
import numpy as np
import pytest

import occgrid_fixtures as F
import occgrid_model as M

RES = 0.5
CELLS = (8, 8, 2)
CENTRE = (0.0, 0.0, 0.0)


def one_cell(mean, cov):
    mean = np.asarray(mean, dtype=np.float64).reshape(1, 3)
    idx = np.stack([M.cell_index(mean[:, a], CENTRE[a], RES, CELLS[a]) for a in range(3)], axis=1)
    return mean, np.asarray(cov, dtype=np.float64).reshape(1, 3, 3), idx


def pixel_of(x, y, r):
    w, h, (ox, oy) = M.grid_dims(RES, CELLS, CENTRE, r)
    return int(np.floor((y - oy) / r)), int(np.floor((x - ox) / r))


def test_dims_and_layout():
    w, h, (ox, oy) = M.grid_dims(0.5, (200, 200, 2), (0, 0, 0), 0.05)
    assert (w, h, ox, oy) == (2000, 2000, -50.0, -50.0)
    w, h, (ox, oy) = M.grid_dims(0.5, (25, 20, 2), (1.0, -2.0, 0), 0.1)
    assert (w, h, ox, oy) == (125, 100, 1.0 - 6.25, -2.0 - 5.0)
    grid, v100, face = M.rasterise(0.5, (25, 20, 2), (0, 0, 0), 0.1, np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3), dtype=int))
    assert grid.shape == (100, 125) and (grid == -1).all() and np.isnan(v100).all()


def test_pixel_at_the_mean_is_100_and_far_from_it_55():
    r = 0.125
    # the mean exactly on a pixel centre: origin -2, pixel 17 -> -2 + 17.5 * 0.125 = 0.1875
    mean, cov, idx = one_cell([0.1875, 0.0625, 0.0], np.diag([1e-4, 1e-4, 1e-4]))
    grid, v100, _ = M.rasterise(RES, CELLS, CENTRE, r, mean, cov, idx)
    j, i = pixel_of(0.1875, 0.0625, r)
    assert grid[j, i] == 100 and v100[j, i] == pytest.approx(105.0)
    # two pixels on (0.25 m, 25 sigma) the likelihood is gone: 0.5 + 0.5 * 0.1
    assert grid[j, i - 2] == 55 and grid[j + 1, i] == 55
    assert tuple(idx[0]) == (4, 4, 1)


def test_empty_slot_is_unknown():
    mean, cov, idx = one_cell([0.1, 0.1, 0.0], np.diag([0.02, 0.02, 0.02]))
    grid, _, _ = M.rasterise(RES, CELLS, CENTRE, 0.125, mean, cov, idx)
    ix = M.cell_index(-2 + (np.arange(32) + 0.5) * 0.125, 0.0, RES, 8)
    own = np.outer(ix == 4, ix == 4).T
    assert (grid[~own] == -1).all() and (grid[own] >= 55).all() and own.sum() == 16


def test_free_occupied_and_the_parameter():
    mean, cov, idx = one_cell([0.1, 0.1, 0.0], np.diag([0.02, 0.02, 0.02]))
    occ = np.zeros(CELLS)
    occ[4, 4, 1] = 3.0          # the Gaussian cell
    occ[2, 3, 1] = -1.5         # observed free
    occ[5, 6, 1] = 0.4          # occupied, no Gaussian
    occ[1, 1, 0] = -2.0         # another layer: not probed at z = 0
    grid, v100, _ = M.rasterise(RES, CELLS, CENTRE, 0.25, mean, cov, idx, occ=occ, occupied_no_gaussian=77)
    # 2 x 2 pixels per cell; LazyGrid's cells of an even axis lie half a cell (one pixel) below the pixel lattice: cell (a, b) holds
    # rows 2 b - 1, 2 b and columns 2 a - 1, 2 a
    assert (grid[5:7, 3:5] == 0).all() and (grid[11:13, 9:11] == 77).all() and (grid[7:9, 7:9] >= 55).all()
    assert (grid[1:3, 1:3] == -1).all()
    assert np.count_nonzero(grid != -1) == 12 and np.isfinite(v100).sum() == 4
    # a Gaussian in a cell observed free: free wins; the default parameter is 100
    occ[4, 4, 1] = -0.1
    grid, _, _ = M.rasterise(RES, CELLS, CENTRE, 0.25, mean, cov, idx, occ=occ)
    assert (grid[7:9, 7:9] == 0).all() and (grid[11:13, 9:11] == 100).all()


def test_thin_wall_cell_with_a_tiny_determinant_still_gets_values():
    cov = np.diag([0.008, 8e-6, 8e-6])
    assert np.linalg.det(cov) < 1e-12
    mean, cov, idx = one_cell([0.0, 0.0625, 0.0], cov)
    grid, v100, _ = M.rasterise(RES, CELLS, CENTRE, 0.125, mean, cov, idx)
    j, i = pixel_of(0.0625, 0.0625, 0.125)
    assert grid[j, i] > 55 and grid[j, i - 1] > 55            # on the wall's line
    assert grid[j + 1, i] == 55                               # 0.125 m (44 sigma) off it
    assert (grid[grid != -1] >= 55).all()
    # a covariance that is no covariance gives no value
    _, bad, _ = one_cell([0.0, 0.0625, 0.0], np.diag([0.01, 0.01, -0.01]))
    grid, _, _ = M.rasterise(RES, CELLS, CENTRE, 0.125, mean, bad, idx)
    assert (grid == -1).all()


def test_pixel_centres_on_cell_faces_follow_the_floor():
    """dyadic numbers: res 0.5, r 1.0.  A pixel centre exactly on a cell face belongs to the cell floor(x / res + 0.5) names -- the
    upper one."""
    px = np.array([-1.25, -0.25, 0.25, 1.75])                        # faces of the cells of 8 x 0.5 m around 0
    assert (M.face_distance(px, 0.0, RES) == 0).all()
    assert list(M.cell_index(px, 0.0, RES, 8)) == [int(np.floor(x / RES + 0.5)) + 4 for x in px[:3]] + [-1] == [2, 4, 5, -1]
    # (1.75 is the upper face of the last cell: the last half cell of an even axis belongs to no cell)
    assert M.cell_index(1.8, 0.0, RES, 8) == -1 and M.cell_index(-2.2, 0.0, RES, 8) == 0
    # rasterised at r = 1.0 on an odd axis (7 cells: 3.5 m, origin -1.75): every pixel centre -1.25 + i is a face in x and y
    cells7 = (7, 7, 2)
    w, h, (ox, oy) = M.grid_dims(RES, cells7, CENTRE, 1.0)
    assert (w, h, ox, oy) == (3, 3, -1.75, -1.75)
    px = ox + (np.arange(3) + 0.5) * 1.0
    want = [int(np.floor(x / RES + 0.5) + 3.5) for x in px]
    assert list(px) == [-1.25, -0.25, 0.75] and want == [1, 3, 5] and list(M.cell_index(px, 0.0, RES, 7)) == want
    mean, cov = np.array([[0.9, -0.1, 0.0]]), np.diag([0.02, 0.02, 0.02])[None]
    grid, _, face = M.rasterise(RES, cells7, CENTRE, 1.0, mean, cov, np.array([[5, 3, 1]]))
    assert (face == 0).all()
    jj, ii = np.nonzero(grid != -1)
    assert list(jj) == [1] and list(ii) == [2]                       # cell (5, 3): column 2, row 1
    # ... and the cell below the face is not that pixel's
    grid, _, _ = M.rasterise(RES, cells7, CENTRE, 1.0, mean, cov, np.array([[4, 2, 1]]))
    assert (grid == -1).all()


def test_z_outside_the_grid():
    mean, cov, idx = one_cell([0.1, 0.1, 0.0], np.diag([0.02, 0.02, 0.02]))
    grid, _, _ = M.rasterise(RES, CELLS, CENTRE, 0.125, mean, cov, idx, z=5.0)
    assert (grid == -1).all()


@pytest.mark.parametrize("r", [0.125, 0.1])
def test_the_band_leaves_out_few_pixels_of_the_gpu_tests_inputs(r):
    """The inputs of tests/test_gpu_occgrid.py, cells from the NumPy builder: pixels whose 100 v lies within 1e-8 of an integer,
    and pixels whose centre lies within 1e-9 m of a cell face."""
    xyz, chosen = F.scans()
    for m in range(F.N_MAPS):
        mean, cov, idx = F.build_cells(xyz[m], F.CENTRES[m])
        assert mean.shape[0] == F.CELLS_PER_SCAN
        grid, v100, face = M.rasterise(F.RES, F.CELLS, F.CENTRES[m], r, mean, cov, idx)
        vb, fb = M.bands(v100, face)
        print("map %d r %.3f: %d pixels, %d with a likelihood, %d in the value band, %d in the face band" % (
            m, r, grid.size, np.isfinite(v100).sum(), vb.sum(), fb.sum()))
        assert np.isfinite(v100).sum() > 0.04 * grid.size
        assert vb.sum() < 1e-3 * grid.size
        if r == 0.125:
            assert fb.sum() == 0
        else:
            # r = 0.1 on the even y axis: the centres of rows 2, 7, 12, ... are -5 + 0.25, -5 + 0.75, ...: cell faces in exact
            # arithmetic, whatever the map's centre.  The geometry fixes this fifth of the grid; the GPU test compares these rows too.
            assert fb.sum() == grid.shape[1] * (grid.shape[0] // 5)
            assert not fb[:, :].any(axis=1)[[0, 1, 3, 4]].any() and fb[2].all()
