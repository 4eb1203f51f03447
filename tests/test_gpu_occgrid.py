"""The occupancy-grid export on the device (ndtgpu_mapset_occupancy_grid*, csrc/ndt_occgrid.hip) against the NumPy model
(tests/occgrid_model.py) on the cells the maps export: a set of 3 maps on 25 x 20 x 2 cells of 0.5 m (an odd axis; at r = 0.1 an odd
width of 125, three of four row starts unaligned, map 1 starting at byte 12500), built from synthetic scans of 3000 points.

The band (a condition, not a measurement).  The device's exp and quadratic form may differ from NumPy's by a few ulps:
d(100 v) = 25 e^(-l/2) dl, dl <~ 1e3 l 2^-50 for the eigen-floored condition number, at most ~1e-10.  So a pixel is left out where
100 v lies within 1e-8 of an integer, or where its centre lies within 1e-9 m of a cell face; everything else must be equal.  At most
0.1 % of a grid's pixels may be left out by the value band (tests/test_occgrid_model.py asserts it for these inputs on the CPU; here
it is asserted again on the cells the device built, and printed).
The face band cannot stay below 0.1 % at r = 0.1: the centres of rows 2, 7, 12, ... of the even y axis (-5 + 0.25, -5 + 0.75, ...
relative to the map's centre) are cell faces in exact arithmetic -- a fifth of the grid, fixed by the geometry.  Those rows are
therefore compared as well (test_face_rows_agree_too): pixel centre and cell index are the same sequence of correctly rounded fp64
operations on both sides, so nothing may differ there either."""
import numpy as np
import pytest

import occgrid_fixtures as F
import occgrid_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


@pytest.fixture(scope="module")
def built(N):
    """the set of 3 maps, built once; the cells each map exports"""
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=F.N_MAPS)
    assert ms.info()["cells_per_axis"] == list(F.CELLS)
    for m in range(F.N_MAPS):
        ms.set_centre(m, F.CENTRES[m])
    xyz, _ = F.scans()
    ms.build(xyz)
    cells = [ms.export_cells(m)[:3] for m in range(F.N_MAPS)]
    assert all(c[0].shape[0] == F.CELLS_PER_SCAN for c in cells)
    return ms, cells


_models = {}


def model(cells, m, r, **kw):
    key = (m, r, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = M.rasterise(F.RES, F.CELLS, F.CENTRES[m], r, *cells[m], **kw)
    return _models[key]


def compare(got, want, v100, face, what, face_rows_too=True):
    vb, fb = M.bands(v100, face)
    left_out = vb | fb
    n_diff = int(np.count_nonzero((got != want) & ~left_out))
    print("%s: %d pixels, %d with a likelihood, %d in the value band, %d in the face band, %d differ outside both" % (
        what, got.size, np.isfinite(v100).sum(), vb.sum(), fb.sum(), n_diff))
    assert vb.sum() <= 1e-3 * got.size
    assert n_diff == 0
    if face_rows_too:
        assert np.count_nonzero((got != want) & ~vb) == 0
    return vb, fb


@pytest.mark.parametrize("r,shape", [(0.125, (80, 100)), (0.1, (100, 125))])
def test_all_three_maps_in_one_call_equal_the_model(N, built, r, shape):
    ms, cells = built
    grid, info = ms.occupancy_grid(0, 3, r)
    assert grid.shape == (3,) + shape and grid.dtype == np.int8
    for m in range(3):
        want, v100, face = model(cells, m, r)
        vb, fb = compare(grid[m], want, v100, face, "map %d r %.3f" % (m, r), face_rows_too=False)
        if r == 0.125:
            assert fb.sum() == 0
        assert (grid[m] >= 55).sum() > 500 and (grid[m] == -1).sum() > 5000
        assert (info[m]["width"], info[m]["height"], info[m]["resolution"]) == (shape[1], shape[0], r)
        assert info[m]["origin"] == [F.CENTRES[m][0] - 6.25, F.CENTRES[m][1] - 5.0, 0.0]
        assert (info[m]["n_unknown"], info[m]["n_free"], info[m]["n_occupied"]) == ((grid[m] < 0).sum(), (grid[m] == 0).sum(), (grid[m] > 0).sum())


def test_face_rows_agree_too(N, built):
    ms, cells = built
    grid, _ = ms.occupancy_grid(0, 3, 0.1)
    for m in range(3):
        want, v100, face = model(cells, m, 0.1)
        vb, fb = M.bands(v100, face)
        assert fb.sum() == 125 * 20 and fb[2].all() and not fb[3].any()
        assert np.count_nonzero((grid[m] != want) & fb & ~vb) == 0


@pytest.mark.parametrize("r", [0.125, 0.1])
def test_one_at_a_time_and_reordered_give_the_batch_bytes(N, built, r):
    ms, _ = built
    batch, _ = ms.occupancy_grid(0, 3, r)
    for m in (2, 0, 1):
        one, _ = ms.occupancy_grid(m, 1, r)
        assert one.shape[0] == 1 and one[0].tobytes() == batch[m].tobytes()
    pair, _ = ms.occupancy_grid(1, 2, r)
    assert pair.tobytes() == batch[1:3].tobytes()
    again, _ = ms.occupancy_grid(0, 3, r)
    assert again.tobytes() == batch.tobytes()
    empty, info = ms.occupancy_grid(3, 0, r)
    assert empty.shape[0] == 0 and info == []


@pytest.mark.parametrize("r", [0.125, 0.1])
def test_device_form_into_a_tensor_equals_the_host_form(N, built, r):
    import torch
    ms, _ = built
    host, info = ms.occupancy_grid(0, 3, r)
    h, w = host.shape[1:]
    # a tensor whose first byte is not 4-aligned as well: the bytes must not depend on it
    for shift in (0, 1, 2):
        buf = torch.full((3 * h * w + 8,), 7, dtype=torch.int8, device="cuda")
        out, dinfo = ms.occupancy_grid(0, 3, r, out=buf[shift:shift + 3 * h * w])
        torch.cuda.synchronize()
        assert out.shape == (3, h, w) and (dinfo[0]["width"], dinfo[0]["height"]) == (w, h)
        assert out.cpu().numpy().tobytes() == host.tobytes()
        assert (buf[:shift] == 7).all() and (buf[shift + 3 * h * w:] == 7).all()       # nothing written outside the grids


def test_z_outside_the_grid_is_all_unknown(N, built):
    ms, cells = built
    for z in (0.8, -0.8, 1e30):
        grid, _ = ms.occupancy_grid(0, 3, 0.125, z=z)
        assert (grid == -1).all()
    # the other layer of cells (z in [-0.75, -0.25)) is another map
    grid, _ = ms.occupancy_grid(0, 1, 0.125, z=-0.5)
    want, v100, face = model(cells, 0, 0.125, z=-0.5)
    compare(grid[0], want, v100, face, "map 0 z -0.5")
    assert (grid[0] >= 55).sum() == 10 * 16


def test_never_built_map_is_all_unknown(N):
    ms = N.MapSet(F.RES, [0, 0, 0], F.SIZE_M, n_maps=2)
    grid, info = ms.occupancy_grid(0, 2, 0.1)
    assert grid.shape == (2, 100, 125) and (grid == -1).all()
    assert info[1]["n_unknown"] == 12500 and info[1]["n_occupied"] == 0
    ms.enable_occupancy()
    grid, _ = ms.occupancy_grid(0, 2, 0.1)
    assert (grid == -1).all()


def test_occupancy_enabled_set_after_add_cloud(N):
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=1)
    ms.enable_occupancy()
    xyz, chosen = F.scans()
    ms.add_cloud(xyz[0], [[0.1, 0.1, 0.0]])
    # one Gaussian cell of the probed layer loses its Gaussian and stays occupied
    victim = next(c for c in chosen[0] if c[2] == 1)
    lo = np.array([F.cell_lower(victim[a], F.CENTRES[0][a], F.CELLS[a]) for a in range(3)])
    ms.discard_cells(0, (lo + 0.25).astype(np.float32)[None])
    mean, cov, idx, _ = ms.export_cells(0)
    occ = ms.occupancy(0)
    assert occ[tuple(victim)] > 0 and not (idx == victim).all(axis=1).any()
    assert (occ[:, :, 1] < 0).sum() > 20 and mean.shape[0] > 20
    for param in (100, 77):
        grid, info = ms.occupancy_grid(0, 1, 0.125, occupied_no_gaussian=param)
        want, v100, face = M.rasterise(F.RES, F.CELLS, F.CENTRES[0], 0.125, mean, cov, idx, occ=occ, occupied_no_gaussian=param)
        compare(grid[0], want, v100, face, "fused map, parameter %d" % param)
        # the classes, cell by cell (16 pixels each)
        ix = M.cell_index(-6.25 + (np.arange(100) + 0.5) * 0.125, 0.0, F.RES, 25)
        iy = M.cell_index(-5.0 + (np.arange(80) + 0.5) * 0.125, 0.0, F.RES, 20)
        IX, IY = np.meshgrid(ix, iy)
        o = np.where(IY >= 0, occ[IX, np.maximum(IY, 0), 1], 0.0)
        has = np.zeros(F.CELLS, dtype=bool)
        has[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        g = np.where(IY >= 0, has[IX, np.maximum(IY, 0), 1], False)
        assert (grid[0][o < 0] == 0).all() and (o < 0).sum() > 300
        assert (grid[0][(o > 0) & g] >= 55).all() and ((o > 0) & g).sum() > 300
        assert (grid[0][(o > 0) & ~g] == param).all() and ((o > 0) & ~g).sum() >= 16
        assert (grid[0][o == 0] == -1).all()
        assert info[0]["n_free"] == (o < 0).sum()


def test_world_of_two_nodes_against_the_model(N, built):
    ms, cells = built

    def pose(x, y, yaw):
        T = np.eye(4)
        T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        T[:2, 3] = [x, y]
        return T

    for with_occ in (False, True):
        world = N.MapSet(F.RES, [0.5, 0.0, 0.0], F.SIZE_M, n_maps=1)
        if with_occ:
            world.enable_occupancy()
        res = N.assemble_world(world, 0, ms, [[0, 2]], [np.stack([pose(0.3, -0.2, 0.2), pose(-0.4, 0.35, -0.15)])])
        assert res[0]["n_cells"] > 40 and res[0]["overflow"] == 0
        mean, cov, idx, _ = world.export_cells(0)
        occ = world.occupancy(0) if with_occ else None
        for r in (0.125, 0.1):
            grid, _ = world.occupancy_grid(0, 1, r)
            want, v100, face = M.rasterise(F.RES, F.CELLS, [0.5, 0.0, 0.0], r, mean, cov, idx, occ=occ)
            compare(grid[0], want, v100, face, "world r %.3f%s" % (r, " with occupancies" if with_occ else ""))
            assert (grid[0] >= 55).sum() > 400 and (grid[0] == 0).sum() == 0


def test_wall_cell_with_a_tiny_determinant_gets_values(N):
    """A set_cells-installed wall cell, eigenvalues (0.008, 8e-6, 8e-6): det 5e-13, below the matcher's 1e-12 gate.  (Most pixels
    of a wall's own cell lie at 55 + 50 e^(-l/2) with e^(-l/2) < 2e-10, inside the value band by construction: the 0.1 % limit on
    left-out pixels is not what this case is about; what is outside the band is compared.)"""
    ms = N.MapSet(F.RES, [0, 0, 0], F.SIZE_M, n_maps=1)
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    mean = np.array([[1.03, 0.52, 0.01], [-2.0, -1.025, 0.0]])     # (the second wall runs along a row of pixel centres at r = 0.05)
    cov = np.stack([R @ np.diag([0.008, 8e-6, 8e-6]) @ R.T, np.diag([0.008, 8e-6, 8e-6])])
    assert (np.linalg.det(cov) < 1e-12).all() and (np.linalg.det(cov) > 0).all()
    ms.set_cells(0, mean, cov)
    m2, c2, i2, _ = ms.export_cells(0)
    assert m2.shape[0] == 2
    for r in (0.125, 0.05):
        grid, _ = ms.occupancy_grid(0, 1, r)
        want, v100, face = M.rasterise(F.RES, F.CELLS, [0, 0, 0], r, m2, c2, i2)
        vb, fb = M.bands(v100, face)
        assert np.count_nonzero((grid[0] != want) & ~(vb | fb)) == 0
        print("wall cells r %.3f: %d pixels with a likelihood, %d in the value band, %d above 55" % (r, np.isfinite(v100).sum(), vb.sum(), (grid[0] > 55).sum()))
        assert (grid[0] >= 55).sum() == np.isfinite(v100).sum() == 2 * round(0.5 / r) ** 2      # none refused: no -1 inside the cells
        # near the means (within two sigma of the wall's line) the values rise above 55
        w, h, (ox, oy) = M.grid_dims(F.RES, F.CELLS, [0, 0, 0], r)
        for k in range(2):
            jj, ii = np.nonzero(np.isfinite(v100))
            d = np.stack([ox + (ii + 0.5) * r, oy + (jj + 0.5) * r, np.zeros(ii.shape)], axis=1) - m2[k]
            l = np.einsum("na,ab,nb->n", d, np.linalg.inv(c2[k]), d)
            near = l < 4.0
            if r == 0.05 and abs(m2[k, 0] + 2.0) < 1e-9:
                assert near.sum() >= 4
            assert (grid[0][jj[near], ii[near]] > 55).all()
        if r == 0.05:
            assert (grid[0] > 55).sum() >= 6 and grid[0].max() >= 70


def test_live_resources_are_unchanged_by_the_calls(N, built):
    import torch
    ms, _ = built
    ms.occupancy_grid(0, 3, 0.1)                          # (whatever a first call may set up)
    buf = torch.empty(3 * 100 * 125, dtype=torch.int8, device="cuda")
    before = N.binding.live_resources()
    ms.occupancy_grid(0, 3, 0.1)
    ms.occupancy_grid(1, 1, 0.125, z=0.1, occupied_no_gaussian=50)
    ms.occupancy_grid(0, 3, 0.1, out=buf)
    torch.cuda.synchronize()
    with pytest.raises(N.NdtGpuError):
        ms.occupancy_grid(2, 2, 0.1)
    assert N.binding.live_resources() == before


def test_invalid_calls_on_a_real_set(N, built):
    ms, _ = built
    for first, count, r in ((1, 3, 0.1), (4, 0, 0.1), (0, 1, 20.0), (0, 3, 1e-5), (0, 1, float("nan")), (0, 1, 0.0)):
        with pytest.raises(N.NdtGpuError) as e:
            ms.occupancy_grid(first, count, r)
        assert e.value.status == -1, (first, count, r)
    with pytest.raises(N.NdtGpuError) as e:
        ms.occupancy_grid(0, 1, 0.1, occupied_no_gaussian=300)
    assert e.value.status == -1


def test_overflowed_map_is_refused_like_by_the_other_readers(N):
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=1, max_cells=8)
    xyz, _ = F.scans()
    ms.build(xyz[0])
    with pytest.raises(N.NdtGpuError) as e:
        ms.num_cells(0)
    assert e.value.status == -4
    with pytest.raises(N.NdtGpuError) as e:
        ms.occupancy_grid(0, 1, 0.125)
    assert e.value.status == -4
    import torch
    buf = torch.full((80 * 100,), 7, dtype=torch.int8, device="cuda")
    ms.occupancy_grid(0, 1, 0.125, out=buf)               # the asynchronous form cannot report it: the map's grid is unknown
    torch.cuda.synchronize()
    assert (buf == -1).all()
