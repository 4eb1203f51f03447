"""CPU-side checks of the occupancy-grid export's C-ABI (ndtgpu_occgrid_* / ndtgpu_mapset_occupancy_grid*): the header declares it
with its provenance and deviations, the ctypes signatures and structs agree with it, the grid geometry on plain numbers, every
NDTGPU_ERR_INVALID case is refused without a device, ndtgpu_occgrid_move against a NumPy product, and without a device the call
fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_occgrid_params", "ndtgpu_occgrid_dims", "ndtgpu_occgrid_check", "ndtgpu_mapset_occupancy_grid_device",
           "ndtgpu_mapset_occupancy_grid", "ndtgpu_occgrid_move")
I32P = ctypes.POINTER(ctypes.c_int32)
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndtgpu.h")).read(), flags=re.S)


def test_header_declares_the_entries(N):
    from ndt_feature_graph_amd import binding
    code = header_code()
    for fn in ENTRIES:
        assert re.search(r"\b%s\s*\(" % fn, code), fn
        assert fn in binding.EXPORTS
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("occupancy-grid export"):text.index("ndtgpu_occgrid_move(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "OURS" in sec and "from memory" in sec
    for site in ("ndt_feature2d_fuser.cpp:428-433", ":450-454", "ros_utils.h:12-18", "toOccupancyGrid", "moveOccupancyMap",
                 "getIndexForPoint", "lazygrid_index_half", "ndt_conversions.h"):
        assert site in sec, site
    for word in ("pixel count", "inverse covariance", "1e-12", "NDTGPU_ERR_CAPACITY", "occupied_no_gaussian", "builder-run"):
        assert word in sec, word
    for exported in ("occupancy_grid_dims", "occupancy_grid_move", "occgrid_params", "OccGridParams", "OccGridInfo"):
        assert hasattr(N, exported), exported
    assert hasattr(N.MapSet, "occupancy_grid")


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_sizes_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    fields_p = ("z", "occupied_no_gaussian", "reserved_")
    fields_i = ("width", "height", "resolution", "origin", "n_unknown", "n_free", "n_occupied")
    items = ["sizeof(ndtgpu_occgrid_params)", "sizeof(ndtgpu_occgrid_info)"]
    items += ["offsetof(ndtgpu_occgrid_params, %s)" % f for f in fields_p] + ["offsetof(ndtgpu_occgrid_info, %s)" % f for f in fields_i]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%s\\n", %s); return 0;}\n'
                   % (" ".join(["%zu"] * len(items)), ", ".join("(size_t)" + i for i in items)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(binding.OccGridParams), ctypes.sizeof(binding.OccGridInfo)]
    want += [getattr(binding.OccGridParams, f).offset for f in fields_p] + [getattr(binding.OccGridInfo, f).offset for f in fields_i]
    assert got == want


def test_defaults_are_the_documented_ones(N):
    from ndt_feature_graph_amd import binding
    p = binding.occgrid_params()
    assert (p.z, p.occupied_no_gaussian) == (0.0, 100) and list(p.reserved_) == [0] * 5
    assert binding.occgrid_params(z=0.3, occupied_no_gaussian=77).occupied_no_gaussian == 77
    with pytest.raises(TypeError):
        binding.occgrid_params(no_such_field=1)
    N.lib().ndtgpu_default_occgrid_params(None)            # (a null pointer is ignored)


def test_dims_on_plain_numbers(N):
    import occgrid_model as M
    assert N.occupancy_grid_dims(0.5, [200, 200, 2], [0, 0, 0], 0.05) == (2000, 2000, [-50.0, -50.0, 0.0])
    assert N.occupancy_grid_dims(0.5, [25, 20, 2], [0, 0, 0], 0.1) == (125, 100, [-6.25, -5.0, 0.0])         # an odd axis, an odd width
    assert N.occupancy_grid_dims(0.5, [25, 20, 2], [0, 0, 0], 0.125) == (100, 80, [-6.25, -5.0, 0.0])
    assert N.occupancy_grid_dims(0.5, [25, 20, 2], [1.0, -2.5, 7.0], 0.1) == (125, 100, [-5.25, -7.5, 0.0])  # a shifted centre moves the origin
    assert N.occupancy_grid_dims(0.5, [1360, 1200, 2], [0, 0, 0], 0.05)[:2] == (13600, 12000)                # the replay's world: 163 M pixels
    rng = np.random.default_rng(3)
    for _ in range(200):                                   # ... and the model's geometry is the library's, to the bit
        res, r = rng.uniform(0.05, 2.0), rng.uniform(0.01, 0.5)
        cells = [int(x) for x in rng.integers(1, 300, 3)]
        c = rng.uniform(-100, 100, 3)
        w, h, (ox, oy) = M.grid_dims(res, cells, c, r)
        if w == 0 or h == 0:
            continue
        assert N.occupancy_grid_dims(res, cells, c, r) == (w, h, [float(ox), float(oy), 0.0])


def _dims_rc(N, res, cells, r, centre=(0.0, 0.0, 0.0)):
    cpa = (ctypes.c_int32 * 3)(*cells)
    c = (ctypes.c_double * 3)(*centre)
    w, h, o = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_double * 3)()
    return N.lib().ndtgpu_occgrid_dims(res, cpa, c, r, ctypes.byref(w), ctypes.byref(h), o)


def test_every_invalid_case_is_refused_without_a_device(N):
    L = N.lib()
    inf, nan = float("inf"), float("nan")
    assert _dims_rc(N, 0.5, (25, 20, 2), 0.1) == 0
    for r in (0.0, -0.05, inf, nan):
        assert _dims_rc(N, 0.5, (25, 20, 2), r) == -1 and b"occ_resolution" in L.ndtgpu_last_error(), r
    for res in (0.0, -1.0, inf, nan):
        assert _dims_rc(N, res, (25, 20, 2), 0.1) == -1, res
    assert _dims_rc(N, 0.5, (25, 0, 2), 0.1) == -1 and b"empty grid axis" in L.ndtgpu_last_error()
    assert _dims_rc(N, 0.5, (25, 20, 2), 10.5) == -1 and b"width or height 0" in L.ndtgpu_last_error()      # height (int)(10 / 10.5)
    assert _dims_rc(N, 0.5, (25, 20, 2), 12.6) == -1 and b"width or height 0" in L.ndtgpu_last_error()
    assert _dims_rc(N, 0.5, (25, 20, 2), 1e-9) == -1 and b"2^30" in L.ndtgpu_last_error()
    assert L.ndtgpu_occgrid_dims(0.5, None, None, 0.1, None, None, None) == -1
    # what the calls check with the handle's numbers: maps out of range, an empty grid, 2^40 bytes
    assert L.ndtgpu_occgrid_check(3, 0, 3, 125, 100) == 0 and L.ndtgpu_occgrid_check(3, 3, 0, 125, 100) == 0
    assert L.ndtgpu_occgrid_check(3, 1, 3, 125, 100) == -1 and b"out of range" in L.ndtgpu_last_error()
    assert L.ndtgpu_occgrid_check(3, 4, 0, 125, 100) == -1
    assert L.ndtgpu_occgrid_check(3, 0, 2**64 - 1, 125, 100) == -1 and b"out of range" in L.ndtgpu_last_error()
    assert L.ndtgpu_occgrid_check(3, 0, 3, 0, 100) == -1 and b"width or height 0" in L.ndtgpu_last_error()
    assert L.ndtgpu_occgrid_check(1, 0, 1, 2**20, 2**20) == 0
    assert L.ndtgpu_occgrid_check(2, 0, 2, 2**20, 2**20) == -1 and b"2^40" in L.ndtgpu_last_error()
    assert L.ndtgpu_occgrid_check(64, 0, 64, 13600, 12000) == 0
    # the calls themselves: what needs no handle is refused before one is read (placeholder handle: there is no map set without
    # a device) and before the device is looked for
    h = ctypes.c_void_p(1)
    out = np.zeros(16, dtype=np.int8)
    for fn, extra in ((L.ndtgpu_mapset_occupancy_grid_device, (None,)), (L.ndtgpu_mapset_occupancy_grid, (None, None))):
        for r in (0.0, -1.0, inf, nan):
            assert fn(h, 0, 1, r, None, ctypes.c_void_p(out.ctypes.data), *extra) == -1 and b"occ_resolution" in L.ndtgpu_last_error()
        assert fn(h, 0, 1, 0.1, None, None, *extra) == -1 and b"null output" in L.ndtgpu_last_error()
        assert fn(None, 0, 1, 0.1, None, ctypes.c_void_p(out.ctypes.data), *extra) == -1 and b"null map set" in L.ndtgpu_last_error()


def test_move_is_the_4x4_product(N):
    rng = np.random.default_rng(11)
    for _ in range(5):
        T, P = rng.normal(size=(4, 4)), rng.normal(size=(4, 4))
        np.testing.assert_allclose(N.occupancy_grid_move(T, P), T @ P, rtol=0, atol=1e-14 * np.abs(T).sum() * np.abs(P).sum())
    # a planar pose on an origin pose without rotation: the origin's position is moved, the data is not resampled
    a = 0.3
    T = np.array([[np.cos(a), -np.sin(a), 0, 2.0], [np.sin(a), np.cos(a), 0, -1.0], [0, 0, 1, 0], [0, 0, 0, 1]])
    P = np.eye(4)
    P[:3, 3] = [-50.0, -50.0, 0.0]
    np.testing.assert_allclose(N.occupancy_grid_move(T, P)[:3, 3], T[:3, :3] @ P[:3, 3] + T[:3, 3], atol=1e-13)
    # in place
    m = np.ascontiguousarray(P.T).reshape(-1).copy()
    t = np.ascontiguousarray(T.T).reshape(-1)
    N.lib().ndtgpu_occgrid_move(t.ctypes.data_as(DP), m.ctypes.data_as(DP), m.ctypes.data_as(DP))
    np.testing.assert_allclose(m.reshape(4, 4).T, T @ P, atol=1e-13)


def test_the_call_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: the handle-dependent checks run on a real set)
        ms = N.MapSet(0.5, [0, 0, 0], [12.5, 10, 1], n_maps=3)
        for first, count, r in ((1, 3, 0.1), (0, 1, 20.0), (0, 3, 1e-5)):
            with pytest.raises(N.NdtGpuError) as e:
                ms.occupancy_grid(first, count, r)
            assert e.value.status == -1
        return
    L = N.lib()
    with pytest.raises(N.NdtGpuError) as e:
        N.MapSet(0.5, [0, 0, 0], [12.5, 10, 1], n_maps=3)
    assert e.value.status == -3 and "no HIP device" in str(e.value)
