"""CPU-side checks of the marker export's C-ABI (ndtgpu_marker_*, ndtgpu_mapset_markers*, ndtgpu_mcl_markers*): the header declares it
with its semantics, provenance and deviations, the ctypes signatures and the struct agree with it, every bad argument or parameter is
refused with a message that names it before the handle is read and the device is looked for, the pure host entries agree with
tests/marker_model.py BIT FOR BIT on every fixture cell and pose, and the device entries fail loudly without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import marker_fixtures as MF
import marker_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_marker_params", "ndtgpu_marker_tile", "ndtgpu_marker_check", "ndtgpu_marker_eig3", "ndtgpu_marker_cell",
           "ndtgpu_marker_create", "ndtgpu_marker_destroy", "ndtgpu_mapset_markers_device", "ndtgpu_mapset_markers", "ndtgpu_marker_count",
           "ndtgpu_marker_links_device", "ndtgpu_marker_links", "ndtgpu_mcl_markers_device", "ndtgpu_mcl_markers")


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
        assert fn in binding.EXPORTS and hasattr(N.lib(), fn), fn
    assert sorted(e for e in binding.EXPORTS if "marker" in e) == sorted(ENTRIES)
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("---- marker export"):text.index("ndtgpu_mcl_markers(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Limits" in sec
    for site in ("ndt_rviz.h:1090-1153", "1163-1233", "1277-1297", "ndt_feature_rviz.h:282-313", "ndt_feature2d_fuser.cpp:425-433",
                 "ndt_feature_fuser.cpp:253", "ndt_feature_mcl_node.cpp:287", "markerNDTCells", "markerParticlesNDTMCL3D",
                 "markerNDTFeatureLinks"):
        assert site in sec, site
    for word in ("RECOMPUTED", "cyclic Jacobi", "stable sort", "largest magnitude", "not finite", "min_eval", "column-major", "LINE_LIST",
                 "0.02", "skipOdom", "overflow"):
        assert word in sec, word
    assert "0.13.0" in N.lib().ndtgpu_version().decode()


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    assert L.ndtgpu_marker_tile() == N.MARKER_TILE == 256


def test_struct_layout_and_defaults_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    cls = binding.MarkerParams
    prints = ['printf(" %zu", sizeof(ndtgpu_marker_params));']
    want = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        prints.append('printf(" %%zu", offsetof(ndtgpu_marker_params, %s));' % f)
        want.append(getattr(cls, f).offset)
    prints += ['printf(" %u", NDTGPU_MARKER_NONFINITE);', 'printf(" %u", NDTGPU_MARKER_BAD_INDEX);']
    want += [N.MARKER_NONFINITE, N.MARKER_BAD_INDEX]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' + "\n".join(prints) + "\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[0] == 24 and (M.NONFINITE, M.BAD_INDEX) == (N.MARKER_NONFINITE, N.MARKER_BAD_INDEX)
    p = N.marker_params()
    assert (p.min_eval, p.particle_length, p.skip_negative) == (0.0001, 0.3, 0) == (M.MIN_EVAL, M.PARTICLE_LENGTH, 0)
    assert N.MARKER_SCALE_X == 0.02
    with pytest.raises(TypeError):
        N.marker_params(threshold=1.0)
    with pytest.raises(TypeError):
        N.marker_params(reserved=1)


GOOD = dict(max_maps_per_call=8, max_links=1000, n_maps=8, first=2, count=3, max_cells=1000, n_nodes=40, n_links=300, capacity=5000)


def _check(N, prm=None, **kw):
    a = dict(GOOD)
    a.update(kw)
    return N.lib().ndtgpu_marker_check(a["max_maps_per_call"], a["max_links"], a["n_maps"], a["first"], a["count"], a["max_cells"], a["n_nodes"],
                                       a["n_links"], a["capacity"], None if prm is None else ctypes.byref(prm))


def test_refusals_need_no_device(N):
    L = N.lib()
    assert _check(N) == 0
    assert _check(N, count=0, n_links=0, capacity=0) == 0
    nan, inf = float("nan"), float("inf")
    bad = [(dict(max_maps_per_call=0), None, b"max_maps_per_call"), (dict(max_maps_per_call=(1 << 20) + 1), None, b"max_maps_per_call"),
           (dict(max_links=(1 << 28) + 1), None, b"max_links"), (dict(first=9), None, b"first"), (dict(first=6, count=3), None, b"first"),
           (dict(count=9, n_maps=20, first=0), None, b"more maps than the handle"), (dict(capacity=1 << 32), None, b"capacity"),
           (dict(n_maps=1 << 20, count=1 << 20, first=0, max_maps_per_call=1 << 20, max_cells=1 << 20), None, b"tiles"),
           (dict(n_nodes=1 << 32), None, b"n_nodes"), (dict(n_links=1001), None, b"more links than the handle"),
           (dict(n_links=(1 << 28) + 1, max_links=1 << 28), None, b"n_links"),
           ({}, dict(min_eval=-1e-9), b"min_eval"), ({}, dict(min_eval=nan), b"min_eval"), ({}, dict(min_eval=inf), b"min_eval"),
           ({}, dict(particle_length=nan), b"particle_length"), ({}, dict(particle_length=inf), b"particle_length"),
           ({}, dict(skip_negative=2), b"skip_negative"), ({}, dict(skip_negative=-1), b"skip_negative")]
    for kw, fields, word in bad:
        prm = None if fields is None else N.marker_params(**fields)
        assert _check(N, prm, **kw) == -1, (kw, fields)
        assert word in L.ndtgpu_last_error(), (kw, fields, L.ndtgpu_last_error())
    # the entries themselves: parameters and sizes are refused before a handle, a set or a device is looked at
    h = ctypes.c_void_p(1)
    assert L.ndtgpu_marker_create(0, 0, ctypes.byref(h)) == -1 and h.value is None and b"max_maps_per_call" in L.ndtgpu_last_error()
    assert L.ndtgpu_marker_create(1, 0, None) == -1
    p = N.marker_params(min_eval=-1.0)
    n = ctypes.c_size_t()
    assert L.ndtgpu_mapset_markers_device(None, None, 0, 1, None, ctypes.byref(p), None, None, 0, None) == -1
    assert b"min_eval" in L.ndtgpu_last_error()
    assert L.ndtgpu_mapset_markers_device(None, None, 0, 1, None, None, None, None, 4, None) == -1 and b"null points" in L.ndtgpu_last_error()
    assert L.ndtgpu_mapset_markers_device(None, None, 0, 1, None, None, None, None, 0, None) == -1 and b"null map set" in L.ndtgpu_last_error()
    assert L.ndtgpu_mapset_markers(None, None, 0, 1, None, None, None, None, 0, ctypes.byref(n), None, None) == -1
    assert L.ndtgpu_marker_links_device(None, None, 0, None, None, None, 1, None, None, 0, None) == -1 and b"null ref" in L.ndtgpu_last_error()
    assert L.ndtgpu_marker_links_device(None, None, 0, None, None, None, 0, None, None, 0, None) == -1 and b"null handle" in L.ndtgpu_last_error()
    poses, ref, mov, score = MF.links()
    ref = ref.copy()
    ref[5] = 40
    T = np.ascontiguousarray(np.transpose(poses, (0, 2, 1))).reshape(-1, 16)
    dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    pts = np.zeros((300, 6))
    assert L.ndtgpu_marker_links(None, T.ctypes.data_as(dp), 40, ref.ctypes.data_as(up), mov.ctypes.data_as(up), None, 300, None,
                                 pts.ctypes.data_as(dp), 300, ctypes.byref(n), None) == -1
    assert b"node index" in L.ndtgpu_last_error()
    assert L.ndtgpu_mcl_markers_device(None, 0, 1, None, None, None) == -1 and b"null points_dev" in L.ndtgpu_last_error()
    assert L.ndtgpu_mcl_markers(None, 0, 1, None, pts.ctypes.data_as(dp)) == -1 and b"null handle" in L.ndtgpu_last_error()
    assert L.ndtgpu_marker_count(None, ctypes.byref(n), None, None) == -1
    assert L.ndtgpu_marker_destroy(None) == -1
    assert L.ndtgpu_marker_eig3(None, None, None) == -1
    if N.device_count() == 0:
        h = ctypes.c_void_p(1)
        assert L.ndtgpu_marker_create(4, 100, ctypes.byref(h)) == -3 and h.value is None          # NDTGPU_ERR_NO_DEVICE: no CPU fallback
        with pytest.raises(N.NdtGpuError):
            N.Marker(4, 100)


def _all_cells():
    cells = [MF.designed_cells(m)[:2] for m in range(MF.N_MAPS)] + MF.built_cells()
    return np.concatenate([c[0] for c in cells]), np.concatenate([c[1] for c in cells])


def test_eig3_against_the_model_bit_for_bit(N):
    _, cov = _all_cells()
    cov6 = M.cov6_of(cov)
    ev_m, V_m = M.eig3(cov6)
    L = N.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    ev, V = np.zeros(3), np.zeros(9)
    for k in range(cov6.shape[0]):
        c = np.ascontiguousarray(cov6[k])
        assert L.ndtgpu_marker_eig3(c.ctypes.data_as(dp), ev.ctypes.data_as(dp), V.ctypes.data_as(dp)) == 0
        assert (ev == ev_m[k]).all() and (V.reshape(3, 3) == V_m[k]).all(), k
    e2, V2 = N.marker_eig3(cov[0])
    assert (e2 == ev_m[0]).all() and (V2 == V_m[0]).all()


@pytest.mark.parametrize("pose", [None, MF.POSES_YAW[0], MF.POSES_YAW[1], MF.POSES_YAW[2], MF.POSES_ROLL[0]],
                         ids=["none", "yaw0", "yaw1", "yaw2", "roll"])
def test_cell_against_the_model_bit_for_bit(N, pose):
    mean, cov = _all_cells()
    cov6 = M.cov6_of(cov)
    seg_m, kept_m, ev_m, flags_m = M.cell_segments(mean, cov6, pose)
    assert flags_m == 0
    L = N.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    T = None if pose is None else np.ascontiguousarray(pose.T).reshape(16)
    seg, ev = np.zeros(18), np.zeros(3)
    n, flags = ctypes.c_uint32(), ctypes.c_uint32()
    total = 0
    for k in range(mean.shape[0]):
        m, c = np.ascontiguousarray(mean[k]), np.ascontiguousarray(cov6[k])
        assert L.ndtgpu_marker_cell(m.ctypes.data_as(dp), c.ctypes.data_as(dp), None if T is None else T.ctypes.data_as(dp), None,
                                    seg.ctypes.data_as(dp), ev.ctypes.data_as(dp), ctypes.byref(n), ctypes.byref(flags)) == 0
        want = seg_m[k][kept_m[k]]
        assert n.value == want.shape[0] and flags.value == 0, k
        assert (ev == ev_m[k]).all(), k
        assert (seg.reshape(3, 2, 3)[:n.value] == want).all(), k
        assert (seg.reshape(3, 2, 3)[n.value:] == 0).all()
        total += n.value
    assert total > 2000
    s, e, f = N.marker_cell(mean[0], cov[0], pose)
    assert (s == seg_m[0][kept_m[0]]).all() and (e == ev_m[0]).all() and f == 0


def test_cell_parameters_and_flags(N):
    mean, cov = np.array([0.5, -0.25, 0.125]), np.diag([1e-4, 0.01, 5e-5])
    s, e, f = N.marker_cell(mean, cov)
    assert s.shape[0] == 2 and (e == [5e-5, 1e-4, 0.01]).all() and f == 0
    assert (s[0] == [[0.5, -0.25 - 0.0, 0.125], [0.5, -0.25, 0.125]] + np.array([[-1.0], [1.0]]) * [np.sqrt(1e-4), 0, 0]).all()
    s, _, _ = N.marker_cell(mean, cov, min_eval=0.0)
    assert s.shape[0] == 3
    s, _, _ = N.marker_cell(mean, cov, min_eval=np.nextafter(1e-4, 1.0))
    assert s.shape[0] == 1
    s, e, f = N.marker_cell(mean, np.diag([np.nan, 0.01, 0.02]))
    assert f == N.MARKER_NONFINITE and s.shape[0] == 2
    with pytest.raises(N.NdtGpuError):
        N.marker_cell(mean, cov, min_eval=-1.0)
