"""CPU-side checks of the laser-scan projection's C-ABI (ndtgpu_scanproj_*): the header declares it with its semantics, provenance,
deviations and citations, the ctypes signatures and the struct agree with it, and every argument and parameter check returns its
error before the handle is read and the device is looked for."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_scanproject_params", "ndtgpu_scanproj_tile", "ndtgpu_scanproj_check", "ndtgpu_scanproj_beam",
           "ndtgpu_scanproj_create", "ndtgpu_scanproj_destroy", "ndtgpu_scanproj_project_device", "ndtgpu_scanproj_project")


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
    sec = text[text.index("laser-scan projection"):text.index("ndtgpu_scanproj_project(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Measured on MI355X" in sec
    for site in ("ndt_feature2d_fuser.cpp:747-765", ":875-888", "publish_graph_message.cpp:1356-1381", ":1523-1535",
                 "ndt_feature_fuser.cpp:325-336", ":378-390", "ndt_feature2d_reg_node.cpp:75-86", "ndt_feature2d_view.cpp:119-129",
                 "gustav_laser_tf.launch:20-23", "publish_graph_message.cpp:1377", "projectLaser", "laser_geometry is not vendored"):
        assert site in sec, site
    for word in ("gate is on r itself", "counter-based", "range_min / range_max", "NaN-padded", "one angle_min / angle_increment",
                 "ranges are doubles", "discard_cells", "cloud.back()", "ndt_hash_uniform", "BEAM index", "1.0f", "left untouched"):
        assert word in sec, word
    assert "PLACEHOLDER" not in text and "not measured yet" not in sec


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    assert "0.10.0" not in L.ndtgpu_version().decode()              # bumped with the new entries
    assert L.ndtgpu_scanproj_tile() == N.SCANPROJECT_TILE == 1024


def test_struct_layout_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    pf = [f for f, _ in binding.ScanProjectParams._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu", '
                   'sizeof(ndtgpu_scanproject_params));\n'
                   + "".join('printf(" %%zu", offsetof(ndtgpu_scanproject_params, %s));\n' % f for f in pf) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.ScanProjectParams)] + [getattr(binding.ScanProjectParams, f).offset for f in pf]
    assert pf == ["r_min", "r_max", "varz", "seed"]
    p = binding.scanproject_params()
    assert (p.r_min, p.r_max, p.varz, p.seed) == (0.5, 30.0, 0.02, 0)
    with pytest.raises(TypeError):
        binding.scanproject_params(range_max=1.0)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph = ctypes.c_void_p(1)
    dv = ctypes.c_void_p(8)
    nan, inf = float("nan"), float("inf")

    def check(n_scans=4, n_beams=16, a0=0.0, inc=0.1, stride=12, mstride=None, prm=None):
        return L.ndtgpu_scanproj_check(n_scans, n_beams, a0, inc, stride, n_beams * stride if mstride is None else mstride,
                                       None if prm is None else ctypes.byref(prm))

    def device(n_scans=4, n_beams=16, a0=0.0, inc=0.1, stride=12, mstride=None, prm=None, rr_p=dv, xyz_p=dv):
        return L.ndtgpu_scanproj_project_device(ph, rr_p, None, n_scans, n_beams, a0, inc, None if prm is None else ctypes.byref(prm), xyz_p,
                                                stride, n_beams * stride if mstride is None else mstride, None, None)

    def host(n_scans=4, n_beams=16, a0=0.0, inc=0.1, stride=12, mstride=None, prm=None, rr_p=dv, xyz_p=dv):
        return L.ndtgpu_scanproj_project(ph, ctypes.cast(rr_p, ctypes.POINTER(ctypes.c_double)), None, n_scans, n_beams, a0, inc,
                                         None if prm is None else ctypes.byref(prm), xyz_p, stride, n_beams * stride if mstride is None else mstride,
                                         None)

    assert check() == 0 and check(n_scans=0) == 0 and check(n_beams=1 << 20, n_scans=1 << 24) == 0
    assert check(stride=16) == 0 and check(stride=32, mstride=16 * 32 + 4) == 0
    assert check(prm=binding.scanproject_params(r_min=0.0, r_max=inf, varz=0.0)) == 0
    for call in (check, device, host):
        for bad, word in ((dict(n_beams=0), b"n_beams"), (dict(n_beams=(1 << 20) + 1), b"n_beams"), (dict(n_scans=(1 << 24) + 1), b"n_scans"),
                          (dict(a0=nan), b"angle_min"), (dict(a0=-inf), b"angle_min"), (dict(inc=inf), b"angle_increment"),
                          (dict(inc=nan), b"angle_increment"), (dict(stride=8), b"stride_bytes"), (dict(stride=0), b"stride_bytes"),
                          (dict(stride=14), b"stride_bytes"), (dict(stride=13), b"stride_bytes"),
                          (dict(mstride=16 * 12 - 4), b"map_stride_bytes"), (dict(mstride=16 * 12 + 2), b"map_stride_bytes"),
                          (dict(stride=16, mstride=16 * 12), b"map_stride_bytes"), (dict(mstride=0), b"map_stride_bytes")):
            assert call(**bad) == -1, (call.__name__, bad)
            assert word in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
        for bad, word in ((dict(r_min=-0.1), b"r_min"), (dict(r_min=nan), b"r_min"), (dict(r_min=inf), b"r_min"), (dict(r_max=0.5), b"r_max"),
                          (dict(r_max=0.4), b"r_max"), (dict(r_max=nan), b"r_max"), (dict(r_max=-inf), b"r_max"), (dict(varz=-1e-9), b"varz"),
                          (dict(varz=nan), b"varz"), (dict(varz=inf), b"varz")):
            assert call(prm=binding.scanproject_params(**bad)) == -1, (call.__name__, bad)
            assert word in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
    assert device(rr_p=None) == -1 and device(xyz_p=None) == -1 and host(rr_p=None) == -1 and host(xyz_p=None) == -1
    h = ctypes.c_void_p()
    for bad in ((0, 16), (1, 0), ((1 << 24) + 1, 16), (1, (1 << 20) + 1)):
        assert L.ndtgpu_scanproj_create(bad[0], bad[1], ctypes.byref(h)) == -1 and not h.value, bad
    assert L.ndtgpu_scanproj_create(1, 16, None) == -1


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    dv = ctypes.c_void_p(8)
    assert L.ndtgpu_scanproj_project_device(None, dv, None, 1, 16, 0.0, 0.1, None, dv, 12, 16 * 12, None, None) == -1
    assert b"null handle" in L.ndtgpu_last_error()
    assert L.ndtgpu_scanproj_project_device(None, None, None, 0, 16, 0.0, 0.1, None, None, 12, 16 * 12, None, None) == -1
    assert L.ndtgpu_scanproj_project(None, ctypes.cast(dv, ctypes.POINTER(ctypes.c_double)), None, 1, 16, 0.0, 0.1, None, dv, 12, 16 * 12, None) == -1
    assert b"null handle" in L.ndtgpu_last_error()
    assert L.ndtgpu_scanproj_project(None, None, None, 0, 16, 0.0, 0.1, None, None, 12, 16 * 12, None) == -1
    assert L.ndtgpu_scanproj_destroy(None) == -1
    L.ndtgpu_default_scanproject_params(None)                   # (a no-op, as the other default functions)
    assert L.ndtgpu_scanproj_beam(None, 0.0, 0.1, 0, 3, 2.0, None) == 1 and L.ndtgpu_scanproj_beam(None, 0.0, 0.1, 0, 3, 0.2, None) == 0


def test_projector_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        sp = N.ScanProjector(2, 64)
        import numpy as np
        with pytest.raises(N.NdtGpuError) as e:
            sp.project(np.ones((3, 16)), 0.0, 0.1)
        assert e.value.status == -4
        with pytest.raises(N.NdtGpuError) as e:
            sp.project(np.ones((1, 65)), 0.0, 0.1)
        assert e.value.status == -4
        sp.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.ScanProjector(4, 1440)
    assert e.value.status == -3
    assert binding.ScanProjector.project and binding.ScanProjector.project_device and binding.ScanProjector.close
