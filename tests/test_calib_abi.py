"""CPU-side checks of the extrinsic calibration's C-ABI (ndtgpu_calib_*): the header declares it with its semantics, provenance and
deviations, the ctypes signatures and the structs agree with it, every bad argument or parameter is refused with a message that
names it before the handle is read and the device is looked for, the pure host entries agree with tests/calib_model.py, and the
search entries fail loudly without a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import calib_fixtures as X
import calib_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_calib_params", "ndtgpu_calib_tile", "ndtgpu_calib_lattice", "ndtgpu_calib_pair_motion", "ndtgpu_calib_select_pairs",
           "ndtgpu_calib_check", "ndtgpu_calib_create", "ndtgpu_calib_destroy", "ndtgpu_calib_search_device", "ndtgpu_calib_search")


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
    sec = text[text.index("extrinsic calibration"):text.index("ndtgpu_calib_search(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Limits" in sec
    for site in ("laser2d_extrinsic_calibration.cpp", ":176-204", ":146-152", ":85-122", ":250-353", "automower_laser2d_calib.launch",
                 "cth_laser2d_calib.launch", "coop_laser2d_calib.launch"):
        assert site in sec, site
    for word in ("sensor-frame form", "float kd-tree", "no 1e6 cap", "z offset", "host tables", "empty cloud", "robust yaw", "Ts^-1 D Ts",
                 "lowest linear index", "not pruned", "chunks"):
        assert word in sec, word
    assert "PLACEHOLDER" not in text


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    assert "0.13.0" in L.ndtgpu_version().decode()
    assert L.ndtgpu_calib_tile() == N.CALIB_TILE == 256


def test_struct_layout_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    rf = [f for f, _ in binding.CalibResult._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu", '
                   'sizeof(ndtgpu_calib_params), offsetof(ndtgpu_calib_params, max_dist), sizeof(ndtgpu_calib_result));\n'
                   + "".join('printf(" %%zu", offsetof(ndtgpu_calib_result, %s));\n' % f for f in rf)
                   + 'printf(" %u %u", NDTGPU_CALIB_NO_RESULT, NDTGPU_CALIB_BAD_PAIR);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(binding.CalibParams), binding.CalibParams.max_dist.offset, ctypes.sizeof(binding.CalibResult)]
    want += [getattr(binding.CalibResult, f).offset for f in rf] + [N.CALIB_NO_RESULT, N.CALIB_BAD_PAIR]
    assert got == want
    assert binding.CALIB_RESULT_DTYPE.itemsize == 24 and list(binding.CALIB_RESULT_DTYPE.names) == rf
    assert [binding.CALIB_RESULT_DTYPE.fields[f][1] for f in rf] == [getattr(binding.CalibResult, f).offset for f in rf]
    assert binding.calib_params().max_dist == 0.1
    with pytest.raises(TypeError):
        binding.calib_params(error_th=1.0)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph, dv = ctypes.c_void_p(1), ctypes.c_void_p(8)
    nan, inf = float("nan"), float("inf")
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    tab = dict(xs=np.array([0.1, 0.2, 0.3]), ys=np.array([0.0, 0.1]), cs=np.cos([0.0, 0.1, 0.2, 0.3]), sn=np.sin([0.0, 0.1, 0.2, 0.3]))

    def ptr(a):
        return a.ctypes.data_as(dp)

    def check(n_scans=4, n_points=16, stride=12, mstride=None, n_pairs=2, nx=3, ny=2, nyaw=4, prm=None, **_):
        return L.ndtgpu_calib_check(n_scans, n_points, stride, n_points * stride if mstride is None else mstride, n_pairs, nx, ny, nyaw,
                                    None if prm is None else ctypes.byref(prm))

    def device(n_scans=4, n_points=16, stride=12, mstride=None, n_pairs=2, nx=3, ny=2, nyaw=4, prm=None, t=tab, xyz_p=dv, res_p=dv):
        return L.ndtgpu_calib_search_device(ph, xyz_p, n_scans, n_points, stride, n_points * stride if mstride is None else mstride, dv, dv, dv,
                                            n_pairs, ptr(t["xs"]), nx, ptr(t["ys"]), ny, ptr(t["cs"]), ptr(t["sn"]), nyaw,
                                            None if prm is None else ctypes.byref(prm), res_p, None, None)

    kept = np.ones(4, dtype=np.uint32)
    poses = M.poses4([(0, 0, 0)] * 4)
    pairs = np.array([[0, 1], [1, 2]], dtype=np.uint32)
    res = binding.CalibResult()

    def host(n_scans=4, n_points=16, stride=12, mstride=None, n_pairs=2, nx=3, ny=2, nyaw=4, prm=None, t=tab, xyz_p=dv, res_p=None, pr=pairs):
        return L.ndtgpu_calib_search(ph, xyz_p, n_scans, n_points, stride, n_points * stride if mstride is None else mstride,
                                     kept.ctypes.data_as(u32p), ptr(poses), pr.ctypes.data_as(u32p), n_pairs, ptr(t["xs"]), nx, ptr(t["ys"]), ny,
                                     ptr(t["cs"]), ptr(t["sn"]), nyaw, None if prm is None else ctypes.byref(prm),
                                     ctypes.byref(res) if res_p is None else res_p, None)

    assert check() == 0 and check(n_scans=1 << 20, n_points=1 << 16, n_pairs=1024, nx=1 << 24, ny=1, nyaw=1) == 0
    assert check(stride=16) == 0 and check(stride=32, mstride=16 * 32 + 4) == 0 and check(prm=binding.calib_params(max_dist=5.0)) == 0
    for call in (check, device, host):
        for bad, word in ((dict(n_scans=0), b"n_scans"), (dict(n_scans=(1 << 20) + 1), b"n_scans"), (dict(n_points=0), b"n_points"),
                          (dict(n_points=(1 << 16) + 1), b"n_points"), (dict(stride=8), b"stride_bytes"), (dict(stride=0), b"stride_bytes"),
                          (dict(stride=14), b"stride_bytes"), (dict(mstride=16 * 12 - 4), b"map_stride_bytes"),
                          (dict(mstride=16 * 12 + 2), b"map_stride_bytes"), (dict(stride=16, mstride=16 * 12), b"map_stride_bytes"),
                          (dict(n_pairs=0), b"n_pairs"), (dict(n_pairs=1025), b"n_pairs"), (dict(nx=0), b"nx"), (dict(ny=0), b"ny"),
                          (dict(nyaw=0), b"nyaw"), (dict(nx=(1 << 24) + 1), b"nx"), (dict(nx=1 << 23, ny=2, nyaw=2), b"candidates"),
                          (dict(nx=1 << 13, ny=1 << 13), b"candidates")):
            assert call(**bad) == -1, (call.__name__, bad)
            assert word in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
        for bad in (0.0, -0.1, nan, inf):
            assert call(prm=binding.calib_params(max_dist=bad)) == -1, (call.__name__, bad)
            assert b"max_dist" in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
    for call in (device, host):
        for key, val, word in (("xs", nan, b"xs"), ("ys", inf, b"ys"), ("cs", 0.5, b"cs / sn"), ("sn", nan, b"cs / sn")):
            t = {k: v.copy() for k, v in tab.items()}
            t[key][1] = val
            assert call(t=t) == -1, (call.__name__, key)
            assert word in L.ndtgpu_last_error(), (call.__name__, key, L.ndtgpu_last_error())
        assert call(xyz_p=None) == -1 and b"null" in L.ndtgpu_last_error()
    assert device(res_p=None) == -1 and b"result_dev" in L.ndtgpu_last_error()
    assert host(pr=np.array([[0, 1], [1, 4]], dtype=np.uint32)) == -1 and b"pairs" in L.ndtgpu_last_error()
    h = ctypes.c_void_p()
    for bad, word in (((0, 16, 10), b"max_pairs"), ((1025, 16, 10), b"max_pairs"), ((1, 0, 10), b"max_points"), ((1, (1 << 16) + 1, 10), b"max_points"),
                      ((1, 16, 0), b"max_candidates"), ((1, 16, (1 << 24) + 1), b"max_candidates")):
        assert L.ndtgpu_calib_create(bad[0], bad[1], bad[2], ctypes.byref(h)) == -1 and not h.value, bad
        assert word in L.ndtgpu_last_error(), bad
    assert L.ndtgpu_calib_create(1, 16, 10, None) == -1


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    dv = ctypes.c_void_p(8)
    one = np.array([0.0])
    c1 = np.array([1.0])
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.ndtgpu_calib_search_device(None, dv, 2, 16, 12, 16 * 12, dv, dv, dv, 1, p(one), 1, p(one), 1, p(c1), p(one), 1, None, dv, None, None) == -1
    assert b"null handle" in L.ndtgpu_last_error()
    assert L.ndtgpu_calib_destroy(None) == -1
    L.ndtgpu_default_calib_params(None)                         # (a no-op, as the other default functions)


def test_lattice_against_the_model(N):
    """counts and nodes bit for bit; the cosine and sine tables within one unit in the last place of the model's (two libraries)"""
    for args in (X.LATTICE, (0.0, 0.0, 0.0, 0.05, 0.05, 0.04, 0.01, 0.001), (0.1, -0.2, 0.3, 0.3, 0.35, 0.2, 0.1, 0.07),
                 (1.0, 2.0, -1.0, 0.01, 0.03, 0.5, 0.02, 1.0), (0.0, 0.0, 0.0, 0.05, 0.05, 0.01, 0.001, 0.001)):
        got, want = N.calib_lattice(*args), M.lattice(*args)
        for k in ("xs", "ys", "yaws"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (args, k)
        for k in ("cs", "sn"):
            assert got[k].shape == want[k].shape and (np.abs(got[k] - want[k]) <= np.spacing(np.abs(want[k]))).all(), (args, k)
    assert len(N.calib_lattice(*X.LATTICE)["xs"]) == 11                # the node that rounding adds
    d = N.calib_lattice(0.0, 0.0, 0.0, 0.05, 0.05, 0.01, 0.001, 0.001)            # the launch files' lattice: about 100 x 100 x 20
    assert len(d["xs"]) == len(d["ys"]) and len(d["xs"]) in (100, 101) and len(d["yaws"]) in (20, 21)
    L = N.lib()
    cnt = (ctypes.c_size_t * 3)()
    nan = float("nan")
    for bad, word in (((nan, 0, 0, 1, 1, 1, 0.1, 0.1), b"ix"), ((0, 0, 0, 0, 1, 1, 0.1, 0.1), b"x_s"), ((0, 0, 0, 1, -1, 1, 0.1, 0.1), b"y_s"),
                      ((0, 0, 0, 1, 1, nan, 0.1, 0.1), b"yaw_s"), ((0, 0, 0, 1, 1, 1, 0.0, 0.1), b"t_r"), ((0, 0, 0, 1, 1, 1, 0.1, -0.1), b"yaw_r"),
                      ((0, 0, 0, 1, 1, 1, 1e-9, 0.1), b"2^24")):
        assert L.ndtgpu_calib_lattice(*[float(v) for v in bad], cnt, None, None, None, None, None, 0) == -1, bad
        assert word in L.ndtgpu_last_error(), (bad, L.ndtgpu_last_error())
    buf = np.zeros(5)
    assert L.ndtgpu_calib_lattice(0.0, 0.0, 0.0, 0.5, 0.5, 0.04, 0.01, 0.004, cnt, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None,
                                  None, None, 5) == -4 and list(cnt) == [100, 100, 20]
    assert L.ndtgpu_calib_lattice(0.0, 0.0, 0.0, 0.5, 0.5, 0.04, 0.01, 0.004, None, None, None, None, None, None, 0) == -1


def test_pair_motion_and_select_pairs_against_the_model(N):
    rng = np.random.default_rng(17)
    for _ in range(50):
        p = M.poses4(rng.uniform(-20, 20, size=(2, 3)))
        got, want = N.calib_pair_motion(p[0], p[1]), M.pair_motion(p[0], p[1])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    same = M.poses4([(1.5, -2.0, 0.0)] * 2)
    assert N.calib_pair_motion(same[0], same[1]).tolist() == [0.0, 0.0, 1.0, 0.0]
    deg = math.pi / 180.0
    walk = [(0, 0, 0), (0.1, 0, 10 * deg), (0.2, 0, 24.9 * deg), (0.3, 0, 25.1 * deg), (0.35, 0, 30 * deg), (2.0, 0, 80 * deg),
            (2.1, 0, 100 * deg), (2.2, 0.1, 50 * deg), (2.2, 0.1, 50 * deg), (2.0, 0.3, 76 * deg)]
    assert N.calib_select_pairs(M.poses4(walk)).tolist() == M.select_pairs(M.poses4(walk)).tolist() == [[0, 3], [5, 7], [7, 9]]
    for seed in range(5):
        r = np.random.default_rng(seed)
        steps = np.cumsum(np.stack([r.normal(0, 0.3, 200), r.normal(0, 0.3, 200), r.normal(0, 0.2, 200)], axis=1), axis=0)
        p4 = M.poses4(steps)
        for mt, my in ((1.0, 25 * deg), (0.5, 10 * deg), (3.0, 60 * deg)):
            got, want = N.calib_select_pairs(p4, mt, my), M.select_pairs(p4, mt, my)
            assert got.dtype == np.uint32 and got.tolist() == want.tolist() and len(want) > 0, (seed, mt, my)
    assert N.calib_select_pairs(np.zeros((0, 4))).shape == (0, 2)
    assert X.planted()["pairs"].tolist() == N.calib_select_pairs(X.planted()["poses4"]).tolist()
    L = N.lib()
    m = ctypes.c_size_t()
    p4 = M.poses4(walk)
    ptr = p4.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.ndtgpu_calib_select_pairs(ptr, 10, -1.0, 0.4, None, 0, ctypes.byref(m)) == -1 and b"max_translation" in L.ndtgpu_last_error()
    assert L.ndtgpu_calib_select_pairs(ptr, 10, 1.0, float("nan"), None, 0, ctypes.byref(m)) == -1 and b"min_yaw" in L.ndtgpu_last_error()
    assert L.ndtgpu_calib_select_pairs(None, 10, 1.0, 0.4, None, 0, ctypes.byref(m)) == -1 and b"poses4" in L.ndtgpu_last_error()
    assert L.ndtgpu_calib_select_pairs(ptr, 10, 1.0, 0.4, None, 0, None) == -1
    assert L.ndtgpu_calib_select_pairs(ptr, 10, 1.0, 25 * deg, None, 0, ctypes.byref(m)) == 0 and m.value == 3


def test_calibrator_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        c = N.Calibrator(1, 8, 4)
        lat = M.lattice(0.0, 0.0, 0.0, 0.02, 0.02, 0.02, 0.01, 0.01)
        xyz = np.zeros((3, 8, 3), dtype=np.float32)
        for args in ((xyz, [1, 1, 1], M.poses4([(0, 0, 0)] * 3), [(0, 1), (1, 2)]), (np.zeros((2, 9, 3), dtype=np.float32), [1, 1], M.poses4([(0, 0, 0)] * 2), [(0, 1)]),
                     (xyz, [1, 1, 1], M.poses4([(0, 0, 0)] * 3), [(0, 1)])):
            with pytest.raises(N.NdtGpuError) as e:
                c.search(*args, lat)
            assert e.value.status == -4
        c.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.Calibrator(16, 720, 200000)
    assert e.value.status == -3
    assert binding.Calibrator.search and binding.Calibrator.search_device and binding.Calibrator.close
