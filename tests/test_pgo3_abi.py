"""CPU-side checks of the SE(3) pose-graph optimiser's C-ABI (ndtgpu_pgo3_*): the three pure host entries -- the code the kernel
runs, compiled for the host -- against the NumPy model (tests/pgo3_model.py), the header's section, the ctypes signatures and
structs, a graph's arguments checked before the handle is read and the device is looked for, and without a device a loud failure
(no CPU fallback).

Tolerances: the conversion of a registered link is compared bit for bit (it is +, -, *, / and sqrt without contraction on both
sides).  The error, its Jacobians and the retraction go through sin / cos / atan2 and some 50 roundings of numbers <= 10 (|t| <= 10,
residual angle <= 2.5 rad): 1e-12 absolute."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pgo3_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_pgo3_params", "ndtgpu_pgo3_create", "ndtgpu_pgo3_destroy", "ndtgpu_pgo3_set_graph",
           "ndtgpu_pgo3_set_links_device", "ndtgpu_pgo3_optimize", "ndtgpu_pgo3_poses", "ndtgpu_pgo3_link_error", "ndtgpu_pgo3_retract",
           "ndtgpu_pgo3_link_from_registration")


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
    L = N.lib()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        assert fn in binding.EXPORTS
        assert len(getattr(L, fn).argtypes) == len([a for a in args.split(",") if a.strip() and a.strip() != "void"]), fn
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("SE(3) pose-graph optimisation"):text.index("ndtgpu_pgo3_link_from_registration(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "FIRST ORDER" in sec
    for site in ("ndt_feature_graph.cpp:296-330", "ndt_feature_link.h:27", "ndt_feature_graph_opt.cpp:147", "ndt_matcher_d2d_fusion.h:1035-1042",
                 "ndt_feature_graph.cpp:300-310", "ndt_offline_mapper.h:45"):
        assert site in sec, site
    assert re.search(r"NDTGPU_PGO3_HALF_TURN\s*=\s*4\b", code) and binding.PGO3_HALF_TURN == 4 == M.HALF_TURN
    assert b"0.13.0" in L.ndtgpu_version()


def test_struct_size_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu\\n",'
                   ' sizeof(ndtgpu_pgo3_params), offsetof(ndtgpu_pgo3_params, prior_information)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.Pgo3Params), binding.Pgo3Params.prior_information.offset]


def test_defaults_are_the_documented_ones(N):
    from ndt_feature_graph_amd import binding
    p, p2 = binding.pgo3_params(), binding.pgo_params()
    assert (p.max_iterations, p.max_linear_iterations, p.eps_step, p.eps_linear) == (50, 2000, 1e-8, 1e-8)
    assert (p.max_iterations, p.max_linear_iterations, p.eps_step, p.eps_linear) == (p2.max_iterations, p2.max_linear_iterations, p2.eps_step, p2.eps_linear)
    assert np.array_equal(np.array(p.prior_information).reshape(6, 6), 100.0 * np.eye(6))
    assert M.DEFAULTS == dict(max_iterations=50, max_linear_iterations=2000, eps_step=1e-8, eps_linear=1e-8)
    with pytest.raises(TypeError):
        binding.pgo3_params(no_such_field=1)


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 0.3, 2.5])
def test_link_error_and_jacobians_against_the_model(N, angle):
    rng = np.random.default_rng(21)
    worst = 0.0
    for _ in range(25):
        Ti, Tj, Z = M.residual_fixture(rng, angle)
        e, Jr, Jm = N.pgo3_link_error(Ti, Tj, Z)
        em, half, Jrm, Jmm = M.link_error(Ti, Tj, Z, jacobians=True)
        assert not half
        worst = max(worst, float(np.max(np.abs(e - em))), float(np.max(np.abs(Jr - Jrm))), float(np.max(np.abs(Jm - Jmm))))
    print("residual rotation %g rad: library against model, error and Jacobians: %.3g (allowed 1e-12)" % (angle, worst))
    assert worst <= 1e-12


def test_link_error_reports_a_half_turn(N):
    Ti, Tj = M.euler_T(1, 2, 3, 0.1, 0.2, 0.3), M.euler_T(-1, 0.5, 2, -0.3, 0.1, 1.0)
    Z = M.inv_T(M.make_T(np.diag([-1.0, 1.0, -1.0]), [0.0, 0.2, 0.0])) @ (M.inv_T(Ti) @ Tj)
    assert M.link_error(Ti, Tj, Z)[1]
    with pytest.raises(N.NdtGpuError) as err:
        N.pgo3_link_error(Ti, Tj, Z)
    assert err.value.status == -1 and "half turn" in str(err.value)


def test_retract_against_the_model(N):
    rng = np.random.default_rng(22)
    worst = 0.0
    for scale in (0.0, 1e-10, 1e-5, 1e-3, 0.5, 2.5):
        for _ in range(10):
            T = M.residual_fixture(rng, 1.0)[0]
            d = np.concatenate([rng.uniform(-1, 1, size=3), rng.normal(size=3) * scale])
            worst = max(worst, float(np.max(np.abs(N.pgo3_retract(T, d) - M.retract(T, d)))))
    print("retract, library against model: %.3g (allowed 1e-12)" % worst)
    assert worst <= 1e-12
    T = M.residual_fixture(rng, 1.0)[0]
    assert np.array_equal(N.pgo3_retract(T, np.zeros(6)), T)


def test_link_from_registration_bit_for_bit(N):
    rng = np.random.default_rng(23)
    T = M.residual_fixture(rng, 1.0)[0]

    def same(cov, flags):
        Z, W = N.pgo3_link_from_registration(T, cov, flags)
        Zm, Wm = M.link_from_registration(T, cov, flags)
        assert np.array_equal(Z, T) and np.array_equal(Zm, T)
        assert W.tobytes() == np.ascontiguousarray(Wm).tobytes(), (cov, flags, np.max(np.abs(W - Wm)))
        return W

    for k in range(40):                                  # covariances of the registrar's kind: SPD, badly scaled, not quite symmetric
        A = rng.normal(size=(6, 6)) * np.array([1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3])[:, None]
        cov = A @ A.T + 1e-7 * np.eye(6) + 1e-9 * rng.normal(size=(6, 6))
        W = same(cov, 0)
        assert np.max(np.abs(W @ (0.5 * (cov + cov.T)) - np.eye(6))) < 1e-6 and np.array_equal(W, W.T)
    assert np.array_equal(same(None, 0), 100.0 * np.eye(6))
    cov = np.diag([1e-4, 2e-4, 3e-4, 1e-5, 2e-5, 3e-5])
    for flags in (M.COV_SINGULAR, M.COV_POSE_UNCHANGED, M.COV_NOT_COMPUTED, 7):
        assert np.array_equal(same(cov, flags), 50.0 * np.eye(6))
    assert not np.array_equal(same(cov, 8), 50.0 * np.eye(6))                    # (another bit is not a reason)
    # the fallback where the matrix does not invert: zero, indefinite, a 3-DoF registration's (rows / columns z, rx, ry empty), NaN,
    # and an inverse that overflows
    planar = np.zeros((6, 6))
    planar[np.ix_([0, 1, 5], [0, 1, 5])] = np.diag([1e-4, 1e-4, 1e-5])
    nan = cov.copy()
    nan[2, 3] = np.nan
    for bad in (np.zeros((6, 6)), np.diag([1, 1, -1, 1, 1, 1.0]), planar, nan, 1e-320 * np.eye(6)):
        assert np.array_equal(same(bad, 0), 50.0 * np.eye(6))


def _set_graph(N, h, n_nodes, ref, mov, poses=True, meas=True):
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    ps = np.tile(np.eye(4).reshape(16), (max(n_nodes, 1), 1))
    ri, mi = np.asarray(ref, dtype=np.uint32), np.asarray(mov, dtype=np.uint32)
    z = np.tile(np.eye(4).reshape(16), (max(len(ri), 1), 1))
    return N.lib().ndtgpu_pgo3_set_graph(h, 0, n_nodes, ps.ctypes.data_as(dp) if poses else None, len(ri), ri.ctypes.data_as(u32p),
                                         mi.ctypes.data_as(u32p), z.ctypes.data_as(dp) if meas else None, None)


def test_bad_graphs_are_refused_before_the_device_is_looked_for(N):
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    h = ctypes.c_void_p(1)
    L = N.lib()
    assert _set_graph(N, h, 3, [0, 1], [1, 3]) == -1 and b"out of range" in L.ndtgpu_last_error()
    assert _set_graph(N, h, 3, [3, 1], [1, 2]) == -1 and b"out of range" in L.ndtgpu_last_error()
    assert _set_graph(N, h, 3, [0, 1, 2], [1, 2, 2]) == -1 and b"to itself" in L.ndtgpu_last_error()
    assert _set_graph(N, h, 4, [0, 2], [1, 3]) == -1 and b"not connected" in L.ndtgpu_last_error()      # {0, 1} and {2, 3}
    assert _set_graph(N, h, 3, [0], [1]) == -1 and b"not connected" in L.ndtgpu_last_error()            # node 2 has no link
    assert _set_graph(N, h, 0, [], []) == -1
    assert _set_graph(N, h, 2, [0], [1], poses=False) == -1
    assert _set_graph(N, h, 2, [0], [1], meas=False) == -1
    # the device form of the links makes the same checks
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    ps = np.tile(np.eye(4).reshape(16), (4, 1))
    ri, mi = np.array([0, 2], dtype=np.uint32), np.array([1, 3], dtype=np.uint32)
    rc = L.ndtgpu_pgo3_set_links_device(h, 0, 4, ps.ctypes.data_as(dp), 2, ri.ctypes.data_as(u32p), mi.ctypes.data_as(u32p),
                                        ctypes.c_void_p(8), None, None)
    assert rc == -1 and b"not connected" in L.ndtgpu_last_error()


def test_entries_refuse_null_arguments_and_bad_sizes(N):
    L = N.lib()
    assert L.ndtgpu_pgo3_destroy(None) == -1
    assert _set_graph(N, None, 2, [0], [1]) == -1
    assert L.ndtgpu_pgo3_optimize(None, 0, 1, None, None) == -1
    assert L.ndtgpu_pgo3_poses(None, 0, None, None) == -1
    assert L.ndtgpu_pgo3_link_error(None, None, None, None, None, None) == -1
    assert L.ndtgpu_pgo3_retract(None, None, None) == -1
    assert L.ndtgpu_pgo3_link_from_registration(None, None, 0, None, None) == -1
    h = ctypes.c_void_p()
    assert L.ndtgpu_pgo3_create(0, 10, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo3_create(1, 0, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo3_create(1, (1 << 24) + 1, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo3_create(1, 10, 10, None) == -1


def test_create_fails_loudly_without_a_device(N):
    h = ctypes.c_void_p()
    rc = N.lib().ndtgpu_pgo3_create(2, 10, 20, ctypes.byref(h))
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        assert rc == 0 and h.value
        assert _set_graph(N, h, 11, list(range(10)), list(range(1, 11))) == -4
        assert N.lib().ndtgpu_pgo3_optimize(h, 0, 1, None, None) == -1 and b"not been set" in N.lib().ndtgpu_last_error()
        assert N.lib().ndtgpu_pgo3_destroy(h) == 0
        return
    assert rc == -3 and not h.value
    assert b"no HIP device" in N.lib().ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO3(1, 10, 10)
    assert e.value.status == -3
