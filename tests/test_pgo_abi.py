"""CPU-side checks of the pose-graph optimiser's C-ABI (ndtgpu_pgo_*): the header declares it with its provenance and citations,
the ctypes signatures and structs agree with it, a graph's arguments are checked before the handle is read and the device is
looked for, and without a device the library fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_pgo_params", "ndtgpu_pgo_create", "ndtgpu_pgo_destroy", "ndtgpu_pgo_set_graph",
           "ndtgpu_pgo_set_links_device", "ndtgpu_pgo_optimize", "ndtgpu_pgo_poses")


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
    sec = text[text.index("SE(2) pose-graph optimisation"):text.index("ndtgpu_pgo_poses(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec
    for site in ("ndt_feature_graph_opt.cpp", ":147", ":152-164", "ndt_offline_mapper.h:8-15", "ndt_offline_mapper.h:17-26",
                 "ndt_offline_mapper.h:40-107", "utils.h:30-40", "ndt_feature_graph.cpp:283-310"):
        assert site in sec, site
    assert "OURS" in sec and "not iSAM's" in sec                 # the stop rule's defaults are declared as the library's own
    for name, value in (("CONVERGED", 0), ("MAX_ITERATIONS", 1), ("LINEAR_CAP", 2), ("NOT_FINITE", 3)):
        assert re.search(r"NDTGPU_PGO_%s\s*=\s*%d\b" % (name, value), code) and getattr(binding, "PGO_" + name) == value


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_sizes_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(ndtgpu_pgo_params), sizeof(ndtgpu_pgo_result), offsetof(ndtgpu_pgo_params, prior_information),'
                   ' offsetof(ndtgpu_pgo_result, cost_initial), offsetof(ndtgpu_pgo_result, max_step),'
                   ' offsetof(ndtgpu_pgo_result, n_edges)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.PgoParams), ctypes.sizeof(binding.PgoResult), binding.PgoParams.prior_information.offset,
                   binding.PgoResult.cost_initial.offset, binding.PgoResult.max_step.offset, binding.PgoResult.n_edges.offset]


def test_defaults_are_the_documented_ones(N):
    from ndt_feature_graph_amd import binding
    p = binding.pgo_params()
    assert (p.max_iterations, p.max_linear_iterations, p.eps_step, p.eps_linear) == (50, 2000, 1e-8, 1e-8)
    assert list(p.prior_information) == [100.0, 0, 0, 0, 100.0, 0, 0, 0, 100.0]          # ndt_offline_mapper.h:45, :61
    import pgo_model as M
    assert M.DEFAULTS == dict(max_iterations=50, max_linear_iterations=2000, eps_step=1e-8, eps_linear=1e-8)
    with pytest.raises(TypeError):
        binding.pgo_params(no_such_field=1)


def _set_graph(N, h, n_nodes, ref, mov, poses=True, meas=True):
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    ps = np.zeros((max(n_nodes, 1), 3))
    ri, mi = np.asarray(ref, dtype=np.uint32), np.asarray(mov, dtype=np.uint32)
    z = np.zeros((max(len(ri), 1), 3))
    return N.lib().ndtgpu_pgo_set_graph(h, 0, n_nodes, ps.ctypes.data_as(dp) if poses else None, len(ri), ri.ctypes.data_as(u32p),
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
    assert _set_graph(N, h, 2, [], []) == -1 and b"not connected" in L.ndtgpu_last_error()
    assert _set_graph(N, h, 0, [], []) == -1
    assert _set_graph(N, h, 2, [0], [1], poses=False) == -1
    assert _set_graph(N, h, 2, [0], [1], meas=False) == -1
    # the device form of the links makes the same checks
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    ps = np.zeros((4, 3))
    ri, mi = np.array([0, 2], dtype=np.uint32), np.array([1, 3], dtype=np.uint32)
    rc = L.ndtgpu_pgo_set_links_device(h, 0, 4, ps.ctypes.data_as(dp), 2, ri.ctypes.data_as(u32p), mi.ctypes.data_as(u32p),
                                       ctypes.c_void_p(8), None, None)
    assert rc == -1 and b"not connected" in L.ndtgpu_last_error()


def test_entries_refuse_a_null_handle_and_bad_sizes(N):
    L = N.lib()
    assert L.ndtgpu_pgo_destroy(None) == -1
    assert _set_graph(N, None, 2, [0], [1]) == -1
    assert L.ndtgpu_pgo_optimize(None, 0, 1, None, None) == -1
    assert L.ndtgpu_pgo_poses(None, 0, None, None, None) == -1
    h = ctypes.c_void_p()
    assert L.ndtgpu_pgo_create(0, 10, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo_create(1, 0, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo_create(1, (1 << 24) + 1, 10, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_pgo_create(1, 10, 10, None) == -1


def test_create_fails_loudly_without_a_device(N):
    h = ctypes.c_void_p()
    rc = N.lib().ndtgpu_pgo_create(2, 10, 20, ctypes.byref(h))
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        assert rc == 0 and h.value
        assert _set_graph(N, h, 11, list(range(10)), list(range(1, 11))) == -4
        assert N.lib().ndtgpu_pgo_optimize(h, 0, 1, None, None) == -1 and b"not been set" in N.lib().ndtgpu_last_error()
        assert N.lib().ndtgpu_pgo_destroy(h) == 0
        return
    assert rc == -3 and not h.value
    assert b"no HIP device" in N.lib().ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO(1, 10, 10)
    assert e.value.status == -3
