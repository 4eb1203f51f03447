"""CPU-side checks of the coarse-to-fine registrar's C-ABI (ndtgpu_multires_*, ndtgpu_register_multires_*): the header declares
it, the ctypes signatures agree with it, arguments are checked before the device is looked for, and without a device the
library fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_resolutions", "ndtgpu_multires_create", "ndtgpu_multires_destroy", "ndtgpu_register_multires_device",
           "ndtgpu_register_multires_host", "ndtgpu_multires_get_info")


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
    assert re.search(r"#define\s+NDTGPU_MAX_LEVELS\s+8\b", code) and binding.MAX_LEVELS == 8
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    assert "ndt_odom_debug.cpp:159-165" in text and "ndt_feature_pcl_eval.cpp:620-642" in text and "DEVIATION" in text


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip()])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    dev = re.search(r"ndtgpu_register_multires_device\s*\((.*?)\);", code, flags=re.S).group(1)
    assert re.search(r"const\s+ndtgpu_match_params\s*\*\s*prm\s*,\s*int\s+use_initial_guess\s*,\s*ndtgpu_match_result\s*\*\s*results_dev\s*,"
                     r"\s*ndtgpu_stream", dev)


def test_struct_sizes_against_gcc(N, tmp_path):
    """the structs the new entries take, as gcc sees the header, against the ctypes mirrors"""
    from ndt_feature_graph_amd import binding
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ndtgpu_grid_params),'
                   ' sizeof(ndtgpu_cell_params), sizeof(ndtgpu_match_params), sizeof(ndtgpu_match_result),'
                   ' sizeof(ndtgpu_multires_info), NDTGPU_MAX_LEVELS);'
                   ' return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.GridParams), ctypes.sizeof(binding.CellParams), ctypes.sizeof(binding.MatchParams),
                   ctypes.sizeof(binding.MatchResult), ctypes.sizeof(binding.MultiResInfo), 8]


def test_default_resolutions(N):
    from ndt_feature_graph_amd import binding
    assert binding.default_resolutions() == (0.2, 0.5, 1.0, 2.0)


def _create(N, resolutions, n_levels=None):
    from ndt_feature_graph_amd import binding
    gp = binding.GridParams()
    gp.res = 0.0
    gp.centre[:] = [0.0, 0.0, 0.0]
    gp.size[:] = [100.0, 100.0, 1.0]
    arr = (ctypes.c_double * max(1, len(resolutions)))(*resolutions)
    h = ctypes.c_void_p()
    n = len(resolutions) if n_levels is None else n_levels
    return N.lib().ndtgpu_multires_create(ctypes.byref(gp), arr, n, 16, ctypes.byref(h)), h


def test_invalid_level_lists_are_refused_before_the_device_is_looked_for(N):
    assert _create(N, [])[0] == -1
    assert _create(N, [0.5] * 9)[0] == -1
    assert _create(N, [0.5, 0.0, 1.0])[0] == -1
    assert _create(N, [0.5, -1.0])[0] == -1
    assert _create(N, [0.5, float("nan")])[0] == -1
    assert _create(N, [0.5], n_levels=0)[0] == -1


def test_create_fails_loudly_without_a_device(N):
    rc, h = _create(N, [0.2, 0.5, 1.0, 2.0])
    if N.device_count() > 0:                 # (a box with a device: the handle is made)
        assert rc == 0 and h.value
        assert N.lib().ndtgpu_multires_destroy(h) == 0
        return
    assert rc == -3 and not h.value
    assert b"no HIP device" in N.lib().ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.MultiRes([0, 0, 0], [100, 100, 1])
    assert e.value.status == -3


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    assert L.ndtgpu_multires_destroy(None) == -1
    assert L.ndtgpu_multires_get_info(None, None) == -1
    assert L.ndtgpu_register_multires_device(None, None, None, 10, 12, 120, -1.0, None, None, 1, None, 1, None, None) == -1
    assert L.ndtgpu_register_multires_host(None, None, None, 10, 12, 120, -1.0, None, None, 1, None, 1, None) == -1
