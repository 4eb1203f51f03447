"""CPU-side checks of the NDT Monte Carlo localisation bank's C-ABI (ndtgpu_mcl_*): the header declares it with its provenance,
the ctypes signatures and structs agree with it, arguments are checked before the device is looked for, and without a device
the library fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_mcl_params", "ndtgpu_mcl_create", "ndtgpu_mcl_destroy", "ndtgpu_mcl_initialize", "ndtgpu_mcl_set_particles",
           "ndtgpu_mcl_update", "ndtgpu_mcl_update_host", "ndtgpu_mcl_particles", "ndtgpu_mcl_mean")


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
    sec = text[text.index("NDT Monte Carlo localisation"):text.index("ndtgpu_mcl_mean")]
    assert "ndt_feature_mcl_node.cpp" in sec and "PROVENANCE" in sec and "DEVIATIONS" in sec
    for site in (":48", ":174", ":175-184", ":335", ":361", ":377-396"):
        assert site in sec, site


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
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   ' sizeof(ndtgpu_mcl_params), sizeof(ndtgpu_mcl_result), offsetof(ndtgpu_mcl_params, seed),'
                   ' offsetof(ndtgpu_mcl_result, overflow)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.MclParams), ctypes.sizeof(binding.MclResult), binding.MclParams.seed.offset,
                   binding.MclResult.overflow.offset]


def test_defaults_cite_the_node(N):
    from ndt_feature_graph_amd import binding
    p = binding.mcl_params()
    assert p.zfilt_min == -5.0 and p.sir_varp_threshold == 0.006 and p.sir_max_iters_wo_resampling == 25 and p.force_sir == 0
    assert list(p.scan_size) == [100.0, 100.0, 8.0] and p.map_res == 0.0 and p.sensor_res == 0.0


def _create(N, n_filters=1, n_particles=100, map_set=ctypes.c_void_p(1), idx=True, **fields):
    from ndt_feature_graph_amd import binding
    p = binding.mcl_params(**fields)
    arr = (ctypes.c_uint32 * max(1, n_filters))()
    h = ctypes.c_void_p()
    rc = N.lib().ndtgpu_mcl_create(map_set, arr if idx else None, ctypes.byref(p), n_filters, n_particles, ctypes.byref(h))
    return rc, h


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    # (a non-NULL placeholder for the map set: every check below fails before it is read)
    assert _create(N, n_particles=0)[0] == -1
    assert _create(N, n_particles=65537)[0] == -1
    assert _create(N, n_filters=0)[0] == -1
    assert _create(N, n_filters=257, n_particles=65536)[0] == -1        # n_filters * n_particles > 2^24
    assert _create(N, map_res=-0.5)[0] == -1
    assert _create(N, map_res=float("nan"))[0] == -1
    assert _create(N, sensor_res=-1.0)[0] == -1
    assert _create(N, scan_size=[100.0, 0.0, 8.0])[0] == -1
    assert _create(N, idx=False)[0] == -1
    assert _create(N, map_set=None)[0] == -1


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    d = (ctypes.c_double * 16)()
    assert L.ndtgpu_mcl_destroy(None) == -1
    assert L.ndtgpu_mcl_initialize(None, 0, 1, d, d) == -1
    assert L.ndtgpu_mcl_set_particles(None, 0, 1, d, None) == -1
    assert L.ndtgpu_mcl_update(None, 0, 1, d, 1.0, None, 0, 12, 0, None) == -1
    assert L.ndtgpu_mcl_update_host(None, 0, 1, d, 1.0, None, 0, 12, 0) == -1
    assert L.ndtgpu_mcl_particles(None, 0, 1, None, None, None) == -1
    assert L.ndtgpu_mcl_mean(None, 0, 1, None, None) == -1


def test_create_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: a real map set, and a resolution that differs is refused)
        ms = N.MapSet(0.5, [0, 0, 0], [40, 40, 1], n_maps=2)
        assert _create(N, map_set=ms.h, map_res=0.25)[0] == -1
        assert b"differs" in N.lib().ndtgpu_last_error()
        rc, h = _create(N, map_set=ms.h, map_res=0.5, scan_size=[40.0, 40.0, 1.0])
        assert rc == 0 and h.value
        assert N.lib().ndtgpu_mcl_destroy(h) == 0
        return
    # (a map set cannot exist without a device; a placeholder is not read before the device check)
    rc, h = _create(N)
    assert rc == -3 and not h.value
    assert b"no HIP device" in N.lib().ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.MapSet(0.5, [0, 0, 0], [40, 40, 1])
    assert e.value.status == -3
