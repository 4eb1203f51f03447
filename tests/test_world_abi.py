"""CPU-side checks of the world-map assembly's C-ABI (ndtgpu_world_*): the header declares it with its provenance, deviations and
call sites, the ctypes signatures and structs agree with it, every NDTGPU_ERR_INVALID case is refused without a device, and
without a device the call fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_world_params", "ndtgpu_world_assemble", "ndtgpu_world_check")
U32P = ctypes.POINTER(ctypes.c_uint32)
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
    sec = text[text.index("world-map assembly"):text.index("ndtgpu_world_check(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "OURS" in sec
    for site in ("ndt_feature_mcl_node.cpp:174", "ndt_feature2d_fuser.cpp:425-432", "ndt_feature_graph_opt.cpp:178-185",
                 "ndt_feature_graph.h:149-152", "ndt_feature2d_fuser.cpp:471", "publish_graph_message.cpp:588", "fuser_hmt.cpp:486",
                 "pseudoTransformNDT", "rescaleCovariance", "getIndexForPoint"):
        assert site in sec, site
    for word in ("n_rejected", "n_dropped", "out of scope", "order independence", "res_dst", "NDTGPU_ERR_CAPACITY", "builder-run"):
        assert word in sec, word
    for exported in ("assemble_world", "WorldParams", "WorldResult"):
        assert hasattr(N, exported), exported
    assert "0.6.6" not in N.lib().ndtgpu_version().decode()          # bumped with the new entries


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_sizes_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    fields_p = ("maxnumpoints", "eval_factor", "occupancy_limit")
    fields_r = ("n_nodes", "n_cells", "n_contributions", "n_dropped", "n_rejected", "n_points", "overflow", "s1_shift", "s2_shift")
    items = ["sizeof(ndtgpu_world_params)", "sizeof(ndtgpu_world_result)"]
    items += ["offsetof(ndtgpu_world_params, %s)" % f for f in fields_p] + ["offsetof(ndtgpu_world_result, %s)" % f for f in fields_r]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%s\\n", %s); return 0;}\n'
                   % (" ".join(["%zu"] * len(items)), ", ".join("(size_t)" + i for i in items)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(binding.WorldParams), ctypes.sizeof(binding.WorldResult)]
    want += [getattr(binding.WorldParams, f).offset for f in fields_p] + [getattr(binding.WorldResult, f).offset for f in fields_r]
    assert got == want


def test_defaults_are_the_documented_ones(N):
    from ndt_feature_graph_amd import binding
    import world_model as W
    p = binding.world_params()
    assert (p.maxnumpoints, p.eval_factor, p.occupancy_limit) == (1e5, 1000.0, 255.0)        # fuser_hmt.cpp:486
    assert list(p.reserved_) == [0.0, 0.0]
    assert W.DEFAULTS == dict(maxnumpoints=1e5, eval_factor=1000.0, occupancy_limit=255.0)
    assert binding.world_params(maxnumpoints=0).maxnumpoints == 0
    with pytest.raises(TypeError):
        binding.world_params(no_such_field=1)


def _check(N, offsets, idx, dst_n=4, dst_res=0.5, dst_first=0, count=None, src_n=8, src_res=0.5, same=0):
    off = np.asarray(offsets, dtype=np.uint32)
    ix = np.asarray(list(idx) + [0], dtype=np.uint32)
    count = len(off) - 1 if count is None else count
    return N.lib().ndtgpu_world_check(dst_n, dst_res, dst_first, count, src_n, src_res, same, off.ctypes.data_as(U32P),
                                      ix.ctypes.data_as(U32P))


def test_every_invalid_case_is_refused_without_a_device(N):
    L = N.lib()
    assert _check(N, [0, 2, 3], [0, 7, 3]) == 0
    assert _check(N, [0, 2, 3], [0, 8, 3]) == -1 and b"node index out of range" in L.ndtgpu_last_error()
    assert _check(N, [0, 2, 1], [0, 1, 2]) == -1 and b"non-decreasing" in L.ndtgpu_last_error()
    assert _check(N, [0, 2, 3], [0, 5, 3], dst_res=0.25) == -1 and b"res" in L.ndtgpu_last_error()
    assert _check(N, [0, 2, 3], [0, 5, 3], dst_res=float("nan")) == -1
    assert _check(N, [0, 2, 3], [0, 5, 3], dst_res=1.0) == 0                       # a coarser destination is fine
    # the same set: maps 2 and 3 are destinations, so neither may be listed
    assert _check(N, [0, 2, 3], [0, 1, 4], dst_n=8, dst_first=2, same=1) == 0
    assert _check(N, [0, 2, 3], [0, 3, 4], dst_n=8, dst_first=2, same=1) == -1 and b"among the listed" in L.ndtgpu_last_error()
    assert _check(N, [0, 2, 3], [0, 3, 4], dst_n=8, dst_first=2, same=0) == 0
    # destination maps out of range
    assert _check(N, [0, 2, 3], [0, 1, 2], dst_n=4, dst_first=3) == -1 and b"out of range" in L.ndtgpu_last_error()
    assert _check(N, [0, 0, 0], []) == 0                                            # empty worlds are worlds
    assert L.ndtgpu_world_check(4, 0.5, 0, 1, 8, 0.5, 0, None, None) == -1


def test_assemble_refuses_what_needs_no_handle_before_the_device_is_looked_for(N):
    # (placeholders for the handles: each check below fails before a handle is read -- there is no map set without a device)
    L = N.lib()
    h, g = ctypes.c_void_p(1), ctypes.c_void_p(2)
    off = np.array([0, 2, 1], dtype=np.uint32)
    idx = np.array([0, 1, 2], dtype=np.uint32)
    T = np.tile(np.eye(4).reshape(-1), (3, 1))
    args = (off.ctypes.data_as(U32P), idx.ctypes.data_as(U32P), T.ctypes.data_as(DP), None, None, None)
    assert L.ndtgpu_world_assemble(h, 0, 2, g, *args) == -1 and b"non-decreasing" in L.ndtgpu_last_error()
    off[:] = [0, 2, 3]
    assert L.ndtgpu_world_assemble(h, 1, 2, h, *args) == -1 and b"among the listed" in L.ndtgpu_last_error()
    assert L.ndtgpu_world_assemble(None, 0, 2, g, *args) == -1
    assert L.ndtgpu_world_assemble(h, 0, 2, None, *args) == -1
    assert L.ndtgpu_world_assemble(h, 0, 2, g, None, idx.ctypes.data_as(U32P), T.ctypes.data_as(DP), None, None, None) == -1
    assert L.ndtgpu_world_assemble(h, 0, 2, g, off.ctypes.data_as(U32P), None, T.ctypes.data_as(DP), None, None, None) == -1
    from ndt_feature_graph_amd import binding
    bad = binding.world_params(eval_factor=0.0)
    assert L.ndtgpu_world_assemble(h, 0, 2, g, *args[:3], ctypes.byref(bad), None, None) == -1


def test_the_call_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: the map sets exist and the handle-dependent checks run on them)
        src = N.MapSet(0.5, [0, 0, 0], [4, 4, 1], n_maps=2)
        dst = N.MapSet(0.25, [0, 0, 0], [4, 4, 1], n_maps=1)
        with pytest.raises(N.NdtGpuError) as e:
            N.assemble_world(dst, 0, src, [[0, 1]], [np.stack([np.eye(4)] * 2)])
        assert e.value.status == -1
        return
    L = N.lib()
    off = np.array([0, 1], dtype=np.uint32)
    idx = np.array([0], dtype=np.uint32)
    T = np.eye(4).reshape(1, 16)
    rc = L.ndtgpu_world_assemble(ctypes.c_void_p(1), 0, 1, ctypes.c_void_p(2), off.ctypes.data_as(U32P), idx.ctypes.data_as(U32P),
                                 T.ctypes.data_as(DP), None, None, None)
    assert rc == -3 and b"no HIP device" in L.ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.MapSet(0.5, [0, 0, 0], [4, 4, 1], n_maps=2)
    assert e.value.status == -3
