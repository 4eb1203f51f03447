"""CPU-side checks of the link gate's C-ABI (ndtgpu_linkgate_*): the header declares it with its semantics, provenance and
deviations, the ctypes signatures and the struct agree with it, the defaults are upstream's, every argument refusal happens
without a device and before a handle is read, and without a device create fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_linkgate_params", "ndtgpu_linkgate_check", "ndtgpu_linkgate_create", "ndtgpu_linkgate_destroy",
           "ndtgpu_linkgate_set_nodes", "ndtgpu_linkgate_set_nodes_device", "ndtgpu_linkgate_candidates", "ndtgpu_linkgate_valid",
           "ndtgpu_linkgate_gather", "ndtgpu_linkgate_count", "ndtgpu_linkgate_keep", "ndtgpu_linkgate_candidates_host",
           "ndtgpu_linkgate_valid_host")


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
    L = ctypes.CDLL(N.library_path())
    for fn in ENTRIES:
        assert re.search(r"\b%s\s*\(" % fn, code), fn
        assert fn in binding.EXPORTS and hasattr(L, fn), fn
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("---- link gating"):text.index("ndtgpu_linkgate_keep(")]
    sec = " ".join(sec.replace(" * ", " ").split())                        # (a phrase may be broken across comment lines)
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "OURS" in sec
    for site in ("ndt_feature_graph.cpp:395-405", "ndt_feature_graph.cpp:527-556", "ndt_feature_graph_opt.cpp:152-173",
                 "ndt_feature_graph_opt.cpp:49-52", "utils.h:42-47", "computeAllPossibleLinks", "getValidLinks", "distanceBetweenAffine3d"):
        assert site in sec, site
    for word in ("rigid transpose", "no rotation of the difference vector", "NOT fused", "clip_cosine", "NaN", "max_rounds", "no grid barrier",
                 "ndt_block_rank"):
        assert word in sec, word
    for exported in ("LinkGate", "LinkGateParams", "linkgate_params", "optimize_gated"):
        assert hasattr(N, exported), exported
    for method in ("set_nodes", "candidates", "valid", "gather", "count", "keep", "close"):
        assert hasattr(N.LinkGate, method), method
    srcs = binding._SOURCES
    assert "ndt_linkgate.hip" in srcs and "ndtgpu_linkgate.hip" in srcs


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_size_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    fields = ("max_score", "max_dist", "max_angle", "min_idx_dist", "clip_cosine")
    items = ["sizeof(ndtgpu_linkgate_params)"] + ["offsetof(ndtgpu_linkgate_params, %s)" % f for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%s\\n", %s); return 0;}\n'
                   % (" ".join(["%zu"] * len(items)), ", ".join("(size_t)" + i for i in items)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.LinkGateParams)] + [getattr(binding.LinkGateParams, f).offset for f in fields]
    assert got[0] == 32


def test_defaults_are_upstreams(N):
    from ndt_feature_graph_amd import binding
    p = binding.linkgate_params()
    assert (p.max_score, p.max_dist, p.max_angle, p.min_idx_dist, p.clip_cosine) == (0.1, 1.0, 0.2, 2, 0)
    assert binding.linkgate_params(clip_cosine=1, max_angle=float("inf")).clip_cosine == 1
    with pytest.raises(TypeError):
        binding.linkgate_params(no_such_field=1)
    N.lib().ndtgpu_default_linkgate_params(None)           # (a null pointer is ignored)


def test_every_refusal_without_a_device(N):
    L = N.lib()
    err = L.ndtgpu_last_error
    # on plain numbers: what the entries check with a handle's numbers
    assert L.ndtgpu_linkgate_check(300, 44850, 300, 44850, 288) == 0
    assert L.ndtgpu_linkgate_check(65536, 2**27, 65536, 2**27, 4096) == 0
    assert L.ndtgpu_linkgate_check(0, 10, 0, 0, 0) == -1 and b"max_nodes" in err()
    assert L.ndtgpu_linkgate_check(65537, 10, 0, 0, 0) == -1 and b"max_nodes" in err()
    assert L.ndtgpu_linkgate_check(10, 2**27 + 1, 0, 0, 0) == -1 and b"max_links" in err()
    assert L.ndtgpu_linkgate_check(300, 100, 301, 0, 0) == -4 and b"more nodes" in err()          # NDTGPU_ERR_CAPACITY
    assert L.ndtgpu_linkgate_check(300, 100, 0, 101, 0) == -4 and b"more links" in err()
    for rb in (1, 2, 3, 6, 127, 4100):
        assert L.ndtgpu_linkgate_check(300, 100, 0, 0, rb) == -1 and b"row_bytes" in err(), rb
    # create: before the device is looked for
    h = ctypes.c_void_p()
    assert L.ndtgpu_linkgate_create(10, 10, None) == -1 and b"out is NULL" in err()
    assert L.ndtgpu_linkgate_create(0, 10, ctypes.byref(h)) == -1 and h.value is None
    assert L.ndtgpu_linkgate_create(65537, 10, ctypes.byref(h)) == -1
    assert L.ndtgpu_linkgate_create(10, 2**27 + 1, ctypes.byref(h)) == -1
    assert L.ndtgpu_linkgate_destroy(None) == -1
    # the entries: a NULL array is refused before the handle is read (placeholder handle: there is none without a device), a
    # NULL handle after it
    ph = ctypes.c_void_p(1)
    buf = (ctypes.c_double * 16)()
    a = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.ndtgpu_linkgate_set_nodes(ph, 1, None) == -1 and b"null poses" in err()
    assert L.ndtgpu_linkgate_set_nodes(None, 1, buf) == -1 and b"null handle" in err()
    assert L.ndtgpu_linkgate_set_nodes_device(ph, 1, None, None) == -1 and b"null poses" in err()
    assert L.ndtgpu_linkgate_set_nodes_device(None, 1, a, None) == -1 and b"null handle" in err()
    assert L.ndtgpu_linkgate_candidates(ph, None, None, a, None, 4, None) == -1 and b"null index output" in err()
    assert L.ndtgpu_linkgate_candidates(ph, None, a, None, None, 4, None) == -1 and b"null index output" in err()
    assert L.ndtgpu_linkgate_candidates(None, None, a, a, None, 4, None) == -1 and b"null handle" in err()
    for ref, mov, T in ((None, a, a), (a, None, a), (a, a, None)):
        assert L.ndtgpu_linkgate_valid(ph, None, 1, ref, mov, T, None, None, 0, None) == -1 and b"null link indices or poses" in err()
    assert L.ndtgpu_linkgate_valid(None, None, 1, a, a, a, None, None, 0, None) == -1 and b"null handle" in err()
    u = ctypes.cast(a, ctypes.POINTER(ctypes.c_uint32))
    assert L.ndtgpu_linkgate_candidates_host(ph, None, None, u, None, 4) == -1 and b"null index output" in err()
    assert L.ndtgpu_linkgate_candidates_host(None, None, u, u, None, 4) == -1 and b"null handle" in err()
    for ref, mov, T in ((None, u, buf), (u, None, buf), (u, u, None)):
        assert L.ndtgpu_linkgate_valid_host(ph, None, 1, ref, mov, T, None) == -1 and b"null link indices or poses" in err()
    assert L.ndtgpu_linkgate_valid_host(None, None, 1, u, u, buf, None) == -1 and b"null handle" in err()
    assert L.ndtgpu_linkgate_gather(ph, None, 128, a, 0, None) == -1 and b"null source or destination" in err()
    assert L.ndtgpu_linkgate_gather(ph, a, 128, None, 0, None) == -1
    for rb in (0, 1, 2, 3, 130, 4100):
        assert L.ndtgpu_linkgate_gather(ph, a, rb, a, 0, None) == -1 and b"row_bytes" in err(), rb
    assert L.ndtgpu_linkgate_gather(None, a, 128, a, 0, None) == -1 and b"null handle" in err()
    n = ctypes.c_size_t()
    assert L.ndtgpu_linkgate_count(ph, None, None) == -1 and b"null count" in err()
    assert L.ndtgpu_linkgate_count(None, ctypes.byref(n), None) == -1 and b"null handle" in err()
    assert L.ndtgpu_linkgate_keep(ph, 0, 1, None) == -1 and b"null output" in err()
    assert L.ndtgpu_linkgate_keep(None, 0, 0, None) == -1 and b"null handle" in err()


def test_create_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: the handle-dependent refusals on a real handle)
        g = N.LinkGate(4, 8)
        L = N.lib()
        buf = (ctypes.c_double * (16 * 5))()
        a = ctypes.c_void_p(ctypes.addressof(buf))
        assert L.ndtgpu_linkgate_set_nodes(g.h, 5, buf) == -4
        assert L.ndtgpu_linkgate_valid(g.h, None, 9, a, a, a, None, None, 0, None) == -4
        assert L.ndtgpu_linkgate_gather(g.h, a, 128, a, 0, None) == -1 and b"no ndtgpu_linkgate_valid call" in L.ndtgpu_last_error()
        n = ctypes.c_size_t()
        assert L.ndtgpu_linkgate_count(g.h, ctypes.byref(n), None) == -1
        g.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.LinkGate(300, 44850)
    assert e.value.status == -3 and "no HIP device" in str(e.value)
