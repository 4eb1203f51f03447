"""CPU-side checks of the feature-set RANSAC matcher's C-ABI (ndtgpu_featbank_*): the header declares it with its provenance,
deviations and citations, the ctypes signatures and structs agree with it, the arguments are checked before the handle is read and
the device is looked for, and without a device the library fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_featmatch_params", "ndtgpu_featbank_create", "ndtgpu_featbank_destroy", "ndtgpu_featbank_set",
           "ndtgpu_featbank_match", "ndtgpu_featbank_match_device", "ndtgpu_featbank_results")


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
    sec = text[text.index("feature-set RANSAC matching"):text.index("ndtgpu_featbank_results(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec
    for site in ("ndt_feature_map.h:104-122", "ndt_feature_node.h:256", "ndt_feature_graph.cpp:162-177", "ndt_feature_graph.cpp:395-405",
                 "ndt_feature_fuser_hmt.cpp:251", "ndt_feature_fuser_hmt.h:213", "flirtlib_utils.h:32-42", "ndt_feature_graph_opt.cpp:95"):
        assert site in sec, site
    assert "boost::mt19937" in sec and "atan2" in sec and "adaptive" in sec         # the deviations a caller must read
    for name, value in (("OK", 0), ("TOO_FEW", 1), ("NO_HYPOTHESIS", 2), ("BAD_INDEX", 3)):
        assert re.search(r"NDTGPU_FEATMATCH_%s\s*=\s*%d\b" % (name, value), code) and getattr(binding, "FEATMATCH_" + name) == value
    assert N.FeatureMatcher is binding.FeatureMatcher


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_layouts_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    pf = [f for f, _ in binding.FeatMatchParams._fields_]
    rf = [f for f, _ in binding.FeatMatchResult._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu", '
                   'sizeof(ndtgpu_featmatch_params), sizeof(ndtgpu_featmatch_result));\n'
                   + "".join('printf(" %%zu", offsetof(ndtgpu_featmatch_params, %s));\n' % f for f in pf)
                   + "".join('printf(" %%zu", offsetof(ndtgpu_featmatch_result, %s));\n' % f for f in rf) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(binding.FeatMatchParams), ctypes.sizeof(binding.FeatMatchResult)]
    want += [getattr(binding.FeatMatchParams, f).offset for f in pf] + [getattr(binding.FeatMatchResult, f).offset for f in rf]
    assert got == want
    assert binding.FEATMATCH_RESULT_DTYPE.itemsize == got[1]
    assert [binding.FEATMATCH_RESULT_DTYPE.fields[f][1] for f in rf] == got[2 + len(pf):]
    assert rf == ["score", "x", "y", "theta", "c", "s", "n_candidates", "n_hypotheses", "n_tested", "best_hypothesis", "n_inliers", "status"]


def test_defaults_are_the_documented_ones(N):
    from ndt_feature_graph_amd import binding
    p = binding.featmatch_params()
    assert (p.acceptance_threshold, p.success_probability, p.inlier_probability, p.distance_threshold, p.rigidity_threshold) == \
        (0.0599, 0.9, 0.1, 0.6, 0.0499)                                     # ndt_feature_map.h:104-122
    assert p.seed == 0 and p.adaptive == 0
    import featmatch_model as M
    assert M.DEFAULTS == dict(acceptance_threshold=0.0599, success_probability=0.9, inlier_probability=0.1, distance_threshold=0.6,
                              rigidity_threshold=0.0499, seed=0)
    with pytest.raises(TypeError):
        binding.featmatch_params(no_such_field=1)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    h = ctypes.c_void_p()
    assert L.ndtgpu_featbank_create(4, 64, 48, None) == -1
    assert L.ndtgpu_featbank_create(0, 64, 48, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_featbank_create(4, 0, 48, ctypes.byref(h)) == -1 and not h.value
    assert L.ndtgpu_featbank_create(4, 64, 0, ctypes.byref(h)) == -1 and not h.value and b"desc_len" in L.ndtgpu_last_error()
    assert L.ndtgpu_featbank_create(4, 1025, 48, ctypes.byref(h)) == -1 and not h.value and b"max_points" in L.ndtgpu_last_error()
    assert L.ndtgpu_featbank_create(4, 64, 129, ctypes.byref(h)) == -1 and not h.value
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph = ctypes.c_void_p(1)
    pos, desc = np.zeros((1025, 3)), np.zeros((1025, 48))
    assert L.ndtgpu_featbank_set(ph, 0, 1025, pos.ctypes.data_as(dp), desc.ctypes.data_as(dp)) == -4       # n > any max_points
    assert L.ndtgpu_featbank_set(ph, 0, 5, None, desc.ctypes.data_as(dp)) == -1
    assert L.ndtgpu_featbank_set(ph, 0, 5, pos.ctypes.data_as(dp), None) == -1
    idx = np.zeros(4, dtype=np.uint32)
    ip = idx.ctypes.data_as(u32p)
    assert L.ndtgpu_featbank_match(ph, None, ip, 4, None, None) == -1
    assert L.ndtgpu_featbank_match(ph, ip, None, 4, None, None) == -1
    assert L.ndtgpu_featbank_match(ph, ip, ip, (1 << 24) + 1, None, None) == -1
    for bad in (dict(adaptive=1), dict(inlier_probability=0.0), dict(inlier_probability=1.0), dict(success_probability=1.0),
                dict(acceptance_threshold=float("nan")), dict(distance_threshold=-1.0), dict(rigidity_threshold=float("inf")),
                dict(inlier_probability=1e-9)):
        p = binding.featmatch_params(**bad)
        assert L.ndtgpu_featbank_match(ph, ip, ip, 4, ctypes.byref(p), None) == -1, bad
        assert L.ndtgpu_featbank_match_device(ph, ctypes.c_void_p(8), ctypes.c_void_p(8), 4, ctypes.byref(p), ctypes.c_void_p(8), None, None,
                                              None) == -1, bad
    p = binding.featmatch_params(adaptive=1)
    assert L.ndtgpu_featbank_match(ph, ip, ip, 4, ctypes.byref(p), None) == -1 and b"adaptive" in L.ndtgpu_last_error()
    assert L.ndtgpu_featbank_match_device(ph, None, ctypes.c_void_p(8), 4, None, ctypes.c_void_p(8), None, None, None) == -1
    assert L.ndtgpu_featbank_match_device(ph, ctypes.c_void_p(8), ctypes.c_void_p(8), 4, None, None, None, None, None) == -1


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    assert L.ndtgpu_featbank_destroy(None) == -1
    assert L.ndtgpu_featbank_set(None, 0, 0, None, None) == -1
    assert L.ndtgpu_featbank_match(None, None, None, 0, None, None) == -1
    assert L.ndtgpu_featbank_match_device(None, None, None, 0, None, None, None, None, None) == -1
    assert L.ndtgpu_featbank_results(None, 0, 0, None, None, None) == -1
    L.ndtgpu_default_featmatch_params(None)                     # (a no-op, as the other default functions)


def test_create_fails_loudly_without_a_device(N):
    h = ctypes.c_void_p()
    rc = N.lib().ndtgpu_featbank_create(2, 10, 48, ctypes.byref(h))
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        assert rc == 0 and h.value
        dp = ctypes.POINTER(ctypes.c_double)
        pos, desc = np.zeros((11, 3)), np.zeros((11, 48))
        assert N.lib().ndtgpu_featbank_set(h, 0, 11, pos.ctypes.data_as(dp), desc.ctypes.data_as(dp)) == -4
        assert N.lib().ndtgpu_featbank_set(h, 2, 1, pos.ctypes.data_as(dp), desc.ctypes.data_as(dp)) == -1
        assert N.lib().ndtgpu_featbank_results(h, 0, 1, None, None, None) == -1
        assert N.lib().ndtgpu_featbank_destroy(h) == 0
        return
    assert rc == -3 and not h.value
    assert b"no HIP device" in N.lib().ndtgpu_last_error()
    with pytest.raises(N.NdtGpuError) as e:
        N.FeatureMatcher(1, 10)
    assert e.value.status == -3
