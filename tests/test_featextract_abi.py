"""CPU-side checks of the laser-scan feature extraction's C-ABI (ndtgpu_featbank_extract*, ndtgpu_featbank_get): the header
declares it with its semantics, provenance, deviations and citations, the ctypes signatures and structs agree with it, and every
argument and parameter check returns its error before the handle is read and the device is looked for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_featextract_params", "ndtgpu_featbank_extract", "ndtgpu_featbank_extract_device",
           "ndtgpu_featbank_extract_results", "ndtgpu_featbank_get")


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
    sec = text[text.index("laser-scan feature extraction"):text.index("ndtgpu_featbank_get(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Measured on MI355X" in sec
    for site in ("ndt_feature2d_fuser.cpp:766-779", "publish_graph_message.cpp:1401-1404", "flirtlib_utils.h:15-42",
                 "conversions.cpp:69-82", "SimpleMinMaxPeakFinder(0.34, 0.001)", "CurvatureDetector(peak, 5, 0.2, 1.4, 2.0)",
                 "BetaGridGenerator(0.02, 1.0, 4, 12)", "setUseMaxRange(false)"):
        assert site in sec, site
    for word in ("minimum spanning tree", "not calibrated", "min_separation", "fixed-step", "n_beams <= 2048"):    # the deviations
        assert word in sec, word
    assert "PLACEHOLDER" not in text
    for name, value in (("OK", 0), ("TOO_FEW_POINTS", 1), ("OVERFLOW", 2), ("BAD_INDEX", 3)):
        assert re.search(r"NDTGPU_FEATEXTRACT_%s\s*=\s*%d\b" % (name, value), code) and getattr(binding, "FEATEXTRACT_" + name) == value


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_layouts_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    pf = [f for f, _ in binding.FeatExtractParams._fields_]
    rf = [f for f, _ in binding.FeatExtractResult._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu", '
                   'sizeof(ndtgpu_featextract_params), sizeof(ndtgpu_featextract_result));\n'
                   + "".join('printf(" %%zu", offsetof(ndtgpu_featextract_params, %s));\n' % f for f in pf)
                   + "".join('printf(" %%zu", offsetof(ndtgpu_featextract_result, %s));\n' % f for f in rf) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(binding.FeatExtractParams), ctypes.sizeof(binding.FeatExtractResult)]
    want += [getattr(binding.FeatExtractParams, f).offset for f in pf] + [getattr(binding.FeatExtractResult, f).offset for f in rf]
    assert got == want
    assert binding.FEATEXTRACT_RESULT_DTYPE.itemsize == got[1]
    assert [binding.FEATEXTRACT_RESULT_DTYPE.fields[f][1] for f in rf] == got[2 + len(pf):]
    assert rf == ["n_valid", "n_segments", "n_peaks", "n_found", "n_stored", "status"]


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph = ctypes.c_void_p(1)
    idx = np.zeros(4, dtype=np.uint32)
    rr = np.ones((4, 16))
    ip, rp = idx.ctypes.data_as(u32p), rr.ctypes.data_as(dp)
    nan, inf = float("nan"), float("inf")
    dv = ctypes.c_void_p(8)

    def host(n_scans=4, n_beams=16, a0=0.0, inc=0.1, prm=None, idx_p=ip, rr_p=rp):
        return L.ndtgpu_featbank_extract(ph, idx_p, rr_p, n_scans, n_beams, a0, inc, None if prm is None else ctypes.byref(prm), None)

    def device(n_scans=4, n_beams=16, a0=0.0, inc=0.1, prm=None, idx_p=dv, rr_p=dv, res_p=dv):
        return L.ndtgpu_featbank_extract_device(ph, idx_p, rr_p, n_scans, n_beams, a0, inc, None if prm is None else ctypes.byref(prm),
                                                res_p, None, None, None, None)

    assert host(idx_p=None) == -1 and host(rr_p=None) == -1
    assert device(idx_p=None) == -1 and device(rr_p=None) == -1 and device(res_p=None) == -1
    for call in (host, device):
        assert call(n_beams=0) == -1 and b"n_beams" in L.ndtgpu_last_error()
        assert call(n_beams=2049) == -1 and b"n_beams" in L.ndtgpu_last_error()
        assert call(n_scans=(1 << 24) + 1) == -1
        assert call(a0=nan) == -1 and call(inc=inf) == -1 and call(a0=-inf) == -1
        for bad in (dict(scales=0), dict(scales=9), dict(base_sigma=0.0), dict(base_sigma=-1.0), dict(base_sigma=nan),
                    dict(sigma_step=1.0), dict(sigma_step=0.5), dict(sigma_step=inf), dict(dmst=0.0), dict(dmst=nan),
                    dict(min_rho=-0.01), dict(min_rho=1.0), dict(min_rho=2.0), dict(max_rho=inf), dict(max_rho=nan), dict(min_rho=nan),
                    dict(bin_rho=0), dict(bin_phi=0), dict(bin_rho=65), dict(bin_rho=8, bin_phi=9), dict(bin_phi=-1),
                    dict(r_min=-0.1), dict(r_min=30.0), dict(r_min=31.0), dict(r_max=inf), dict(r_min=nan), dict(r_max=nan),
                    dict(min_value=nan), dict(min_value=inf), dict(min_diff=nan), dict(min_diff=-inf), dict(min_separation=nan),
                    dict(min_separation=-1.0), dict(min_separation=inf)):
            assert call(prm=binding.featextract_params(**bad)) == -1, bad
    assert host(prm=binding.featextract_params(scales=9)) == -1 and b"scales" in L.ndtgpu_last_error()
    assert host(prm=binding.featextract_params(bin_rho=8, bin_phi=9)) == -1 and b"bin_rho * bin_phi" in L.ndtgpu_last_error()


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    dp, u32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    idx, rr = np.zeros(1, dtype=np.uint32), np.ones((1, 16))
    n = ctypes.c_size_t(7)
    assert L.ndtgpu_featbank_extract(None, idx.ctypes.data_as(u32p), rr.ctypes.data_as(dp), 1, 16, 0.0, 0.1, None, None) == -1
    assert b"null handle" in L.ndtgpu_last_error()
    assert L.ndtgpu_featbank_extract(None, None, None, 0, 16, 0.0, 0.1, None, None) == -1
    assert L.ndtgpu_featbank_extract_device(None, ctypes.c_void_p(8), ctypes.c_void_p(8), 1, 16, 0.0, 0.1, None, ctypes.c_void_p(8), None,
                                            None, None, None) == -1
    assert L.ndtgpu_featbank_extract_results(None, 0, 0, None, None, None, None) == -1
    assert L.ndtgpu_featbank_get(None, 0, ctypes.byref(n), None, None) == -1
    L.ndtgpu_default_featextract_params(None)                   # (a no-op, as the other default functions)


def test_extract_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its shape is enforced)
        fm = N.FeatureMatcher(2, 8, 40)
        with pytest.raises(N.NdtGpuError) as e:
            fm.extract([0], np.ones((1, 16)), 0.0, 0.1)          # 4 x 12 bins into descriptors of 40
        assert e.value.status == -1
        n = ctypes.c_size_t(7)
        assert N.lib().ndtgpu_featbank_get(fm.h, 2, ctypes.byref(n), None, None) == -1 and n.value == 0
        assert N.lib().ndtgpu_featbank_get(fm.h, 0, None, None, None) == -1
        assert N.lib().ndtgpu_featbank_extract_results(fm.h, 0, 1, None, None, None, None) == -1
        fm.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.FeatureMatcher(1, 10)
    assert e.value.status == -3
    assert binding.FeatureMatcher.extract and binding.FeatureMatcher.get and binding.FeatureMatcher.extract_device
