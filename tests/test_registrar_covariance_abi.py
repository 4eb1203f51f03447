"""CPU-side checks of the registrar's covariance entries (ndtgpu_register_batch_cov_device / _host): the header declares them and
the flag bits, the Python layer takes the new arguments, and the C++ mirror's ScanRegistrar::match overload that returns the
covariances compiles against the host headers."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return open(os.path.join(ROOT, "include", "ndtgpu.h")).read()


def test_header_declares_the_covariance_entries_and_flags():
    text = header_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("ndtgpu_register_batch_cov_device", "ndtgpu_register_batch_cov_host"):
        assert re.search(r"\b%s\s*\(" % fn, code), fn
    for name, value in (("NDTGPU_COV_SINGULAR", 1), ("NDTGPU_COV_POSE_UNCHANGED", 2), ("NDTGPU_COV_NOT_COMPUTED", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), code), name
    assert "ndt_feature_graph.cpp:283-310" in text
    # the device entry takes the registrar's arguments, then the covariance mode and the two outputs, then stream and ticket
    sig = re.search(r"ndtgpu_register_batch_cov_device\s*\((.*?)\);", code, flags=re.S).group(1)
    assert re.search(r"int\s+covariance_mode\s*,\s*double\s*\*\s*cov36_dev\s*,\s*int32_t\s*\*\s*cov_flags_dev\s*,\s*ndtgpu_stream", sig)


def test_binding_exports_and_arguments():
    from ndt_feature_graph_amd import binding
    assert "ndtgpu_register_batch_cov_device" in binding.EXPORTS
    assert "ndtgpu_register_batch_cov_host" in binding.EXPORTS
    assert (binding.COV_SINGULAR, binding.COV_POSE_UNCHANGED, binding.COV_NOT_COMPUTED) == (1, 2, 4)
    sub = inspect.signature(binding.Registrar.submit).parameters
    for a in ("covariance_mode", "cov36_dev", "cov_flags_dev"):
        assert a in sub and sub[a].default is None, a
    host = inspect.signature(binding.Registrar.register_host).parameters
    assert "covariance_mode" in host and host["covariance_mode"].default is None


def test_library_exports_the_covariance_entries():
    import ctypes
    import ndt_feature_graph_amd as N
    N.build_library()
    L = ctypes.CDLL(N.library_path())
    assert hasattr(L, "ndtgpu_register_batch_cov_device") and hasattr(L, "ndtgpu_register_batch_cov_host")


def test_scan_registrar_covariance_overload_compiles(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("""#include "lslgeneric_gpu.h"
int probe()
{
    const double c[3] = {0, 0, 0}, sz[3] = {100, 100, 1};
    ndtgpu_host::ScanRegistrar reg(0.5, c, sz, 32, 2, 4096);
    lslgeneric::NDTMatcherD2D matcher;
    matcher.covariance_mode = 1;
    std::vector<pcl::PointCloud<pcl::PointXYZ>> fixed(2), moving(2);
    std::vector<Eigen::Affine3d> T(2);
    std::vector<Eigen::MatrixXd> cov;
    std::vector<int32_t> flags;
    std::vector<ndtgpu_match_result> res;
    std::vector<bool> ok = reg.match(matcher, fixed, moving, T, cov, flags, 30.0, true, &res, 0x23);
    std::vector<bool> plain = reg.match(matcher, fixed, moving, T, 30.0);
    double c00 = cov.empty() ? 0.0 : cov[0](0, 0);
    return (int)ok.size() + (int)plain.size() + (int)c00 + ((flags[0] & NDTGPU_COV_POSE_UNCHANGED) ? 1 : 0);
}
""")
    host = os.path.join(ROOT, "ndt_feature_graph_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", host, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
