"""The host mirror's scan front end (host/ndt_feature_map_gpu.h: LaserScanGPU, detectAndDescribe) compiled with g++:
tests/native/featextract_demo.cpp extracts the interest points of 4 scans the way the fuser's detect + describe loop does and checks
them bit for bit against the ndtgpu_featbank_extract / _get calls it wraps on a GPU, and without one that it fails loudly.
tests/native/featextract_checks.cpp is the stand-alone host program of the shared check functions and the _get unpacking."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_featbank_extract" in N.binding.EXPORTS
    exe = str(tmp_path / "featextract_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "featextract_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_featextract_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_check_functions_and_the_unpacking_on_the_host(tmp_path):
    """the shared checks and ndt_featextract_unpack_desc need no HIP: a plain g++ program calls them on host arrays"""
    exe = str(tmp_path / "featextract_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "featextract_checks.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout


@pytest.mark.gpu
def test_featextract_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "featextract_demo: 4 scans" in out.stdout and "4 scans equal to the C-ABI bit for bit" in out.stdout and "0 failures" in out.stdout
