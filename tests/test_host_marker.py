"""The host mirror's marker functions (host/ndt_rviz_gpu.h: markerNDTCells, markerNDTCells2, markerParticlesNDTMCL3D,
markerNDTFeatureLinks; NDTCell::getEvals / getEvecs in host/lslgeneric_gpu.h) compiled with g++: tests/native/marker_demo.cpp calls
them the way the reference's publish timers do and checks them on a GPU, and without one that it fails loudly.
tests/native/marker_checks.cpp is the stand-alone host program of the shared header, built with the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def build_demo(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_mapset_markers" in N.binding.EXPORTS
    exe = str(tmp_path / "marker_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "marker_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_marker_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = build_demo(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_shared_header_on_the_host_under_the_sanitizers(tmp_path):
    """the eigen-pairs' residuals, the sign rule, the stable order, the count at the threshold, the pose, particles, links and the
    refused arguments need no HIP: a plain g++ program with its own main, built with -fsanitize=address,undefined, works in heap
    blocks of exactly the size a call may touch"""
    exe = str(tmp_path / "marker_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "marker_checks.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout and "12000 eigen-pairs" in out.stdout and "17 of 17 bad arguments refused" in out.stdout


@pytest.mark.gpu
def test_marker_demo_on_gpu(tmp_path):
    exe = build_demo(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "marker_demo: 300 cells" in out.stdout and "600 particle points, 30 + 8 link points, 0 failures" in out.stdout
