"""The host mirror's extrinsic calibration (host/ndt_calibration_gpu.h: ScanPairGPU, errorFunction, bruteForceOptimization,
CalibrationPairCollector) compiled with g++: tests/native/calib_demo.cpp collects pairs the way the reference's callback does,
searches the lattice in one device call and checks the winner and errorFunction / scoreICP against it bit for bit on a GPU, and
without one that it fails loudly.  tests/native/calib_checks.cpp is the stand-alone host program of the shared header, built with
the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_calib_search" in N.binding.EXPORTS
    exe = str(tmp_path / "calib_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "calib_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_calib_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_shared_header_on_the_host_under_the_sanitizers(tmp_path):
    """the lattice, the pair motion, the pair selection, the checks and the chunk arithmetic need no HIP: a plain g++ program with its
    own main, built with -fsanitize=address,undefined, writes every output into heap blocks of exactly the size a call may touch"""
    exe = str(tmp_path / "calib_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "calib_checks.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout and "32 of 32 bad arguments refused" in out.stdout


@pytest.mark.gpu
def test_calib_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "calib_demo: 5 pairs, 440 candidates, winner (0.23, 0.02, 0.01)" in out.stdout and "0 failures" in out.stdout
