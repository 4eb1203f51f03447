"""The host mirror's scan projection (host/ndt_feature_map_gpu.h: projectLaserGPU) compiled with g++:
tests/native/scanproject_demo.cpp projects 4 scans the way every consumer of a scan calls projectLaser, the range gate and the z
jitter, and checks the clouds bit for bit against the ndtgpu_scanproj_project call it wraps on a GPU, and without one that it fails
loudly.  tests/native/scanproject_checks.cpp is the stand-alone host program of the shared checks and the tile arithmetic."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_scanproj_project" in N.binding.EXPORTS
    exe = str(tmp_path / "scanproject_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "scanproject_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_scanproject_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_checks_and_the_tile_arithmetic_on_the_host(tmp_path):
    """the shared checks, the gate and the tile arithmetic need no HIP: a plain g++ program replays the two launches' walk over
    scans of n_beams in {1, T-1, T, T+1, 2T+1, 2^20} on heap blocks of exactly the touched size"""
    exe = str(tmp_path / "scanproject_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "scanproject_checks.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout and "12 of 12 bad parameters refused" in out.stdout


@pytest.mark.gpu
def test_scanproject_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scanproject_demo: 4 scans" in out.stdout and "4 scans equal to the C-ABI bit for bit" in out.stdout and "0 failures" in out.stdout
