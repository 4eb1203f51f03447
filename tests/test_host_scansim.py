"""The host mirror's scan simulation (host/ndt_scan_simulator_gpu.h: simulateRangeScanGPU, generateRefScansGPU, ScanSimulatorGPU)
compiled with g++: tests/native/scansim_demo.cpp simulates scans and generates reference scans the way the reference's node does and
checks them on a GPU, and without one that it fails loudly.  tests/native/scansim_checks.cpp is the stand-alone host program of the
shared header, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_scansim_simulate" in N.binding.EXPORTS
    exe = str(tmp_path / "scansim_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "scansim_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_scansim_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_shared_header_on_the_host_under_the_sanitizers(tmp_path):
    """the reach, the cell of a point, the closed form of a step against the walk's accumulator, walks from every cell of small
    grids, the lattice's positions, the headings and the checks need no HIP: a plain g++ program with its own main, built with
    -fsanitize=address,undefined, works in heap blocks of exactly the size a call may touch"""
    exe = str(tmp_path / "scansim_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "scansim_checks.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failures" in out.stdout and "6561 rays" in out.stdout and "33 of 33 bad arguments refused" in out.stdout


@pytest.mark.gpu
def test_scansim_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scansim_demo: ranges 1.500 1.000 0.750, unknown free 1.500, 120 reference scans (skip 9), 0 failures" in out.stdout
