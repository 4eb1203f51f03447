"""The host mirror's optimizeGraphUsingISAMRobust and optimizeGraph3DRobust (host/ndt_feature_graph_gpu.h) compiled with g++:
tests/native/pgo_robust_demo.cpp calls them on a loop of 12 nodes with one false loop closure and checks the node poses and the
link weights bit for bit against the ndtgpu_pgo_optimize_robust / ndtgpu_pgo3_optimize_robust calls they wrap on a GPU, and
without one that it fails loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    exe = str(tmp_path / "pgo_robust_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "pgo_robust_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pgo_robust_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


@pytest.mark.gpu
def test_pgo_robust_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pgo_robust_demo: 12 nodes, 14 links, SE(2) 12 and SE(3) 12 equal to the C-ABI bit for bit" in out.stdout and "0 failures" in out.stdout
