"""The host mirror's link gate (host/ndt_link_gate_gpu.h: computeCandidateLinks, getValidLinksGPU, optimizeGraphGated) compiled with
g++: tests/native/linkgate_demo.cpp runs them against the scalar NDTFeatureGraph::getValidLinks, the pair loop with
distanceBetweenAffine3d and the offline mapper's loop written out with them on a GPU, and without one checks that they fail loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    exe = str(tmp_path / "linkgate_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "linkgate_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_linkgate_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


@pytest.mark.gpu
def test_linkgate_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linkgate_demo: " in out.stdout and "30 of 30 nodes equal to the scalar loop bit for bit, 0 failures" in out.stdout
