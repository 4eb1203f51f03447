"""The host mirror's feature path (host/ndt_feature_graph_gpu.h: NDTFeatureFuserHMT / NDTFeatureGraph initialize and update with
interest points, getFeatureMap, matchNodesUsingFeatureMap) compiled with g++: tests/native/fuser_feat_demo.cpp runs an initialize and
three updates through the overloads against the same sequence through the C-ABI, bit for bit, reads a feature map back, and matches
two nodes' feature maps on the device; without a GPU it fails loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    assert "ndtgpu_fuser_update_batch_feat_host" in N.binding.EXPORTS
    exe = str(tmp_path / "fuser_feat_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "fuser_feat_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_fuser_feat_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


def test_the_mirror_says_what_is_wired():
    text = open(os.path.join(PKG, "host", "ndt_feature_map_gpu.h")).read()
    assert "NOT WIRED" not in text.replace("NOT WIRED: NDTFeatureGraph::computeLink", "")
    graph = open(os.path.join(PKG, "host", "ndt_feature_graph_gpu.h")).read()
    assert "struct InterestPointVec {};" in graph                      # the placeholder overloads stay
    for name in ("matchNodesUsingFeatureMap", "getFeatureMap", "attachFeatures", "InterestPointGPUVec"):
        assert name in graph, name


@pytest.mark.gpu
def test_fuser_feat_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fuser_feat_demo: 4 of 4 calls equal to the C-ABI bit for bit, 3 RANSAC records OK, 1 node match equal, 0 failures" in out.stdout
