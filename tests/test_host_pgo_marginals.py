"""The host mirror's optimizeGraphUsingISAMWithCov and optimizeGraph3DWithCov (host/ndt_feature_graph_gpu.h) compiled with g++:
tests/native/pgo_marginals_demo.cpp optimises the 12-node graph of pgo_demo.cpp and checks on a GPU that the node poses are those of
optimizeGraphUsingISAM / optimizeGraph3D bit for bit, that every node's getCov() is the block of the C-ABI call bit for bit and that
node 0's is the prior's inverse; without a GPU that it fails loudly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    exe = str(tmp_path / "pgo_marginals_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "pgo_marginals_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pgo_marginals_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


@pytest.mark.gpu
def test_pgo_marginals_demo_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "12 nodes, 25 factors, 12 poses and 12 covariances equal bit for bit" in out.stdout
    assert "SE(3): 12 poses equal" in out.stdout and "0 failures" in out.stdout
