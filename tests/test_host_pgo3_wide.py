"""The host mirror's optimizeGraph3D(..., wide) (host/ndt_feature_graph_gpu.h) compiled with g++: tests/native/pgo3_wide_demo.cpp
calls both forms on the hub graph of tests/pgo3_wide_graphs.py (588 nodes in three node tiles, 1817 links in eight link tiles,
written to a file here) and checks on a GPU that wide = true gives the poses of ndtgpu_pgo3_optimize_wide bit for bit and agrees
with wide = false within twice the graph's tolerance (each form sits within one tolerance of the model), and without a GPU that
it fails loudly."""
import os
import subprocess

import numpy as np
import pytest

import pgo3_wide_graphs as WG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ndt_feature_graph_amd")


def _build(tmp_path):
    import ndt_feature_graph_amd as N
    N.build_library()
    exe = str(tmp_path / "pgo3_wide_demo")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(PKG, "host"),
                           os.path.join(ROOT, "tests", "native", "pgo3_wide_demo.cpp"), "-o", exe, "-L", PKG, "-lndtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _command(tmp_path):
    """the demo on the hub graph (every link at 100 * I6, as the model has it), with twice its tolerance"""
    G = WG.hub_graph()
    assert G.info is None
    cm = lambda T: " ".join("%.17g" % v for v in np.asarray(T).T.reshape(16))         # column-major; 17 digits read back exactly
    path = str(tmp_path / "hub.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (G.n_nodes, G.n_edges))
        for T in G.poses:
            f.write(cm(T) + "\n")
        for a, b, Z in zip(G.ref, G.mov, G.meas):
            f.write("%d %d %s\n" % (a, b, cm(Z)))
    tol, cost_rtol = WG.tolerance("hub")
    return [_build(tmp_path), path, "%.17g" % (2 * tol), "%.17g" % (2 * cost_rtol)]


def test_pgo3_wide_demo_fails_loudly_without_a_device(tmp_path):
    import ndt_feature_graph_amd as N
    out = subprocess.run(_command(tmp_path), capture_output=True, text=True, timeout=300)
    if N.device_count() > 0:                  # (a box with a device: the demo's checks pass)
        assert out.returncode == 0, out.stdout + out.stderr
        return
    assert out.returncode == 3, out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout


@pytest.mark.gpu
def test_pgo3_wide_demo_on_gpu(tmp_path):
    out = subprocess.run(_command(tmp_path), capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pgo3_wide_demo: 588 nodes (3 tiles), 1817 factors (8 tiles), 588 equal to the C-ABI bit for bit" in out.stdout
    assert "0 failures" in out.stdout
