"""csrc/ndt_block.h checked directly: tests/native/block_checks.hip includes the header alone, runs every operation in
workgroups of 256 and 1024 threads and compares by bits with the order restated on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "block_checks.hip")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = str(tmp_path_factory.mktemp("block") / "block_checks")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", SRC, "-o", out])
    return out


def test_block_header_stands_alone(exe):
    """The program -- the header, kernels of its own and the HIP runtime, nothing else -- cross-compiles for gfx950."""
    assert os.path.getsize(exe) > 0


@pytest.mark.gpu
def test_block_checks_on_gpu(exe):
    out = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failures" in out.stdout
