"""CPU-side checks of the chip-wide optimiser's C-ABI (ndtgpu_default_pgo_wide_params, ndtgpu_pgo_wide_plan,
ndtgpu_pgo_optimize_wide): the header declares the entries and says what it must, the ctypes signatures and the struct agree
with it, the plan is pure host arithmetic, and every parameter check returns its error before the handle is read and the device
is looked for."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_pgo_wide_params", "ndtgpu_pgo_wide_plan", "ndtgpu_pgo_optimize_wide")


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndtgpu.h")).read(), flags=re.S)


def test_header_declares_the_entries(N):
    from ndt_feature_graph_amd import binding
    code = header_code()
    for fn in ENTRIES:
        assert re.search(r"\b%s\s*\(" % fn, code), fn
        assert fn in binding.EXPORTS
    assert code.index("ndtgpu_pgo_poses(") < code.index("ndtgpu_default_pgo_wide_params(")      # the section sits behind ndtgpu_pgo_poses
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("the chip-wide form of the optimiser"):text.index("ndtgpu_pgo_optimize_wide(")]
    sec = re.sub(r"\s*\n \*\s*", " ", sec)                              # (the comment's line breaks)
    for word in ("ONE PLAIN LAUNCH", "no grid barrier", "no atomics", "THREE launches", "tiles of 256", "ascending link order",
                 "same bits for every check_every", "bank's capacity", "other graphs", "run to run", "NOT the bits of ndtgpu_pgo_optimize",
                 "SYNCHRONOUS TOWARDS THE HOST", "Measured on MI355X", "tools/pgo_cost.py --wide", "linear_iterations"):
        assert word in sec, word
    assert "0.11.0" not in N.lib().ndtgpu_version().decode()          # bumped with the new entries


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_size_against_gcc_and_defaults(N, tmp_path):
    from ndt_feature_graph_amd import binding
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu\\n",'
                   ' sizeof(ndtgpu_pgo_wide_params), offsetof(ndtgpu_pgo_wide_params, check_every)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(binding.PgoWideParams), binding.PgoWideParams.check_every.offset] == [8, 0]
    assert binding.pgo_wide_params().check_every == 32 and binding.pgo_wide_params(7).check_every == 7
    N.lib().ndtgpu_default_pgo_wide_params(None)                 # (a no-op, as the other default functions)


def test_plan_is_the_tiling_of_the_graph_alone(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    assert binding.pgo_wide_plan(1, 0)[:3] == (256, 1, 0)
    assert binding.pgo_wide_plan(256, 256)[:3] == (256, 1, 1)
    assert binding.pgo_wide_plan(257, 513)[:3] == (256, 2, 3)
    assert binding.pgo_wide_plan(5000, 43509)[:3] == (256, 20, 170)
    # the extra bytes: four per-tile sums per node tile, one per link tile, and the two control blocks
    small, large = binding.pgo_wide_plan(1, 0)[3], binding.pgo_wide_plan(257, 513)[3]
    assert large - small == 8 * (4 * 1 + 3) and 0 < small - 8 * 4 <= 512
    assert binding.pgo_wide_plan(1 << 24, 1 << 27)[:3] == (256, 1 << 16, 1 << 19)
    for bad in (((1 << 24) + 1, 10), (0, 0), (10, (1 << 27) + 1)):
        assert L.ndtgpu_pgo_wide_plan(bad[0], bad[1], None, None, None, None) == -1, bad
    assert L.ndtgpu_pgo_wide_plan(10, 10, None, None, None, None) == 0       # (every out pointer may be NULL)
    import pgo_wide_graphs as WG
    assert WG.TILE == binding.pgo_wide_plan(1, 0)[0]


def test_bad_parameters_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    assert L.ndtgpu_pgo_optimize_wide(None, 0, None, None, None) == -1 and b"null handle" in L.ndtgpu_last_error()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    h = ctypes.c_void_p(1)

    def call(check_every=None, **fields):
        p, w = binding.pgo_params(**fields), binding.pgo_wide_params(check_every)
        return L.ndtgpu_pgo_optimize_wide(h, 0, ctypes.byref(p), ctypes.byref(w), None)

    assert call(check_every=0) == -1 and b"check_every" in L.ndtgpu_last_error()
    assert call(check_every=-3) == -1 and b"check_every" in L.ndtgpu_last_error()
    nan = float("nan")
    for bad in (dict(max_linear_iterations=-1), dict(max_iterations=-1), dict(eps_step=nan), dict(eps_linear=-1e-9),
                dict(prior_information=[100, 0, 0, 0, nan, 0, 0, 0, 100]), dict(prior_information=[float("inf")] + [0.0] * 8)):
        assert call(**bad) == -1 and b"bad parameter" in L.ndtgpu_last_error(), bad


def test_wide_call_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: a graph that has not been set is refused)
        bank = N.PGO(1, 10, 10)
        with pytest.raises(N.NdtGpuError) as e:
            bank.optimize_wide(0)
        assert e.value.status == -1 and "not been set" in str(e.value)
        with pytest.raises(N.NdtGpuError):
            bank.optimize_wide(1)
        bank.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO(1, 10, 10)
    assert e.value.status == -3
    from ndt_feature_graph_amd import binding
    assert binding.PGO.optimize_wide
