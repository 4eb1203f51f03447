"""CPU-side checks of the SE(3) chip-wide optimiser's C-ABI (ndtgpu_pgo3_wide_plan, ndtgpu_pgo3_optimize_wide): the header
declares the entries behind ndtgpu_pgo3_link_from_registration and its section says what it must, the ctypes signatures agree
with it, the plan is pure host arithmetic over n_edges + 1 link items (the prior is the link behind the last), and every
parameter check returns its error before the handle is read and the device is looked for."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_pgo3_wide_plan", "ndtgpu_pgo3_optimize_wide")


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
        assert code.index("ndtgpu_pgo3_link_from_registration(") < code.index(fn + "("), fn      # the section sits behind the SE(3) one
    assert code.index("ndtgpu_pgo3_wide_plan(") < code.index("ndtgpu_world_assemble(")
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    assert text.count("SE(3) pose-graph optimisation") == 1                 # (tests/test_pgo3_abi.py cuts its section at this phrase)
    sec = text[text.index("the chip-wide form of the SE(3) optimiser"):text.index("ndtgpu_pgo3_optimize_wide(")]
    sec = re.sub(r"\s*\n \*\s*", " ", sec)                              # (the comment's line breaks)
    for word in ("ONE PLAIN LAUNCH", "no grid barrier", "no cooperative launch", "no spin on memory", "no atomics", "no captured graph",
                 "THREE launches", "tiles of 256", "ascending link order", "n_edges + 1", "is never 0",
                 "same bits for every check_every", "bank's capacity", "other graphs", "run to run", "NOT the bits of ndtgpu_pgo3_optimize",
                 "SYNCHRONOUS TOWARDS THE HOST", "linear_iterations", "NDTGPU_PGO3_HALF_TURN", "NDTGPU_PGO_NOT_FINITE", "NDTGPU_PGO_LINEAR_CAP",
                 "Two more device buffers", "ndtgpu_pgo3_destroy", "Measured on MI355X", "tools/pgo3_cost.py --wide",
                 "tools/kernel_resources.py pgo3_wide", "no scratch", "csrc/ndt_pgo_wide_core.h"):
        assert word in sec, word
    assert "is the follow-up" not in text
    assert b"0.13.0" in N.lib().ndtgpu_version()                       # (new entries beside the old ones: not bumped)


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_plan_is_the_tiling_of_the_graph_alone(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    assert N.pgo3_wide_plan is binding.pgo3_wide_plan
    assert binding.pgo3_wide_plan(1, 0)[:3] == (256, 1, 1)               # (no links: the prior alone is a link tile)
    assert binding.pgo3_wide_plan(256, 255)[:3] == (256, 1, 1)
    assert binding.pgo3_wide_plan(257, 256)[:3] == (256, 2, 2)           # (the second link tile holds the prior alone)
    assert binding.pgo3_wide_plan(5000, 43509)[:3] == (256, 20, 170)
    # the extra bytes: 8 per per-tile sum -- four per node tile (r.z, r.r, p.Ap, the largest |x|), two per link tile (the cost,
    # the half turns) -- and the two control blocks
    small, large = binding.pgo3_wide_plan(1, 0)[3], binding.pgo3_wide_plan(257, 512)[3]
    assert large - small == 8 * (4 * 1 + 2 * 2) and 0 < small - 8 * (4 + 2) <= 512
    assert binding.pgo3_wide_plan(256, 256)[3] - binding.pgo3_wide_plan(256, 255)[3] == 8 * 2
    assert binding.pgo3_wide_plan(257, 255)[3] - binding.pgo3_wide_plan(256, 255)[3] == 8 * 4
    assert binding.pgo3_wide_plan(1 << 24, 1 << 27)[:3] == (256, 1 << 16, (1 << 19) + 1)
    for bad in (((1 << 24) + 1, 10), (0, 0), (10, (1 << 27) + 1)):      # the limits of ndtgpu_pgo3_create
        assert L.ndtgpu_pgo3_wide_plan(bad[0], bad[1], None, None, None, None) == -1, bad
        assert b"pgo3_wide_plan" in L.ndtgpu_last_error()
    assert L.ndtgpu_pgo3_wide_plan(10, 10, None, None, None, None) == 0      # (every out pointer may be NULL)
    import pgo3_wide_graphs as WG
    assert WG.TILE == binding.pgo3_wide_plan(1, 0)[0]
    for n, m in ((1, 0), (256, 255), (257, 256), (588, 1817)):
        assert binding.pgo3_wide_plan(n, m)[1:3] == (WG.tiles(n), WG.link_tiles(m))


def test_bad_parameters_are_refused_before_the_device_is_looked_for(N):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    assert L.ndtgpu_pgo3_optimize_wide(None, 0, None, None, None) == -1 and b"null handle" in L.ndtgpu_last_error()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    h = ctypes.c_void_p(1)

    def call(check_every=None, **fields):
        p, w = binding.pgo3_params(**fields), binding.pgo_wide_params(check_every)
        return L.ndtgpu_pgo3_optimize_wide(h, 0, ctypes.byref(p), ctypes.byref(w), None)

    assert call(check_every=0) == -1 and b"check_every" in L.ndtgpu_last_error()
    assert call(check_every=-3) == -1 and b"check_every" in L.ndtgpu_last_error()
    nan = float("nan")
    eye = [100.0 if k % 7 == 0 else 0.0 for k in range(36)]
    for bad in (dict(max_linear_iterations=-1), dict(max_iterations=-1), dict(eps_step=nan), dict(eps_step=-1e-9), dict(eps_linear=-1e-9),
                dict(eps_linear=nan), dict(prior_information=eye[:14] + [nan] + eye[15:]), dict(prior_information=[float("inf")] + eye[1:])):
        assert call(**bad) == -1 and b"bad parameter" in L.ndtgpu_last_error(), bad
        assert b"pgo3_optimize_wide" in L.ndtgpu_last_error()


def test_wide_call_fails_loudly_without_a_device(N):
    if N.device_count() > 0:                 # (a box with a device: a graph that has not been set, or is out of range, is refused)
        bank = N.PGO3(1, 10, 10)
        with pytest.raises(N.NdtGpuError) as e:
            bank.optimize_wide(0)
        assert e.value.status == -1 and "not been set" in str(e.value)
        with pytest.raises(N.NdtGpuError) as e:
            bank.optimize_wide(1)
        assert e.value.status == -1
        bank.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO3(1, 10, 10)
    assert e.value.status == -3
    from ndt_feature_graph_amd import binding
    assert binding.PGO3.optimize_wide
