"""CPU-side checks of the marginal covariances' C-ABI (ndtgpu_pgo_marginal_plan, ndtgpu_pgo_marginals, ndtgpu_pgo3_marginals, their
_device forms, ndtgpu_pgo_relative_covariance, ndtgpu_pgo3_relative_covariance): the header declares the entries and says what it
must, the ctypes signatures and structs agree with it, the plan and the relative covariances are pure host arithmetic, and every
check of the outputs and parameters returns its error before the handle is read and the device is looked for.  (The checks of a
query's graph and node indices read the handle: tests/test_gpu_pgo_marginals.py::test_bad_queries_are_refused.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pgo3_model as M3
import pgo_marginals_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_pgo_marginal_params", "ndtgpu_pgo_marginal_plan", "ndtgpu_pgo_marginals", "ndtgpu_pgo_marginals_device",
           "ndtgpu_pgo3_marginals", "ndtgpu_pgo3_marginals_device", "ndtgpu_pgo_relative_covariance", "ndtgpu_pgo3_relative_covariance")


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
        assert getattr(N.lib(), fn)                       # every new symbol is exported
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("Marginal covariances of the pose-graph banks"):text.index("ndtgpu_pgo3_relative_covariance(")]
    sec = re.sub(r"\s*\n \*\s*", " ", sec)                              # (the comment's line breaks)
    for word in ("PROVENANCE", "DEVIATIONS", "never asks iSAM for covariances", "IN THE GRAPH'S FRAME", "OWN TANGENT FRAME",
                 "HAS TO BE THE ONE THE GRAPH WAS OPTIMISED WITH", "three plain launches", "no atomics", "no grid barrier",
                 "same bits", "run to run", "NOT BUILT", "chip-wide form", "covariance-aware link gate", "covariance markers",
                 "into the world frame", "Measured on MI355X", "tools/pgo_marginals_cost.py", "OURS"):
        assert word in sec, word
    assert N.lib().ndtgpu_version().decode().startswith("ndtgpu 0.13.0")


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn


def test_struct_sizes_against_gcc_and_defaults(N, tmp_path):
    from ndt_feature_graph_amd import binding
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   ' sizeof(ndtgpu_pgo_marginal_params), sizeof(ndtgpu_pgo_marginal_result), offsetof(ndtgpu_pgo_marginal_result, capped_columns),'
                   ' offsetof(ndtgpu_pgo_marginal_result, asymmetry)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = binding.PgoMarginalResult
    assert got == [ctypes.sizeof(binding.PgoMarginalParams), ctypes.sizeof(R), R.capped_columns.offset, R.asymmetry.offset] == [8, 24, 12, 16]
    assert binding.PGO_MARGINAL_RESULT.itemsize == 24 and binding.PGO_MARGINAL_RESULT.fields["asymmetry"][1] == 16
    assert binding.pgo_marginal_params().max_workspace_bytes == 1 << 30 and binding.pgo_marginal_params(7).max_workspace_bytes == 7
    N.lib().ndtgpu_default_pgo_marginal_params(None)             # (a no-op, as the other default functions)


@pytest.mark.parametrize("dof", [3, 6])
def test_plan(N, dof):
    """slots >= 1; slots * slot_bytes <= the budget unless slots == 1; launches = ceil(n_queries * dof / slots)"""
    L = N.lib()
    for nodes, edges, queries, budget in ((8, 8, 8, 1), (8, 8, 8, 10_000), (500, 1886, 500, 1 << 20), (500, 1886, 500, 1 << 30),
                                          (1122, 2561, 4, 1 << 40), (1 << 24, 1 << 27, 3, 1 << 30), (5, 0, 1, 0)):
        slot, slots, launches = N.pgo_marginal_plan(nodes, edges, queries, dof, budget)
        per_node, per_edge = (18, 3) if dof == 3 else (36, 6)
        assert slot == 8 * (per_node * nodes + per_edge * (edges + (dof == 6)))
        assert 1 <= slots <= queries * dof
        assert slots * slot <= budget or slots == 1
        assert slots == queries * dof or (slots + 1) * slot > budget          # (no slot the budget has room for is left out)
        assert launches == -(-queries * dof // slots)
    assert N.pgo_marginal_plan(8, 8, 8, dof, 1)[1] == 1                      # a tiny budget: one slot
    assert N.pgo_marginal_plan(500, 1886, 500, dof)[1:] == (500 * dof, 1)    # the default budget: every column of the 500-node graph at once
    for bad in ((0, 0, 1), ((1 << 24) + 1, 10, 1), (10, (1 << 27) + 1, 1), (10, 10, (1 << 27) + 1)):
        assert L.ndtgpu_pgo_marginal_plan(bad[0], bad[1], bad[2], dof, 1 << 30, None, None, None) == -1, bad
    assert L.ndtgpu_pgo_marginal_plan(10, 10, 10, dof, 1 << 30, None, None, None) == 0     # (every out pointer may be NULL)


def test_plan_refuses_another_dof(N):
    for dof in (4, 0, -3, 9):
        assert N.lib().ndtgpu_pgo_marginal_plan(10, 10, 10, dof, 1 << 30, None, None, None) == -1 and b"dof" in N.lib().ndtgpu_last_error()


def test_relative_covariance_se2_bit_for_bit(N):
    rng = np.random.default_rng(3)
    for _ in range(20):
        A = rng.normal(size=(6, 6))
        S = A @ A.T * 0.01
        pr, pm = rng.uniform(-3, 3, size=3), rng.uniform(-3, 3, size=3)
        got = N.pgo_relative_covariance(pr, pm, S[:3, :3], S[3:, 3:], S[3:, :3])
        want = MM.relative_covariance(pr, pm, S[:3, :3], S[3:, 3:], S[3:, :3])
        assert got.tobytes() == want.tobytes()
    assert N.lib().ndtgpu_pgo_relative_covariance(None, None, None, None, None, None) == -1


def test_relative_covariance_se3_against_the_model(N):
    """Not bit for bit: the library forms Z = T_ref^-1 T_mov and the error's Jacobians with its own 3x3 products and libm's atan2,
    NumPy with BLAS and its own; the Jacobians' entries differ by a few units in the last place, and an entry of J S J^T is a
    sum of 144 products of them.  Held to 64 units in the last place of the result's largest entry."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(20):
        A = rng.normal(size=(12, 12))
        S = A @ A.T * 0.01
        Tr, Tm = M3._rand_T(rng, 3.0), M3._rand_T(rng, 3.0)
        got = N.pgo3_relative_covariance(Tr, Tm, S[:6, :6], S[6:, 6:], S[6:, :6])
        want = MM.relative_covariance3(Tr, Tm, S[:6, :6], S[6:, 6:], S[6:, :6])
        worst = max(worst, float(np.max(np.abs(got - want)) / np.spacing(np.max(np.abs(want)))))
    print("pgo3_relative_covariance against the model: %.1f units in the last place of the largest entry" % worst)
    assert worst <= 64
    assert N.lib().ndtgpu_pgo3_relative_covariance(None, None, None, None, None, None) == -1


@pytest.mark.parametrize("bank", ["pgo", "pgo3"])
def test_bad_arguments_are_refused_before_the_device_is_looked_for(N, bank):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    d = 3 if bank == "pgo" else 6
    host, dev = getattr(L, "ndtgpu_%s_marginals" % bank), getattr(L, "ndtgpu_%s_marginals_device" % bank)
    params = binding.pgo_params if bank == "pgo" else binding.pgo3_params
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    h = ctypes.c_void_p(1)
    idx = (ctypes.c_uint32 * 2)(0, 0)
    cov, cross = (ctypes.c_double * (2 * d * d))(), (ctypes.c_double * (2 * d * d))()
    res = (binding.PgoMarginalResult * 2)()
    dp = ctypes.POINTER(ctypes.c_double)
    as_dp = lambda a: ctypes.cast(a, dp)

    def call_host(n=2, g=idx, q=idx, o=None, c=cov, x=None, r=res, **fields):
        p = params(**fields)
        return host(h, n, g, q, o, ctypes.byref(p), None, None if c is None else as_dp(c), None if x is None else as_dp(x), r)

    def call_dev(n=2, g=idx, q=idx, o=None, c=cov, x=None, r=res, **fields):
        p = params(**fields)
        vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)
        return dev(h, n, g, q, o, ctypes.byref(p), None, vp(c), vp(x), vp(r), None)

    nan, inf = float("nan"), float("inf")
    for call in (call_host, call_dev):
        for bad, word in ((dict(c=None), b"NULL output"), (dict(r=None), b"NULL output"), (dict(o=idx, x=None), b"NULL output"),
                          (dict(n=0), b"n_queries"), (dict(g=None), b"graph_idx"), (dict(q=None), b"graph_idx"),
                          (dict(eps_linear=0.0), b"eps_linear"), (dict(eps_linear=-1e-9), b"eps_linear"), (dict(eps_linear=nan), b"eps_linear"),
                          (dict(eps_linear=inf), b"eps_linear"), (dict(max_linear_iterations=0), b"max_linear_iterations"),
                          (dict(max_linear_iterations=-5), b"max_linear_iterations"),
                          (dict(prior_information=[nan] + [0.0] * (d * d - 1)), b"prior_information")):
            assert call(**bad) == -1 and word in L.ndtgpu_last_error(), (call.__name__, bad)
    assert host(None, 2, idx, idx, None, None, None, as_dp(cov), None, res) == -1 and b"null handle" in L.ndtgpu_last_error()
    assert dev(None, 2, idx, idx, None, None, None, ctypes.cast(cov, ctypes.c_void_p), None, ctypes.cast(res, ctypes.c_void_p), None) == -1
    assert b"null handle" in L.ndtgpu_last_error()


def test_marginals_fail_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    assert binding.PGO.marginals and binding.PGO.marginals_device and binding.PGO3.marginals and binding.PGO3.marginals_device
    if N.device_count() > 0:
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO(1, 10, 10)
    assert e.value.status == -3
