"""CPU-side checks of the robust weighting's C-ABI (ndtgpu_pgo_optimize_robust, ndtgpu_pgo3_optimize_robust, the _robust_links,
_robust_links_device and _robust_restore entries, ndtgpu_pgo_robust_weight): the header declares the entries and names what it
restates, the ctypes signatures and structs agree with it, the defaults, the host form of the weights against the model bit for
bit, and every parameter check returns NDTGPU_ERR_INVALID before the handle is read and the device is looked for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pgo_robust_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_pgo_robust_params", "ndtgpu_pgo_robust_weight", "ndtgpu_pgo_optimize_robust", "ndtgpu_pgo3_optimize_robust",
           "ndtgpu_pgo_robust_links", "ndtgpu_pgo3_robust_links", "ndtgpu_pgo_robust_links_device", "ndtgpu_pgo3_robust_links_device",
           "ndtgpu_pgo_robust_restore", "ndtgpu_pgo3_robust_restore", "ndtgpu_pgo_link_information", "ndtgpu_pgo3_link_information")


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


def header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndtgpu.h")).read(), flags=re.S)


def test_header_declares_the_entries_and_names_what_it_restates(N):
    from ndt_feature_graph_amd import binding
    code = header_code()
    for fn in ENTRIES:
        assert re.search(r"\b%s\s*\(" % fn, code), fn
        assert fn in binding.EXPORTS
        assert getattr(N.lib(), fn)
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("robust loop-closure weighting of the pose-graph banks"):text.index("ndtgpu_pgo3_robust_restore(")]
    sec = re.sub(r"\s*\n \*\s*", " ", sec)
    for word in ("PROVENANCE", "DEVIATIONS", "have NO robust cost", "restated from memory", "FREEZES THE WEIGHTS WITHIN A ROUND", "OURS",
                 "Huber(k)", "Cauchy(c)", "DCS(Phi)", "min_index_gap", "never re-weighted", "as the graph was set".upper(), "THE BANK IS LEFT WEIGHTED",
                 "No atomics", "no grid barrier", "same bits", "run to run", "NOT BUILT", "switchable constraints", "covariance-aware",
                 "tools/pgo_robust_cost.py", "ndt_pgo_robust_weigh_kernel", "ndt_pgo3_robust_finish_kernel"):
        assert word in sec, word
    assert N.lib().ndtgpu_version().decode().startswith("ndtgpu 0.13.0")      # (no version bump with this section)


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
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n",'
                   ' sizeof(ndtgpu_pgo_robust_params), offsetof(ndtgpu_pgo_robust_params, scale), offsetof(ndtgpu_pgo_robust_params, inlier_weight),'
                   ' sizeof(ndtgpu_pgo_robust_result), offsetof(ndtgpu_pgo_robust_result, cost_initial), offsetof(ndtgpu_pgo_robust_result, outliers),'
                   ' NDTGPU_PGO_ROBUST_HUBER, NDTGPU_PGO_ROBUST_CAUCHY, NDTGPU_PGO_ROBUST_DCS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, Q = binding.PgoRobustParams, binding.PgoRobustResult
    assert got[:6] == [ctypes.sizeof(P), P.scale.offset, P.inlier_weight.offset, ctypes.sizeof(Q), Q.cost_initial.offset, Q.outliers.offset]
    assert got[:6] == [32, 16, 24, 48, 16, 40]
    assert got[6:] == [binding.PGO_ROBUST_HUBER, binding.PGO_ROBUST_CAUCHY, binding.PGO_ROBUST_DCS] == [R.HUBER, R.CAUCHY, R.DCS] == [1, 2, 3]
    p = binding.pgo_robust_params()
    assert {k: getattr(p, k) for k, _ in P._fields_} == R.ROBUST_DEFAULTS
    assert binding.pgo_robust_params(kind="huber", scale=2.5).kind == 1 and binding.pgo_robust_params(kind="cauchy").kind == 2
    assert binding.PGO_MAX_ROUNDS == binding.PGO_MAX_ITERATIONS == R.MAX_ROUNDS
    N.lib().ndtgpu_default_pgo_robust_params(None)               # (a no-op, as the other default functions)


def test_host_weights_are_the_models_bits(N):
    rng = np.random.default_rng(5)
    chi2 = np.concatenate([[0.0, 1.0, 4.0, 1e-300, 1e300, np.inf], 10.0 ** rng.uniform(-8, 8, size=400)])
    for kind in ("huber", "cauchy", "dcs"):
        for scale in (0.3, 1.0, 7.5):
            got, want = N.pgo_robust_weight(kind, scale, chi2), R.weights(kind, scale, chi2)
            assert got.tobytes() == want.tobytes(), (kind, scale)
        assert np.isnan(N.pgo_robust_weight(kind, 1.0, np.nan))
    w = ctypes.c_double()
    for bad in ((0, 1.0), (4, 1.0), (1, 0.0), (1, -1.0), (3, float("nan")), (2, float("inf"))):
        assert N.lib().ndtgpu_pgo_robust_weight(bad[0], bad[1], 1.0, ctypes.byref(w)) == -1, bad
    assert N.lib().ndtgpu_pgo_robust_weight(1, 1.0, 1.0, None) == -1


@pytest.mark.parametrize("bank", ["pgo", "pgo3"])
def test_bad_parameters_are_refused_before_the_device_is_looked_for(N, bank):
    from ndt_feature_graph_amd import binding
    L = N.lib()
    fn = getattr(L, "ndtgpu_%s_optimize_robust" % bank)
    params = binding.pgo_params if bank == "pgo" else binding.pgo3_params
    h = ctypes.c_void_p(1)            # (a placeholder: every check below fails before the handle is read)
    nan, inf = float("nan"), float("inf")

    def call(count=1, wide=None, pgo=None, **fields):
        rp = binding.PgoRobustParams()
        L.ndtgpu_default_pgo_robust_params(ctypes.byref(rp))
        for k, v in fields.items():
            setattr(rp, k, v)
        p = params(**(pgo or {}))
        w = None if wide is None else ctypes.byref(binding.pgo_wide_params(wide))
        return fn(h, 0, count, ctypes.byref(p), ctypes.byref(rp), w, None)

    for bad in (dict(kind=0), dict(kind=4), dict(kind=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf),
                dict(max_rounds=-1), dict(updates_per_round=0), dict(updates_per_round=-3), dict(min_index_gap=0), dict(min_index_gap=-2),
                dict(inlier_weight=-0.1), dict(inlier_weight=1.5), dict(inlier_weight=nan)):
        assert call(**bad) == -1 and b"bad robust parameter" in L.ndtgpu_last_error(), bad
    # the optimiser's own checks, and the wide form's
    assert call(pgo=dict(eps_step=-1.0)) == -1 and call(pgo=dict(max_linear_iterations=-1)) == -1
    assert call(wide=0) == -1 and b"check_every" in L.ndtgpu_last_error()
    assert call(count=2, wide=32) == -1 and b"count == 1" in L.ndtgpu_last_error()
    rp = binding.pgo_robust_params()
    assert fn(None, 0, 1, None, ctypes.byref(rp), None, None) == -1 and b"null handle" in L.ndtgpu_last_error()
    for name in ("robust_links", "robust_restore"):
        e = getattr(L, "ndtgpu_%s_%s" % (bank, name))
        assert (e(None, 0, None, None, None, None) if name == "robust_links" else e(None, 0)) == -1
    assert getattr(L, "ndtgpu_%s_robust_links_device" % bank)(None, 0, None, None, None) == -1


def test_robust_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    for cls in (binding.PGO, binding.PGO3):
        assert cls.optimize_robust and cls.robust_links and cls.robust_restore
    if N.device_count() > 0:
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.PGO(1, 10, 10)
    assert e.value.status == -3
