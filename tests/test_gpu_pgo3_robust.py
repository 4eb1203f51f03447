"""ndtgpu_pgo3_optimize_robust: robust loop-closure weighting of the SE(3) pose-graph bank on the device (-m gpu) against
tests/pgo_robust_model.py.  The checks are those of tests/pgo_robust_checks.py, shared with the SE(2) bank.

Tolerances.  Weights and flags: the model's functions of the device's own chi2, bit for bit.  chi2: the carried bound of
tests/pgo_robust_bounds.py, bound 1.  Poses and robust cost against the model's dense IRLS: ten times the floors
pgo_robust_model.ROBUST3_FLOOR (2.3e-15) and ROBUST3_COST_FLOOR (7.2e-16), which tests/test_pgo_robust_model.py::test_floor measures
on the CPU between the dense and the conjugate-gradient IRLS.  Two device runs are compared bit for bit."""
import numpy as np
import pytest

import pgo3_model as M
import pgo_robust_checks as C
import pgo_robust_model as R

pytestmark = pytest.mark.gpu
DOF = 6


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


@pytest.mark.parametrize("n_edges", C.EDGES)
def test_evaluate_only(N, n_edges):
    C.check_evaluate_only(N, DOF, n_edges)


def test_protected_links_and_restore(N):
    C.check_protected_and_restore(N, DOF)


def test_reduces_to_the_plain_optimiser(N):
    C.check_reduces_to_plain(N, DOF)


@pytest.mark.parametrize("kind", ["dcs", "cauchy", "huber"])
def test_outlier_graph(N, kind):
    C.check_outlier_graph(N, DOF, "grid3d", kind)


def test_batch_and_rerun(N):
    C.check_batch_and_rerun(N, DOF)


def test_wide_same_bits_for_every_check_every(N):
    C.check_wide(N, DOF)


def test_nan_measurement_ends_not_finite(N):
    G = C.batch_graphs(DOF)[3]
    meas = G.meas.copy()
    meas[5, 1, 3] = np.nan
    C.check_bad_graph(N, DOF, M.Graph(G.poses, G.ref, G.mov, meas), R.NOT_FINITE)


def test_exact_half_turn_ends_half_turn(N):
    G = M.chain(4)
    Z = G.meas.copy()
    Z[1] = Z[1] @ M.make_T(np.diag([1.0, -1.0, -1.0]), np.zeros(3))
    C.check_bad_graph(N, DOF, M.Graph(G.poses, G.ref, G.mov, Z), R.HALF_TURN)


def test_live_resources(N):
    C.check_live_resources(N, DOF)
