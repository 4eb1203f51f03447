"""binding.optimize_gated with robust= on the device (-m gpu), on the 30-node loop of the link gate's tests: robust=None is the
path as it was, call for call -- the bits of a call that does not name the keyword --, and robust={...} optimises every round
with PGO.optimize_robust: replayed by hand from the kept lists it returns, the same bits."""
import numpy as np
import pytest

import linkgate_fixtures as F
import pgo_robust_model as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


def cm(T):
    """[m, 4, 4] -> [m, 16] column-major"""
    return np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4), (0, 2, 1))).reshape(-1, 16)


def test_optimize_gated_robust(N):
    import torch
    g = F.loop_graph()
    n, k, m = len(g["start"]), len(g["incr_ref"]), len(g["ref"])
    T16 = cm(g["T"])
    T16_dev, score_dev = torch.tensor(T16, device="cuda"), torch.tensor(g["score"], device="cuda")
    incr_dev = torch.tensor(cm(g["incr_T"]), device="cuda")

    def gated(**kw):
        gate, bank = N.LinkGate(n, m), N.PGO(2, n, k + m)
        rounds, poses = N.optimize_gated(bank, 0, gate, g["start"], g["incr_ref"], g["incr_mov"], incr_dev, g["ref"], g["mov"], T16_dev,
                                         score_dev, max_rounds=8, **kw)
        gate.close()
        return bank, rounds, poses

    # robust=None: the path as it was
    bank, rounds0, poses0 = gated()
    bank.close()
    bank, rounds1, poses1 = gated(robust=None)
    bank.close()
    assert len(rounds0) == len(rounds1) and all(np.array_equal(a, b) for a, b in zip(rounds0, rounds1))
    assert poses0.tobytes() == poses1.tobytes()

    # robust: every round is PGO.optimize_robust on incremental + kept links from the poses so far
    robust = dict(kind="cauchy", scale=2.0, max_rounds=20)
    bank, rounds, poses = gated(robust=robust)
    chi2, w, inl, res = bank.robust_links(0)
    assert len(rounds) >= 1 and rounds[-1].size > 0
    assert w.shape == (k + rounds[-1].size,) and np.all(w[:k] == 1.0)        # (the incremental links are never re-weighted)
    assert np.all((w > 0.0) & (w <= 1.0)) and np.any(w[k:] < 1.0) and res["rounds"] >= 1
    assert w.tobytes() == np.where(np.arange(w.size) < k, 1.0, R.weights("cauchy", 2.0, chi2)).tobytes()
    p = np.array(g["start"], dtype=np.float64)
    for kept in rounds:
        if kept.size == 0:
            break
        T_h = torch.tensor(np.concatenate([cm(g["incr_T"]), T16[kept]]), device="cuda")
        bank.set_links_device(1, p, np.concatenate([g["incr_ref"], g["ref"][kept]]), np.concatenate([g["incr_mov"], g["mov"][kept]]), T_h)
        bank.optimize_robust(1, 1, robust=robust)
        p = bank.poses(1)[0][:n].copy()
    assert p.tobytes() == poses.tobytes()
    assert bank.robust_links(1)[1].tobytes() == w.tobytes()
    bank.close()
    assert poses.tobytes() != poses0.tobytes()
