"""The carried bound of a link's chi2 = e^T W e, restated from tests/test_pgo_direct.py (check_graph2 / check_graph3, "te and cost /
their carried bounds"), vectorised over a graph's links: the unit in which tests/test_gpu_pgo_robust.py and
tests/test_gpu_pgo3_robust.py hold the device's chi2 against the model's, bound 1.

u = 2^-52.  The link bodies do not return e, so its error is bounded per component (be) and carried through W:
  SE(2): be = 8 u max(1, |dx|, |dy|) for all three components; a product's own rounding 32 u |W_ij e_j|
  SE(3): be = 16 u scale for the translation, 16 u amp for the rotation vector -- scale = max(1, |t| of the two poses and of Z),
         amp = theta / sin(theta) of the residual rotation (1 where it is tiny) --; a product's own rounding 8 u |W_ij e_j|
  tb_i = sum_j |W_ij| be_j + c u |W_ij e_j|                                   (the bound of te = W e)
  cb   = sum_i |e_i| tb_i + |te_i| be_i + c u |e_i te_i|                      (the bound of e^T W e)
test_pgo_direct.py measures the device at 0.023 (SE(2)) and 0.035 (SE(3)) of cb against mpmath; the NumPy model's own error is of
the same size, so the two sit within cb of each other."""
import numpy as np

import pgo3_model as M3
import pgo_model as M2

U = 2.0 ** -52


def _carry(e, W, be, c):
    aW = np.abs(W)
    te = np.einsum("mab,mb->ma", W, e)
    tb = np.einsum("mab,mb->ma", aW, be) + c * U * np.einsum("mab,mb->ma", aW, np.abs(e))
    return np.sum(np.abs(e) * tb + np.abs(te) * be + c * U * np.abs(e * te), axis=1)


def chi2_bound2(G, P, W):
    """[m]: the bound of every link's chi2 at the poses P [n, 3], W [m, 3, 3]"""
    pi, pj = P[G.ref], P[G.mov]
    m = np.maximum(1.0, np.maximum(np.abs(pj[:, 0] - pi[:, 0]), np.abs(pj[:, 1] - pi[:, 1])))
    e = M2.link_error(pi, pj, G.meas)
    return _carry(e, W, np.repeat((8 * U * m)[:, None], 3, axis=1), 32)


def chi2_bound3(G, P, W):
    """[m]: the same at the poses P [n, 4, 4], W [m, 6, 6]"""
    Ti, Tj, Z = P[G.ref], P[G.mov], G.meas
    e, _ = M3.link_error(Ti, Tj, Z)
    scale = np.maximum(1.0, np.max(np.abs(np.concatenate([Ti[:, :3, 3], Tj[:, :3, 3], Z[:, :3, 3]], axis=1)), axis=1))
    theta = np.linalg.norm(e[:, 3:], axis=1)
    n = np.sin(theta)
    amp = np.where(n >= M3.TINY, theta / np.where(n >= M3.TINY, n, 1.0), 1.0)
    be = np.concatenate([np.repeat((16 * U * scale)[:, None], 3, axis=1), np.repeat((16 * U * amp)[:, None], 3, axis=1)], axis=1)
    return _carry(e, W, be, 8)
