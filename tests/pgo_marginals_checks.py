"""What tests/test_gpu_pgo_marginals.py (SE(2), dof 3) and tests/test_gpu_pgo3_marginals.py (SE(3), dof 6) share: a bank with graphs
set, and the comparison of a marginals call with the dense inverse of the model's system built at the poses THE DEVICE holds.
The tolerance is ten times the graph's floor of tests/pgo_marginals_model.py, relative to each block's largest entry."""
import numpy as np

import pgo_marginals_model as MM


def make_bank(N, dof, graphs, optimize=True, **params):
    """every graph in one bank (and one optimise call) -> bank; the caller closes it"""
    cls = N.PGO if dof == 3 else N.PGO3
    bank = cls(len(graphs), max(G.n_nodes for G in graphs), max(max(G.n_edges for G in graphs), 1))
    for k, G in enumerate(graphs):
        bank.set_graph(k, G.poses, G.ref, G.mov, G.meas, G.info)
    if optimize:
        bank.optimize(**params)
    return bank


def dense_at_device_poses(bank, k, G, prior_information=None):
    """(the model's system, H^-1 as blocks, the poses) of graph k at the poses the bank holds"""
    P = bank.poses(k)[0]
    S = MM.system(G, P, prior_information)
    return S, MM.dense_inverse(S), P


def assert_blocks(name, tol, cov, cross, Hi, qs, os_):
    """every queried block against the dense inverse, the largest entry difference relative to the block's largest entry"""
    worst = 0.0
    for i, (q, o) in enumerate(zip(qs, os_)):
        d = MM.block_diff(cov[i], Hi[q, q])
        if cross is not None:
            d = max(d, MM.block_diff(cross[i], Hi[o, q]))
        worst = max(worst, d)
    print("%s: %d queries, largest relative block difference %.3g (allowed %.3g)" % (name, len(qs), worst, tol))
    assert worst <= tol, name


def same_bits(a, b):
    return a.tobytes() == b.tobytes()
