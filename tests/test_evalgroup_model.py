"""tests/evalgroup_model.py against the oracle's restatement of derivativesNDT, on the CPU.

On the seven lattices of test_gpu_parity.py::test_probe_rank_bitmap_windows the score summed over the model's pair set (the
formula of pairterm_model in doubles) agrees with oracle.derivatives to n 2^-52 sum |term|, n the number of pairs; with one
pair taken out of the set the same comparison fails.  The index of a mean is held to the oracle's index_for_point, and the
model's treatment of a mean without an index (see its docstring) is compared with what the oracle does for one.
"""
import numpy as np
import pytest

import evalgroup_model as E
import pairterm_model as M


@pytest.fixture(scope="module")
def O():
    import oracle as O
    return O


def _pairs(grid, smean, nn):
    src, tgt = [], []
    for i, m in enumerate(smean):
        idx = [E.cell_index(m[a], grid.centre[a], grid.res, grid.size[a]) for a in range(3)]
        for k in grid.neighbours(idx, nn):
            src.append(i)
            tgt.append(k)
    return np.array(src, dtype=np.int64), np.array(tgt, dtype=np.int64)


def _oracle_map(O, grid, mean, cov):
    ot = O.OracleMap(grid.res, list(grid.centre), [c * grid.res for c in grid.size])
    ot.set_cells(mean, cov)
    return ot


@pytest.mark.parametrize("size_cells,nn", E.PROBE_LATTICES + [((6, 6, 6), 1), ((12, 9, 7), 0)])
def test_pair_set_gives_the_oracles_score(O, size_cells, nn):
    grid, mean, cov, smean, scov = E.probe_lattice(size_cells, nn)
    ot = _oracle_map(O, grid, mean, cov)
    so, _, _ = O.derivatives(ot, smean, scov, n_neighbours=nn)
    src, tgt = _pairs(grid, smean, nn)
    n = len(src)
    assert n >= 50
    term = E.scores(smean[src], scov[src], mean[tgt], cov[tgt])
    bound = n * 2.0 ** -52 * np.abs(term).sum()
    total = float(np.sum(term))                     # (pairwise summation: its own error is far inside the bound)
    print("%s nn %d: %d pairs, |model - oracle| = %.3e, bound %.3e" % (size_cells, nn, n, abs(total - so), bound))
    assert abs(total - so) <= bound
    # teeth: without its largest pair, and without its median pair, the set no longer passes
    order = np.argsort(np.abs(term))
    for drop in (order[-1], order[n // 2]):
        if abs(term[drop]) <= 2.0 * bound:
            continue
        assert abs(total - term[drop] - so) > bound
    assert abs(term[order[-1]]) > 2.0 * bound


def test_scores_is_the_formula_of_pairterm_model():
    grid, mean, cov, smean, scov = E.probe_lattice((6, 6, 6), 1)
    src, tgt = _pairs(grid, smean[:60], 1)
    assert len(src) >= 20
    got = E.scores(smean[src], scov[src], mean[tgt], cov[tgt])
    for k in range(0, len(src), max(1, len(src) // 20)):
        case = np.array(list(smean[src[k]]) + E.six(scov[src[k]]) + list(mean[tgt[k]]) + E.six(cov[tgt[k]]) + [1.0, 0.05])
        want = M.formula(case, M.DOUBLE)[0]
        assert abs(got[k] - want) <= 8 * np.spacing(abs(want)), (k, got[k], want)


def test_index_is_the_oracles(O):
    rng = np.random.default_rng(3)
    for size_cells, centre, res in (((12, 9, 7), (0.0, 0.0, 0.0), 0.5), ((5, 70, 3), (3.25, -8.0, 1e3), 0.3), ((40, 33, 1), (0, 0, 0), 0.2)):
        grid = E.Grid(size_cells, centre, res, [])
        ot = O.OracleMap(res, list(centre), [c * res for c in size_cells])
        half = np.array(size_cells) * res / 2.0
        pts = rng.uniform(-half - 2 * res, half + 2 * res, (300, 3)) + np.array(centre)
        # cell faces and one ulp either side of them
        faces = np.array(centre) + (np.arange(-3, 4)[:, None] + 0.5) * res
        faces = np.concatenate([faces, np.nextafter(faces, np.inf), np.nextafter(faces, -np.inf)])
        for p in np.concatenate([pts, faces]):
            ic, _ = ot.index_for_point(p)
            assert tuple(int(v) for v in ic) == tuple(grid.indices([p])[0]), p


def test_a_mean_without_an_index(O):
    """NaN, infinite and far means: the model (the kernel's bounds checks) pairs them with the cells 0..n-1 of that axis, the
    oracle with none; the score is the same because every such pair adds nothing."""
    grid, mean, cov, smean, scov = E.probe_lattice((6, 6, 6), 1)
    ot = _oracle_map(O, grid, mean, cov)
    inside = np.array(grid.cell_centre(0, 2, 3))
    for bad in (np.nan, np.inf, -np.inf, 3.0e9 * grid.res, -3.0e9 * grid.res):
        p = inside.copy()
        p[0] = bad
        assert E.cell_index(p[0], 0.0, grid.res, 6) == -1
        idx = grid.indices([p])[0]
        assert tuple(idx) == (-1, 2, 3)
        got = grid.neighbours(idx, 1)
        want = [grid.rank[grid.slot(0, y, z)] for y in (1, 2, 3) for z in (2, 3, 4) if grid.slot(0, y, z) in grid.rank]
        assert got == want and len(got) >= 1
        assert grid.neighbours(idx, 0) == []
        so, go, Ho = O.derivatives(ot, p[None, :], scov[:1], n_neighbours=1)
        assert so == 0.0 and not np.any(go) and not np.any(Ho)
        with np.errstate(all="ignore"):
            term = E.scores(np.repeat(p[None, :], len(got), 0), np.repeat(scov[:1], len(got), 0), mean[got], cov[got])
        assert np.all((term == 0.0) | np.isnan(term))      # (pair_term's guards turn the NaNs into +0: tests/test_gpu_pairterm.py)


def test_list_order_and_passes():
    grid = E.Grid((3, 3, 3), (0, 0, 0), 1.0, [0, 4, 13, 14, 26])
    centre = grid.cell_centre(1, 1, 1)
    assert tuple(grid.indices([centre])[0]) == (1, 1, 1)
    means = [None] * 64
    means[2] = centre
    means[63] = grid.cell_centre(0, 0, 0)
    assert E.pair_list(grid, means, 1) == [(2 << 24) | k for k in range(5)] + [(63 << 24) | 0, (63 << 24) | 1, (63 << 24) | 2]
    assert E.pair_list(grid, means, 0) == [(2 << 24) | 2, (63 << 24) | 0]
    assert E.lanes_of(3, 5, 30) == [3, 8, 13, 18, 23, 28] + [None] * 58
    ent = list(range(130))
    assert E.last_pass(ent, 64) == [128, 129] and E.last_pass(ent[:128], 64) == ent[64:128] and E.last_pass(ent[:64], 64) == ent[:64]
    assert E.last_pass([], 64) == [] and E.last_pass(ent, 1024) == ent
