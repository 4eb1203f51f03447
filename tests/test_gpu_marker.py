"""The marker export on the device (ndtgpu_mapset_markers*, ndtgpu_marker_links*, ndtgpu_mcl_markers*) against tests/marker_model.py
BIT FOR BIT: points, src, counts and flags of the designed set and of the built maps, with and without poses, through the host form
and the device form; batch invariance; the capacity rule; links; particles; the host mirror; and the library's resources.  The
model's input is always what export_cells returns."""
import subprocess

import numpy as np
import pytest

import marker_fixtures as MF
import marker_model as M
import occgrid_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    return N


@pytest.fixture(scope="module")
def designed(N):
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=MF.N_MAPS, max_cells=MF.MAX_CELLS)
    cells = []
    for m in range(MF.N_MAPS):
        ms.set_centre(m, F.CENTRES[m])
        mean, cov, _ = MF.designed_cells(m)
        if mean.shape[0]:
            ms.set_cells(m, mean, cov)
        got = ms.export_cells(m)[:2]
        # set_cells floors nothing and refuses nothing here: what was set comes back, in slot order
        assert got[0].shape[0] == MF.N_CELLS[m] and (got[0] == mean).all() and (got[1] == cov).all()
        cells.append(got)
    return ms, cells


@pytest.fixture(scope="module")
def built(N):
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=F.N_MAPS)
    for m in range(F.N_MAPS):
        ms.set_centre(m, F.CENTRES[m])
    ms.build(F.scans()[0])
    cells = [ms.export_cells(m)[:2] for m in range(F.N_MAPS)]
    assert all(c[0].shape[0] == F.CELLS_PER_SCAN for c in cells)
    return ms, cells


_models = {}
GUARD = np.uint32(2 ** 32 - 7)          # the int32 -7 of the guard rows, read as uint32


def model(which, cells, pose_set, first=0, count=3):
    key = (which, pose_set, first, count)
    if key not in _models:
        poses = MF.POSE_SETS[pose_set]
        _models[key] = M.map_markers(cells[first:first + count], None if poses is None else poses[first:first + count], first=first)
    return _models[key]


def device_form(N, ms, marker, first, count, poses, capacity, want_src=True, fill=None):
    """-> (points [capacity + 4, 6] with four guard rows, src, (n, overflow, flags))"""
    import torch
    pts = torch.full((capacity + 4, 6), -7.0 if fill is None else fill, dtype=torch.float64, device="cuda")
    src = torch.full((capacity + 4, 2), -7, dtype=torch.int32, device="cuda") if want_src else None
    T = None if poses is None else torch.tensor(np.ascontiguousarray(np.transpose(poses, (0, 2, 1))).reshape(-1, 16), device="cuda")
    ms.markers_device(marker, first, count, pts, src_t=src, poses_t=T, capacity=capacity)
    cnt = marker.count()
    return pts.cpu().numpy(), None if src is None else src.cpu().numpy().view(np.uint32), cnt


@pytest.mark.parametrize("pose_set", ["none", "yaw", "roll"])
@pytest.mark.parametrize("which", ["designed", "built"])
def test_cells_against_the_model_bit_for_bit(N, designed, built, which, pose_set):
    ms, cells = designed if which == "designed" else built
    want, want_src, want_flags = model(which, cells, pose_set)
    n = want.shape[0]
    assert n > 100 and want_flags == 0
    poses = MF.POSE_SETS[pose_set]
    # the host form
    pts, src, info = ms.markers(0, 3, poses=poses)
    assert info == dict(n_segments=n, overflow=False, flags=0)
    assert pts.shape == (n, 2, 3) and (pts == want).all()
    assert (src == want_src).all()
    # segments in (map, cell, axis) order; the empty map contributes nothing and shifts nothing
    key = src[:, 0].astype(np.int64) * 100000 + src[:, 1]
    assert (np.diff(key) >= 0).all()
    if which == "designed":
        assert set(src[:, 0]) == {0, 2}
        fam = MF.designed_cells(0)[2]
        per_cell = np.bincount(src[src[:, 0] == 0, 1], minlength=MF.N_CELLS[0])
        assert (per_cell == [MF.SEGMENTS[f] for f in fam]).all()
    # the device form, with a handle that is reused
    with_marker = N.Marker(3, 0)
    try:
        for _ in range(2):
            dp, ds, cnt = device_form(N, ms, with_marker, 0, 3, poses, n)
            assert cnt == (n, False, 0)
            assert (dp[:n].reshape(n, 2, 3) == want).all() and (ds[:n] == want_src).all()
            assert (dp[n:] == -7.0).all()
    finally:
        with_marker.close()


def test_batch_invariance(N, designed):
    ms, cells = designed
    poses = MF.POSES_ROLL
    all_pts, all_src, info = ms.markers(0, 3, poses=poses)
    n0 = int((all_src[:, 0] == 0).sum())
    off = {0: 0, 1: n0, 2: n0}
    for m in range(3):
        pts, src, inf = ms.markers(m, 1, poses=poses[m:m + 1])
        k = pts.shape[0]
        assert inf["n_segments"] == k == int((all_src[:, 0] == m).sum())
        assert pts.tobytes() == all_pts[off[m]:off[m] + k].tobytes() and src.tobytes() == all_src[off[m]:off[m] + k].tobytes()
    pts, src, inf = ms.markers(1, 2, poses=poses[1:3])
    assert pts.tobytes() == all_pts[n0:].tobytes() and src.tobytes() == all_src[n0:].tobytes()
    again = ms.markers(0, 3, poses=poses)
    assert again[0].tobytes() == all_pts.tobytes() and again[1].tobytes() == all_src.tobytes()
    # no maps at all
    pts, src, inf = ms.markers(1, 0)
    assert pts.shape[0] == 0 and inf == dict(n_segments=0, overflow=False, flags=0)
    pts, src, inf = ms.markers(1, 1)
    assert pts.shape[0] == 0 and inf["n_segments"] == 0


def test_capacity(N, designed):
    ms, cells = designed
    want, want_src, _ = model("designed", cells, "yaw")
    n = want.shape[0]
    mk = N.Marker(3, 0)
    try:
        dp, ds, cnt = device_form(N, ms, mk, 0, 3, MF.POSES_YAW, n)                    # exact
        assert cnt == (n, False, 0) and (dp[:n].reshape(n, 2, 3) == want).all() and (dp[n:] == -7.0).all() and (ds[n:] == GUARD).all()
        dp, ds, cnt = device_form(N, ms, mk, 0, 3, MF.POSES_YAW, n - 1)                # one short: the true count, nothing behind the last row
        assert cnt == (n, True, 0)
        assert (dp[:n - 1].reshape(n - 1, 2, 3) == want[:n - 1]).all() and (ds[:n - 1] == want_src[:n - 1]).all()
        assert (dp[n - 1:] == -7.0).all() and (ds[n - 1:] == GUARD).all()
        dp, ds, cnt = device_form(N, ms, mk, 0, 3, MF.POSES_YAW, 0)                    # zero capacity: a count and nothing else
        assert cnt == (n, True, 0) and (dp == -7.0).all() and (ds == GUARD).all()
        with pytest.raises(N.NdtGpuError) as e:
            device_form(N, ms, mk, 0, 4, None, 8)
        assert e.value.status == -1
        one = N.Marker(1, 0)
        with pytest.raises(N.NdtGpuError) as e:
            device_form(N, ms, one, 0, 3, None, 8)
        assert e.value.status == -4                                                    # NDTGPU_ERR_CAPACITY: the handle's maps
        one.close()
    finally:
        mk.close()
    pts, src, info = ms.markers(0, 3, poses=MF.POSES_YAW, capacity=100)               # the host form
    assert info == dict(n_segments=n, overflow=True, flags=0) and pts.shape[0] == 100 and (pts == want[:100]).all()
    pts, src, info = ms.markers(0, 3, capacity=0)
    assert info["n_segments"] == n and info["overflow"] and pts.shape[0] == 0


def test_parameters_and_the_flag(N, designed):
    ms, cells = designed
    mean, cov = cells[2]
    for min_eval in (0.0, 3e-5, 0.011):
        want, want_src, _ = M.map_markers([cells[2]], MF.POSES_YAW[2:], first=2, min_eval=min_eval)
        pts, src, info = ms.markers(2, 1, poses=MF.POSES_YAW[2:], min_eval=min_eval)
        assert info["n_segments"] == want.shape[0] and (pts == want).all() and (src == want_src).all()
    # a covariance that is not finite: nothing of that axis, and the flag
    flagged = N.MapSet(F.RES, F.CENTRES[2], F.SIZE_M, n_maps=1, max_cells=MF.MAX_CELLS)
    try:
        c = cov[:40].copy()
        c[7] = np.diag([np.nan, 0.01, 0.02])
        flagged.set_cells(0, mean[:40], c)
        got = flagged.export_cells(0)[:2]
        assert got[0].shape[0] == 40 and np.isnan(got[1][7, 0, 0])
        want, want_src, flags = M.map_markers([got])
        assert flags == M.NONFINITE
        pts, src, info = flagged.markers(0, 1)
        assert info["flags"] == N.MARKER_NONFINITE and info["n_segments"] == want.shape[0]
        assert (pts == want).all() and (src == want_src).all()
    finally:
        flagged.close()


def test_links(N):
    import torch
    poses, ref, mov, score = MF.links()
    mk = N.Marker(1, 300)
    try:
        for skip in (0, 1):
            want, _ = M.link_markers(poses, ref, mov, score, skip_negative=skip)
            n = want.shape[0]
            assert n == (300, 200)[skip]
            pts, info = mk.links(poses, ref, mov, score, skip_negative=skip)
            assert info == dict(n_segments=n, overflow=False) and (pts == want).all()
            pts, info = mk.links(poses, ref, mov, score, skip_negative=skip, capacity=150)
            assert info == dict(n_segments=n, overflow=True) and (pts == want[:150]).all()
        pts, info = mk.links(poses, ref, mov, None, skip_negative=1)                   # no scores: nothing to skip
        assert info["n_segments"] == 300
        pts, info = N.link_markers(poses, ref, mov, score, skip_negative=1)
        assert (pts == M.link_markers(poses, ref, mov, score, skip_negative=1)[0]).all()
        # a node index out of range: refused by the host form, flagged by the device form
        bad = ref.copy()
        bad[7] = 40                                                                    # (score[7] > 0: kept under both settings)
        assert score[7] > 0
        with pytest.raises(N.NdtGpuError) as e:
            mk.links(poses, bad, mov, score)
        assert e.value.status == -1 and "node index" in str(e.value)
        # ... on a link that skip_negative skips it is never looked at (upstream does not look either)
        skipped = ref.copy()
        skipped[0] = 40
        assert score[0] < 0
        pts, info = mk.links(poses, skipped, mov, score, skip_negative=1)
        assert (pts == M.link_markers(poses, ref, mov, score, skip_negative=1)[0]).all() and info["n_segments"] == 200
        with pytest.raises(N.NdtGpuError):
            mk.links(poses, skipped, mov, score, skip_negative=0)
        T = torch.tensor(np.ascontiguousarray(np.transpose(poses, (0, 2, 1))).reshape(-1, 16), device="cuda")
        r = torch.tensor(bad.view(np.int32), device="cuda")
        mv = torch.tensor(mov.view(np.int32), device="cuda")
        sc = torch.tensor(score, device="cuda")
        out = torch.full((304, 6), -7.0, dtype=torch.float64, device="cuda")
        mk.links_device(T, r, mv, out, score_t=sc, capacity=300, skip_negative=1)
        cnt = mk.count()
        want, flags = M.link_markers(poses, bad, mov, score, skip_negative=1)
        assert flags == M.BAD_INDEX and cnt == (199, False, N.MARKER_BAD_INDEX)
        got = out.cpu().numpy()
        assert (got[:199].reshape(199, 2, 3) == want).all() and (got[199:] == -7.0).all()
        with pytest.raises(N.NdtGpuError) as e:
            N.Marker(1, 10).links(poses, ref, mov, score)
        assert e.value.status == -4
    finally:
        mk.close()


def test_particles(N, built):
    import torch
    ms, _ = built
    T = MF.particles()
    bank = N.MCL(ms, [0, 2], 300, scan_size=F.SIZE_M, max_scan_cells=1000)
    try:
        bank.set_particles(T)
        T_back = bank.particles()[0]                     # the T16 that ndtgpu_mcl_particles returns
        assert (T_back[..., :3, :] == T[..., :3, :]).all()
        want = M.particle_markers(T_back)
        got = bank.particle_markers()
        assert got.shape == (2, 300, 2, 3) and (got == want).all()
        got1 = bank.particle_markers(first=1, count=1)
        assert (got1 == want[1:]).all()
        got2 = bank.particle_markers(particle_length=-1.5)
        assert (got2 == M.particle_markers(T_back, -1.5)).all()
        out = torch.full((2 * 300 * 6 + 6,), -7.0, dtype=torch.float64, device="cuda")
        view = bank.particle_markers(out=out)
        torch.cuda.synchronize()
        assert (view.cpu().numpy() == want).all() and (out[-6:].cpu().numpy() == -7.0).all()
        with pytest.raises(N.NdtGpuError):
            bank.particle_markers(first=1, count=2)
    finally:
        bank.close()


def test_the_mirror_returns_the_same_points(N, designed, tmp_path):
    """markerNDTCells(map, pose, id, name) of tests/native/marker_demo.cpp on the designed map 0: the points of the first test"""
    from test_host_marker import build_demo
    ms, cells = designed
    mean, cov = cells[0]
    pose = MF.POSES_ROLL[0]
    want, _, _ = model("designed", cells, "roll", 0, 1)
    inp, outp = tmp_path / "cells.bin", tmp_path / "points.bin"
    np.concatenate([[float(mean.shape[0]), 1.0], mean.ravel(), cov.ravel(), np.ascontiguousarray(pose.T).ravel()]).tofile(str(inp))
    exe = build_demo(tmp_path)
    run = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.fromfile(str(outp)).reshape(-1, 2, 3)
    assert got.shape == want.shape and (got == want).all()
    assert (ms.markers(0, 1, poses=pose[None])[0] == got).all()


def test_live_resources_return_after_every_handle_is_destroyed(N):
    import gc
    import torch
    from ndt_feature_graph_amd.binding import live_resources
    gc.collect()
    torch.cuda.synchronize()
    before = live_resources()
    ms = N.MapSet(F.RES, F.CENTRES[0], F.SIZE_M, n_maps=2, max_cells=MF.MAX_CELLS)
    mean, cov, _ = MF.designed_cells(2)
    ms.set_centre(1, F.CENTRES[2])
    ms.set_cells(1, mean, cov)
    mk = N.Marker(2, 300)
    assert live_resources() != before
    n = ms.markers(0, 2, marker=mk)[2]["n_segments"]
    assert n == ms.markers(0, 2)[2]["n_segments"] > 400          # (a handle made for the call, and gone with it)
    ms.markers(0, 2, marker=mk, capacity=10 * n)                 # (the staging grows)
    poses, ref, mov, score = MF.links()
    mk.links(poses, ref, mov, score)
    bank = N.MCL(ms, [1], 64, scan_size=F.SIZE_M, max_scan_cells=1000)
    bank.particle_markers()
    bank.close()
    mk.close()
    ms.close()
    assert live_resources() == before
