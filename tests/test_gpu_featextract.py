"""ndtgpu_featbank_extract*: batched feature extraction from laser scans on the device (-m gpu) against tests/flirt_model.py.

The integer outputs (the record's fields, beams, levels) must EQUAL the model's, and so must the descriptors, which are quotients of
equal integers; positions, theta and responses must be within 1e-9 absolute (metres, radians, response units) of it.  Equality is a
fair demand only where the model's own decisions are not within rounding of a threshold, so every comparison first asserts ON THE
MODEL that all of the fixture's margins (flirt_model.MARGIN_CLASSES) exceed 1e-9: about 10^6 times the fp64 rounding of quantities
up to 30, and well below the roughly 1e-6 that the closest of about 10^5 samples is expected to come to a bin edge.  A fixture that
fails that gets another seed or geometry; it is never skipped."""
import numpy as np
import pytest

import featmatch_model as FM
import flirt_fixtures as X
import flirt_model as F

pytestmark = pytest.mark.gpu
TOL = 1e-9
MARGIN = 1e-9
REC_FIELDS = ("n_valid", "n_segments", "n_peaks", "n_found", "n_stored", "status")


@pytest.fixture(scope="module")
def N():
    import ndt_feature_graph_amd as N
    N.build_library()
    if N.device_count() < 1:
        pytest.fail("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return N


def padded(scans, n_beams=None):
    """scans of one angle_min / angle_increment as rows of one array; the beams a scan does not have are NaN"""
    n_beams = n_beams or max(len(s) for s in scans)
    out = np.full((len(scans), n_beams), np.nan)
    for b, s in enumerate(scans):
        out[b, :len(s)] = s
    return out


def assert_margins(m):
    for k in F.MARGIN_CLASSES:
        assert m["margins"][k] > MARGIN, (k, m["margins"])


def assert_equals_model(rec, per_point, pos, desc, m):
    for f in REC_FIELDS:
        assert int(rec[f]) == m[f], (f, int(rec[f]), m[f])
    assert np.array_equal(per_point["beam"], m["beam"]) and np.array_equal(per_point["level"], m["level"])
    assert pos.shape == m["pos"].shape and desc.shape == m["desc"].shape
    assert np.array_equal(desc, m["desc"])
    if not len(m["beam"]):
        return
    dth = pos[:, 2] - m["pos"][:, 2]
    worst = (np.max(np.abs(pos[:, :2] - m["pos"][:, :2])), np.max(np.abs(np.arctan2(np.sin(dth), np.cos(dth)))),
             np.max(np.abs(per_point["response"] - m["response"])))
    print("points %d: worst |d pos| %.3e m, |d theta| %.3e rad, |d response| %.3e" % ((len(m["beam"]),) + worst))
    assert max(worst) <= TOL


@pytest.fixture(scope="module")
def scans():
    """the fixtures' scans and the model's results for them: computed once, shared, not modified"""
    s = dict(corner=X.l_corner(), hall360=X.hall(1, 360), hall1081=X.hall(1, 1081))
    return dict(scans=s, model={k: F.extract(*v) for k, v in s.items()})


def run_batch(N, rows, a0, inc, set_idx=None, max_points=32, n_sets=None, **params):
    fm = N.FeatureMatcher(n_sets or len(rows), max_points, 48)
    idx = list(range(len(rows))) if set_idx is None else set_idx
    res, per_point = fm.extract(idx, padded(rows), a0, inc, **params)
    return fm, res, per_point


@pytest.mark.parametrize("name", ["corner", "hall360", "hall1081"])
def test_against_the_model(N, scans, name):
    """three scans of three sizes, each a call of its own number of beams (a call has ONE n_beams, angle_min and angle_increment)"""
    r, a0, inc = scans["scans"][name]
    m = scans["model"][name]
    assert_margins(m)
    assert m["n_found"] >= 1
    fm, res, per_point = run_batch(N, [r], a0, inc)
    pos, desc = fm.get(0)
    fm.close()
    assert_equals_model(res[0], per_point[0], pos, desc, m)


def test_three_scans_in_one_batch(N, scans):
    """the 181-beam L corner, a 360-beam hall and the 1081-beam hall in ONE launch of 1081 beams: the shorter scans end in NaN
    beams, and all three are read with the hall's angles (the model is given the same rows)"""
    _, a0, inc = scans["scans"]["hall1081"]
    rows = padded([scans["scans"]["corner"][0], scans["scans"]["hall360"][0], scans["scans"]["hall1081"][0]])
    assert rows.shape == (3, 1081)
    model = [F.extract(row, a0, inc) for row in rows[:2]] + [scans["model"]["hall1081"]]
    fm, res, per_point = run_batch(N, list(rows), a0, inc)
    for b in range(3):
        assert_margins(model[b])
        pos, desc = fm.get(b)
        assert_equals_model(res[b], per_point[b], pos, desc, model[b])
    fm.close()
    assert [int(x) for x in res["n_valid"]] == [181, 360, 1081]


def test_the_largest_scan(N):
    """2048 beams: the size at which a workgroup asks for more than 64 KB of LDS"""
    r, a0, inc = X.hall(1, 2048)
    m = F.extract(r, a0, inc)
    assert_margins(m)
    fm, res, per_point = run_batch(N, [r], a0, inc)
    pos, desc = fm.get(0)
    fm.close()
    assert_equals_model(res[0], per_point[0], pos, desc, m)


def test_a_scan_does_not_depend_on_its_batch(N, scans):
    r, a0, inc = scans["scans"]["hall360"]
    fm, res1, pp1 = run_batch(N, [r], a0, inc)
    alone = (res1[0].tobytes(), fm.get(0), pp1[0])
    fm.close()
    others = [X.hall(s, 360)[0] for s in (2, 3, 4, 5, 6)]
    fm, res, pp = run_batch(N, [r] + others + [r], a0, inc)
    for b in (0, 6):
        pos, desc = fm.get(b)
        assert res[b].tobytes() == alone[0]
        assert pos.tobytes() == alone[1][0].tobytes() and desc.tobytes() == alone[1][1].tobytes()
        for f in ("beam", "level", "response"):
            assert pp[b][f].tobytes() == alone[2][f].tobytes(), f
    assert res[1].tobytes() != res[0].tobytes() and all(int(s) == F.OK for s in res["status"])
    fm.close()


def test_invalid_input_in_one_batch(N, scans):
    r, a0, inc = scans["scans"]["hall360"]
    dirty = r.copy()
    dirty[[150, 100, 101]] = np.nan
    dirty[[17, 200]] = np.inf
    dirty[33] = -np.inf
    dirty[[50, 51]] = 31.0
    dirty[[260, 300]] = [0.2, -1.0]
    m = F.extract(dirty, a0, inc)
    assert_margins(m)
    assert m["n_valid"] == 360 - 10 and m["n_found"] >= 1
    nothing = np.full(360, np.nan)
    two = nothing.copy()
    two[[7, 301]] = 3.0
    fm = N.FeatureMatcher(3, 32, 48)
    for k in range(3):                                      # the sets hold something before the call
        fm.set(k, np.ones((2, 3)), np.full((2, 48), 0.5))
    res, pp = fm.extract([0, 1, 2], np.stack([dirty, nothing, two]), a0, inc)
    pos, desc = fm.get(0)
    assert_equals_model(res[0], pp[0], pos, desc, m)
    for b, n_valid in ((1, 0), (2, 2)):
        assert [int(res[b][f]) for f in REC_FIELDS] == [n_valid, 0, 0, 0, 0, F.TOO_FEW_POINTS]
        pos, desc = fm.get(b)
        assert pos.shape == (0, 3) and desc.shape == (0, 48) and len(pp[b]["beam"]) == 0
    fm.close()


def test_overflow_stores_the_first_points_in_beam_order(N, scans):
    r, a0, inc = scans["scans"]["hall360"]
    full = scans["model"]["hall360"]
    m = F.extract(r, a0, inc, max_points=4)
    assert_margins(m)
    assert full["n_found"] > 4 and m["status"] == F.OVERFLOW and m["n_stored"] == 4
    fm, res, pp = run_batch(N, [r], a0, inc, max_points=4)
    pos, desc = fm.get(0)
    fm.close()
    assert int(res[0]["status"]) == F.OVERFLOW and int(res[0]["n_found"]) == full["n_found"] and int(res[0]["n_stored"]) == 4
    assert_equals_model(res[0], pp[0], pos, desc, m)
    assert np.array_equal(pp[0]["beam"], full["beam"][:4])


def test_a_bad_set_index_fails_that_scan_only(N, scans):
    r, a0, inc = scans["scans"]["hall360"]
    m = scans["model"]["hall360"]
    fm, res, pp = run_batch(N, [r, r, r], a0, inc, set_idx=[1, 2, 2 ** 32 - 1], n_sets=2)
    assert [int(res[1][f]) for f in REC_FIELDS] == [0, 0, 0, 0, 0, F.BAD_INDEX]
    assert [int(res[2][f]) for f in REC_FIELDS] == [0, 0, 0, 0, 0, F.BAD_INDEX]
    pos, desc = fm.get(1)
    assert_equals_model(res[0], pp[0], pos, desc, m)
    assert fm.get(0)[0].shape == (0, 3)                     # nobody wrote set 0
    fm.close()


def test_a_desc_len_mismatch_is_refused(N, scans):
    r, a0, inc = scans["scans"]["hall360"]
    fm = N.FeatureMatcher(1, 8, 40)
    with pytest.raises(N.NdtGpuError) as e:
        fm.extract([0], r[None, :], a0, inc)
    assert e.value.status == -1 and "desc_len" in str(e.value)
    res, _ = fm.extract([0], r[None, :], a0, inc, bin_rho=4, bin_phi=10)        # 40 bins fit
    fm.close()
    assert int(res[0]["status"]) in (F.OK, F.OVERFLOW)


def test_extract_then_match_with_no_host_copy_of_the_sets(N):
    """two scans of one hall, extracted on the device from device ranges, then matched: the model chain's integers, its doubles to
    1e-9, and the planted pose within 0.10 m and 0.01 rad"""
    import torch
    from ndt_feature_graph_amd import binding
    ra, a0, inc = X.hall(1, 720)
    rb = X.hall(1, 720, X.PLANTED)[0]
    ma, mb = F.extract(ra, a0, inc), F.extract(rb, a0, inc)
    assert_margins(ma)
    assert_margins(mb)
    mm = FM.match(ma["pos"], ma["desc"], mb["pos"], mb["desc"], inlier_probability=0.5, success_probability=0.99)
    assert mm["status"] == FM.OK
    for k in ("descriptor", "score", "acceptance"):
        assert mm["margins"][k] > 1e-6, (k, mm["margins"])
    dev = torch.device("cuda", 0)
    fm = N.FeatureMatcher(2, 32, 48)
    ranges = torch.tensor(np.stack([ra, rb]), dtype=torch.float64, device=dev)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    recs = torch.zeros((2, binding.FEATEXTRACT_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    out = torch.zeros((1, binding.FEATMATCH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    T16 = torch.zeros((1, 16), dtype=torch.float64, device=dev)
    corr = torch.zeros((1, 32, 2), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    fm.extract_device(idx, ranges, a0, inc, recs, stream=st)
    fm.match_device(idx[0:1], idx[1:2], out, T16, corr, stream=st, inlier_probability=0.5, success_probability=0.99)
    st.synchronize()
    rec = recs.cpu().numpy().view(binding.FEATEXTRACT_RESULT_DTYPE).reshape(-1)
    assert [int(x) for x in rec["n_found"]] == [ma["n_found"], mb["n_found"]] and all(int(s) == F.OK for s in rec["status"])
    r = out.cpu().numpy().view(binding.FEATMATCH_RESULT_DTYPE).reshape(-1)[0]
    fm.close()
    for f in ("status", "n_candidates", "n_hypotheses", "n_tested", "best_hypothesis", "n_inliers"):
        assert int(r[f]) == mm[f], (f, int(r[f]), mm[f])
    assert np.array_equal(corr.cpu().numpy().view(np.uint32)[0, :mm["n_inliers"]], mm["corr"])
    for f in ("score", "c", "s", "x", "y", "theta"):
        print("%-6s device %.17g model %.17g diff %.3e" % (f, r[f], mm[f], abs(r[f] - mm[f])))
        assert abs(r[f] - mm[f]) <= TOL, f
    assert abs(r["x"] - X.PLANTED[0]) < 0.10 and abs(r["y"] - X.PLANTED[1]) < 0.10 and abs(r["theta"] - X.PLANTED[2]) < 0.01


def test_get_returns_a_set_installed_with_set(N):
    from ndt_feature_graph_amd import synth
    f = synth.feature_sets(5, 9, 7, 5, (0.1, 0.2, 0.3))
    fm = N.FeatureMatcher(3, 11, 48)
    fm.set(2, f["ref_pos"].numpy(), f["ref_desc"].numpy())
    fm.set(0, f["mov_pos"].numpy(), f["mov_desc"].numpy())
    pos, desc = fm.get(2)
    assert pos.tobytes() == f["ref_pos"].numpy().tobytes() and desc.tobytes() == f["ref_desc"].numpy().tobytes()
    pos, desc = fm.get(0)
    assert pos.tobytes() == f["mov_pos"].numpy().tobytes() and desc.tobytes() == f["mov_desc"].numpy().tobytes()
    assert fm.get(1)[0].shape == (0, 3) and fm.get(1)[1].shape == (0, 48)
    fm.close()


def test_lifecycle_returns_every_resource(N, scans):
    from ndt_feature_graph_amd.binding import live_resources
    r, a0, inc = scans["scans"]["hall360"]
    before = live_resources()
    fm = N.FeatureMatcher(4, 16, 48)
    fm.extract([0], r[None, :], a0, inc)
    during = live_resources()
    assert during[0] > before[0] and during[1] > before[1]
    fm.extract([0, 1, 2], np.stack([r, r, r]), a0, inc)    # (the staging and result buffers grow)
    fm.match([0], [1], inlier_probability=0.5, success_probability=0.99)
    fm.get(2)
    fm.close()
    assert live_resources() == before
