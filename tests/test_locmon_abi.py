"""CPU-side checks of the localisation monitor's C-ABI (ndtgpu_locmon_*): the header declares it with its semantics, provenance and
deviations, the ctypes signatures and the structs agree with it, every bad argument or parameter is refused with a message that
names it before the handle is read and the device is looked for, the pure host entries agree with tests/locmon_model.py, and the
device entries fail loudly without a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import locmon_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_locmon_params", "ndtgpu_locmon_tile", "ndtgpu_locmon_check", "ndtgpu_locmon_radius", "ndtgpu_locmon_beam_table",
           "ndtgpu_locmon_pixel", "ndtgpu_locmon_metres", "ndtgpu_locmon_compose", "ndtgpu_locmon_create", "ndtgpu_locmon_destroy",
           "ndtgpu_locmon_set_beams", "ndtgpu_locmon_set_grids_device", "ndtgpu_locmon_set_grids", "ndtgpu_locmon_field_get",
           "ndtgpu_locmon_evaluate_device", "ndtgpu_locmon_evaluate", "ndtgpu_locmon_adjust_device", "ndtgpu_locmon_adjust",
           "ndtgpu_locmon_pick_device")
STRUCTS = (("ndtgpu_locmon_params", "LocmonParams"), ("ndtgpu_locmon_query", "LocmonQuery"), ("ndtgpu_locmon_result", "LocmonResult"),
           ("ndtgpu_locmon_adjust_result", "LocmonAdjustResult"), ("ndtgpu_locmon_pick", "LocmonPick"))


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
    assert sorted(e for e in binding.EXPORTS if "locmon" in e) == sorted(ENTRIES)
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("---- localisation monitor"):text.index("ndtgpu_locmon_pick_device(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Limits" in sec and "Measured on MI355X" in sec
    for site in ("localization_monitor.cpp:41-120", "localization_monitor.h:41-63", ":61-65", "scanCB :498-537", ":214", ":324", ":529", ":331-413",
                 ":209", "common.cpp:56-66", "common.cpp:58", "startup_loc.cpp:262-329", "occupancy_grid_utils", "distanceField", "pointCell",
                 "withinBounds"):
        assert site in sec, site
    for word in ("occupied_min", "wavefront", "angle-addition", "range gate", "0x10001", "0x10000", "upper median", "lowest linear index",
                 "first of equals", "database", "one-day expiry", "navigation counter", "odometry compensation", "radix select",
                 "workgroup-per-query"):
        assert word in sec, word
    assert "PLACEHOLDER" not in text


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    assert "ndtgpu 0." in L.ndtgpu_version().decode()          # (the version is pinned elsewhere; this entry does not bump it)
    assert L.ndtgpu_locmon_tile() == N.LOCMON_TILE == 256


def test_struct_layout_against_gcc(N, tmp_path):
    from ndt_feature_graph_amd import binding
    prints, want = [], []
    for cname, pyname in STRUCTS:
        cls = getattr(binding, pyname)
        prints.append('printf(" %%zu", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            prints.append('printf(" %%zu", offsetof(%s, %s));' % (cname, f))
            want.append(getattr(cls, f).offset)
    flags = ("NO_BEAMS", "BAD_INDEX", "NO_QUERY", "NO_RESULT", "NO_PICK")
    prints += ['printf(" %%u", NDTGPU_LOCMON_%s);' % f for f in flags] + ['printf(" %zu", sizeof(ndtgpu_featmatch_result));']
    want += [getattr(N, "LOCMON_" + f) for f in flags] + [binding.FEATMATCH_RESULT_DTYPE.itemsize]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' + "\n".join(prints) + "\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    for dt, pyname in ((N.LOCMON_QUERY_DTYPE, "LocmonQuery"), (N.LOCMON_RESULT_DTYPE, "LocmonResult"), (N.LOCMON_ADJUST_DTYPE, "LocmonAdjustResult"),
                       (N.LOCMON_PICK_DTYPE, "LocmonPick")):
        cls = getattr(binding, pyname)
        assert dt.itemsize == ctypes.sizeof(cls) and [dt.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    p = N.locmon_params()
    assert (p.max_dist, p.r_min, p.r_max, p.post_x, p.post_y, p.occupied_min, p.min_num_matches) == (0.375, 0.0, math.inf, -0.275, 0.0, 55, 8)
    assert (M.KEY_FAR, M.KEY_OFFMAP, M.NO_SCAN) == (N.LOCMON_KEY_FAR, N.LOCMON_KEY_OFFMAP, N.LOCMON_NO_SCAN)
    with pytest.raises(TypeError):
        N.locmon_params(threshold=1.0)


def test_pure_host_functions_against_the_model(N):
    rng = np.random.default_rng(11)
    for md, res in ((0.375, 0.05), (0.375, 0.1), (0.375, 0.125), (12.0, 0.05), (1.0, 1.0), (0.05, 0.05), (254.0, 1.0)):
        assert N.locmon_radius(md, res) == M.radius(md, res) >= 1, (md, res)
    L = N.lib()
    R = ctypes.c_int32(5)
    for md, res, word in ((0.04, 0.05, b"radius"), (255.0, 1.0, b"radius"), (0.0, 0.05, b"max_dist"), (float("nan"), 0.05, b"max_dist"),
                          (0.375, 0.0, b"resolution"), (0.375, float("inf"), b"resolution")):
        assert L.ndtgpu_locmon_radius(md, res, ctypes.byref(R)) == -1 and R.value == 0 and word in L.ndtgpu_last_error(), (md, res)
        assert M.radius(md, res) == 0 if math.isfinite(md) and res > 0 and math.isfinite(res) else True
    assert L.ndtgpu_locmon_radius(0.375, 0.05, None) == -1
    # the beam table: the angles by one multiplication and one addition; cos / sin within one unit in the last place (two libraries)
    for nb, a0, inc in ((1, 0.3, 0.0), (181, -math.pi / 2, math.pi / 180), (1440, 0.5 * 2 * math.pi / 1440 - math.pi, 2 * math.pi / 1440), (8192, -3.0, 7e-4)):
        cb, sb = N.locmon_beam_table(nb, a0, inc)
        wc, ws = M.beam_table(nb, a0, inc)
        assert cb.shape == (nb,) and (np.abs(cb - wc) <= np.spacing(np.abs(wc))).all() and (np.abs(sb - ws) <= np.spacing(np.abs(ws))).all()
    # the pixel of an endpoint, the badness of a key, the composed pose: bit for bit
    cb, sb = N.locmon_beam_table(64, -1.0, 0.03)
    n_in = n_out = 0
    for _ in range(400):
        pose = np.array([rng.uniform(-2, 4), rng.uniform(-3, 3), 0.0, 0.0])
        yaw = rng.uniform(-3, 3)
        pose[2], pose[3] = math.cos(yaw), math.sin(yaw)
        i = int(rng.integers(64))
        r = rng.uniform(0.0, 4.0)
        origin, res, w, h = (-1.0, -2.0), 0.05, 67, 65
        got = N.locmon_pixel(pose, cb[i], sb[i], r, origin, res, w, h)
        inb, fi, fj = M.pixels(pose, cb[i:i + 1], sb[i:i + 1], np.array([r]), origin, res, w, h)
        assert (got is not None) == bool(inb[0]) and (got is None or got == (int(fi[0]), int(fj[0])))
        n_in += bool(inb[0])
        n_out += not inb[0]
    assert n_in > 50 and n_out > 50
    assert N.locmon_pixel((0.0, 0.0, 1.0, 0.0), 1.0, 0.0, float("nan"), (0.0, 0.0), 0.05, 10, 10) is None
    assert N.locmon_pixel((0.0, 0.0, 1.0, 0.0), 1.0, 0.0, 0.5, (0.0, 0.0), 0.05, 10, 10) is None           # fi = 10 = width
    assert N.locmon_pixel((0.0, 0.0, 1.0, 0.0), 1.0, 0.0, 0.49, (0.0, 0.0), 0.05, 10, 10) == (9, 0)
    assert N.locmon_pixel((-1e-12, 0.0, 1.0, 0.0), 1.0, 0.0, 0.0, (0.0, 0.0), 0.05, 10, 10) is None        # fi = -1
    for key in list(range(0, 50)) + [64516, M.KEY_FAR, M.KEY_OFFMAP, 0xFFFFFFFF]:
        for res, md in ((0.05, 0.375), (0.1, 0.375), (0.125, 2.0)):
            assert np.float64(N.locmon_metres(key, res, md)).view(np.uint64) == np.float64(M.metres(key, res, md)).view(np.uint64), (key, res)
    for _ in range(100):
        a, b = rng.uniform(-3, 3, 2)
        ref = (rng.uniform(-20, 20), rng.uniform(-20, 20), math.cos(a), math.sin(a))
        m = (rng.uniform(-2, 2), rng.uniform(-2, 2), math.cos(b), math.sin(b))
        post = (rng.uniform(-1, 1), rng.uniform(-1, 1)) if _ % 2 else (-0.275, 0.0)
        assert np.array_equal(N.locmon_compose(ref, m, post).view(np.uint64), M.compose(ref, m, post).view(np.uint64))
    assert N.locmon_compose((1.0, 2.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0)).tolist() == [0.725, 2.0, 1.0, 0.0]


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    L = N.lib()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph, dv = ctypes.c_void_p(1), ctypes.c_void_p(8)
    nan, inf = float("nan"), float("inf")
    dp = ctypes.POINTER(ctypes.c_double)
    origins = np.zeros((3, 2))
    tab = dict(xs=np.array([0.1, 0.2, 0.3]), ys=np.array([0.0, 0.1]), cs=np.cos([0.0, 0.1, 0.2, 0.3]), sn=np.sin([0.0, 0.1, 0.2, 0.3]))
    refused = 0

    def ptr(a):
        return a.ctypes.data_as(dp)

    def prm(**kw):
        return ctypes.byref(N.locmon_params(**kw)) if kw else None

    def check(n_grids=2, width=8, height=6, resolution=0.05, n_beams=16, angle_min=-1.0, angle_increment=0.1, n_scans=3, n_queries=5, **kw):
        return L.ndtgpu_locmon_check(n_grids, width, height, resolution, n_beams, angle_min, angle_increment, n_scans, n_queries, prm(**kw))

    def grids_dev(n_grids=2, width=8, height=6, resolution=0.05, g=dv, o=origins, **kw):
        return L.ndtgpu_locmon_set_grids_device(ph, g, n_grids, width, height, resolution, None if o is None else ptr(o), prm(**kw), None)

    def grids_host(n_grids=2, width=8, height=6, resolution=0.05, g=dv, o=origins, **kw):
        return L.ndtgpu_locmon_set_grids(ph, g, n_grids, width, height, resolution, None if o is None else ptr(o), prm(**kw))

    def beams(n_beams=16, angle_min=-1.0, angle_increment=0.1):
        return L.ndtgpu_locmon_set_beams(ph, n_beams, angle_min, angle_increment, None)

    def ev_dev(n_scans=3, n_queries=5, r=dv, q=dv, res=dv, **kw):
        return L.ndtgpu_locmon_evaluate_device(ph, r, n_scans, q, n_queries, prm(**kw), res, None)

    def ev_host(n_scans=3, n_queries=5, r=ptr(origins), q=dv, res=dv, **kw):
        return L.ndtgpu_locmon_evaluate(ph, r, n_scans, q, n_queries, prm(**kw), res)

    def adj_dev(n_scans=3, scan=0, nx=3, ny=2, nyaw=4, t=tab, r=dv, res=dv, **kw):
        return L.ndtgpu_locmon_adjust_device(ph, r, n_scans, scan, 0, ptr(t["xs"]), nx, ptr(t["ys"]), ny, ptr(t["cs"]), ptr(t["sn"]), nyaw, prm(**kw),
                                             res, None, None)

    def adj_host(n_scans=3, scan=0, nx=3, ny=2, nyaw=4, t=tab, r=ptr(origins), res=dv, **kw):
        return L.ndtgpu_locmon_adjust(ph, r, n_scans, scan, 0, ptr(t["xs"]), nx, ptr(t["ys"]), ny, ptr(t["cs"]), ptr(t["sn"]), nyaw, prm(**kw),
                                      ctypes.cast(res, ctypes.POINTER(N.LocmonAdjustResult)), None)

    def pick(n_pairs=4, m=dv, refs=dv, q=dv, p=dv, **kw):
        return L.ndtgpu_locmon_pick_device(ph, m, refs, n_pairs, 0, 0, prm(**kw), q, p, None)

    def refuse(call, word, **bad):
        nonlocal refused
        assert call(**bad) == -1, (call.__name__, bad)
        assert word in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
        refused += 1

    assert check() == 0 and check(n_grids=1024, width=1 << 15, height=1 << 6, resolution=0.05) == 0 and check(n_queries=0) == 0
    assert check(max_dist=12.7, resolution=0.05) == 0 and check(r_min=0.5, r_max=30.0) == 0 and check(n_beams=8192) == 0
    for call in (check, grids_dev, grids_host):
        for bad, word in ((dict(n_grids=0), b"n_grids"), (dict(n_grids=1025), b"n_grids"), (dict(width=0), b"width"), (dict(width=(1 << 15) + 1), b"width"),
                          (dict(height=0), b"height"), (dict(height=(1 << 15) + 1), b"height"), (dict(n_grids=4, width=1 << 15, height=1 << 15), b"pixels"),
                          (dict(resolution=0.0), b"resolution"), (dict(resolution=-0.05), b"resolution"), (dict(resolution=nan), b"resolution"),
                          (dict(resolution=inf), b"resolution"), (dict(max_dist=0.0), b"max_dist"), (dict(max_dist=nan), b"max_dist"),
                          (dict(max_dist=inf), b"max_dist"), (dict(max_dist=0.04), b"radius"), (dict(max_dist=12.75), b"radius"),
                          (dict(occupied_min=128), b"occupied_min"), (dict(occupied_min=-129), b"occupied_min")):
            refuse(call, word, **bad)
    for call in (grids_dev, grids_host):
        refuse(call, b"null", g=None)
        refuse(call, b"null", o=None)
    bad_o = origins.copy()
    bad_o[1, 1] = nan
    refuse(grids_dev, b"origins2", o=bad_o)
    for call in (check, beams):
        for bad, word in ((dict(n_beams=0), b"n_beams"), (dict(n_beams=8193), b"n_beams"), (dict(angle_min=nan), b"angle_min"),
                          (dict(angle_increment=inf), b"angle_increment")):
            refuse(call, word, **bad)
    for call in (check, ev_dev, ev_host):
        for bad, word in ((dict(n_scans=0), b"n_scans"), (dict(n_scans=(1 << 24) + 1), b"n_scans"), (dict(n_queries=(1 << 24) + 1), b"n_queries"),
                          (dict(r_min=-0.1), b"r_min"), (dict(r_min=nan), b"r_min"), (dict(r_min=1.0, r_max=1.0), b"r_max"), (dict(r_max=nan), b"r_max")):
            refuse(call, word, **bad)
    for call in (ev_dev, ev_host):
        refuse(call, b"null", r=None)
        refuse(call, b"null", q=None)
        refuse(call, b"null", res=None)
    for call in (adj_dev, adj_host):
        for bad, word in ((dict(n_scans=0), b"n_scans"), (dict(nx=0), b"nx"), (dict(ny=0), b"ny"), (dict(nyaw=0), b"nyaw"), (dict(nx=(1 << 24) + 1), b"nx"),
                          (dict(nx=1 << 23, ny=2, nyaw=2), b"candidates"), (dict(nx=1 << 13, ny=1 << 13), b"candidates"), (dict(r_max=0.0), b"r_max")):
            refuse(call, word, **bad)
        for key, val, word in (("xs", nan, b"xs"), ("ys", inf, b"ys"), ("cs", 0.5, b"cs / sn"), ("sn", nan, b"cs / sn")):
            t = {k: v.copy() for k, v in tab.items()}
            t[key][1] = val
            refuse(call, word, t=t)
        refuse(call, b"null", r=None)
        refuse(call, b"null", res=None)
    refuse(adj_host, b"scan", scan=3)
    for bad, word in ((dict(n_pairs=(1 << 20) + 1), b"n_pairs"), (dict(min_num_matches=-1), b"min_num_matches"), (dict(post_x=nan), b"post_x"),
                      (dict(post_y=inf), b"post_y"), (dict(m=None), b"null"), (dict(refs=None), b"null"), (dict(q=None), b"null"), (dict(p=None), b"null")):
        refuse(pick, word, **bad)
    h = ctypes.c_void_p()
    for bad, word in (((0, 16, 8, 1), b"max_grids"), ((1025, 16, 8, 1), b"max_grids"), ((1, 0, 8, 1), b"max_pixels"), ((1, (1 << 31) + 1, 8, 1), b"max_pixels"),
                      ((1, 16, 0, 1), b"max_beams"), ((1, 16, 8193, 1), b"max_beams"), ((1, 16, 8, 0), b"max_candidates"),
                      ((1, 16, 8, (1 << 24) + 1), b"max_candidates")):
        assert L.ndtgpu_locmon_create(*bad, ctypes.byref(h)) == -1 and not h.value and word in L.ndtgpu_last_error(), bad
        refused += 1
    assert L.ndtgpu_locmon_create(1, 16, 8, 1, None) == -1
    assert L.ndtgpu_locmon_field_get(ph, 0, None) == -1 and b"field" in L.ndtgpu_last_error()
    one = np.zeros(1)
    assert L.ndtgpu_locmon_beam_table(1, 0.0, 0.0, None, ptr(one)) == -1 and L.ndtgpu_locmon_beam_table(0, 0.0, 0.0, ptr(one), ptr(one)) == -1
    assert L.ndtgpu_locmon_metres(0, 0.05, 0.375, None) == -1 and L.ndtgpu_locmon_compose(None, ptr(one), ptr(one), ptr(one)) == -1
    cell, inb = (ctypes.c_int32 * 2)(), ctypes.c_int32()
    p4 = np.array([0.0, 0.0, 1.0, 0.0])
    for bad, word in (((0.0, 4, 4), b"resolution"), ((0.05, 0, 4), b"width"), ((0.05, 4, (1 << 15) + 1), b"height")):
        assert L.ndtgpu_locmon_pixel(ptr(p4), 1.0, 0.0, 1.0, ptr(one), bad[0], bad[1], bad[2], cell, ctypes.byref(inb)) == -1
        assert word in L.ndtgpu_last_error()
    assert L.ndtgpu_locmon_pixel(None, 1.0, 0.0, 1.0, ptr(one), 0.05, 4, 4, cell, ctypes.byref(inb)) == -1
    assert refused == 139


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    dv = ctypes.c_void_p(8)
    one, c1 = np.array([0.0]), np.array([1.0])
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    calls = (lambda: L.ndtgpu_locmon_set_beams(None, 4, 0.0, 0.1, None),
             lambda: L.ndtgpu_locmon_set_grids_device(None, dv, 1, 4, 4, 0.05, p(np.zeros(2)), None, None),
             lambda: L.ndtgpu_locmon_set_grids(None, dv, 1, 4, 4, 0.05, p(np.zeros(2)), None),
             lambda: L.ndtgpu_locmon_field_get(None, 0, dv),
             lambda: L.ndtgpu_locmon_evaluate_device(None, dv, 1, dv, 1, None, dv, None),
             lambda: L.ndtgpu_locmon_evaluate(None, p(one), 1, dv, 1, None, dv),
             lambda: L.ndtgpu_locmon_adjust_device(None, dv, 1, 0, 0, p(one), 1, p(one), 1, p(c1), p(one), 1, None, dv, None, None),
             lambda: L.ndtgpu_locmon_adjust(None, p(one), 1, 0, 0, p(one), 1, p(one), 1, p(c1), p(one), 1, None,
                                            ctypes.pointer(N.LocmonAdjustResult()), None),
             lambda: L.ndtgpu_locmon_pick_device(None, dv, dv, 1, 0, 0, None, dv, dv, None))
    for k, call in enumerate(calls):
        assert call() == -1 and b"null handle" in L.ndtgpu_last_error(), k
    assert L.ndtgpu_locmon_destroy(None) == -1
    L.ndtgpu_default_locmon_params(None)                        # (a no-op, as the other default functions)


def test_monitor_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        mon = N.LocalizationMonitor(1, 16, 8, 4)
        with pytest.raises(N.NdtGpuError) as e:
            mon.set_grids(np.zeros((2, 2, 2), dtype=np.int8), 0.05, np.zeros((2, 2)))
        assert e.value.status == -4
        with pytest.raises(N.NdtGpuError) as e:
            mon.set_grids(np.zeros((1, 5, 4), dtype=np.int8), 0.05, np.zeros((1, 2)))
        assert e.value.status == -4
        with pytest.raises(N.NdtGpuError) as e:                  # nothing installed yet
            mon.n_beams = 8
            mon.evaluate(np.ones((1, 8)), N.LocalizationMonitor.queries(0, 0, 0.0, 0.0, 1.0, 0.0))
        assert e.value.status == -1
        mon.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.LocalizationMonitor(1, 600 * 600, 1440, 126000)
    assert e.value.status == -3
    for name in ("set_grids", "set_grids_device", "field", "evaluate", "evaluate_device", "adjust", "adjust_device", "pick_device"):
        assert callable(getattr(binding.LocalizationMonitor, name))
