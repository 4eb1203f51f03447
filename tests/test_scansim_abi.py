"""CPU-side checks of the scan simulator's C-ABI (ndtgpu_scansim_*): the header declares it with its semantics, provenance and
deviations, the ctypes signatures and the structs agree with it, every bad argument or parameter is refused with a message that
names it before the handle is read and the device is looked for, the pure host entries agree with tests/scansim_model.py bit for bit,
and the device entries fail loudly without a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import scansim_fixtures as F
import scansim_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndtgpu_default_scansim_params", "ndtgpu_scansim_tile", "ndtgpu_scansim_check", "ndtgpu_scansim_reach", "ndtgpu_scansim_skip",
           "ndtgpu_scansim_cell", "ndtgpu_scansim_beam", "ndtgpu_scansim_headings", "ndtgpu_scansim_create", "ndtgpu_scansim_destroy",
           "ndtgpu_scansim_set_beams", "ndtgpu_scansim_set_grids_device", "ndtgpu_scansim_set_grids", "ndtgpu_scansim_lattice_device",
           "ndtgpu_scansim_lattice", "ndtgpu_scansim_simulate_device", "ndtgpu_scansim_simulate")
STRUCTS = (("ndtgpu_scansim_params", "ScansimParams"), ("ndtgpu_scansim_result", "ScansimResult"))


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
    assert sorted(e for e in binding.EXPORTS if "scansim" in e) == sorted(ENTRIES)
    text = open(os.path.join(ROOT, "include", "ndtgpu.h")).read()
    sec = text[text.index("---- scan simulation"):text.index("ndtgpu_scansim_simulate(")]
    assert "PROVENANCE" in sec and "DEVIATIONS" in sec and "restated" in sec and "Limits" in sec
    for site in ("place_rec_test.cpp:203-260", ":242", "simulate_scans.cpp:131", "simulate_scans.cpp:120-142", ":218-237", ":245-254",
                 "occupancy_grid_utils", "simulateRangeScan", "generateRefScans"):
        assert site in sec, site
    for word in ("cell centres", "integer test", "leaving the grid", "occupied_min", "repeated addition", "Flags replace".lower(),
                 "unknown_is_obstacle", "R + 2", "count_dev[1]", "workgroup-per-pose", "never tested"):
        assert word in sec, word
    assert "0.13.0" in N.lib().ndtgpu_version().decode()


def test_ctypes_signatures_match_the_header(N):
    L = N.lib()
    code = header_code()
    for fn in ENTRIES:
        args = re.search(r"\b%s\s*\((.*?)\);" % fn, code, flags=re.S).group(1)
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, fn).argtypes) == n_args, fn
    assert L.ndtgpu_scansim_tile() == N.SCANSIM_TILE == 256


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
    flags = ("OFFMAP", "BAD_INDEX", "NO_POSE")
    prints += ['printf(" %%u", NDTGPU_SCANSIM_%s);' % f for f in flags]
    want += [getattr(N, "SCANSIM_" + f) for f in flags]
    src = tmp_path / "sz.c"
    src.write_text('#include "ndtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' + "\n".join(prints) + "\nreturn 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert want[0] == 24 and N.SCANSIM_RESULT_DTYPE.itemsize == ctypes.sizeof(binding.ScansimResult) == 8
    assert (M.OFFMAP, M.BAD_INDEX, M.NO_POSE) == (N.SCANSIM_OFFMAP, N.SCANSIM_BAD_INDEX, N.SCANSIM_NO_POSE)
    assert M.RESULT_DTYPE == N.SCANSIM_RESULT_DTYPE
    p = N.scansim_params()
    assert (p.range_max, p.miss, p.occupied_min, p.unknown_is_obstacle) == (10.0, 11.0, 55, 1)
    with pytest.raises(TypeError):
        N.scansim_params(threshold=1.0)


def test_pure_host_functions_against_the_model(N):
    rng = np.random.default_rng(21)
    L = N.lib()
    for rm, res in ((10.0, 0.05), (30.0, 0.05), (0.06, 0.05), (1.0, 1.0), (4094.5, 1.0), (2.0, 0.125), (0.36, 0.05)):
        assert N.scansim_reach(rm, res) == M.reach(rm, res) >= 1, (rm, res)
    R = ctypes.c_int32(5)
    for rm, res, word in ((0.04, 0.05, b"reach"), (4095.0, 1.0, b"reach"), (0.0, 0.05, b"range_max"), (float("nan"), 0.05, b"range_max"),
                          (10.0, 0.0, b"resolution"), (10.0, float("inf"), b"resolution")):
        assert L.ndtgpu_scansim_reach(rm, res, ctypes.byref(R)) == -1 and R.value == 0 and word in L.ndtgpu_last_error(), (rm, res)
    for rp, res in ((1.0, 0.05), (0.35, 0.05), (0.05, 0.05), (2.0, 0.3), (1638.4, 0.05)):
        assert N.scansim_skip(rp, res) == M.skip_of(rp, res) >= 1, (rp, res)
    k = ctypes.c_uint32(5)
    for rp, res, word in ((0.04, 0.05, b"skip"), (1e6, 0.05, b"skip"), (0.0, 0.05, b"ref_pos_resolution"), (1.0, float("nan"), b"resolution")):
        assert L.ndtgpu_scansim_skip(rp, res, ctypes.byref(k)) == -1 and k.value == 0 and word in L.ndtgpu_last_error(), (rp, res)
    # the closed form of a step
    for di in range(-12, 13):
        for dj in range(-12, 13):
            a, b, _ = M.ray_cells(di, dj)
            for kk in range(0, max(abs(di), abs(dj)) + 1):
                assert N.scansim_cell(di, dj, kk) == ((int(a[kk - 1]), int(b[kk - 1])) if kk else (0, 0)), (di, dj, kk)
    assert N.scansim_cell(32768, -32768, 32768) == (32768, -32768) and N.scansim_cell(4094, 1, 2047) == M.cell(4094, 1, 2047)
    # the headings: counts exactly, cos / sin within one unit in the last place (two libraries)
    for step in (math.pi / 4, 0.785, 3.2, 7.0, 6.28, 0.1, 2.1):
        cs, sn = N.scansim_headings(step)
        wc, ws = M.headings(step)
        assert cs.shape == wc.shape and (np.abs(cs - wc) <= np.spacing(1.0)).all() and (np.abs(sn - ws) <= np.spacing(1.0)).all(), step
    assert len(N.scansim_headings(math.pi / 4)[0]) == 8 and len(N.scansim_headings(6.28)[0]) == 1
    # one beam on a host grid, bit for bit: random grids, every kind of pixel, poses on and off the map
    n_hit = n_miss = n_off = 0
    for trial in range(30):
        h, w = int(rng.integers(1, 50)), int(rng.integers(1, 50))
        g = F.random_grid(rng, h, w, 0.02)
        origin = (rng.uniform(-3, 3), rng.uniform(-3, 3))
        res = (0.05, 0.1, 0.125)[trial % 3]
        prm = dict(range_max=res * int(rng.integers(1, 70)) + 0.3 * res, miss=rng.uniform(-1, 99), occupied_min=(55, 70)[trial % 2],
                   unknown_is_obstacle=(trial // 2) % 2)
        for _ in range(40):
            th, a = rng.uniform(-4, 4, 2)
            pose = (origin[0] + rng.uniform(-0.1, 1.1) * w * res, origin[1] + rng.uniform(-0.1, 1.1) * h * res, math.cos(th), math.sin(th))
            r, hit, flags = N.scansim_beam(g, origin, res, pose, math.cos(a), math.sin(a), **prm)
            want = M.beam(g, origin, res, pose, math.cos(a), math.sin(a), **prm)
            if want is None:
                assert (r, hit, flags) == (prm["miss"], 0, M.OFFMAP)
                n_off += 1
                continue
            assert flags == 0 and hit == want[1] and np.float64(r).view(np.uint64) == np.float64(want[0]).view(np.uint64)
            n_hit += hit
            n_miss += 1 - hit
    assert n_hit > 100 and n_miss > 100 and n_off > 50, (n_hit, n_miss, n_off)
    g = F.room()
    assert N.scansim_beam(g, F.ROOM_ORIGIN, F.RES, (float("nan"), 0.0, 1.0, 0.0), 1.0, 0.0) == (11.0, 0, M.OFFMAP)
    assert N.scansim_beam(g, F.ROOM_ORIGIN, F.RES, F.centre(30, 30) + (float("nan"), 0.0), 1.0, 0.0) == (11.0, 0, 0)
    assert N.scansim_beam(g, F.ROOM_ORIGIN, F.RES, F.centre(30, 30) + (1e9, 0.0), 1.0, 0.0) == (11.0, 0, 0)
    assert N.scansim_beam(g, F.ROOM_ORIGIN, F.RES, F.centre(30, 30) + (1.0, 0.0), 1.0, 0.0) == (F.RES * math.sqrt(100.0), 1, 0)      # (the post of row 30)


def test_bad_arguments_are_refused_before_the_device_is_looked_for(N):
    L = N.lib()
    # (a placeholder for the handle: every check below fails before it is read -- there is no handle without a device)
    ph, dv = ctypes.c_void_p(1), ctypes.c_void_p(8)
    nan, inf = float("nan"), float("inf")
    dp = ctypes.POINTER(ctypes.c_double)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    origins = np.zeros((3, 2))
    tab = dict(cs=np.cos([0.0, 0.1, 0.2, 0.3]), sn=np.sin([0.0, 0.1, 0.2, 0.3]))
    refused = 0

    def ptr(a):
        return None if a is None else a.ctypes.data_as(dp)

    def prm(**kw):
        return ctypes.byref(N.scansim_params(**kw)) if kw else None

    def check(n_grids=2, width=8, height=6, resolution=0.05, n_beams=16, angle_min=-1.0, angle_increment=0.1, n_poses=5, **kw):
        return L.ndtgpu_scansim_check(n_grids, width, height, resolution, n_beams, angle_min, angle_increment, n_poses, prm(**kw))

    def grids_dev(n_grids=2, width=8, height=6, resolution=0.05, g=dv, o=origins):
        return L.ndtgpu_scansim_set_grids_device(ph, g, n_grids, width, height, resolution, ptr(o), None)

    def grids_host(n_grids=2, width=8, height=6, resolution=0.05, g=dv, o=origins):
        return L.ndtgpu_scansim_set_grids(ph, g, n_grids, width, height, resolution, ptr(o))

    def beams(n_beams=16, angle_min=-1.0, angle_increment=0.1):
        return L.ndtgpu_scansim_set_beams(ph, n_beams, angle_min, angle_increment, None)

    def sim_dev(n_poses=5, p=dv, r=dv, **kw):
        return L.ndtgpu_scansim_simulate_device(ph, p, None, n_poses, None, prm(**kw), r, None, None)

    def sim_host(n_poses=5, p=origins, r=origins, **kw):
        return L.ndtgpu_scansim_simulate(ph, ptr(p), None, n_poses, prm(**kw), ptr(r), None)

    def lat_dev(skip=2, nyaw=4, t=tab, box=None, capacity=10, p=dv, c=dv):
        return L.ndtgpu_scansim_lattice_device(ph, 0, skip, ptr(t["cs"]), ptr(t["sn"]), nyaw, ptr(box), capacity, p, None, c, None)

    def lat_host(skip=2, nyaw=4, t=tab, box=None, capacity=10, p=origins, c=np.zeros(2, dtype=np.uint32)):
        return L.ndtgpu_scansim_lattice(ph, 0, skip, ptr(t["cs"]), ptr(t["sn"]), nyaw, ptr(box), capacity, ptr(p),
                                        None, None if c is None else c.ctypes.data_as(u32p))

    def beam(width=8, height=6, resolution=0.05, g=dv, o=origins, **kw):
        r, hit, fl = ctypes.c_double(), ctypes.c_int32(), ctypes.c_uint32()
        return L.ndtgpu_scansim_beam(g, width, height, ptr(o), resolution, ptr(origins), 1.0, 0.0, prm(**kw), ctypes.byref(r), ctypes.byref(hit),
                                     ctypes.byref(fl))

    def refuse(call, word, **bad):
        nonlocal refused
        assert call(**bad) == -1, (call.__name__, bad)
        assert word in L.ndtgpu_last_error(), (call.__name__, bad, L.ndtgpu_last_error())
        refused += 1

    assert check() == 0 and check(n_grids=1024, width=1 << 15, height=1 << 15) == 0 and check(n_beams=8192, n_poses=1 << 24) == 0
    assert check(range_max=204.7, resolution=0.05) == 0 and check(miss=-1.0, unknown_is_obstacle=0, occupied_min=-128) == 0
    for call in (check, grids_dev, grids_host):
        for bad, word in ((dict(n_grids=0), b"n_grids"), (dict(n_grids=1025), b"n_grids"), (dict(width=0), b"width"), (dict(width=(1 << 15) + 1), b"width"),
                          (dict(height=0), b"height"), (dict(height=(1 << 15) + 1), b"height"), (dict(resolution=0.0), b"resolution"),
                          (dict(resolution=-0.05), b"resolution"), (dict(resolution=nan), b"resolution"), (dict(resolution=inf), b"resolution")):
            refuse(call, word, **bad)
    for call in (grids_dev, grids_host):
        refuse(call, b"null", g=None)
        refuse(call, b"null", o=None)
        bad_o = origins.copy()
        bad_o[1, 1] = nan
        refuse(call, b"origins2", o=bad_o)
    for call in (check, beams):
        for bad, word in ((dict(n_beams=0), b"n_beams"), (dict(n_beams=8193), b"n_beams"), (dict(angle_min=nan), b"angle_min"),
                          (dict(angle_increment=inf), b"angle_increment")):
            refuse(call, word, **bad)
    for call in (check, sim_dev, sim_host):
        for bad, word in ((dict(n_poses=0), b"n_poses"), (dict(n_poses=(1 << 24) + 1), b"n_poses"), (dict(range_max=0.0), b"range_max"),
                          (dict(range_max=nan), b"range_max"), (dict(range_max=inf), b"range_max"), (dict(miss=nan), b"miss"), (dict(miss=inf), b"miss"),
                          (dict(occupied_min=128), b"occupied_min"), (dict(occupied_min=-129), b"occupied_min"),
                          (dict(unknown_is_obstacle=2), b"unknown_is_obstacle"), (dict(unknown_is_obstacle=-1), b"unknown_is_obstacle")):
            refuse(call, word, **bad)
    for bad, word in ((dict(range_max=0.04), b"reach"), (dict(range_max=204.8), b"reach")):
        refuse(check, word, **bad)
        refuse(beam, word, **bad)
    for call in (sim_dev, sim_host):
        refuse(call, b"null", p=None)
        refuse(call, b"null", r=None)
    for call in (lat_dev, lat_host):
        for bad, word in ((dict(skip=0), b"skip"), (dict(skip=(1 << 15) + 1), b"skip"), (dict(nyaw=0), b"nyaw"), (dict(nyaw=(1 << 24) + 1), b"nyaw"),
                          (dict(capacity=0), b"capacity"), (dict(capacity=(1 << 24) + 1), b"capacity"),
                          (dict(box=np.array([0.0, nan, 1.0, 1.0])), b"box4")):
            refuse(call, word, **bad)
        for key, val in (("cs", 0.5), ("sn", nan)):
            t = {k: v.copy() for k, v in tab.items()}
            t[key][1] = val
            refuse(call, b"cs / sn", t=t)
        refuse(call, b"null", t=dict(cs=None, sn=tab["sn"]))
        refuse(call, b"null", p=None)
        refuse(call, b"null", c=None)
    for bad, word in ((dict(width=0), b"width"), (dict(height=(1 << 15) + 1), b"height"), (dict(resolution=0.0), b"resolution"), (dict(g=None), b"null"),
                      (dict(o=None), b"null"), (dict(miss=nan), b"miss")):
        refuse(beam, word, **bad)
    h = ctypes.c_void_p()
    for bad, word in (((0, 8, 1), b"max_grids"), ((1025, 8, 1), b"max_grids"), ((1, 0, 1), b"max_beams"), ((1, 8193, 1), b"max_beams"),
                      ((1, 8, 0), b"max_poses"), ((1, 8, (1 << 24) + 1), b"max_poses")):
        assert L.ndtgpu_scansim_create(*bad, ctypes.byref(h)) == -1 and not h.value and word in L.ndtgpu_last_error(), bad
        refused += 1
    assert L.ndtgpu_scansim_create(1, 8, 1, None) == -1
    cell = (ctypes.c_int32 * 2)()
    for bad, word in (((32769, 0, 1), b"di"), ((0, -32769, 1), b"dj"), ((3, 2, 4), b"k must"), ((3, 2, -1), b"k must")):
        assert L.ndtgpu_scansim_cell(*bad, cell) == -1 and word in L.ndtgpu_last_error(), bad
        refused += 1
    assert L.ndtgpu_scansim_cell(1, 1, 1, None) == -1
    n = ctypes.c_size_t(7)
    for step, word in ((0.0, b"angle_step"), (-1.0, b"angle_step"), (nan, b"angle_step"), (1e-9, b"2^24")):
        assert L.ndtgpu_scansim_headings(step, ctypes.byref(n), None, None, 0) == -1 and n.value == 0 and word in L.ndtgpu_last_error(), step
        refused += 1
    one = np.zeros(1)
    assert L.ndtgpu_scansim_headings(1.0, ctypes.byref(n), ptr(one), ptr(one), 1) == -4 and n.value == 7
    assert L.ndtgpu_scansim_headings(1.0, None, None, None, 0) == -1
    assert L.ndtgpu_scansim_reach(1.0, 0.05, None) == -1 and L.ndtgpu_scansim_skip(1.0, 0.05, None) == -1
    assert refused == 129


def test_entries_refuse_a_null_handle(N):
    L = N.lib()
    dv = ctypes.c_void_p(8)
    one, c1 = np.array([0.0, 0.0]), np.array([1.0])
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cnt = (ctypes.c_uint32 * 2)()
    calls = (lambda: L.ndtgpu_scansim_set_beams(None, 4, 0.0, 0.1, None),
             lambda: L.ndtgpu_scansim_set_grids_device(None, dv, 1, 4, 4, 0.05, p(one), None),
             lambda: L.ndtgpu_scansim_set_grids(None, dv, 1, 4, 4, 0.05, p(one)),
             lambda: L.ndtgpu_scansim_lattice_device(None, 0, 1, p(c1), p(one), 1, None, 4, dv, None, dv, None),
             lambda: L.ndtgpu_scansim_lattice(None, 0, 1, p(c1), p(one), 1, None, 4, p(one), None, cnt),
             lambda: L.ndtgpu_scansim_simulate_device(None, dv, None, 1, None, None, dv, None, None),
             lambda: L.ndtgpu_scansim_simulate(None, p(one), None, 1, None, p(one), None))
    for k, call in enumerate(calls):
        assert call() == -1 and b"null handle" in L.ndtgpu_last_error(), k
    assert L.ndtgpu_scansim_destroy(None) == -1
    L.ndtgpu_default_scansim_params(None)                        # (a no-op, as the other default functions)


def test_simulator_fails_loudly_without_a_device(N):
    from ndt_feature_graph_amd import binding
    if N.device_count() > 0:                 # (a box with a device: the handle exists, and its capacity is enforced)
        sim = N.ScanSimulator(1, 8, 4)
        with pytest.raises(N.NdtGpuError) as e:
            sim.set_grids(np.zeros((2, 2, 2), dtype=np.int8), 0.05, np.zeros((2, 2)))
        assert e.value.status == -4
        with pytest.raises(N.NdtGpuError) as e:
            sim.set_beams(9, 0.0, 0.1)
        assert e.value.status == -4
        sim.close()
        return
    with pytest.raises(N.NdtGpuError) as e:
        N.ScanSimulator(1, 181, 1 << 20)
    assert e.value.status == -3
    for name in ("set_beams", "set_grids", "set_grids_device", "lattice", "lattice_device", "simulate", "simulate_device"):
        assert callable(getattr(binding.ScanSimulator, name))
