"""The registrar's split rule (csrc/ndtgpu_split.h) on the host: tests/native/split_checks.cpp includes only that header, reads cases
from stdin and writes the header's decisions, which are compared EXACTLY (integers, and doubles as hexadecimal floats) with fixed
values and with the restatement of the rule below (written from DESIGN.md section 6 and the header's comments).  No GPU.

Small chips: on 32 CUs the guard `g8 < 16 || g8 > n_cu - 16` of the whole-rounds refinement lets exactly one candidate through, 16, and
the rule takes it; on fewer than 32 CUs it rejects every candidate and the proportional value stands.  Both are checked."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split") / "split_checks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "native", "split_checks.cpp"),
                           "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.splitlines()
    return run


def values(line):
    """the numbers of an output line: integers, and doubles from their hexadecimal form"""
    return [float.fromhex(v) if "x" in v else int(v) for v in line.split()]


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def groups_of(maps, k, n_cu):
    """the most matcher CUs that leave the builds k rounds: ceil(maps / 4k) build CUs, rounded up to eight; at least 16 matcher CUs"""
    f8 = -(-(-(-maps // (4 * k))) // 8) * 8
    return n_cu - f8 if n_cu > f8 + 15 else 0


def model(B, M_raw, pairs, n_cu):
    """(proportional, chosen): n_cu M / (M + B) with M = 1.125 M_raw and the share kept in 0.25 .. 0.9, rounded to eight; then, of the
    splits within 32 CUs that leave both sides 16, the one whose slower side -- M / g, or whole rounds of the mean build workgroup --
    is fastest: a new one wins outright by 1 %, or within 1 % when it is no slower and closer to the proportional one"""
    M = M_raw * 1.125
    share = M / (M + B) if M + B > 0 else 0.5
    share = min(0.9, max(0.25, share))
    prop = max(8, int(share * n_cu + 4.0) // 8 * 8)
    if not (B > 0 and M > 0):
        return prop, prop
    wg = 4.0 * B / (2.0 * pairs)
    best_t, best_g = 0.0, prop
    for g8 in range(prop - 32, prop + 33, 8):
        if g8 < 16 or g8 > n_cu - 16:
            continue
        t = max(M / g8, math.ceil(2.0 * pairs / (4.0 * (n_cu - g8))) * wg)
        closer = abs(g8 - prop) < abs(best_g - prop)
        if best_t == 0 or t < 0.99 * best_t or (t <= 1.01 * best_t and closer and t <= best_t):
            best_t, best_g = t, g8
    return prop, best_g


def ask_model(ask, cases):
    out = ask(["M %s %s %d %d" % (float(B).hex(), float(M).hex(), pairs, n_cu) for B, M, pairs, n_cu in cases])
    return [tuple(int(v) for v in line.split()) for line in out]


def ask_probe(ask, model_groups, M_raw, w, fail=0, maps=2048, n_cu=256):
    line, = ask(["P %d %d %d %s %s %s %d" % (model_groups, maps, n_cu, float(M_raw).hex(), (0.85 * 2400000).hex(), float(w).hex(), fail)])
    head, asked, cand = line.split("|")
    ok, groups = (int(v) for v in head.split())
    return ok, groups, [int(v) for v in asked.split()], [int(v) for v in cand.split()]


# ---- (a) fixed cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps,expect", [(2048, [0, 0, 80, 128, 152, 168, 176, 192]), (768, [64, 160, 192, 208, 216, 224, 224, 232]),
                                         (64, [240, 248, 248, 248]),
                                         # the floor of 16 matcher CUs: 960 maps in one round leave exactly 16, 992 leave 8 (none)
                                         (960, [16, 136, 176, 192]), (992, [0, 128])])
def test_groups_of(ask, maps, expect):
    got = [int(v) for v in ask(["G %d %d 256" % (maps, k) for k in range(1, len(expect) + 1)])]
    assert got == expect
    assert [groups_of(maps, k, 256) for k in range(1, len(expect) + 1)] == expect


def test_groups_of_floor_of_16(ask):
    """(chips whose CU count is no multiple of eight: 15 matcher CUs are none, 23 are)"""
    assert ask(["G 960 1 255", "G 960 1 256", "G 960 1 263"]) == ["0", "16", "23"]
    assert [groups_of(960, 1, n) for n in (255, 256, 263)] == [0, 16, 23]


def test_model_split_fixed(ask):
    cases = [(1e9, 1e9, 1024, 256), (1e9, 1.2e9, 1024, 256), (1e9, 4e9, 1024, 256), (4e9, 1e9, 1024, 256), (1e9, 1e11, 1024, 256),
             (1e8, 1e8, 32, 256),            # one build round fits at every split: the proportional one stands
             (0.0, 1e9, 32, 256), (1e9, 0.0, 32, 256)]          # no clocks on one side: no refinement
    expect = [(136, 128), (144, 144), (208, 208), (64, 64), (232, 240), (136, 136), (232, 232), (64, 64)]
    assert ask_model(ask, cases) == expect
    assert [model(*c) for c in cases] == expect


def test_probe_search_fixed(ask):
    assert ask_probe(ask, 128, 1e9, 0.3) == (1, 192, [128, 80, 152, 168, 176, 192], [128, 80, 152, 168, 176, 192])
    assert ask_probe(ask, 128, 1e9, 0.35) == (1, 176, [128, 80, 152, 168, 176, 192], [128, 80, 152, 168, 176, 192])
    assert ask_probe(ask, 128, 1e9, 0.5) == (1, 168, [128, 80, 152, 168, 176], [128, 80, 152, 168, 176])
    assert ask_probe(ask, 208, 4e9, 0.3) == (1, 208, [208, 200], [208, 200])


def test_probe_search_edges(ask):
    w, clk_bound, build_bound = 0.3, 1e10, 1e6         # (M_raw so large / so small that the matcher / the build side decides)
    # the model's split stands for ONE round (k0 = 1): the second candidate is k0 + 2; one round is fastest and nothing is beyond it
    assert ask_probe(ask, 64, build_bound, w, maps=768) == (1, 64, [64, 192, 160], [64, 192, 160])
    # the edge keeps winning: three extensions and no fourth (192, eight rounds, is never asked)
    assert ask_probe(ask, 80, clk_bound, w) == (1, 176, [80, 128, 152, 168, 176], [80, 128, 152, 168, 176])
    # k = 2 leaves no matcher CUs worth having: skipped, not probed
    assert ask_probe(ask, 80, build_bound, w) == (1, 80, [80, 128], [80, 128])
    # sixteen rounds are the most that is asked for: the model's split stands for them, seventeen are not probed
    assert ask_probe(ask, 128, build_bound, w, maps=8192) == (1, 80, [128, 112, 104, 96, 80], [128, 112, 104, 96, 80])
    # equal times: the first candidate stays the best, so nothing is added around the others
    assert ask_probe(ask, 128, 0.0, 0.0) == (1, 128, [128, 80, 152], [128, 80, 152])


def test_probe_failure_keeps_the_models_split(ask):
    """the first failure ends the search: nothing is asked after it, and the split is the model's"""
    assert ask_probe(ask, 128, 1e9, 0.3, fail=2) == (0, 128, [128, 80], [128])
    assert ask_probe(ask, 128, 1e9, 0.3, fail=1) == (0, 128, [128], [])
    assert ask_probe(ask, 128, 1e9, 0.3, fail=5) == (0, 128, [128, 80, 152, 168, 176], [128, 80, 152, 168])


# ---- (b) edges ----------------------------------------------------------------------------------------------------------------
def test_slot_rule_at_448(ask):
    cells = (448.0, float(np.nextafter(448.0, 1e9)), 0.0, 449.0, float(np.nextafter(448.0, 0.0)))
    assert ask(["S %s" % v.hex() for v in cells]) == ["3", "2", "3", "2", "3"]


def _clock_sums(ask, maps, results):
    lines = ["C %d %d" % (len(maps), len(results))] + ["%d %d %d %d %d" % m for m in maps] + ["%d %d" % r for r in results]
    line, = ask(lines)
    head, sane = line.split("|")
    B, M, cells, bad = head.split()
    return float.fromhex(B), float.fromhex(M), float.fromhex(cells), int(bad), [int(v) for v in sane.split()]


def test_clock_sums_and_the_sanity_filter(ask):
    maps = [(1, 2, 3, 4, 10), (5, 6, 7, 8, 20), (4294967295, 0, 0, 1, 4294967295)]
    B = (10.0 + 26.0 + 4294967296.0) / 4.0
    cells = 30.0 + 4294967295.0
    lim = 1 << 44
    # every result sane; the limits of the filter: 0 <= c < 2^44 on both words
    assert _clock_sums(ask, maps, [(100, 80), (lim - 1, 0), (0, lim - 1)]) == \
        (B, (110.0 + float(lim - 1)) + float(lim - 1) / 8.0, cells, 0, [1, 1, 1])
    assert _clock_sums(ask, maps, [(100, 80), (lim, 0), (0, lim)])[3:] == (2, [1, 0, 0])
    # one cycles_eval of 2^63 - 1 / one negative value: left out, the rest scaled by n / (n - bad)
    assert _clock_sums(ask, maps, [(100, 80), (2 ** 63 - 1, 0), (300, 0)]) == (B, 410.0 * (3.0 / 2.0), cells, 1, [1, 0, 1])
    assert _clock_sums(ask, maps, [(100, 80), (7, -1), (-5, 3), (300, 0)]) == (B, 410.0 * (4.0 / 2.0), cells, 2, [1, 0, 0, 1])
    # all bad: M stays 0 (nothing is divided by zero), and no result at all
    assert _clock_sums(ask, maps, [(-1, 0), (0, 2 ** 63 - 1)]) == (B, 0.0, cells, 2, [0, 0])
    assert _clock_sums(ask, [], []) == (0.0, 0.0, 0.0, 0, [])


def test_small_chips(ask):
    """32 CUs: 16 is the only split the guard lets through, so the refinement takes it whatever the proportional one is; 24 CUs: none
    passes and the proportional value stands"""
    cases32 = [(1e9, 1e8, 32, 32), (1e9, 1e9, 32, 32), (1e9, 1e11, 32, 32), (1e9, 1e9, 1024, 32)]
    assert ask_model(ask, cases32) == [(8, 16), (16, 16), (32, 16), (16, 16)]
    cases24 = [(1e9, 1e8, 32, 24), (1e9, 1e9, 32, 24), (1e9, 1e11, 32, 24)]
    assert ask_model(ask, cases24) == [(8, 8), (16, 16), (24, 24)]
    assert [model(*c) for c in cases32 + cases24] == [(8, 16), (16, 16), (32, 16), (16, 16), (8, 8), (16, 16), (24, 24)]


def test_recalibration_window_gates(ask):
    """each condition alone keeps a deviation far beyond pct from asking: too few samples, too early, no figure to compare with (the
    mean is then not even formed: -1 is what the harness put there)"""
    depth, pct, far = 8, 25, (300.0).hex()
    out = ask(["W new", "W calib %s 10" % (128.0).hex()] + ["W sample %s %d" % (far, depth)] * 3 +
              ["W ask 26 %d %d" % (depth, pct),              # one sample fewer than min(depth, 4)
               "W sample %s %d" % (far, depth),
               "W ask 26 %d %d" % (depth, pct),              # ... the fourth sample: yes
               "W ask 25 %d %d" % (depth, pct),              # j one short of calib_at + 2 depth
               "W new"] + ["W sample %s %d" % (far, depth)] * 4 +
              ["W ask 1000 %d %d" % (depth, pct),            # calib_cells 0
               "W new", "W calib %s 10" % (128.0).hex(), "W sample %s 1" % far,
               "W ask 11 1 %d" % pct, "W ask 12 1 %d" % pct])          # depth 1: one sample is enough, from calib_at + 2
    out = [values(v) for v in out]
    assert out[3] == [0, -1.0] and out[5] == [1, 300.0] and out[6] == [0, -1.0]
    assert out[11] == [0, -1.0]
    assert out[-2] == [0, -1.0] and out[-1] == [1, 300.0]


def test_recalibration_window(ask):
    depth, pct = 8, 25
    up = float(np.nextafter(160.0, 1e9))             # 160 / 128 - 1 is exactly a quarter; the next double is above it
    out = ask(["W new", "W calib %s 10" % (128.0).hex()] +
              ["W sample %s %d" % ((160.0).hex(), depth)] * 3 +
              ["W sample %s %d" % (up.hex(), depth),
               "W ask 26 %d %d" % (depth, pct),              # (3 x 160 + up) / 4 rounds to 160: a deviation of exactly pct
               "W new", "W calib %s 10" % (128.0).hex()] +
              ["W sample %s %d" % (up.hex(), depth)] * 4 +
              ["W ask 26 %d %d" % (depth, pct),              # the next double above it
               "W ask 26 %d %d" % (depth, pct + 1)])
    out = [values(v) for v in out]
    assert out[:3] == [[1, 160.0], [2, 160.0], [3, 160.0]]
    assert out[4] == [0, 160.0]
    assert out[-2] == [1, up] and out[-1] == [0, up]
    # the oldest sample goes at `depth` samples; min(depth, 4) with depth 2
    out = ask(["W new", "W calib %s 0" % (100.0).hex()] + ["W sample %s 2" % float(v).hex() for v in (100, 200, 300)] +
              ["W ask 4 2 25", "W ask 3 2 25"])
    out = [values(v) for v in out]
    assert out[:3] == [[1, 100.0], [2, 100.0], [2, 200.0]]
    assert out[3] == [1, 250.0] and out[4][0] == 0
    # a measurement: recal_ref carried into calib_cells (else the sub-batch's own figure), the window cleared
    out = ask(["W new", "W sample 0x1p+3 4", "W ref %s" % (250.0).hex(), "W measured %s 77" % (300.0).hex(), "W measured %s 99" % (300.0).hex(),
               "W ask 1000 4 25"])
    assert [values(v) for v in out[1:]] == [[250.0, 77, 0.0, 0], [300.0, 99, 0.0, 0], [0, -1.0]]


# ---- (c) a sweep ----------------------------------------------------------------------------------------------------------------
def test_model_split_sweep(ask):
    g = np.random.default_rng(6)
    cases = [(float(10.0 ** g.uniform(5, 11)), float(10.0 ** g.uniform(5, 11)), int(g.choice([1, 32, 384, 1024])),
              int(g.choice([32, 64, 256, 304]))) for _ in range(2000)]
    got = ask_model(ask, cases)
    want = [model(*c) for c in cases]
    assert got == want
    assert len({w for w in want}) > 40 and any(p != c for p, c in want)          # (the sweep does reach the refinement)
