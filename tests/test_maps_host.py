"""Arrival maps (include/geoac_map.h), everything that needs no GPU: the host-only spec validation, the numpy reference against a table whose
answer is written out by hand, the compiler's resource report of the map kernels, and the proof that the grid literals of the GPU parity cases
meet their non-vacuity conditions on the CPU oracle's records alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import geoac_amd as G
import harness as H
import map_cases as MC
import map_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
INF, NAN = float("inf"), float("nan")
GOOD = dict(origin=(20.0, -10.0), step=(0.5, 0.25), n=(40, 80))


@pytest.fixture(scope="module")
def lib():
    return G.load_library()


def _check(lib, eq, **kw):
    cells = ctypes.c_int64(-7)
    rc = lib.geoac_map_check(eq, ctypes.byref(G.map_spec(**kw)), ctypes.byref(cells))
    return rc, cells.value


def test_map_check_accepts_good_specs(lib):
    assert _check(lib, G.EQ_GLOBAL, **GOOD) == (0, 3200)
    assert _check(lib, G.EQ_GLOBAL_RNGDEP, wrap_lon=True, detect_db=-60.0, **GOOD) == (0, 3200)
    assert _check(lib, G.EQ_3D, leg_min=1, leg_max=1, turn_min=-INF, turn_max=60.0, **GOOD) == (0, 3200)
    assert _check(lib, G.EQ_3D_RNGDEP, turn_min=60.0, turn_max=INF, **GOOD) == (0, 3200)
    assert _check(lib, G.EQ_2D, origin=0.0, step=10.0, n=500) == (0, 500)
    assert _check(lib, G.EQ_GLOBAL, origin=(0.0, 0.0), step=(1.0, 1.0), n=(4096, 4096)) == (0, 1 << 24)
    assert G.map_check(G.EQ_GLOBAL, G.map_spec(**GOOD)) == 3200
    assert ctypes.sizeof(G.MapSpec) == 80          # the C struct's layout: 4 doubles, 5 ints + padding, 3 doubles


BAD = [
    ("origin nan", G.EQ_GLOBAL, dict(GOOD, origin=(NAN, 0.0))),
    ("origin inf", G.EQ_GLOBAL, dict(GOOD, origin=(0.0, INF))),
    ("step zero", G.EQ_GLOBAL, dict(GOOD, step=(0.0, 1.0))),
    ("step negative", G.EQ_GLOBAL, dict(GOOD, step=(1.0, -0.5))),
    ("step inf", G.EQ_GLOBAL, dict(GOOD, step=(INF, 1.0))),
    ("step nan", G.EQ_GLOBAL, dict(GOOD, step=(1.0, NAN))),
    ("n zero", G.EQ_GLOBAL, dict(GOOD, n=(0, 10))),
    ("n negative", G.EQ_GLOBAL, dict(GOOD, n=(10, -1))),
    ("too many cells", G.EQ_GLOBAL, dict(GOOD, n=(4096, 4097))),
    ("2-D set with two axes", G.EQ_2D, dict(GOOD)),
    ("wrap_lon on EQ_3D", G.EQ_3D, dict(GOOD, wrap_lon=True)),
    ("wrap_lon on EQ_3D_RNGDEP", G.EQ_3D_RNGDEP, dict(GOOD, wrap_lon=True)),
    ("wrap_lon on EQ_2D", G.EQ_2D, dict(origin=0.0, step=1.0, n=10, wrap_lon=True)),
    ("leg_min negative", G.EQ_GLOBAL, dict(GOOD, leg_min=-1)),
    ("leg_max below leg_min", G.EQ_GLOBAL, dict(GOOD, leg_min=2, leg_max=1)),
    ("turn_min nan", G.EQ_GLOBAL, dict(GOOD, turn_min=NAN)),
    ("turn_max nan", G.EQ_GLOBAL, dict(GOOD, turn_max=NAN)),
    ("empty turning band", G.EQ_GLOBAL, dict(GOOD, turn_min=50.0, turn_max=50.0)),
    ("unknown equation set", 9, dict(GOOD)),
]


@pytest.mark.parametrize("what,eq,kw", BAD, ids=[b[0] for b in BAD])
def test_map_check_rejects_each_bad_field(lib, what, eq, kw):
    rc, cells = _check(lib, eq, **kw)
    assert rc == E_INVALID, what
    assert cells == -7                              # (nothing is reported for a refused spec)
    with pytest.raises(G.GeoAcError):
        G.map_check(eq, G.map_spec(**kw))


def test_map_check_null_spec(lib):
    assert lib.geoac_map_check(G.EQ_GLOBAL, None, None) == E_INVALID


def test_key_order():
    v = np.array([-INF, -3.5, -1e-300, -0.0, 0.0, 1e-300, 2.0, INF])
    k = MR.key(v)
    assert (np.diff(k.astype(object)) > 0).all()            # strictly increasing, -0 below +0
    assert np.array_equal(MR.unkey(k).view(np.uint64), v.view(np.uint64))


def _rec(rows, n_rays, legs):
    """records from (ray, leg, x, y, ttime, range, turn, amp, atten) rows; every other (ray, leg) is not VALID"""
    rec = np.zeros((1, n_rays, legs, 32))
    for ray, leg, x, y, tt, rng, turn, amp, att in rows:
        r = rec[0, ray, leg]
        r[0], r[3], r[4], r[5], r[8], r[9], r[12], r[13] = 1.0, tt, att, turn, amp, rng, x, y
    return rec


def test_reference_against_a_table_written_out_by_hand():
    """EQ_3D, grid x 0 .. 30, y 0 .. 20 in 10 km cells (3 x 2).  Nine arrivals:
      a ray 0 leg 0  (5, 5)    cell (0,0)  t 100  range 30  amp 10   att 1   level 19
      b ray 0 leg 1  (7, 9)    cell (0,0)  t  90  range 36  amp 10   att 1   level 19   (ties a: BEST keeps the smaller index, a)
      c ray 1 leg 0  (10, 0)   cell (1,0)  exactly on the edges x = 10 and y = 0: belongs to the upper cell in x, the first in y
      d ray 1 leg 1  (29, 19)  cell (2,1)  amp 0: level -inf, counted, not in LEVEL_MAX / BEST
      e ray 2 leg 0  (30, 5)   outside (x = 30 is the far edge of the grid)
      f ray 2 leg 1  (-0.1, 5) outside
      g ray 3 leg 0  (15, 15)  cell (1,1)  amp -1: level NaN, counted, not in LEVEL_MAX
      h ray 3 leg 1  (15, 12)  cell (1,1)  level 20 log10(100) - 50 = -10
      i ray 4 leg 0  (5, 5)    turn 120: removed by the band [0, 100) of the second spec only"""
    rows = [(0, 0, 5.0, 5.0, 100.0, 30.0, 50.0, 10.0, 1.0), (0, 1, 7.0, 9.0, 90.0, 36.0, 50.0, 10.0, 1.0),
            (1, 0, 10.0, 0.0, 200.0, 50.0, 40.0, 1.0, 0.5), (1, 1, 29.0, 19.0, 300.0, 60.0, 40.0, 0.0, 2.0),
            (2, 0, 30.0, 5.0, 10.0, 1.0, 40.0, 1.0, 0.0), (2, 1, -0.1, 5.0, 10.0, 1.0, 40.0, 1.0, 0.0),
            (3, 0, 15.0, 15.0, 400.0, 100.0, 45.0, -1.0, 0.0), (3, 1, 15.0, 12.0, 500.0, 100.0, 45.0, 100.0, 50.0),
            (4, 0, 5.0, 5.0, 80.0, 16.0, 120.0, 1.0, 3.0)]
    rec = _rec(rows, n_rays=6, legs=2)
    level = MR.level_numpy(rec, rec[0, :, :, 4][None], calc_amp=1)
    assert level.shape == (1, 1, 6, 2) and np.isnan(level[0, 0, 5]).all() and np.isnan(level[0, 0, 4, 1])
    assert level[0, 0, 0, 0] == 19.0 and level[0, 0, 1, 1] == -INF and np.isnan(level[0, 0, 3, 0]) and level[0, 0, 3, 1] == -10.0
    sp = MR.spec(origin=(0.0, 0.0), step=(10.0, 10.0), n=(3, 2), detect_db=0.0)
    m = MR.reference_map(G.EQ_3D, rec, level, sp)
    assert m["n_pass"] == 9 and m["outside"].tolist() == [2]
    assert m["count"][0].tolist() == [[3, 0], [1, 2], [0, 1]]
    assert m["ttime_min"][0].tolist() == [[80.0, INF], [200.0, 400.0], [INF, 300.0]]
    assert m["cel_max"][0].tolist() == [[0.4, -INF], [0.25, 0.25], [-INF, 0.2]]
    assert m["level_max"][0, 0].tolist() == [[19.0, -INF], [-0.5, -10.0], [-INF, -INF]]
    assert m["best"][0, 0].tolist() == [[0, -1], [2, 7], [-1, -1]]
    assert m["detect"][0].tolist() == [[1, 0], [0, 0], [0, 0]] and m["detect"].dtype == np.uint32
    assert m["count"].dtype == np.uint64 and m["best"].dtype == np.int64 and m["outside"].dtype == np.uint64
    # turning-height band [0, 100) drops arrival i; legs 1 .. 1 keep b, d, f, h
    m2 = MR.reference_map(G.EQ_3D, rec, level, MR.spec(origin=(0.0, 0.0), step=(10.0, 10.0), n=(3, 2), turn_min=0.0, turn_max=100.0))
    assert m2["n_pass"] == 8 and m2["count"][0].tolist() == [[2, 0], [1, 2], [0, 1]] and m2["ttime_min"][0, 0, 0] == 90.0 and "detect" not in m2
    m3 = MR.reference_map(G.EQ_3D, rec, level, MR.spec(origin=(0.0, 0.0), step=(10.0, 10.0), n=(3, 2), leg_min=1, leg_max=1))
    assert m3["n_pass"] == 4 and m3["count"][0].tolist() == [[1, 0], [0, 1], [0, 1]] and m3["outside"].tolist() == [1]
    assert m3["best"][0, 0].tolist() == [[1, -1], [-1, 7], [-1, -1]]


def test_reference_signed_zero_and_wrap():
    """-0.0 < +0.0 in key order (the device's atomics see the same keys); the longitude wrap brings 185 deg to -175 on a grid from -180"""
    rec = np.zeros((1, 2, 1, 32))
    for ray, (tt, lon) in enumerate([(0.0, 185.0), (-0.0, -175.0)]):
        rec[0, ray, 0, [0, 3, 5, 9, 13, 14]] = [1.0, tt, 50.0, 1.0, np.radians(10.0), np.radians(lon)]
    level = np.zeros((1, 1, 2, 1))
    grid = dict(origin=(0.0, -180.0), step=(20.0, 10.0), n=(1, 36))
    m = MR.reference_map(G.EQ_GLOBAL, rec, level, MR.spec(wrap_lon=True, **grid))
    assert m["count"][0, 0, 0] == 2 and m["outside"].tolist() == [0]
    assert np.signbit(m["ttime_min"][0, 0, 0]) and m["best"][0, 0, 0, 0] == 0
    m = MR.reference_map(G.EQ_GLOBAL, rec, level, MR.spec(**grid))
    assert m["count"][0, 0, 0] == 1 and m["outside"].tolist() == [1]


def test_map_kernels_use_no_scratch():
    """the compiler's own report of the shipped build (written by the Makefile), parsed as tests/test_kernel_resources.py parses it"""
    path = os.path.join(ROOT, "geoac_amd", "csrc", "build", "geoac_map.hip.resource_usage.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(ROOT, "geoac_amd", "csrc"), "ARCH=gfx950"])
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"remark: .*?(Function Name|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    names = {n for r in rows for n in re.findall(r"k_map_[a-z]+", r["name"])}
    assert names == {"k_map_fill", "k_map_level", "k_map_bin", "k_map_best", "k_map_finish", "k_map_detect"}, names
    shared = [r for r in rows if re.search(r"k_map_(fill|finish|detect)", r["name"])]     # the layers' kernels, which the tube map runs as well
    assert len(shared) == 3, [r["name"] for r in shared]
    for r in rows:
        assert "ScratchSize" in r and "VGPRs Spill" in r and "SGPRs Spill" in r and "LDS Size" in r, r
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    for r in shared:
        assert r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_grid_literals_meet_the_conditions_on_the_oracle(name, tmp_path):
    """the non-vacuity conditions of the GPU parity cases hold for the reference map of the CPU oracle's records: they come from the physics and
    the chosen literals, not from the code under test"""
    case = MC.CASES[name]
    rec, atten = MC.oracle_tables(case, tmp_path)
    sp, ref = MC.reference_of(case, rec, atten)
    print(name, "arrivals", ref["n_pass"], "inside", int(ref["count"].sum()), "fullest cell", int(ref["count"].max()),
          "detect cells", [int((ref["detect"] == k).sum()) for k in range(rec.shape[0] + 1)])
    MR.check_non_vacuity(ref, sp, rec.shape[0])


def test_wrap_grids_on_the_oracle():
    """the date-line fan: on the grid from lon 0 nothing needs the wrap (the state's longitude is continuous, 164 .. 190 deg); on the grid from
    -180 the arrivals beyond 180 deg are inside with wrap_lon and outside without"""
    O = H.Oracle(H.EQ_GLOBAL, H.TOYATMO)
    th, ph = MC._angles()
    rec = O.fan(H.make_cfg(H.EQ_GLOBAL, bounces=2, calc_amp=True, src=MC.WRAP_SRC), th, ph)[1][None]
    level = MR.level_numpy(rec, rec[0, :, :, 4][None], 1)
    lon = np.degrees(rec[0, :, :, 14])[rec[0, :, :, 0] != 0]
    beyond = int((lon >= 180.0).sum())
    assert beyond >= 10 and lon.min() > 0.0 and lon.max() < 360.0
    for grid in (MC.WRAP_GRID_0, MC.WRAP_GRID_180):
        sp = MR.spec(wrap_lon=True, **grid)
        ref = MR.reference_map(H.EQ_GLOBAL, rec, level, sp)
        MR.check_non_vacuity(ref, sp, 1)
        assert ref["outside"].tolist() == [0]
    assert MR.reference_map(H.EQ_GLOBAL, rec, level, MR.spec(**MC.WRAP_GRID_0))["outside"].tolist() == [0]
    assert MR.reference_map(H.EQ_GLOBAL, rec, level, MR.spec(**MC.WRAP_GRID_180))["outside"].tolist() == [beyond]
