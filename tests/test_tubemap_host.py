"""Tube maps without a GPU (include/geoac_tubemap.h): the symbols of the header in the built library, geoac_tube_check on the host - every
refusal with its code and a named fault - the numpy restatement (tests/tubemap_reference.py) on a table whose answer is known in closed form, and
the proof that every grid literal of the GPU cases (tests/tubemap_cases.py) meets its non-vacuity conditions on the CPU oracle's records alone."""
import ctypes
import functools

import numpy as np
import pytest

import geoac_amd as G
import harness as H
import station_reference as SR
import tubemap_cases as TC
import tubemap_reference as TR

INF, NAN = float("inf"), float("nan")
E_INVALID, E_UNSUPPORTED = -1, -4
GOOD = dict(origin=(20.0, -10.0), step=(0.5, 0.25), n=(40, 80), n_theta=9, n_phi=7, edge_max=2.0)
N_RAYS = 63


@pytest.fixture(scope="module")
def lib():
    lib = G.load_library()
    lib.geoac_tube_fault.restype = ctypes.c_char_p
    return lib


def _check(lib, eq, n_rays=N_RAYS, **kw):
    cells = ctypes.c_int64(-7)
    spec = G.tube_spec(**kw)
    rc = lib.geoac_tube_check(eq, ctypes.byref(spec), n_rays, ctypes.byref(cells))
    return rc, cells.value, lib.geoac_tube_fault(eq, ctypes.byref(spec), n_rays)


def test_header_symbols_exist_in_the_built_library(lib):
    for name in ("geoac_tube_check", "geoac_tube_fault", "geoac_fan_tubemap", "geoac_fan_tubemap_shape", "geoac_fan_tubemap_fetch", "geoac_fan_tubemap_dev",
                 "geoac_fan_tubemap_fetch_detect", "geoac_fan_tubemap_timing", "geoac_fan_tubemap_stats"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    assert hasattr(G.FanContext, "tubemap") and hasattr(G.FanContext, "tubemap_timing")
    assert ctypes.sizeof(G.TubeSpec) == 104        # the C struct's layout: 4 doubles, 8 ints, 5 doubles
    assert G.TUBE == dict(COUNT=0, TTIME_MIN=1, CEL_MAX=2, LEVEL_MAX=3, BEST=4)


def test_tube_check_accepts_good_specs(lib):
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        assert _check(lib, eq, **GOOD) == (0, 3200, None)
        assert _check(lib, eq, phi_periodic=True, leg_min=1, leg_max=1, turn_tol=0.0, turn_min=-INF, turn_max=60.0, detect_db=-60.0, **GOOD) == (0, 3200, None)
    assert _check(lib, G.EQ_GLOBAL, wrap_lon=True, **GOOD)[:2] == (0, 3200)
    assert _check(lib, G.EQ_GLOBAL, **dict(GOOD, step=(0.5, 4.5)))[:2] == (0, 3200)                       # n[1] * step[1] = 360 exactly
    assert _check(lib, G.EQ_3D, **dict(GOOD, edge_max=500.0, step=(50.0, 50.0)))[:2] == (0, 3200)          # no 180-degree bound on a Cartesian set
    assert G.tube_check(G.EQ_GLOBAL, G.tube_spec(**GOOD), N_RAYS) == 3200


BAD = [
    ("origin nan", G.EQ_GLOBAL, dict(GOOD, origin=(NAN, 0.0)), N_RAYS, "origin"),
    ("step zero", G.EQ_GLOBAL, dict(GOOD, step=(0.0, 1.0)), N_RAYS, "step"),
    ("step inf", G.EQ_GLOBAL, dict(GOOD, step=(INF, 1.0)), N_RAYS, "step"),
    ("n zero", G.EQ_GLOBAL, dict(GOOD, n=(0, 10)), N_RAYS, "at least 1"),
    ("too many cells", G.EQ_3D, dict(GOOD, n=(4096, 4097), step=(50.0, 50.0)), N_RAYS, "GEOAC_MAP_MAX_CELLS"),
    ("wrap_lon on EQ_3D", G.EQ_3D, dict(GOOD, wrap_lon=True), N_RAYS, "wrap_lon"),
    ("leg_min negative", G.EQ_GLOBAL, dict(GOOD, leg_min=-1), N_RAYS, "leg_min"),
    ("leg_max below leg_min", G.EQ_GLOBAL, dict(GOOD, leg_min=2, leg_max=1), N_RAYS, "leg_min"),
    ("turn_min nan", G.EQ_GLOBAL, dict(GOOD, turn_min=NAN), N_RAYS, "turn_min < turn_max"),
    ("empty turning band", G.EQ_GLOBAL, dict(GOOD, turn_min=50.0, turn_max=50.0), N_RAYS, "turn_min < turn_max"),
    ("not the ray count", G.EQ_GLOBAL, dict(GOOD), N_RAYS + 1, "n_theta \\* n_phi"),
    ("one inclination", G.EQ_GLOBAL, dict(GOOD, n_theta=1, n_phi=63), N_RAYS, "at least 2"),
    ("turn_tol nan", G.EQ_GLOBAL, dict(GOOD, turn_tol=NAN), N_RAYS, "turn_tol"),
    ("turn_tol negative", G.EQ_GLOBAL, dict(GOOD, turn_tol=-1.0), N_RAYS, "turn_tol"),
    ("edge_max zero", G.EQ_GLOBAL, dict(GOOD, edge_max=0.0), N_RAYS, "edge_max"),
    ("edge_max nan", G.EQ_GLOBAL, dict(GOOD, edge_max=NAN), N_RAYS, "edge_max"),
    ("edge_max inf", G.EQ_3D, dict(GOOD, edge_max=INF), N_RAYS, "edge_max must be finite"),
    ("edge_max 180 on a sphere", G.EQ_GLOBAL, dict(GOOD, edge_max=180.0, step=(5.0, 4.0)), N_RAYS, "below 180"),
    ("grid wider than the globe", G.EQ_GLOBAL_RNGDEP, dict(GOOD, step=(0.5, 4.75)), N_RAYS, "360 degrees"),
    ("span", G.EQ_GLOBAL, dict(GOOD, step=(0.002, 0.002)), N_RAYS, "GEOAC_TUBE_MAX_SPAN"),
    ("span on a Cartesian set", G.EQ_3D, dict(GOOD, edge_max=5000.0, step=(5.0, 5.0)), N_RAYS, "GEOAC_TUBE_MAX_SPAN"),
    ("unknown equation set", 9, dict(GOOD), N_RAYS, "unknown equation set"),
]


@pytest.mark.parametrize("what,eq,kw,n_rays,word", BAD, ids=[b[0] for b in BAD])
def test_tube_check_refuses_each_bad_field_and_names_it(lib, what, eq, kw, n_rays, word):
    rc, cells, fault = _check(lib, eq, n_rays, **kw)
    assert rc == E_INVALID and cells == -7 and fault is not None, what
    with pytest.raises(G.GeoAcError, match="invalid.*" + word):
        G.tube_check(eq, G.tube_spec(**kw), n_rays)


def test_tube_check_2d_phi_periodic_and_null(lib):
    rc, cells, fault = _check(lib, G.EQ_2D, **GOOD)
    assert rc == E_UNSUPPORTED and cells == -7 and b"2-D set" in fault
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.tube_check(G.EQ_2D, G.tube_spec(**GOOD), N_RAYS)
    spec = G.tube_spec(**GOOD)
    spec.phi_periodic = 2
    assert lib.geoac_tube_check(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS, None) == E_INVALID and b"phi_periodic" in lib.geoac_tube_fault(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS)
    spec = G.tube_spec(**GOOD)
    spec.wrap_lon = 2
    assert lib.geoac_tube_check(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS, None) == E_INVALID and b"wrap_lon" in lib.geoac_tube_fault(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS)
    assert lib.geoac_tube_check(G.EQ_GLOBAL, None, N_RAYS, None) == E_INVALID and lib.geoac_tube_fault(G.EQ_GLOBAL, None, N_RAYS) == b"spec is NULL"
    assert lib.geoac_tube_check(G.EQ_GLOBAL, ctypes.byref(G.tube_spec(**GOOD)), N_RAYS, None) == 0          # cells may be NULL


def test_python_spec_mirrors_the_reference_spec():
    kw = dict(origin=(1.0, 2.0), step=(0.5, 0.25), n=(3, 4), n_theta=9, n_phi=7, edge_max=40.0, wrap_lon=True, phi_periodic=True, leg_min=1, leg_max=3, turn_tol=2.5,
              turn_min=10.0, turn_max=90.0, detect_db=-3.0)
    sp, ref = G.tube_spec(**kw), TR.spec(**kw)
    got = {k: (tuple(getattr(sp, k)) if k in ("origin", "step", "n") else bool(getattr(sp, k)) if k in ("wrap_lon", "phi_periodic") else getattr(sp, k)) for k in kw}
    assert got == ref


def test_reference_on_an_identity_landing_map():
    """landing point = launch angles (exact arithmetic), two legs landing at the same place: every centre strictly inside the lattice's range and
    off the lattice lines has one hit per leg, a centre on a cell's diagonal two; the reduced values are those of the interpolant"""
    n_theta, n_phi = 5, 4
    th_ax, ph_ax = 2.0 + 2.0 * np.arange(n_theta), 10.0 + 2.0 * np.arange(n_phi)                    # theta 2 .. 10, phi 10 .. 16
    theta, phi = np.tile(th_ax, n_phi), np.repeat(ph_ax, n_theta)
    rec = np.zeros((1, theta.size, 2, H.REC_STRIDE))
    for leg in range(2):
        r = rec[0, :, leg]
        r[:, H.REC["VALID"]], r[:, H.REC["STATE"]], r[:, H.REC["STATE"] + 1] = 1.0, theta, phi
        r[:, H.REC["TTIME"]] = 100.0 * (leg + 1) + theta + phi
        r[:, H.REC["RANGE"]] = 30.0 * (leg + 1) + 0.25 * theta
        r[:, H.REC["TURN"]] = 40.0 + 50.0 * leg + 0.5 * theta
    level = -(rec[..., H.REC["TTIME"]] / 100.0)[:, None]
    # centres 1.25, 1.75, .. in x and 9.75, 10.25, .. in y: the first and the last lie outside the lattice, x = y - 8 lies on a diagonal
    sp = TR.spec(origin=(1.0, 9.5), step=(0.5, 0.5), n=(19, 14), n_theta=n_theta, n_phi=n_phi, edge_max=3.0, detect_db=-1.5)
    m = TR.reference_tubemap(H.EQ_3D, rec, theta, phi, level, sp)
    c = TR.centres(sp).reshape(19, 14, 2)
    x, y = c[..., 0], c[..., 1]
    inside = (x > 2.0) & (x < 10.0) & (y > 10.0) & (y < 16.0)
    diagonal = inside & ((x - 2.0) % 2.0 == (y - 10.0) % 2.0)
    assert np.array_equal(m["count"][0], np.where(inside, np.where(diagonal, 4, 2), 0).astype(np.uint64)) and diagonal.any()
    assert np.allclose(m["ttime_min"][0][inside], (100.0 + x + y)[inside], rtol=1e-13) and (m["ttime_min"][0][~inside] == INF).all()
    assert np.allclose(m["cel_max"][0][inside], np.maximum((30.0 + 0.25 * x) / (100.0 + x + y), (60.0 + 0.25 * x) / (200.0 + x + y))[inside], rtol=1e-13) and (m["cel_max"][0][~inside] == -INF).all()
    assert np.allclose(m["level_max"][0, 0][inside], -(100.0 + x + y)[inside] / 100.0, rtol=1e-13)
    n_tri = 2 * (n_theta - 1) * (n_phi - 1)
    assert (m["best"][0, 0][inside] < n_tri).all() and (m["best"][0, 0][inside] >= 0).all() and (m["best"][0, 0][~inside] == -1).all()      # leg 0 is the louder
    assert np.array_equal(m["detect"][0], (inside & (-(100.0 + x + y) / 100.0 >= -1.5)).astype(np.uint32))
    # the band on the interpolated turning height: leg 0 turns at 41 .. 45, leg 1 at 91 .. 95
    hi = TR.reference_tubemap(H.EQ_3D, rec, theta, phi, level, dict(sp, turn_min=60.0))
    assert np.array_equal(2 * hi["count"], m["count"]) and (hi["best"][0, 0][inside] >= n_tri).all()
    cut = TR.reference_tubemap(H.EQ_3D, rec, theta, phi, level, dict(sp, turn_min=-INF, turn_max=43.0))
    assert np.array_equal(cut["count"][0] > 0, inside & (40.0 + 0.5 * x < 43.0))


@functools.lru_cache(maxsize=None)
def _oracle(launch):
    import tempfile
    member0 = _oracle("3drd")[0][0] if TC.LAUNCHES[launch]["kind"] == "gridens" else None
    return TC.oracle_tables(TC.LAUNCHES[launch], tempfile.mkdtemp(), member0=member0)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_grid_literals_meet_the_conditions_on_the_oracle(name):
    """the non-vacuity conditions of the GPU cases hold for the reference tube map of the CPU oracle's records: cells with COUNT 0, 1 and >= 2,
    a quarter of the cells reached, no centre with more hits than a station list holds.  They come from the physics and the chosen literals,
    not from the code under test."""
    case = TC.CASES[name]
    rec, level, th, ph, nt, nph = _oracle(case["launch"])
    sp = TC.spec_of(case, nt, nph)
    assert sp["n"][0] <= 32 and sp["n"][1] <= 48
    G.tube_check(TC.LAUNCHES[case["launch"]]["eq"], G.tube_spec(**sp), th.size)
    ref = TR.reference_tubemap(TC.LAUNCHES[case["launch"]]["eq"], rec, th, ph, level, sp)
    print(name, "cells with COUNT 0 / 1 / >= 2:", TR.check_non_vacuity(ref, name), "most hits at a centre", int(ref["count"].max()))
    if TC.LAUNCHES[case["launch"]]["kind"] == "gridens":
        # both members reach the grid, and they are different atmospheres: a member read twice would not pass the GPU case
        assert ref["count"].shape[0] == 2 and (ref["count"].reshape(2, -1) > 0).sum(axis=1).min() >= sp["n"][0] * sp["n"][1] // 4
        assert not np.array_equal(ref["ttime_min"][0], ref["ttime_min"][1])
    if case.get("cooperative"):
        # cells several times smaller than the landing triangles: the reached cells outnumber the triangles of both legs several times over
        assert int((ref["count"][0] >= 1).sum()) >= 3 * 2 * 2 * (nt - 1) * (nph - 1)


def test_small_lattice_literals_on_the_oracle():
    """the small-lattice step of the repeated-call GPU tests (tests/tubemap_cases.py small_lattice_step) is not vacuous: on the CPU oracle's records
    of the 7 x 5 fan the reference tube map on SMALL_GRID has hits, and so has at least one of the five stations"""
    rec, level, th, ph, nt, nph = TC.oracle_tables(dict(TC.LAUNCHES["global"], lattice=TC.SMALL_LATTICE), None)
    assert (nt, nph) == (7, 5) and TC.SMALL_GRID["n"] == (6, 7)
    sp = TR.spec(n_theta=nt, n_phi=nph, **TC.SMALL_GRID)
    G.tube_check(H.EQ_GLOBAL, G.tube_spec(**sp), th.size)
    ref = TR.reference_tubemap(H.EQ_GLOBAL, rec, th, ph, level, sp)
    hits = SR.reference_stations(H.EQ_GLOBAL, rec, th, ph, level, SR.spec(n_theta=nt, n_phi=nph, edge_max=TC.SMALL_GRID["edge_max"], cap=TC.SMALL_CAP), TC.SMALL_STATIONS)[0]
    print("7 x 5 fan: hits on the grid", int(ref["count"].sum()), "cells reached", int((ref["count"] > 0).sum()), "station hits", hits[0].tolist())
    assert len(TC.SMALL_STATIONS) == 5 and ref["count"].sum() > 0 and (hits > 0).any()
    assert int(hits.max()) <= TC.SMALL_CAP
