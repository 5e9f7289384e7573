"""Level tube maps without a GPU (include/geoac_ltubemap.h): geoac_ltube_check on the host - every refusal with its code and a named fault - the
symbols of the header in the built library, the numpy restatement (tests/ltubemap_reference.py) alone on synthetic affine crossing tables of
tests/test_lstations_host.py's kind, where the answer is known by construction, and the proof that every grid literal of the GPU cases
(tests/ltubemap_cases.py) meets its non-vacuity conditions on the CPU oracle's path rows alone."""
import ctypes
import functools

import numpy as np
import pytest

import geoac_amd as G
import harness as H
import ltubemap_cases as LC
import ltubemap_reference as LT
import test_lstations_host as TLH
from levels_reference import LVL, LVL_STRIDE

INF, NAN = float("inf"), float("nan")
E_INVALID, E_NODEVICE, E_UNSUPPORTED = -1, -2, -4
GOOD = dict(origin=(20.0, -10.0), step=(0.5, 0.25), n=(40, 80), n_theta=9, n_phi=7, edge_max=2.0, level_mask=0b101)
N_RAYS, N_LEVELS = 63, 3
NT, NP = TLH.NT, TLH.NP
N_TRI = 2 * (NT - 1) * (NP - 1)


@pytest.fixture(scope="module")
def lib():
    lib = G.load_library()
    lib.geoac_ltube_fault.restype = ctypes.c_char_p
    return lib


def _check(lib, eq, n_rays=N_RAYS, n_levels=N_LEVELS, **kw):
    cells, n_sel = ctypes.c_int64(-7), ctypes.c_int(-7)
    spec = G.ltube_spec(**kw)
    rc = lib.geoac_ltube_check(eq, ctypes.byref(spec), n_rays, n_levels, ctypes.byref(cells), ctypes.byref(n_sel))
    return rc, cells.value, n_sel.value, lib.geoac_ltube_fault(eq, ctypes.byref(spec), n_rays, n_levels)


# ---------------------------------------------------------------- the host-only check
def test_header_symbols_and_python_mirror(lib):
    for name in ("geoac_ltube_check", "geoac_ltube_fault", "geoac_fan_level_tubemap", "geoac_fan_level_tubemap_shape", "geoac_fan_level_tubemap_fetch",
                 "geoac_fan_level_tubemap_dev", "geoac_fan_level_tubemap_fetch_reach", "geoac_fan_level_tubemap_timing", "geoac_fan_level_tubemap_stats"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    for name in ("level_tubemap", "level_tubemap_timing", "level_tubemap_stats"):
        assert hasattr(G.FanContext, name)
    assert ctypes.sizeof(G.LTubeSpec) == 88          # the C struct's layout: 4 doubles, 9 ints (and padding), a double, 2 ints
    assert G.LTUBE == dict(COUNT=0, TTIME_MIN=1, ATTEN_MIN=2, FIRST=3)
    kw = dict(origin=(1.0, 2.0), step=(0.5, 0.25), n=(3, 4), n_theta=9, n_phi=7, edge_max=40.0, level_mask=0b110, wrap_lon=True, phi_periodic=True, leg_min=1,
              leg_max=3, ord_max=2, dir_mask=2)
    sp, ref = G.ltube_spec(**kw), LT.spec(**kw)
    got = {k: (tuple(getattr(sp, k)) if k in ("origin", "step", "n") else bool(getattr(sp, k)) if k in ("wrap_lon", "phi_periodic") else getattr(sp, k)) for k in kw}
    assert got == ref
    d = G.ltube_spec(**GOOD)
    assert (d.leg_min, d.leg_max, d.ord_max, d.dir_mask) == (0, 2**31 - 1, 1, 3) == tuple(LT.spec(**GOOD)[k] for k in ("leg_min", "leg_max", "ord_max", "dir_mask"))


def test_ltube_check_accepts_good_specs(lib):
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        assert _check(lib, eq, **GOOD) == (0, 3200, 2, None)
        assert _check(lib, eq, phi_periodic=True, leg_min=1, leg_max=1, ord_max=64, dir_mask=1, **dict(GOOD, level_mask=0b111)) == (0, 3200, 3, None)
        assert _check(lib, eq, dir_mask=2, **dict(GOOD, level_mask=0b100))[:3] == (0, 3200, 1)
    assert _check(lib, G.EQ_GLOBAL, wrap_lon=True, **GOOD)[:2] == (0, 3200)
    assert _check(lib, G.EQ_GLOBAL, **dict(GOOD, step=(0.5, 4.5)))[:2] == (0, 3200)                       # n[1] * step[1] = 360 exactly
    assert _check(lib, G.EQ_3D, **dict(GOOD, edge_max=500.0, step=(50.0, 50.0)))[:2] == (0, 3200)          # no 180-degree bound on a Cartesian set
    assert _check(lib, G.EQ_GLOBAL, n_levels=8, **dict(GOOD, level_mask=0b11111111))[:3] == (0, 3200, 8)
    assert G.ltube_check(G.EQ_GLOBAL, G.ltube_spec(**GOOD), N_RAYS, N_LEVELS) == (3200, 2)
    assert lib.geoac_ltube_check(G.EQ_GLOBAL, ctypes.byref(G.ltube_spec(**GOOD)), N_RAYS, N_LEVELS, None, None) == 0          # either pointer may be NULL


BAD = [
    ("origin nan", G.EQ_GLOBAL, dict(GOOD, origin=(NAN, 0.0)), N_RAYS, N_LEVELS, "origin"),
    ("step zero", G.EQ_GLOBAL, dict(GOOD, step=(0.0, 1.0)), N_RAYS, N_LEVELS, "step"),
    ("step inf", G.EQ_GLOBAL, dict(GOOD, step=(INF, 1.0)), N_RAYS, N_LEVELS, "step"),
    ("n zero", G.EQ_GLOBAL, dict(GOOD, n=(0, 10)), N_RAYS, N_LEVELS, "at least 1"),
    ("too many cells", G.EQ_3D, dict(GOOD, n=(4096, 4097), step=(50.0, 50.0)), N_RAYS, N_LEVELS, "GEOAC_MAP_MAX_CELLS"),
    ("wrap_lon on EQ_3D", G.EQ_3D, dict(GOOD, wrap_lon=True), N_RAYS, N_LEVELS, "wrap_lon"),
    ("not the ray count", G.EQ_GLOBAL, dict(GOOD), N_RAYS + 1, N_LEVELS, "n_theta \\* n_phi"),
    ("one inclination", G.EQ_GLOBAL, dict(GOOD, n_theta=1, n_phi=63), N_RAYS, N_LEVELS, "at least 2"),
    ("leg_min negative", G.EQ_GLOBAL, dict(GOOD, leg_min=-1), N_RAYS, N_LEVELS, "leg_min"),
    ("leg_max below leg_min", G.EQ_GLOBAL, dict(GOOD, leg_min=2, leg_max=1), N_RAYS, N_LEVELS, "leg_min"),
    ("ord_max zero", G.EQ_GLOBAL, dict(GOOD, ord_max=0), N_RAYS, N_LEVELS, "ord_max"),
    ("ord_max 65", G.EQ_GLOBAL, dict(GOOD, ord_max=65), N_RAYS, N_LEVELS, "ord_max"),
    ("edge_max zero", G.EQ_GLOBAL, dict(GOOD, edge_max=0.0), N_RAYS, N_LEVELS, "edge_max"),
    ("edge_max nan", G.EQ_GLOBAL, dict(GOOD, edge_max=NAN), N_RAYS, N_LEVELS, "edge_max"),
    ("edge_max inf", G.EQ_3D, dict(GOOD, edge_max=INF), N_RAYS, N_LEVELS, "edge_max must be finite"),
    ("edge_max 180 on a sphere", G.EQ_GLOBAL, dict(GOOD, edge_max=180.0, step=(5.0, 4.0)), N_RAYS, N_LEVELS, "below 180"),
    ("grid wider than the globe", G.EQ_GLOBAL_RNGDEP, dict(GOOD, step=(0.5, 4.75)), N_RAYS, N_LEVELS, "360 degrees"),
    ("span", G.EQ_GLOBAL, dict(GOOD, step=(0.002, 0.002)), N_RAYS, N_LEVELS, "GEOAC_TUBE_MAX_SPAN"),
    ("span on a Cartesian set", G.EQ_3D, dict(GOOD, edge_max=5000.0, step=(5.0, 5.0)), N_RAYS, N_LEVELS, "GEOAC_TUBE_MAX_SPAN"),
    ("dir_mask 0", G.EQ_GLOBAL, dict(GOOD, dir_mask=0), N_RAYS, N_LEVELS, "dir_mask"),
    ("dir_mask 4", G.EQ_GLOBAL, dict(GOOD, dir_mask=4), N_RAYS, N_LEVELS, "dir_mask"),
    ("level_mask 0", G.EQ_GLOBAL, dict(GOOD, level_mask=0), N_RAYS, N_LEVELS, "level_mask selects no level"),
    ("level_mask bit at the level count", G.EQ_GLOBAL, dict(GOOD, level_mask=0b1000), N_RAYS, N_LEVELS, "level_mask has a bit"),
    ("level_mask bit above one level", G.EQ_GLOBAL, dict(GOOD, level_mask=0b11), N_RAYS, 1, "level_mask has a bit"),
    ("level_mask negative", G.EQ_GLOBAL, dict(GOOD, level_mask=-1), N_RAYS, N_LEVELS, "level_mask has a bit"),
    ("no levels", G.EQ_GLOBAL, dict(GOOD), N_RAYS, 0, "n_levels"),
    ("nine levels", G.EQ_GLOBAL, dict(GOOD), N_RAYS, 9, "n_levels"),
    ("unknown equation set", 9, dict(GOOD), N_RAYS, N_LEVELS, "unknown equation set"),
]


@pytest.mark.parametrize("what,eq,kw,n_rays,n_levels,word", BAD, ids=[b[0] for b in BAD])
def test_ltube_check_refuses_each_bad_field_and_names_it(lib, what, eq, kw, n_rays, n_levels, word):
    rc, cells, n_sel, fault = _check(lib, eq, n_rays, n_levels, **kw)
    assert rc == E_INVALID and cells == -7 and n_sel == -7 and fault is not None, what
    with pytest.raises(G.GeoAcError, match="invalid.*" + word):
        G.ltube_check(eq, G.ltube_spec(**kw), n_rays, n_levels)


def test_ltube_check_2d_phi_periodic_and_null(lib):
    rc, cells, n_sel, fault = _check(lib, G.EQ_2D, **GOOD)
    assert rc == E_UNSUPPORTED and cells == -7 and b"2-D set" in fault
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.ltube_check(G.EQ_2D, G.ltube_spec(**GOOD), N_RAYS, N_LEVELS)
    for field in ("phi_periodic", "wrap_lon"):
        spec = G.ltube_spec(**GOOD)
        setattr(spec, field, 2)
        assert lib.geoac_ltube_check(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS, N_LEVELS, None, None) == E_INVALID
        assert field.encode() in lib.geoac_ltube_fault(G.EQ_GLOBAL, ctypes.byref(spec), N_RAYS, N_LEVELS)
    assert lib.geoac_ltube_check(G.EQ_GLOBAL, None, N_RAYS, N_LEVELS, None, None) == E_INVALID
    assert lib.geoac_ltube_fault(G.EQ_GLOBAL, None, N_RAYS, N_LEVELS) == b"spec is NULL"


def test_compute_entry_points_need_a_device(lib):
    """there is no host path: a context is what every compute entry point of the header takes, and without a usable HIP device none can be made
    (GEOAC_E_NODEVICE); with one, the call is refused until a launch with levels has completed"""
    import torch
    h = ctypes.c_void_p()
    rc = lib.geoac_create(ctypes.byref(h), G.EQ_3D, 0)
    spec = G.ltube_spec(**GOOD)
    if not torch.cuda.is_available():
        assert rc == E_NODEVICE and not h
        with pytest.raises(G.GeoAcError, match="no usable HIP device"):
            G.FanContext(G.EQ_3D)
    else:
        assert rc == 0
        assert lib.geoac_fan_level_tubemap(h, ctypes.byref(spec)) == E_INVALID
        lib.geoac_destroy(h)
    word = (ctypes.c_uint64 * 4)()
    assert lib.geoac_fan_level_tubemap(None, ctypes.byref(spec)) < 0                                         # (no context: never a result)
    assert lib.geoac_fan_level_tubemap_fetch(None, 0, word) < 0 and lib.geoac_fan_level_tubemap_fetch_reach(None, word) < 0
    assert lib.geoac_fan_level_tubemap_shape(None, None, None, None, None) < 0 and lib.geoac_fan_level_tubemap_dev(None, 0, None, None) < 0
    assert lib.geoac_fan_level_tubemap_timing(None, None) < 0 and lib.geoac_fan_level_tubemap_stats(None, word) < 0


# ---------------------------------------------------------------- the restatement on tables known by construction
# Crossing points are an affine image X = A (theta, phi) + B0 + (shift, -0.4 shift) of the launch angles (tests/test_lstations_host.py), so a
# branch's crossing triangles tile the image of the lattice rectangle, a centre's pre-image says which triangle holds it, and every column affine
# in the angles is reproduced by the interpolant.
A_INV = np.linalg.inv(TLH.A)
TH0, DTH, PH0, DPH = 2.0, 1.5, -30.0, 10.0                      # the lattice axes of TLH._lattice
GRID = dict(origin=(-121.3, -283.7), step=(15.0, 25.0), n=(27, 27))          # covers the images of shifts 0 .. 180
EDGE = 120.0                                                                # (a crossing triangle's longest side is the image of a cell's side or diagonal: below 100)
MARGIN = 1e-9                                                               # cells: centres closer than this to a triangle's edge are left out


def _spec(**kw):
    return LT.spec(n_theta=NT, n_phi=NP, edge_max=EDGE, **dict(GRID, **kw))


def _pre_image(cen, shift):
    """lattice coordinates (u, v) of the centres' pre-images under the image of `shift`: cell (floor u, floor v), inside while 0 < u < NT - 1,
    0 < v < NP - 1; and the distance [cells of the grid] of each centre from the nearest triangle edge of that image"""
    X = cen - TLH.B0 - np.array([shift, -0.4 * shift])
    ang = X @ A_INV.T
    u, v = (ang[:, 0] - TH0) / DTH, (ang[:, 1] - PH0) / DPH
    # lines u = k, v = k, u - v = k in lattice coordinates; a unit of u is DTH * |A[:, 0]| km, of v DPH * |A[:, 1]| km, of u - v less than either
    unit = min(DTH * np.linalg.norm(TLH.A[:, 0]), DPH * np.linalg.norm(TLH.A[:, 1])) / (3.0 * max(GRID["step"]))
    off = np.minimum.reduce([np.abs(q - np.rint(q)) for q in (u, v, u - v)]) * unit
    return u, v, off


def _expected(cen, branches, n_tri=N_TRI):
    """branches: [(b, shift), ...] of the selected branches.  COUNT, TTIME_MIN, FIRST per centre by construction, and the centres kept"""
    n = len(cen)
    count, tmin, first, keep = np.zeros(n, dtype=np.uint64), np.full(n, INF), np.full(n, -1, dtype=np.int64), np.ones(n, dtype=bool)
    for b, shift in branches:
        u, v, off = _pre_image(cen, shift)
        keep &= off > MARGIN
        inside = (u > 0) & (u < NT - 1) & (v > 0) & (v < NP - 1)
        i, j = np.floor(u).astype(int), np.floor(v).astype(int)
        tri = 2 * (j * (NT - 1) + i) + np.where(u - i > v - j, 0, 1)               # (a, b, c) lies on the side of corner b = (i + 1, j)
        t = 100.0 + 3.0 * (TH0 + DTH * u) + 0.5 * (PH0 + DPH * v) + shift
        count += inside.astype(np.uint64)
        better = inside & (t < tmin)
        tmin, first = np.where(better, t, tmin), np.where(better, b * n_tri + tri, first)
    return count, tmin, first, keep


def _compare(layers, ls, cen, branches, what):
    count, tmin, first, keep = _expected(cen, branches)
    shape = layers["count"].shape[2:]
    assert keep.mean() > 0.99, what
    got_c, got_t, got_f = (layers[k][0, ls].reshape(-1) for k in ("count", "ttime_min", "first"))
    assert np.array_equal(got_c[keep], count[keep]), (what, np.flatnonzero(keep & (got_c != count))[:5])
    assert np.array_equal(got_f[keep], first[keep]), (what, np.flatnonzero(keep & (got_f != first))[:5])
    some = keep & (count > 0)
    assert np.allclose(got_t[some], tmin[some], rtol=1e-12) and (got_t[keep & (count == 0)] == INF).all(), what
    assert np.allclose(layers["atten_min"][0, ls].reshape(-1)[some], 1.0 + 0.01 * (TH0 + DTH * _best_u(cen, branches, first))[some], rtol=1e-12), what
    assert np.array_equal(layers["reach"][ls].reshape(-1)[keep], (count[keep] > 0).astype(np.uint32)), what
    assert shape == GRID["n"]
    return count.reshape(shape), keep.reshape(shape)


def _best_u(cen, branches, first):
    """u of the pre-image under the branch that FIRST names (ATTEN is 1 + 0.01 theta on every branch: ATTEN_MIN is the smallest over the hits)"""
    u_min = np.full(len(cen), INF)
    for b, shift in branches:
        u, v, _ = _pre_image(cen, shift)
        inside = (u > 0) & (u < NT - 1) & (v > 0) & (v < NP - 1)
        u_min = np.where(inside & (u < u_min), u, u_min)
    return np.where(np.isfinite(u_min), u_min, 0.0)


def test_count_first_and_ttime_on_affine_images_and_the_direction_mask():
    theta, phi = TLH._lattice()
    count, lrec = TLH._table(theta, phi, lambda r, t, p: [(0, 1.0, 0.0), (0, -1.0, 60.0)])
    cen = LT.centres(_spec(level_mask=1))
    maps = {}
    for mask, branches in ((1, [(0, 0.0)]), (2, [(1, 60.0)]), (3, [(0, 0.0), (1, 60.0)])):
        sp = _spec(level_mask=1, dir_mask=mask)
        maps[mask] = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, sp)
        want, keep = _compare(maps[mask], 0, cen, branches, f"dir_mask {mask}")
        assert set(np.unique(want[keep])) == ({0, 1, 2} if mask == 3 else {0, 1})
    assert np.array_equal(maps[1]["count"] + maps[2]["count"], maps[3]["count"])
    assert int(maps[3]["count"].max()) <= LT.CAP


def test_a_ducts_second_passage_is_mapped_with_ord_max_2():
    theta, phi = TLH._lattice()
    seq = [(0, 1.0, 0.0), (0, -1.0, 60.0), (0, 1.0, 120.0), (0, -1.0, 180.0)]
    count, lrec = TLH._table(theta, phi, lambda r, t, p: seq)
    cen = LT.centres(_spec(level_mask=1))
    one = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, _spec(level_mask=1, ord_max=1))
    _compare(one, 0, cen, [(0, 0.0), (1, 60.0)], "ord_max 1")
    two = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, _spec(level_mask=1, ord_max=2))
    # b = ((leg - leg_min) * 2 + d) * ord_max + o: up 0 -> 0, up 1 -> 1, down 0 -> 2, down 1 -> 3
    want, keep = _compare(two, 0, cen, [(0, 0.0), (1, 120.0), (2, 60.0), (3, 180.0)], "ord_max 2")
    assert want[keep].max() >= 3 and (two["count"] >= one["count"]).all() and int(two["count"].sum()) > int(one["count"].sum())


def test_a_two_bit_level_mask_maps_each_level_on_its_own_layer():
    theta, phi = TLH._lattice()
    c0, r0 = TLH._table(theta, phi, lambda r, t, p: [(0, 1.0, 0.0)], n_levels=3, level=0)
    c2, r2 = TLH._table(theta, phi, lambda r, t, p: [(0, 1.0, 90.0), (0, -1.0, 150.0)], n_levels=3, level=2)
    count, lrec = c0 + c2, r0 + r2
    cen = LT.centres(_spec(level_mask=1))
    both = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, _spec(level_mask=0b101))
    assert both["count"].shape == (1, 2) + GRID["n"] and both["reach"].shape == (2,) + GRID["n"]
    _compare(both, 0, cen, [(0, 0.0)], "level 0 of 0b101")
    _compare(both, 1, cen, [(0, 90.0), (1, 150.0)], "level 2 of 0b101")
    for ls, bit in enumerate((0b001, 0b100)):
        alone = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, _spec(level_mask=bit))
        for name in ("count", "ttime_min", "atten_min", "first"):
            assert np.array_equal(LT.SR.bits(alone[name][:, 0]), LT.SR.bits(both[name][:, ls])), (bit, name)
    empty = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, _spec(level_mask=0b010))          # a level nothing crosses
    assert (empty["count"] == 0).all() and (empty["ttime_min"] == INF).all() and (empty["atten_min"] == INF).all() and (empty["first"] == -1).all() and (empty["reach"] == 0).all()


def test_a_count_past_the_crossing_cap_still_maps_the_kept_branches():
    theta, phi = TLH._lattice()
    seq = [(0, 1.0, 0.0), (0, -1.0, 60.0), (0, 1.0, 120.0), (0, -1.0, 180.0), (1, 1.0, 30.0)]
    count, lrec = TLH._table(theta, phi, lambda r, t, p: seq, cap=2)
    assert (count == 5).all() and lrec.shape[3] == 2
    cen = LT.centres(_spec(level_mask=1))
    got = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 2, _spec(level_mask=1, ord_max=2))
    _compare(got, 0, cen, [(0, 0.0), (2, 60.0)], "two crossings kept of five")          # the first two passages are mapped, the ones past the cap do not exist


def test_a_centre_exactly_on_a_shared_edge_is_a_hit_of_both_triangles():
    theta, phi = TLH._lattice()
    count = np.ones((1, theta.size, 1), dtype=np.int32)
    lrec = np.zeros((1, theta.size, 1, 1, LVL_STRIDE))
    lrec[0, :, 0, 0, LVL["DIR"]] = 1.0
    lrec[0, :, 0, 0, LVL["P0"]], lrec[0, :, 0, 0, LVL["P0"] + 1] = theta, phi           # crossing point = launch angles: exact arithmetic
    lrec[0, :, 0, 0, LVL["TTIME"]], lrec[0, :, 0, 0, LVL["ATTEN"]] = 100.0 + theta + phi, 2.0
    # centres at theta = 2 + 0.75 k, phi = -30 + 5 m, exactly: half of them on lattice lines, every (odd k, odd m) on a cell's diagonal a - c
    sp = LT.spec(origin=(TH0 - 0.375, PH0 - 2.5), step=(0.75, 5.0), n=(17, 13), n_theta=NT, n_phi=NP, edge_max=20.0, level_mask=1)
    cen = LT.centres(sp).reshape(17, 13, 2)
    assert np.array_equal(cen[..., 0], np.broadcast_to((TH0 + 0.75 * np.arange(17))[:, None], (17, 13))) and np.array_equal(cen[..., 1], np.broadcast_to(PH0 + 5.0 * np.arange(13), (17, 13)))
    m = LT.reference_level_tubemap(H.EQ_3D, count, lrec, theta, phi, 1, sp)
    c, f = m["count"][0, 0], m["first"][0, 0]
    cell = 2 * (NT - 1) + 3                                                            # cell (i, j) = (3, 2)
    assert c[7, 5] == 2 and f[7, 5] == 2 * cell                                        # on the diagonal of cell (3, 2): both its triangles, the smaller key first
    assert c[6, 5] == 2 and f[6, 5] == 2 * (cell - 1)                                  # on the edge a - d shared with cell (2, 2)
    assert c[6, 4] == 6                                                                # on the crossing point of ray (3, 2): six triangles meet there
    assert c[7, 4] == 2 and c[0, 5] == 1 and c[0, 0] == 2 and c[16, 0] == 1                # an edge along theta; the lattice's own border; corner a of a cell (both its triangles), corner b (one)
    k, mm = np.meshgrid(np.arange(17), np.arange(13), indexing="ij")
    interior = (k > 0) & (k < 16) & (mm > 0) & (mm < 12)
    assert (c[interior & (k % 2 == 1) & (mm % 2 == 1)] == 2).all() and (c[interior & ((k % 2 == 0) ^ (mm % 2 == 0))] == 2).all() and (c[interior & (k % 2 == 0) & (mm % 2 == 0)] == 6).all()
    assert np.array_equal(m["ttime_min"][0, 0], 100.0 + cen[..., 0] + cen[..., 1])      # exact: the weights are dyadic


# ---------------------------------------------------------------- the GPU cases' grids on the oracle
@functools.lru_cache(maxsize=None)
def _oracle(launch):
    import tempfile
    if LC.LAUNCHES[launch]["kind"] == "gridens":
        return _oracle("3drd")                                                         # (member 0 of the grid ensemble is that grid: the same bytes)
    return LC.oracle_crossings(LC.LAUNCHES[launch], tempfile.mkdtemp())


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_grid_literals_meet_the_conditions_on_the_oracle(name):
    """the non-vacuity conditions of the GPU cases hold for the reference map of the CPU oracle's path rows (tests/levels_reference.py makes the
    crossing tables of them): on every selected level cells with COUNT 0 and 1, and with COUNT >= 2 where the case claims multipath; no centre
    with more than 256 hits - the condition under which the list reduction is the definition.  They come from the physics and the chosen
    literals, not from the code under test."""
    case = LC.CASES[name]
    L = LC.LAUNCHES[case["launch"]]
    count, lrec, th, ph, nt, nph, legs = _oracle(case["launch"])
    sp = LC.spec_of(case, nt, nph)
    assert sp["n"][0] <= 32 and sp["n"][1] <= 48
    assert G.ltube_check(L["eq"], G.ltube_spec(**sp), th.size, len(L.get("levels", LC.LEVELS))) == (sp["n"][0] * sp["n"][1], len(LT.selected(sp)))
    ref = LT.reference_level_tubemap(L["eq"], count, lrec, th, ph, legs, sp)
    print(name, "cells with COUNT 0 / 1 / >= 2 per selected level:", LC.check_non_vacuity(ref, name), "most hits at a centre", int(ref["count"].max()))
    assert int(ref["count"].max()) <= LT.CAP
    if name == "slot-mix":
        n = LC.mixed_slot_hits(L["eq"], count, lrec, th, ph, legs, sp)
        print("hits whose corners hold their branch in different record slots:", n)
        assert n >= 3
    if case.get("cooperative"):
        # cells several times smaller than the crossing triangles: on the level the fan reaches widest the reached cells outnumber its triangles
        assert max(n1 + n2 for _, n1, n2 in LT.counts_per_level(ref)) >= 2 * 2 * (nt - 1) * (nph - 1)


def test_the_direction_and_level_cases_partition_the_base_case_on_the_oracle():
    count, lrec, th, ph, nt, nph, legs = _oracle("global")
    ref = {n: LT.reference_level_tubemap(H.EQ_GLOBAL, count, lrec, th, ph, legs, LC.spec_of(LC.CASES[n], nt, nph)) for n in ("global", "dir-up", "dir-down", "level-1", "levels-0-2", "edge-max", "leg-min-1")}
    assert np.array_equal(ref["dir-up"]["count"] + ref["dir-down"]["count"], ref["global"]["count"])
    for d in ("dir-up", "dir-down"):                                                   # each direction's branch planes reach cells on every selected level
        assert all(n1 + n2 > 0 for _, n1, n2 in LT.counts_per_level(ref[d])), (d, LT.counts_per_level(ref[d]))
    n_tri = 2 * (nt - 1) * (nph - 1)
    seen = {int(b) for b in np.unique(ref["global"]["first"][ref["global"]["first"] >= 0] // n_tri)}
    assert {0, 2, 4} <= seen, seen                                                     # FIRST names (leg 0, up), (leg 0, down) and (leg 1, up): b = ((leg * 2) + d) * 2
    assert np.array_equal(ref["level-1"]["count"][:, 0], ref["global"]["count"][:, 1]) and np.array_equal(ref["levels-0-2"]["count"], ref["global"]["count"][:, [0, 2]])
    for part in ("edge-max", ):
        assert (ref[part]["count"] <= ref["global"]["count"]).all() and int(ref[part]["count"].sum()) < int(ref["global"]["count"].sum())
    assert (ref["leg-min-1"]["count"] <= ref["global"]["count"][:, :2]).all() and 0 < int(ref["leg-min-1"]["count"].sum()) < int(ref["global"]["count"][:, :2].sum())


# ---------------------------------------------------------------- the closed form on the oracle
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form_under_a_raised_ground_on_the_oracle(eq, tmp_path):
    """the restatement on the oracle's paths through the raised-ground medium, held to the form that tests/test_gpu_ltubemap.py holds the device to:
    this proves the form, the conditions on the grid and the two bounds without the code under test"""
    import levels_reference as LV
    import raised_ground as RGD
    O = RGD.oracle(eq, tmp_path)
    cfg = H.make_cfg(eq, calc_amp=False, src=RGD.SRC[eq], z_grnd=RGD.Z_GRND, **RGD.LEVEL_PARAMS)
    th, ph, nt, nph = RGD.lattice()
    count, lrec = LV.restate_fan(eq, [O.trace_path(cfg, t, p) for t, p in zip(th, ph)], RGD.LEVELS, 8)
    sp = LC.rg_spec(eq)
    G.ltube_check(eq, G.ltube_spec(**sp), th.size, len(RGD.LEVELS))
    layers = LT.reference_level_tubemap(eq, count[None], lrec[None], th, ph, 2, sp)
    print(f"raised ground, oracle, {H.EQ_NAMES[eq]}, level tube map: " + LC.rg_figures(LC.check_raised_ground(eq, layers, count, lrec)))
