"""Level stations without a GPU (include/geoac_lstations.h): geoac_lstation_check on the host, the symbols of the header in the built library, and the
numpy restatement (tests/lstation_reference.py) alone on synthetic crossing tables whose answer is known by construction - an affine image of the
launch angles, neighbours whose leg-0 passages differ, a duct's second passage, a ray whose count ran past the crossing cap, and stations exactly on
an edge and on a crossing point."""
import ctypes

import numpy as np
import pytest

import harness as H
import lstation_reference as LS
from levels_reference import LVL, LVL_STRIDE

S = LS.LSTA
E_INVALID, E_NODEVICE, E_UNSUPPORTED = -1, -2, -4
NT, NP = 9, 7


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _lattice(n_theta=NT, n_phi=NP, theta0=2.0, dtheta=1.5, phi0=-30.0, dphi=10.0):
    th_ax, ph_ax = theta0 + dtheta * np.arange(n_theta), phi0 + dphi * np.arange(n_phi)
    return np.tile(th_ax, n_phi), np.repeat(ph_ax, n_theta)


# an affine (invertible) image of the launch angles, shifted per passage so that no two branches share their image
A = np.array([[12.0, -3.0], [2.0, 9.0]])
B0 = np.array([-40.0, 15.0])


def _affine(theta, phi, shift=0.0):
    return A[0, 0] * theta + A[0, 1] * phi + B0[0] + shift, A[1, 0] * theta + A[1, 1] * phi + B0[1] - 0.4 * shift


def _table(theta, phi, passages, cap=8, n_levels=1, level=0):
    """Cartesian crossing tables count [1][n_rays][L], lrec [1][n_rays][L][cap][12]: passages(i_ray, theta, phi) -> the ray's passages through
    `level` in path order, each (leg, dir, shift); a passage lies at _affine(theta, phi, shift), its other columns are affine in the angles too.
    The count runs past cap, the records keep the first cap."""
    n = theta.size
    count = np.zeros((1, n, n_levels), dtype=np.int32)
    lrec = np.zeros((1, n, n_levels, cap, LVL_STRIDE))
    for r in range(n):
        seq = passages(r, theta[r], phi[r])
        count[0, r, level] = len(seq)
        for k, (leg, direction, shift) in enumerate(seq[:cap]):
            x, y = _affine(theta[r], phi[r], shift)
            R = lrec[0, r, level, k]
            R[LVL["LEG"]], R[LVL["DIR"]], R[LVL["FRAC"]] = leg, direction, 0.5
            R[LVL["TTIME"]] = 100.0 + 3.0 * theta[r] + 0.5 * phi[r] + shift
            R[LVL["ATTEN"]] = 1.0 + 0.01 * theta[r]
            R[LVL["P0"]:LVL["P0"] + 6] = x, y, 35.0, 0.002 * theta[r], -0.001 * phi[r], 0.003
    return count, lrec


def _pre_images(n, seed, theta, phi):
    rng = np.random.default_rng(seed)
    return rng.uniform(theta.min(), theta.max(), n), rng.uniform(phi.min(), phi.max(), n)


def _spec(G, **kw):
    return G.lstation_spec(**dict(dict(n_theta=NT, n_phi=NP), **kw))


# ---------------------------------------------------------------- the host-only check
def test_lstation_check_accepts_and_refuses(G):
    lv = [0, 2, 1, 2]
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        G.lstation_check(eq, _spec(G), 63, 3, lv)
        G.lstation_check(eq, _spec(G, phi_periodic=True, leg_min=1, leg_max=1, ord_max=64, edge_max=5.0, cap=256), 63, 8, [7])
    bad = [(dict(), 64, 3, lv, "n_theta \\* n_phi"), (dict(n_theta=1, n_phi=63), 63, 3, lv, "at least 2"), (dict(cap=0), 63, 3, lv, "cap"), (dict(cap=257), 63, 3, lv, "cap"),
           (dict(ord_max=0), 63, 3, lv, "ord_max"), (dict(ord_max=65), 63, 3, lv, "ord_max"), (dict(edge_max=0.0), 63, 3, lv, "edge_max"),
           (dict(edge_max=float("nan")), 63, 3, lv, "edge_max"), (dict(leg_min=2, leg_max=1), 63, 3, lv, "leg_min"), (dict(leg_min=-1), 63, 3, lv, "leg_min"),
           (dict(), 63, 0, lv, "n_levels"), (dict(), 63, 9, lv, "n_levels"), (dict(), 63, 3, [], "n_sta")]
    for kw, n_rays, n_levels, level_of, word in bad:
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            G.lstation_check(G.EQ_3D, _spec(G, **kw), n_rays, n_levels, level_of)
    spec = _spec(G)
    spec.phi_periodic = 2
    with pytest.raises(G.GeoAcError, match="phi_periodic"):
        G.lstation_check(G.EQ_GLOBAL, spec, 63, 3, lv)


def test_level_of_out_of_range_is_refused(G):
    for level_of in ([0, 3], [-1, 0], [0, 1, 2, 8]):
        with pytest.raises(G.GeoAcError, match="invalid.*level_of.*0 \\.\\. n_levels - 1"):
            G.lstation_check(G.EQ_3D, _spec(G), 63, 3, level_of)
    lib = G.load_library()
    lib.geoac_lstation_fault.restype = ctypes.c_char_p
    assert lib.geoac_lstation_check(G.EQ_3D, ctypes.byref(_spec(G)), 63, 3, 2, None) == E_INVALID
    assert b"level_of is NULL" in lib.geoac_lstation_fault(G.EQ_3D, ctypes.byref(_spec(G)), 63, 3, 2, None)
    assert lib.geoac_lstation_fault(G.EQ_3D, ctypes.byref(_spec(G)), 63, 3, 2, (ctypes.c_int32 * 2)(2, 0)) is None


def test_two_d_set_is_unsupported(G):
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.lstation_check(G.EQ_2D, _spec(G), 63, 3, [0])
    assert G.load_library().geoac_lstation_check(G.EQ_2D, ctypes.byref(_spec(G)), 63, 3, 1, (ctypes.c_int32 * 1)(0)) == E_UNSUPPORTED


def test_header_symbols_and_python_mirror(G):
    lib = G.load_library()
    for name in ("geoac_lstation_check", "geoac_lstation_fault", "geoac_fan_level_stations", "geoac_fan_level_stations_shape", "geoac_fan_level_stations_fetch",
                 "geoac_fan_level_stations_dev", "geoac_fan_level_stations_timing"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    assert hasattr(G.FanContext, "level_stations") and hasattr(G.FanContext, "level_stations_timing")
    kw = dict(n_theta=9, n_phi=7, phi_periodic=True, leg_min=1, leg_max=3, ord_max=2, edge_max=40.0, cap=5)
    sp, ref = G.lstation_spec(**kw), LS.spec(**kw)
    assert {k: (bool(getattr(sp, k)) if k == "phi_periodic" else getattr(sp, k)) for k in kw} == ref
    assert G.LSTA == LS.LSTA and G.LSTA_STRIDE == LS.LSTA_STRIDE


def test_compute_entry_points_need_a_device(G):
    """there is no host path: a context is what every compute entry point of the header takes, and without a usable HIP device none can be made
    (GEOAC_E_NODEVICE); with one, the call is refused until a launch with levels has completed"""
    import torch
    lib = G.load_library()
    h = ctypes.c_void_p()
    rc = lib.geoac_create(ctypes.byref(h), G.EQ_3D, 0)
    if not torch.cuda.is_available():
        assert rc == E_NODEVICE and not h
        with pytest.raises(G.GeoAcError, match="no usable HIP device"):
            G.FanContext(G.EQ_3D)
    else:
        assert rc == 0
        lv = (ctypes.c_int32 * 1)(0)
        sta = (ctypes.c_double * 2)(0.0, 0.0)
        assert lib.geoac_fan_level_stations(h, ctypes.byref(_spec(G)), 1, sta, lv) == E_INVALID
        lib.geoac_destroy(h)
    hits = (ctypes.c_uint32 * 1)()
    assert lib.geoac_fan_level_stations(None, ctypes.byref(_spec(G)), 1, None, None) < 0                     # (no context: never a result)
    assert lib.geoac_fan_level_stations_fetch(None, hits, None) < 0 and lib.geoac_fan_level_stations_timing(None, None) < 0


# ---------------------------------------------------------------- the restatement on tables known by construction
def test_affine_image_returns_the_pre_image():
    theta, phi = _lattice()
    count, lrec = _table(theta, phi, lambda r, t, p: [(0, 1.0, 0.0), (0, -1.0, 700.0)], n_levels=2, level=1)
    t_in, p_in = _pre_images(120, 7, theta, phi)
    up = np.stack(_affine(t_in, p_in, 0.0), axis=1)
    down = np.stack(_affine(t_in, p_in, 700.0), axis=1)
    sta = np.concatenate([up, down, up])
    level_of = np.concatenate([np.full(240, 1), np.full(120, 0)])                      # the last 120: the same places on a level nothing crosses
    hits, rows = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 2, LS.spec(NT, NP, cap=4), sta, level_of)
    assert hits.shape == (1, 360) and rows.shape == (1, 360, 4, 16)
    assert (hits[0, :240] == 1).all() and (hits[0, 240:] == 0).all() and (rows[0, 240:] == 0).all() and (rows[0, :, 1:] == 0).all()
    r = rows[0, :240, 0]
    assert np.allclose(r[:, S["THETA"]], np.tile(t_in, 2), rtol=1e-12, atol=0) and np.allclose(r[:, S["PHI"]], np.tile(p_in, 2), rtol=1e-12, atol=1e-12)
    assert (r[:, S["LEG"]] == 0).all() and (r[:, S["ORD"]] == 0).all() and (r[:120, S["DIR"]] == 1.0).all() and (r[120:, S["DIR"]] == -1.0).all()
    assert np.allclose(r[:, S["W0"]] + r[:, S["W1"]] + r[:, S["W2"]], 1.0, rtol=1e-14) and len(set(r[:, S["ORIENT"]])) == 1
    # the other columns are affine in the angles too: the interpolant reproduces them
    assert np.allclose(r[:, S["TTIME"]], 100.0 + 3.0 * np.tile(t_in, 2) + 0.5 * np.tile(p_in, 2) + np.repeat([0.0, 700.0], 120), rtol=1e-12)
    assert np.allclose(r[:, S["ATTEN"]], 1.0 + 0.01 * np.tile(t_in, 2), rtol=1e-12)
    assert np.allclose(r[:, S["N0"]], 0.002 * np.tile(t_in, 2), rtol=1e-12) and np.allclose(r[:, S["N0"] + 1], -0.001 * np.tile(p_in, 2), rtol=1e-12, atol=1e-15)
    assert np.allclose(r[:, S["N0"] + 2], 0.003, rtol=1e-12)


def test_neighbours_with_different_leg0_passages_pair_their_leg1_branch():
    """inclination rows 0 .. 4 turn below the level on leg 0 (no passage), rows 5 .. 8 pass it upward and downward; every ray passes it upward on leg 1.
    The leg-1 passage sits in slot 0 of the first and in slot 2 of the others: matched by slot the cells of column i = 4 would pair a leg-1 with a
    leg-0 passage, matched by branch every cell has its leg-1 triangle and the leg-0 branches have none in that column"""
    theta, phi = _lattice()

    def passages(r, t, p):
        return ([(0, 1.0, 0.0), (0, -1.0, 700.0)] if r % NT >= 5 else []) + [(1, 1.0, 2000.0)]
    count, lrec = _table(theta, phi, passages)
    assert set(count[0, :, 0]) == {1, 3}
    t_in, p_in = _pre_images(150, 11, theta, phi)
    sp = LS.spec(NT, NP, cap=4)
    c0, c1, slot, present = LS.branch_table(H.EQ_3D, count, lrec, sp, 2)
    assert present.shape == (1, 1, 4, 63) and present[0, 0, 2].all() and not present[0, 0, 3].any()          # branch 2 = (leg 1, up, 0), 3 = (leg 1, down, 0)
    assert set(slot[0, 0, 2]) == {0, 2}
    hits, rows = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 2, sp, np.stack(_affine(t_in, p_in, 2000.0), axis=1), np.zeros(150, dtype=int))
    assert (hits == 1).all()
    r = rows[0, :, 0]
    assert (r[:, S["LEG"]] == 1).all() and (r[:, S["DIR"]] == 1.0).all() and (r[:, S["ORD"]] == 0).all()
    assert np.allclose(r[:, S["THETA"]], t_in, rtol=1e-12) and np.allclose(r[:, S["PHI"]], p_in, rtol=1e-12, atol=1e-12)
    straddle = (r[:, S["TRI"]].astype(int) // 2) % (NT - 1) == 4
    assert straddle.sum() >= 5                                                         # (some of the stations lie in the column where the slots differ)
    assert np.allclose(r[:, S["TTIME"]], 2100.0 + 3.0 * t_in + 0.5 * p_in, rtol=1e-12)   # ... and read the leg-1 record of every corner
    # leg 0 upward: only where all three corners pass (rows 5 .. 8: the cells of columns i = 5, 6, 7)
    h0, r0 = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 2, LS.spec(NT, NP, leg_max=0, cap=4), np.stack(_affine(t_in, p_in, 0.0), axis=1), np.zeros(150, dtype=int))
    inside = t_in > theta[5]
    assert np.array_equal(h0[0] == 1, inside) and (h0[0][~inside] == 0).all()


def test_a_ducted_ray_serves_its_second_passage_as_ordinal_1():
    theta, phi = _lattice()
    count, lrec = _table(theta, phi, lambda r, t, p: [(0, 1.0, 0.0), (0, -1.0, 700.0), (0, 1.0, 1400.0), (0, -1.0, 2100.0)])
    t_in, p_in = _pre_images(80, 13, theta, phi)
    sta = np.stack(_affine(t_in, p_in, 1400.0), axis=1)
    lv = np.zeros(80, dtype=int)
    h1, _ = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 1, LS.spec(NT, NP, ord_max=1, cap=4), sta, lv)
    assert (h1 == 0).all()                                                             # ord_max = 1: the second upward passage takes no part
    h2, r2 = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 1, LS.spec(NT, NP, ord_max=2, cap=4), sta, lv)
    assert (h2 == 1).all()
    r = r2[0, :, 0]
    assert (r[:, S["ORD"]] == 1).all() and (r[:, S["DIR"]] == 1.0).all() and (r[:, S["LEG"]] == 0).all()
    assert np.allclose(r[:, S["THETA"]], t_in, rtol=1e-12) and np.allclose(r[:, S["TTIME"]], 1500.0 + 3.0 * t_in + 0.5 * p_in, rtol=1e-12)


def test_a_count_past_the_crossing_cap_still_serves_the_kept_branches():
    theta, phi = _lattice()
    seq = [(0, 1.0, 0.0), (0, -1.0, 700.0), (0, 1.0, 1400.0), (0, -1.0, 2100.0), (1, 1.0, 2800.0)]
    count, lrec = _table(theta, phi, lambda r, t, p: seq, cap=2)
    assert (count == 5).all() and lrec.shape[3] == 2
    t_in, p_in = _pre_images(60, 17, theta, phi)
    sta = np.concatenate([np.stack(_affine(t_in, p_in, sh), axis=1) for sh in (0.0, 700.0, 1400.0, 2800.0)])
    hits, rows = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 2, LS.spec(NT, NP, ord_max=2, cap=4), sta, np.zeros(240, dtype=int))
    assert (hits[0, :120] == 1).all() and (hits[0, 120:] == 0).all()                    # the first two passages hit, the ones past the cap do not exist
    assert (rows[0, :60, 0, S["DIR"]] == 1.0).all() and (rows[0, 60:120, 0, S["DIR"]] == -1.0).all()
    full = _table(theta, phi, lambda r, t, p: seq, cap=8)
    hf, rf = LS.reference_level_stations(H.EQ_3D, *full, theta, phi, 2, LS.spec(NT, NP, ord_max=2, cap=4), sta, np.zeros(240, dtype=int))
    assert (hf == 1).all() and np.array_equal(rf[0, :120], rows[0, :120])               # ... with the ordinals they have in the uncapped records


def test_shared_edge_and_crossing_point():
    theta, phi = _lattice()
    count = np.ones((1, theta.size, 1), dtype=np.int32)
    lrec = np.zeros((1, theta.size, 1, 1, LVL_STRIDE))
    lrec[0, :, 0, 0, LVL["DIR"]] = 1.0
    lrec[0, :, 0, 0, LVL["P0"]], lrec[0, :, 0, 0, LVL["P0"] + 1] = theta, phi           # crossing point = launch angles: exact arithmetic
    sta = np.array([[2.0 + 1.5 * 3 + 0.75, -30.0 + 10.0 * 2 + 5.0],                     # on the diagonal a - c of cell (3, 2)
                    [2.0 + 1.5 * 3, -30.0 + 10.0 * 2 + 5.0],                            # on the edge a - d shared with cell (2, 2)
                    [2.0 + 1.5 * 3, -30.0 + 10.0 * 2]])                                 # on the crossing point of ray (3, 2): six triangles meet there
    hits, rows = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 1, LS.spec(NT, NP, cap=8), sta, [0, 0, 0])
    assert hits[0].tolist() == [2, 2, 6]
    cell = 2 * 8 + 3
    assert rows[0, 0, :2, S["TRI"]].tolist() == [2 * cell, 2 * cell + 1]
    assert rows[0, 1, :2, S["TRI"]].tolist() == [2 * (cell - 1), 2 * cell + 1]
    assert (np.diff(rows[0, 2, :6, S["TRI"]]) > 0).all()                                # key order
    assert np.allclose(rows[0, :, :2, S["THETA"]], sta[:, :1]) and np.allclose(rows[0, :, :2, S["PHI"]], sta[:, 1:])
    # the cap keeps the smallest keys and hits counts all
    h2, r2 = LS.reference_level_stations(H.EQ_3D, count, lrec, theta, phi, 1, LS.spec(NT, NP, cap=3), sta, [0, 0, 0])
    assert np.array_equal(h2, hits) and np.array_equal(r2, rows[:, :, :3])
