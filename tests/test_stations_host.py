"""Station arrivals without a GPU (include/geoac_stations.h): geoac_station_check on the host, the numpy restatement (tests/station_reference.py) on
synthetic record tables whose landing map is known in closed form - an affine map, a map folded once, filters, the azimuth seam - and the symbols
of the header in the built library."""
import ctypes

import numpy as np
import pytest

import harness as H
import station_reference as SR

S = SR.STA


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _lattice(n_theta=9, n_phi=7, theta0=2.0, dtheta=1.5, phi0=-30.0, dphi=10.0):
    th_ax, ph_ax = theta0 + dtheta * np.arange(n_theta), phi0 + dphi * np.arange(n_phi)
    return np.tile(th_ax, n_phi), np.repeat(ph_ax, n_theta)


def _table(theta, phi, land, legs=2, turn=None):
    """a Cartesian record table [1][n_rays][legs][32] whose landing point on leg l is land(theta, phi, l); the other columns are smooth in the angles"""
    n = theta.size
    rec = np.zeros((1, n, legs, H.REC_STRIDE))
    for leg in range(legs):
        x, y = land(theta, phi, leg)
        rec[0, :, leg, H.REC["VALID"]] = 1.0
        rec[0, :, leg, H.REC["STATE"] + 0] = x
        rec[0, :, leg, H.REC["STATE"] + 1] = y
        rec[0, :, leg, H.REC["TTIME"]] = 1000.0 * (leg + 1) + 3.0 * theta + 0.5 * phi
        rec[0, :, leg, H.REC["RANGE"]] = 300.0 * (leg + 1) + theta - 0.25 * phi
        rec[0, :, leg, H.REC["TURN"]] = (40.0 + theta) if turn is None else turn(theta, phi, leg)
        rec[0, :, leg, H.REC["INCL"]] = theta
        rec[0, :, leg, H.REC["BACKAZ"]] = phi
    level = -(rec[..., H.REC["TTIME"]] / 100.0)[:, None]
    return rec, level


# an affine landing map (invertible): x = A (theta, phi) + b, shifted per leg
A = np.array([[12.0, -3.0], [2.0, 9.0]])
B = np.array([-40.0, 15.0])


def _affine(theta, phi, leg):
    return A[0, 0] * theta + A[0, 1] * phi + B[0] + 500.0 * leg, A[1, 0] * theta + A[1, 1] * phi + B[1] - 200.0 * leg


def test_station_check_accepts_and_refuses(G):
    good = dict(n_theta=9, n_phi=7)
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        G.station_check(eq, G.station_spec(**good), 63, 200)
        G.station_check(eq, G.station_spec(phi_periodic=True, leg_min=1, leg_max=1, turn_tol=0.0, edge_max=5.0, cap=256, **good), 63, 1)
    bad = [(dict(good), 64, 10, "n_theta \\* n_phi"), (dict(good, n_theta=1, n_phi=63), 63, 10, "at least 2"), (dict(good, cap=0), 63, 10, "cap"), (dict(good, cap=257), 63, 10, "cap"),
           (dict(good, turn_tol=float("nan")), 63, 10, "turn_tol"), (dict(good, turn_tol=-1.0), 63, 10, "turn_tol"), (dict(good, edge_max=0.0), 63, 10, "edge_max"),
           (dict(good, edge_max=float("nan")), 63, 10, "edge_max"), (dict(good, leg_min=2, leg_max=1), 63, 10, "leg_min"), (dict(good, leg_min=-1), 63, 10, "leg_min"),
           (dict(good), 63, 0, "n_sta")]
    for kw, n_rays, n_sta, word in bad:
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            G.station_check(G.EQ_3D, G.station_spec(**kw), n_rays, n_sta)
    spec = G.station_spec(**good)
    spec.phi_periodic = 2
    with pytest.raises(G.GeoAcError, match="phi_periodic"):
        G.station_check(G.EQ_GLOBAL, spec, 63, 10)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set.*interval"):
        G.station_check(G.EQ_2D, G.station_spec(**good), 63, 10)
    assert G.load_library().geoac_station_check(G.EQ_2D, ctypes.byref(G.station_spec(**good)), 63, 10) == -4


def test_python_spec_mirrors_the_reference_spec(G):
    kw = dict(n_theta=9, n_phi=7, phi_periodic=True, leg_min=1, leg_max=3, turn_tol=2.5, edge_max=40.0, cap=5)
    sp, ref = G.station_spec(**kw), SR.spec(**kw)
    assert {k: (bool(getattr(sp, k)) if k == "phi_periodic" else getattr(sp, k)) for k in kw} == ref
    assert G.STA == SR.STA and G.STA_STRIDE == SR.STA_STRIDE


def test_affine_map_one_hit_per_leg_at_the_pre_image():
    theta, phi = _lattice()
    rec, level = _table(theta, phi, _affine)
    rng = np.random.default_rng(7)
    n_in = 150
    # pre-images strictly inside the lattice's range, away from lattice lines (a station on a shared edge is a hit of both triangles)
    t_in = rng.uniform(theta.min(), theta.max(), n_in)
    p_in = rng.uniform(phi.min(), phi.max(), n_in)
    inside = np.stack(_affine(t_in, p_in, 0), axis=1)
    t_out = np.concatenate([rng.uniform(theta.max() + 0.5, theta.max() + 9.0, 25), rng.uniform(theta.min() - 9.0, theta.min() - 0.5, 25)])
    p_out = rng.uniform(phi.min() - 40.0, phi.max() + 40.0, 50)
    outside = np.stack(_affine(t_out, p_out, 0), axis=1)
    sta = np.concatenate([inside, outside])
    sp = SR.spec(9, 7, leg_max=0, cap=4)
    hits, rows, lvl = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, sp, sta)
    assert hits.shape == (1, 200) and rows.shape == (1, 200, 4, 16) and lvl.shape == (1, 200, 4, 1)
    assert (hits[0, :n_in] == 1).all() and (hits[0, n_in:] == 0).all()
    r = rows[0, :n_in, 0]
    assert np.allclose(r[:, S["THETA"]], t_in, rtol=1e-12, atol=0) and np.allclose(r[:, S["PHI"]], p_in, rtol=1e-12, atol=1e-12)
    assert (r[:, S["LEG"]] == 0).all() and np.allclose(r[:, S["W0"]] + r[:, S["W1"]] + r[:, S["W2"]], 1.0, rtol=1e-14)
    # every other column is affine in the angles too: the interpolant reproduces it
    assert np.allclose(r[:, S["TTIME"]], 1000.0 + 3.0 * t_in + 0.5 * p_in, rtol=1e-12)
    assert np.allclose(r[:, S["CELERITY"]], (300.0 + t_in - 0.25 * p_in) / r[:, S["TTIME"]], rtol=1e-12)
    assert np.allclose(r[:, S["TURN"]], 40.0 + t_in, rtol=1e-12) and np.allclose(r[:, S["INCL"]], t_in, rtol=1e-12) and np.allclose(r[:, S["BACKAZ"]], p_in, rtol=1e-12, atol=1e-12)
    assert np.allclose(lvl[0, :n_in, 0, 0], -r[:, S["TTIME"]] / 100.0, rtol=1e-12)
    assert (rows[0, :, 1:] == 0).all() and (rows[0, n_in:] == 0).all() and (rows[..., 14:] == 0).all()
    assert len(set(r[:, S["ORIENT"]])) == 1                                        # an affine map has one orientation
    # both legs: the stations of leg 0 are not in the image of leg 1 (shifted by 500 km), its own stations are
    sta1 = np.stack(_affine(t_in, p_in, 1), axis=1)
    hits2, rows2, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, cap=4), np.concatenate([inside, sta1]))
    assert (hits2 == 1).all() and (rows2[0, :n_in, 0, S["LEG"]] == 0).all() and (rows2[0, n_in:, 0, S["LEG"]] == 1).all()
    assert np.allclose(rows2[0, n_in:, 0, S["THETA"]], t_in, rtol=1e-12)


def test_shared_edge_is_a_hit_of_both_triangles():
    theta, phi = _lattice()
    ident = lambda t, p, leg: (t.copy(), p.copy())                                  # noqa: E731  landing point = launch angles: exact arithmetic
    rec, level = _table(theta, phi, ident, legs=1)
    sta = np.array([[2.0 + 1.5 * 3 + 0.75, -30.0 + 10.0 * 2 + 5.0],                 # on the diagonal a - c of cell (3, 2)
                    [2.0 + 1.5 * 3, -30.0 + 10.0 * 2 + 5.0],                        # on the edge a - d shared with cell (2, 2)
                    [2.0 + 1.5 * 3, -30.0 + 10.0 * 2]])                             # on lattice point (3, 2): six triangles meet there
    hits, rows, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, cap=8), sta)
    assert hits[0].tolist() == [2, 2, 6]
    cell = 2 * 8 + 3
    assert rows[0, 0, :2, S["TRI"]].tolist() == [2 * cell, 2 * cell + 1]
    assert rows[0, 1, :2, S["TRI"]].tolist() == [2 * (cell - 1), 2 * cell + 1]
    assert (np.diff(rows[0, 2, :6, S["TRI"]]) > 0).all()                            # key order
    assert np.allclose(rows[0, :, :2, S["THETA"]], sta[:, :1]) and np.allclose(rows[0, :, :2, S["PHI"]], sta[:, 1:])


def test_fold_gives_two_hits_of_opposite_orientation():
    theta, phi = _lattice(n_theta=21, dtheta=1.0)                                   # theta 2 .. 22
    fold = lambda t, p, leg: (100.0 - (t - 12.0) ** 2, 3.0 * p)                     # noqa: E731  x folds at theta = 12: x <= 100, two pre-images below
    rec, level = _table(theta, phi, fold, legs=1)
    rng = np.random.default_rng(11)
    n = 60
    x = rng.uniform(100.0 - 9.0 ** 2, 100.0 - 1.5 ** 2, n)                          # both pre-images 12 -+ sqrt(100 - x) lie inside 2 .. 22, off the fold's cell
    y = rng.uniform(3.0 * phi.min() + 1.0, 3.0 * phi.max() - 1.0, n)
    beyond = np.stack([rng.uniform(100.5, 140.0, 20), rng.uniform(3.0 * phi.min(), 3.0 * phi.max(), 20)], axis=1)          # past the fold: no ray lands there
    hits, rows, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(21, 7, cap=4), np.concatenate([np.stack([x, y], axis=1), beyond]))
    assert (hits[0, :n] == 2).all() and (hits[0, n:] == 0).all()
    assert (rows[0, :n, 0, S["ORIENT"]] * rows[0, :n, 1, S["ORIENT"]] == -1.0).all()
    root = np.sqrt(100.0 - x)
    got = np.sort(rows[0, :n, :2, S["THETA"]], axis=1)
    assert np.abs(got[:, 0] - (12.0 - root)).max() < 0.2 and np.abs(got[:, 1] - (12.0 + root)).max() < 0.2               # first order: within a fraction of the 1-degree step
    assert np.allclose(rows[0, :n, :2, S["PHI"]], (y / 3.0)[:, None], rtol=1e-12, atol=1e-12)


def test_turn_tol_and_edge_max_remove_exactly_their_triangles():
    theta, phi = _lattice()
    nt = 9
    # turning height jumps by 60 km between inclination rows 4 and 5: exactly the triangles of cell column i = 4 span the jump
    turn = lambda t, p, leg: np.where(t > 2.0 + 1.5 * 4.5, 110.0, 50.0) + 0.01 * t  # noqa: E731
    # and the landing map jumps by 1 000 km in x between azimuth columns 2 and 3: the cells j = 2 have long sides
    land = lambda t, p, leg: (12.0 * t + np.where(p > -30.0 + 10.0 * 2.5, 1000.0, 0.0), 9.0 * p)          # noqa: E731
    rec, level = _table(theta, phi, land, legs=1, turn=turn)
    tri = SR.triangles(SR.spec(9, 7))
    cent = np.stack([rec[0, tri, 0, 12].mean(axis=1), rec[0, tri, 0, 13].mean(axis=1)], axis=1)          # every triangle's centroid is a station
    cell = np.arange(len(tri)) // 2
    ci, cj = cell % (nt - 1), cell // (nt - 1)

    def found(**kw):
        hits, rows, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, cap=8, **kw), cent)
        own = np.array([k in rows[0, k, :hits[0, k], S["TRI"]] for k in range(len(tri))])
        return own

    assert found().all()
    assert np.array_equal(found(turn_tol=5.0), ci != 4)
    assert np.array_equal(found(edge_max=200.0), cj != 2)
    assert np.array_equal(found(turn_tol=5.0, edge_max=200.0), (ci != 4) & (cj != 2))
    assert found(turn_tol=60.1, edge_max=1100.0).all()


def test_periodic_seam():
    n_theta, n_phi = 6, 36
    theta, phi = _lattice(n_theta=n_theta, n_phi=n_phi, theta0=5.0, dtheta=5.0, phi0=-180.0, dphi=10.0)               # azimuths -180 .. 170
    ring = lambda t, p, leg: ((100.0 + 10.0 * t) * np.sin(np.radians(p)), (100.0 + 10.0 * t) * np.cos(np.radians(p)))   # noqa: E731
    rec, level = _table(theta, phi, ring, legs=1)
    rec[0, :, 0, H.REC["BACKAZ"]] = np.where(phi + 180.0 >= 180.0, phi + 180.0 - 360.0, phi + 180.0)                 # back azimuth, itself wrapped into -180 .. 180
    az = np.array([172.0, 175.0, 178.5])                                                                            # between column 35 (170) and column 0 (-180 = 180)
    rad = np.array([170.0, 220.0, 260.0])
    behind = np.stack([rad * np.sin(np.radians(az)), rad * np.cos(np.radians(az))], axis=1)
    front = np.stack([rad * np.sin(np.radians(az - 90.0)), rad * np.cos(np.radians(az - 90.0))], axis=1)
    sta = np.concatenate([behind, front])
    h0, _, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(n_theta, n_phi, cap=4), sta)
    h1, r1, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(n_theta, n_phi, phi_periodic=True, cap=4), sta)
    assert h0[0].tolist() == [0, 0, 0, 1, 1, 1] and h1[0].tolist() == [1, 1, 1, 1, 1, 1]
    seam = r1[0, :3, 0]
    ray0 = seam[:, S["RAY0"]].astype(int)
    assert (ray0 // n_theta == n_phi - 1).all()                                     # corner 0 lies in the last column, phi = 170
    assert ((seam[:, S["PHI"]] > 170.0) & (seam[:, S["PHI"]] < 180.0)).all()          # continuous with corner 0: 170 .. 180, not an average of 170 and -180
    assert np.abs(seam[:, S["PHI"]] - az).max() < 1.0
    assert np.abs(seam[:, S["BACKAZ"]] - (az - 180.0)).max() < 1.0                  # corner 0's back azimuth is -10; the corners at +0 are brought to it
    assert np.abs(r1[0, 3:, 0, S["PHI"]] - (az - 90.0)).max() < 1.0


def test_spherical_longitude_difference_is_wrapped():
    theta, phi = _lattice()
    # landing points around lon 180: lon runs 176 .. 188 (the state's longitude is continuous), stations given as -178 .. -172
    land = lambda t, p, leg: (np.radians(20.0 + 0.5 * t), np.radians(182.0 + 0.1 * p))          # noqa: E731
    rec, level = _table(theta, phi, lambda t, p, leg: (0 * t, 0 * t), legs=1)
    lat, lon = land(theta, phi, 0)
    rec[0, :, 0, 13], rec[0, :, 0, 14] = lat, lon
    sta = np.array([[23.1, 183.3], [23.1, 183.3 - 360.0], [23.1, 3.3]])
    hits, rows, _ = SR.reference_stations(H.EQ_GLOBAL, rec, theta, phi, level, SR.spec(9, 7, cap=2, edge_max=5.0), sta)
    assert hits[0].tolist() == [1, 1, 0]
    assert np.allclose(rows[0, 0, 0, [S["THETA"], S["PHI"]]], [6.2, 13.0], rtol=1e-9) and np.allclose(rows[0, 1, 0, 7:9], rows[0, 0, 0, 7:9], rtol=1e-12)


def test_cap_keeps_the_smallest_keys_and_hits_counts_all():
    theta, phi = _lattice()
    rec, level = _table(theta, phi, lambda t, p, leg: (t.copy(), p.copy()), legs=3)          # every leg lands at the same place: three hits per station
    sta = np.array([[5.3, -11.0], [9.9, 22.0]])
    full = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, cap=8), sta)
    assert full[0][0].tolist() == [3, 3] and full[1][0, :, :3, S["LEG"]].tolist() == [[0, 1, 2]] * 2
    for cap in (1, 2):
        h, r, lv = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, cap=cap), sta)
        assert np.array_equal(h, full[0]) and np.array_equal(r, full[1][:, :, :cap]) and np.array_equal(lv, full[2][:, :, :cap])
    h, r, _ = SR.reference_stations(H.EQ_3D, rec, theta, phi, level, SR.spec(9, 7, leg_min=1, leg_max=7, cap=8), sta)
    assert h[0].tolist() == [2, 2] and r[0, :, :2, S["LEG"]].tolist() == [[1, 2]] * 2


def test_lattice_check():
    theta, phi = _lattice()
    assert SR.is_lattice(theta, phi, 9, 7) and not SR.is_lattice(theta, phi, 7, 9) and not SR.is_lattice(theta[:-1], phi[:-1], 9, 7)
    t2 = theta.copy()
    t2[20] = np.nextafter(t2[20], 100.0)
    assert not SR.is_lattice(t2, phi, 9, 7)
    th, ph = H.fan_angles(theta_min=1.0, theta_max=30.0, theta_step=0.7, phi_min=-60.0, phi_max=-20.0, phi_step=3.3)          # the reference's repeated additions
    n_theta = int(np.flatnonzero(ph != ph[0])[0])
    assert SR.is_lattice(th, ph, n_theta, th.size // n_theta)


def test_header_symbols_exist_in_the_built_library(G):
    lib = G.load_library()
    for name in ("geoac_station_check", "geoac_station_fault", "geoac_fan_stations", "geoac_fan_stations_shape", "geoac_fan_stations_fetch", "geoac_fan_stations_dev",
                 "geoac_fan_stations_timing"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    assert hasattr(G.FanContext, "stations") and hasattr(G.FanContext, "stations_timing")
