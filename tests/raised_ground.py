"""One medium in which every post-launch product has an answer that owes nothing to the code: the isothermal windless profile of
tests/known_answers.py, a source 20 km above a ground raised to 1.5 km, and a full-circle lattice of rays launched downward.  Pure numpy, no GPU
code: tests/test_raised_ground_host.py holds the plain-C oracle's records and the numpy restatements to these forms, tests/test_gpu_raised_ground.py
the device.

Cartesian sets: the ray (theta, phi), a = |theta|, lands at src_xy + (h / tan a)(sin phi, cos phi) on z = z_grnd after h / (c sin a) seconds.  The
reference's arrival record is the first row BELOW the ground, at most its shortest step (1 m of path) on: the launch records are held to these forms
at that row's own height (to 1e-9), and to the forms on z = z_grnd itself within that step.
Spherical sets: the reference's rays bend in this medium (known_answers.check_straight_rays), so there is no chord formula; the launch is
axially symmetric about the source's vertical, which the tests assert on the launch's own records before they take the ring radius of an
inclination from its phi = 0 column."""
import os

import numpy as np

import harness as H
import known_answers as K
import station_cases as SC
import station_reference as SR

T0 = 250.0
C = float(np.sqrt(K.GAM_R * T0))
Z_GRND, Z_SRC = 1.5, 21.5
HGT = Z_SRC - Z_GRND                                 # the source stands 20 km above the ground
R_EARTH = K.R_EARTH
RG = R_EARTH + Z_GRND                                # ground radius: what a miss on the ground is measured on
SCALE_HEIGHT = 8.0
CARTESIAN = (H.EQ_3D, H.EQ_3D_RNGDEP)
SPHERICAL = (H.EQ_GLOBAL, H.EQ_GLOBAL_RNGDEP)
ALL_SETS = [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP]
# off the origin (RANGE and CELERITY of the ground products are measured from the origin, GEOAC_LRF_CELERITY from the source point); the spherical
# landing ring of the stratified set straddles the date line; the grid's longitude axis is monotone, so its source stays away from a seam
SRC = {H.EQ_3D: (30.0, -40.0, Z_SRC), H.EQ_GLOBAL: (Z_SRC, 40.0, 179.5), H.EQ_3D_RNGDEP: (30.0, -40.0, Z_SRC), H.EQ_GLOBAL_RNGDEP: (Z_SRC, 40.0, 1.25)}
LATTICE = dict(theta_min=-80.0, theta_max=-10.0, theta_step=5.0, phi_min=0.0, phi_max=345.0, phi_step=15.0)          # 15 x 24, phi_periodic
N_THETA, N_PHI = 15, 24
# twelve targets, none on a lattice line; the last two lie in the cell that closes the circle (345 .. 360)
THETA_STAR = -np.array([13.7, 21.3, 28.9, 33.1, 41.8, 47.2, 52.6, 58.3, 63.9, 68.4, 73.6, 77.7])
PHI_STAR = np.array([21.3, 52.7, 97.9, 131.2, 163.4, 201.6, 229.3, 258.8, 291.1, 318.7, 348.9, 356.2])
TOL = 0.01                                           # refinement tolerance [km]
LEVELS = [8.0, 15.0]

# "The same for all 24 phi" on the spherical sets: the spread of the oracle's RANGE and TTIME over an inclination's 24 azimuths, relative to their
# mean, measured on the CPU (tests/test_raised_ground_host.py prints it): RANGE 2.4e-11 (stratified) and 7.6e-12 (grid), TTIME 3.4e-12 and
# 2.9e-12.  The gate is ten times the larger.
SPH_SPREAD_MEASURED = dict(RANGE=2.4e-11, TTIME=3.4e-12)
SPH_SPREAD_GATE = {k: 10.0 * v for k, v in SPH_SPREAD_MEASURED.items()}
# the track leaves the source on bearing phi: the initial great-circle bearing from the source to the landing point, against phi [degrees]; measured on the
# oracle 8.8e-10 (stratified) and 4.1e-10 (grid)
BEARING_MEASURED = 8.8e-10
BEARING_GATE = 10.0 * BEARING_MEASURED


def lattice():
    th, ph, nt, nph = SC.lattice(**LATTICE)
    assert (nt, nph) == (N_THETA, N_PHI)
    return th, ph, nt, nph


def profile():
    return K.isothermal_profile(T0=T0, scale_height=SCALE_HEIGHT)


def params(eq, bounces=0):
    return dict(bounces=bounces, calc_amp=1, mode=0, src=SRC[eq], z_grnd=Z_GRND)


def cfg(eq, bounces=0):
    return H.make_cfg(eq, bounces=bounces, calc_amp=True, src=SRC[eq], z_grnd=Z_GRND)


# ---- a uniform grid: the isothermal profile in every column, 5 x 5 columns, +-240 km (+-3 degrees) about the source ----
def grid_nodes(eq):
    s = SRC[eq]
    if eq == H.EQ_3D_RNGDEP:
        return s[0] + 120.0 * np.arange(-2.0, 3.0), s[1] + 120.0 * np.arange(-2.0, 3.0)
    return s[1] + 1.5 * np.arange(-2.0, 3.0), s[2] + 1.5 * np.arange(-2.0, 3.0)


def write_uniform_grid(eq, dirpath):
    """the files of a 5 x 5 grid whose every column is the isothermal profile, written as tests/rngdep_data.py writes its own (six columns, file
    index i * 5 + j, the node files in km or degrees); returns (prefix, loc_a, loc_b)"""
    os.makedirs(dirpath, exist_ok=True)
    z, T, u, v, rho = profile()
    p = rho * 287.058 * T * 10.0                                                    # (the pressure column is read and not used)
    na, nb = grid_nodes(eq)
    prefix = os.path.join(dirpath, "u")
    body = "".join(f"{z[k]:.10g} {T[k]:.12g} {u[k]:.12g} {v[k]:.12g} {rho[k]:.12g} {p[k]:.10g}\n" for k in range(len(z)))
    for n in range(len(na) * len(nb)):
        with open(f"{prefix}{n}.met", "w") as fh:
            fh.write(body)
    loc_a, loc_b = os.path.join(dirpath, "loc_a.dat"), os.path.join(dirpath, "loc_b.dat")
    with open(loc_a, "w") as fh:
        fh.write("".join(f"{x:.10g}\n" for x in na))
    with open(loc_b, "w") as fh:
        fh.write("".join(f"{y:.10g}\n" for y in nb))
    return prefix, loc_a, loc_b


def oracle(eq, tmpdir=None):
    """the plain-C oracle holding the medium of set eq"""
    O = H.Oracle(eq, met=None)
    if eq in (H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP):
        O.load_grid(*write_uniform_grid(eq, str(tmpdir)), z_grnd=Z_GRND)
    else:
        O.load_arrays(*profile())
    return O


# ---- closed forms, Cartesian sets ----
def landing_xy(eq, theta, phi, height=HGT):
    """where the ray (theta, phi) has come down by `height` km: src_xy + (height / tan a)(sin phi, cos phi)"""
    a, az = np.radians(np.abs(theta)), np.radians(phi)
    d = height / np.tan(a)
    return np.stack([SRC[eq][0] + d * np.sin(az), SRC[eq][1] + d * np.cos(az)], axis=-1)


def travel_time(theta, height=HGT):
    return height / (C * np.sin(np.radians(np.abs(theta))))


def amplitude(theta, height=HGT):
    """spherical spreading 1 / (4 pi L) with the density factor of check_straight_rays, the ground's density taken at z_grnd (an arrival's own row lies up
    to 1 m of path lower: 6e-5 of the amplitude at most, inside what the refinement's tolerance allows)"""
    L = height / np.sin(np.radians(np.abs(theta)))
    return np.exp(0.5 * (Z_SRC - Z_GRND) / SCALE_HEIGHT) / (4.0 * np.pi * L)


# ---- spherical sets: what symmetry dictates ----
def sph_unit(lat, lon):
    lat, lon = np.asarray(lat, dtype=np.longdouble), np.asarray(lon, dtype=np.longdouble)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def great_circle(lat1, lon1, lat2, lon2, radius):
    """great-circle distance in numpy.longdouble (angles in radians), by the vector form atan2(|a x b|, a . b)"""
    a, b = sph_unit(lat1, lon1), sph_unit(lat2, lon2)
    cr = np.cross(a, b)
    return np.longdouble(radius) * np.arctan2(np.sqrt((cr * cr).sum(axis=-1)), (a * b).sum(axis=-1))


def bearing(lat1, lon1, lat2, lon2):
    """initial great-circle bearing from point 1 to point 2 [degrees, 0 .. 360), angles in radians"""
    dl = lon2 - lon1
    y = np.sin(dl) * np.cos(lat2)
    x = np.cos(lat1) * np.sin(lat2) - np.sin(lat1) * np.cos(lat2) * np.cos(dl)
    return np.degrees(np.arctan2(y, x)) % 360.0


def destination(eq, delta_km, phi, radius=RG):
    """(lat, lon) [degrees] of the point at arc length delta_km (on the sphere of `radius`) on bearing phi from the source of set eq; the longitude is
    continuous through the date line (not wrapped)"""
    lat0, lon0 = np.radians(SRC[eq][1]), np.radians(SRC[eq][2])
    d, az = np.asarray(delta_km) / radius, np.radians(phi)
    lat = np.arcsin(np.sin(lat0) * np.cos(d) + np.cos(lat0) * np.sin(d) * np.cos(az))
    lon = lon0 + np.arctan2(np.sin(az) * np.sin(d) * np.cos(lat0), np.cos(d) - np.sin(lat0) * np.sin(lat))
    return np.stack([np.degrees(lat), np.degrees(lon)], axis=-1)


def check_axial_symmetry(eq, rec, what=""):
    """spherical sets, records [360][legs][32] of the lattice: every ray arrives; per theta RANGE and TTIME are the same over the 24 phi (the measured
    gate above) and the landing point lies on bearing phi from the source.  Returns (delta [15] from the phi = 0 column at ground radius, ttime [15], the
    worst spreads and bearing error)"""
    th, ph, nt, nph = lattice()
    assert (rec[:, 0, H.REC["VALID"]] == 1.0).all(), what
    out = {}
    for f in ("RANGE", "TTIME"):
        v = rec[:, 0, H.REC[f]].reshape(nph, nt)
        out[f] = float(((v.max(axis=0) - v.min(axis=0)) / v.mean(axis=0)).max())
        assert out[f] <= SPH_SPREAD_GATE[f], f"{what}: {f} differs over phi by {out[f]:.3e} of its mean"
    S = H.REC["STATE"]
    lat, lon = rec[:, 0, S + 1], rec[:, 0, S + 2]
    lat0, lon0 = np.radians(SRC[eq][1]), np.radians(SRC[eq][2])
    eb = np.abs(SR._wrap180(bearing(lat0, lon0, lat, lon) - ph))
    out["BEARING"] = float(eb.max())
    assert out["BEARING"] <= BEARING_GATE, f"{what}: the landing points lie off bearing phi by {out['BEARING']:.3e} degrees"
    delta = np.asarray(great_circle(lat0, lon0, lat[:nt], lon[:nt], RG), dtype=np.float64)
    assert (np.diff(delta) > 0.0).all()                                             # shallower rays land farther: the landing map is monotone in theta
    return delta, rec[:nt, 0, H.REC["TTIME"]].copy(), out


def cell_of(theta_star, phi_star):
    """lattice cell (i, j) that contains (theta*, phi*), and the two triangle numbers of that cell (station_reference.triangles: 2 cell, 2 cell + 1 with
    cell = j (n_theta - 1) + i)"""
    i = np.floor((np.asarray(theta_star) + 80.0) / 5.0).astype(int)
    j = np.floor(np.asarray(phi_star) / 15.0).astype(int)
    cell = j * (N_THETA - 1) + i
    return i, j, cell


# ---- polygons ----
def winding_number(px, py, vx, vy):
    """winding number of the closed polygon (vx, vy) about every point (px, py), and the distance of the point from the polygon's nearest edge"""
    px, py = np.asarray(px, dtype=np.float64)[:, None], np.asarray(py, dtype=np.float64)[:, None]
    ax, ay = vx[None, :] - px, vy[None, :] - py
    bx, by = np.roll(vx, -1)[None, :] - px, np.roll(vy, -1)[None, :] - py
    cross, dot = ax * by - ay * bx, ax * bx + ay * by
    wn = np.rint(np.arctan2(cross, dot).sum(axis=1) / (2.0 * np.pi)).astype(int)
    ex, ey = bx - ax, by - ay
    t = np.clip(-(ax * ex + ay * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    dist = np.sqrt((ax + t * ex) ** 2 + (ay + t * ey) ** 2).min(axis=1)
    return wn, dist


# ---------------------------------------------------------------- the checks, shared by the CPU twin and the GPU tests
# Each takes plain arrays (records, lists, rows, layers) and returns the measured worst errors of what it gates as a dict; `launch(theta, phi)` is a
# callable that integrates launch angles in a plain context of the set with bounces = 0 and returns records [n][1][32].
S0 = H.REC["STATE"]
STA = SR.STA
GROUND_SPEC = dict(max_iter=12, max_shrink=4, tol=TOL, step_max_deg=1.0)


def check_launch(eq, rec):
    """a. the records of the lattice fan, bounces = 0.  Cartesian sets: check_straight_rays with z_grnd (end point on the launch line, slowness = launch
    direction, time = length / c to 1e-9, amplitude = spherical spreading to 1e-7, the end row at most DS_MIN below the ground); the landing point and
    the travel time are the closed forms evaluated at the end row's own height, so they hold to 1e-9 as well, and RANGE is the landing point's distance
    from the ORIGIN.  Spherical sets: great-circle plane and eikonal (check_straight_rays), the end row at most DS_MIN below the ground radius, and
    axial symmetry."""
    th, ph, nt, nph = lattice()
    n, off, et, ea = K.check_straight_rays(eq, rec, th, ph, SRC[eq], T0=T0, scale_height=SCALE_HEIGHT, z_grnd=Z_GRND)
    assert n == len(th) and (rec[:, 0, H.REC["BROKE"]] == 0.0).all()
    steps = rec[:, 0, H.REC["STEPS"]].reshape(nph, nt)
    assert (steps == steps[:1]).all(), "the step count of an inclination depends on the azimuth"          # (the step depends on the height alone, and the height on theta)
    out = dict(off_line=off, time_or_eikonal=et, amplitude=ea)
    if eq in CARTESIAN:
        down = Z_SRC - rec[:, 0, S0 + 2]
        xy = landing_xy(eq, th, ph, down)
        L = down / np.sin(np.radians(-th))
        out["landing"] = float((np.linalg.norm(rec[:, 0, S0:S0 + 2] - xy, axis=1) / L).max())
        out["ttime"] = float(np.abs(rec[:, 0, H.REC["TTIME"]] / travel_time(th, down) - 1.0).max())
        out["range_from_origin"] = float(np.abs(rec[:, 0, H.REC["RANGE"]] / np.hypot(xy[:, 0], xy[:, 1]) - 1.0).max())
        out["ground_plane"] = float(np.linalg.norm(rec[:, 0, S0:S0 + 2] - landing_xy(eq, th, ph), axis=1).max())
        assert out["landing"] <= 1e-9 and out["ttime"] <= 1e-9 and out["range_from_origin"] <= 1e-9, out
        assert out["ground_plane"] <= K.DS_MIN, out                                 # the closed form on z = z_grnd itself: to the last step
        from_src = np.hypot(xy[:, 0] - SRC[eq][0], xy[:, 1] - SRC[eq][1])
        assert (np.abs(rec[:, 0, H.REC["RANGE"]] / from_src - 1.0) > 1e-3).sum() >= 300          # (the two meanings of range differ on this source)
    else:
        below = RG - rec[:, 0, S0]
        assert (below > 0.0).all() and (below <= K.DS_MIN).all(), (below.min(), below.max())
        _, _, sym = check_axial_symmetry(eq, rec)
        out.update(sym)
    return out


def ring_columns(eq, rec_star):
    """spherical sets: Delta(theta*) at ground radius and the travel time of the twelve rays (theta*, phi = 0), from their own records [12][1][32]"""
    assert (rec_star[:, 0, H.REC["VALID"]] == 1.0).all()
    lat0, lon0 = np.radians(SRC[eq][1]), np.radians(SRC[eq][2])
    d = great_circle(lat0, lon0, rec_star[:, 0, S0 + 1], rec_star[:, 0, S0 + 2], RG)
    return np.asarray(d, dtype=np.float64), rec_star[:, 0, H.REC["TTIME"]].copy()


def ground_stations(eq, launch):
    """b. the twelve stations and the travel times t* of their eigenrays.  Cartesian: the closed-form landing points on z = z_grnd.  Spherical: at distance
    Delta(theta*) on bearing phi* from the source at ground radius, Delta(theta*) from a launch of (theta*, phi = 0) - the only thing taken from the code
    is the range of an inclination, which axial symmetry (check_launch) makes the same on every bearing."""
    if eq in CARTESIAN:
        return landing_xy(eq, THETA_STAR, PHI_STAR), travel_time(THETA_STAR), None
    delta, tt = ring_columns(eq, launch(THETA_STAR.copy(), np.zeros(len(THETA_STAR))))
    sta = destination(eq, delta, PHI_STAR)
    sta[:, 1] = SR._wrap180(sta[:, 1])
    return sta, tt, delta


def check_station_lists(hits, rows, t_star):
    """b. hits [12], rows [12][cap][16] of one member: one hit each, on leg 0, in a triangle of the lattice cell that contains (theta*, phi*), the
    estimate's angles inside that cell.  The estimate's own errors are returned, not gated (a first-order estimate has no derivable bound here)."""
    assert (hits == 1).all(), hits
    r = rows[:, 0]
    i, j, cell = cell_of(THETA_STAR, PHI_STAR)
    assert (j == N_PHI - 1).sum() >= 1                                              # the cell that closes the circle
    assert (r[:, STA["LEG"]] == 0).all()
    tri = r[:, STA["TRI"]].astype(int)
    assert ((tri == 2 * cell) | (tri == 2 * cell + 1)).all(), (tri, cell)
    t0, p0 = -80.0 + 5.0 * i, 15.0 * j
    assert ((r[:, STA["THETA"]] >= t0) & (r[:, STA["THETA"]] <= t0 + 5.0)).all(), r[:, STA["THETA"]]
    assert ((r[:, STA["PHI"]] >= p0) & (r[:, STA["PHI"]] <= p0 + 15.0)).all(), r[:, STA["PHI"]]
    return dict(est_theta_deg=float(np.abs(r[:, STA["THETA"]] - THETA_STAR).max()), est_phi_deg=float(np.abs(SR._wrap180(r[:, STA["PHI"]] - PHI_STAR)).max()),
                est_ttime_rel=float(np.abs(r[:, STA["TTIME"]] / t_star - 1.0).max()))


def check_refined(eq, rows, sta, t_star, delta, lattice_delta):
    """c. rows [12][16] of the refinement with GROUND_SPEC.  Every seed converges.  Cartesian, from d = h / tan a: |theta - theta*| <= tol sin^2 a / h,
    |phi - phi*| <= tol tan a / h, |TTIME - t*| <= tol / c + 1e-6 TTIME; AMP = spherical spreading within amp_rtol + tol / L; CELERITY bit for bit
    the station's distance from the ORIGIN over the row's TTIME.  Spherical: |phi - phi*| <= tol / (rg sin(Delta / rg)), |theta - theta*| <= tol |d theta /
    d Delta| with the slope from the lattice's own Delta(theta) column by differences - the steepest secant of the cell and its two neighbours, since
    Delta(theta) is convex; CELERITY the great circle from the source at r_earth (the header's range) over TTIME, to rounding of the series."""
    import refine_reference as RR
    R = RR.RFN
    assert len(rows) == 12 and (rows[:, R["STATUS"]] == RR.CONVERGED).all(), rows[:, R["STATUS"]]
    assert np.array_equal(rows[:, R["STATION"]], np.arange(12.0)) and (rows[:, R["LEG"]] == 0).all() and (rows[:, R["MISS"]] <= TOL).all()
    a = np.radians(-THETA_STAR)
    e_th = np.abs(rows[:, R["THETA"]] - THETA_STAR)
    e_ph = np.abs(SR._wrap180(rows[:, R["PHI"]] - PHI_STAR))
    e_t = np.abs(rows[:, R["TTIME"]] - t_star)
    b_t = TOL / C + 1e-6 * rows[:, R["TTIME"]]
    out = {}
    if eq in CARTESIAN:
        b_th, b_ph = np.degrees(TOL * np.sin(a) ** 2 / HGT), np.degrees(TOL * np.tan(a) / HGT)
        L = HGT / np.sin(a)
        e_a = np.abs(rows[:, R["AMP"]] / amplitude(THETA_STAR) - 1.0)
        b_a = 1e-7 + TOL / L
        out["amp_of_bound"] = float((e_a / b_a).max())
        assert (e_a <= b_a).all(), (e_a, b_a)
        d_origin = np.sqrt(sta[:, 0] * sta[:, 0] + sta[:, 1] * sta[:, 1])
        assert np.array_equal(SR.bits(rows[:, R["CELERITY"]]), SR.bits(d_origin / rows[:, R["TTIME"]]))
        d_src = np.hypot(sta[:, 0] - SRC[eq][0], sta[:, 1] - SRC[eq][1])
        assert (np.abs(d_origin / d_src - 1.0) >= 1e-2).all(), d_origin / d_src        # the distance from the source is another number, in the second digit
    else:
        b_ph = np.degrees(TOL / (RG * np.sin(delta / RG)))
        i = cell_of(THETA_STAR, PHI_STAR)[0]
        sec = 5.0 / np.abs(np.diff(lattice_delta))                                 # [14] degrees per km, cell by cell
        b_th = TOL * np.array([sec[max(k - 1, 0):k + 2].max() for k in i])
        rng = RR.DIST(np.full(12, SRC[eq][1]), np.full(12, SRC[eq][2]), sta[:, 0], sta[:, 1], R_EARTH)
        assert np.array_equal(SR.bits(rows[:, R["CELERITY"]]), SR.bits(rng / rows[:, R["TTIME"]]))
        want = np.asarray(great_circle(np.radians(SRC[eq][1]), np.radians(SRC[eq][2]), np.radians(sta[:, 0]), np.radians(sta[:, 1]), R_EARTH), dtype=np.float64)
        out["range_vs_longdouble"] = float(np.abs(rng / want - 1.0).max())
        assert out["range_vs_longdouble"] <= 1e-12
    out.update(theta_of_bound=float((e_th / b_th).max()), phi_of_bound=float((e_ph / b_ph).max()), ttime_of_bound=float((e_t / b_t).max()),
               theta_deg=float(e_th.max()), phi_deg=float(e_ph.max()), ttime_s=float(e_t.max()), miss_km=float(rows[:, R["MISS"]].max()))
    assert (e_th <= b_th).all() and (e_ph <= b_ph).all() and (e_t <= b_t).all(), out
    return out


MISS_RTOL, MISS_FLOOR = 1e-9, 1e-11        # [km]: positions near 6 400 km carry 2^-53 x 6 400 = 7e-13 km of rounding each; a miss cannot be known closer


def independent_miss(eq, rec_rows, sta, radius):
    """distance [n] of records' end points rec_rows [n][32] from stations sta [n][2], by numpy.longdouble and numpy's own functions"""
    if eq in CARTESIAN:
        x, y = np.asarray(rec_rows[:, S0], dtype=np.longdouble), np.asarray(rec_rows[:, S0 + 1], dtype=np.longdouble)
        return np.sqrt((sta[:, 0] - x) ** 2 + (sta[:, 1] - y) ** 2)
    rad = np.pi / np.longdouble(180.0)
    return great_circle(rec_rows[:, S0 + 1], rec_rows[:, S0 + 2], np.asarray(sta[:, 0], dtype=np.longdouble) * rad, np.asarray(sta[:, 1], dtype=np.longdouble) * rad, radius)


def check_miss(eq, rows, sta, launch, separated):
    """c. GEOAC_RFN_MISS of every row against an independent computation at the GROUND radius: the row's angles launched again in a plain context, the
    great circle from that record's end point to the station in numpy.longdouble.  Agreement to MISS_RTOL relative (plus MISS_FLOOR).  separated: the
    rows are first misses of kilometres (a one-round refinement), and the same number at r_earth - 2.4e-4 smaller - lies at least 1e3 gates away."""
    import refine_reference as RR
    R = RR.RFN
    again = launch(rows[:, R["THETA"]].copy(), rows[:, R["PHI"]].copy())
    assert (again[:, 0, H.REC["VALID"]] == 1.0).all()
    k = rows[:, R["STATION"]].astype(int)
    want = independent_miss(eq, again[:, 0], sta[k], RG)
    gate = MISS_RTOL * want + MISS_FLOOR
    err = np.abs(np.asarray(rows[:, R["MISS"]], dtype=np.longdouble) - want)
    out = dict(miss_of_gate=float((err / gate).max()), miss_rel=float((err / want).max()), miss_min_km=float(want.min()), miss_max_km=float(want.max()))
    assert (err <= gate).all(), out
    if separated and eq in SPHERICAL:
        other = independent_miss(eq, again[:, 0], sta[k], R_EARTH)
        sep = np.abs(other - want) / gate
        out["r_earth_separation_gates"] = float(sep.min())
        assert (sep >= 1e3).all(), sep
        assert abs(float((1.0 - other / want).max()) - Z_GRND / RG) < 1e-9
    return out


# ---- d. tube map and arrival map ----
N_CELLS = 64
FRAC = (float(np.sqrt(3.0) - 1.0) / 2.0, float(np.sqrt(2.0) - 1.0) / 4.0)          # the origin's offset, in cells: irrational, so that no centre lies on a lattice edge
MARGIN_CELLS = 1e-9                                  # centres closer than this to a ring polygon are left out


def map_grid(eq, east_half=False):
    """origin, step, n of the 64 x 64 grid about the source that covers the outer ring (113.4 km; 0.97 degrees of latitude, 1.267 of longitude): cells of
    4 km, 0.04 degrees on the sphere.  east_half: its eastern 64 x 32 cells alone, moved east by 1 / pi of a cell - the grid's western border then cuts
    through the ring, and a landing triangle whose first corner lies west of it reaches the grid's columns only modulo 360 degrees on the spherical sets"""
    step = 4.0 if eq in CARTESIAN else 0.04
    c = SRC[eq][0:2] if eq in CARTESIAN else SRC[eq][1:3]
    origin = [c[k] - step * N_CELLS / 2 + FRAC[k] * step for k in (0, 1)]
    if east_half:
        origin[1] += (N_CELLS // 2 + 1.0 / np.pi) * step
    return dict(origin=tuple(origin), step=(step, step), n=(N_CELLS, N_CELLS // 2 if east_half else N_CELLS))


def tube_spec(eq, east_half=False):
    import tubemap_reference as TR
    # edge_max removes no triangle: the longest side of a landing triangle is the outer ring's 15-degree chord to the next ring, below 50 km (0.6 degrees)
    return TR.spec(n_theta=N_THETA, n_phi=N_PHI, edge_max=60.0 if eq in CARTESIAN else 0.9, phi_periodic=True, wrap_lon=eq in SPHERICAL, **map_grid(eq, east_half))


def map_spec(eq):
    import map_reference as MR
    return MR.spec(wrap_lon=eq in SPHERICAL, **map_grid(eq))


def _rule_coordinates(eq, c0, c1):
    """points in the station rule's coordinates: as they are, or (latitude, longitude relative to the source, wrapped)"""
    return (c0, c1) if eq in CARTESIAN else (c0, SR._wrap180(c1 - SRC[eq][2]))


def landing_points(eq, rec):
    """c0, c1 [360] of the leg-0 arrival records in the map's axes, from the record layout of include/geoac_hip.h itself: the Cartesian state begins
    x, y, z [km], the spherical r, lat, lon [km, rad, rad] (the layout check_straight_rays reads its positions by)"""
    if eq in CARTESIAN:
        return rec[:, 0, S0 + 0], rec[:, 0, S0 + 1]
    return np.degrees(rec[:, 0, S0 + 1]), np.degrees(rec[:, 0, S0 + 2])


def cell_centres(sp):
    """cell centres [n0 * n1][2], row-major: origin + (i + 1 / 2) step on each axis (the header's definition of a tube map's stations)"""
    a0 = sp["origin"][0] + (np.arange(sp["n"][0]) + 0.5) * sp["step"][0]
    a1 = sp["origin"][1] + (np.arange(sp["n"][1]) + 0.5) * sp["step"][1]
    return np.stack([np.repeat(a0, sp["n"][1]), np.tile(a1, sp["n"][0])], axis=1)


def ring_polygons(eq, rec):
    """the 24-gons through the landing points of theta = -10 (outer) and theta = -80 (inner), in the station rule's coordinates"""
    c0, c1 = landing_points(eq, rec)
    c0, c1 = c0.reshape(N_PHI, N_THETA), c1.reshape(N_PHI, N_THETA)
    return _rule_coordinates(eq, c0[:, -1], c1[:, -1]), _rule_coordinates(eq, c0[:, 0], c1[:, 0])


def check_tubemap(eq, count, rec, sp):
    """d. COUNT [64][64] of the tube map of the lattice records rec [360][1][32].  The lattice's quadrilaterals tile the region between the two ring
    polygons (neighbours share their edges), so a cell centre outside a margin of both polygons is counted once if it lies inside the outer and outside
    the inner polygon, and not at all otherwise - by a winding number in plain numpy, not by the triangle rule; vertices and centres are formed here,
    not by the restatements."""
    cen = cell_centres(sp)
    px, py = _rule_coordinates(eq, cen[:, 0], cen[:, 1])
    (ox, oy), (ix, iy) = ring_polygons(eq, rec)
    n0, n1 = sp["n"]
    full = n1 == N_CELLS
    o = np.array(sp["origin"]) if eq in CARTESIAN else np.array([sp["origin"][0], sp["origin"][1] - SRC[eq][2]])
    width = np.array(sp["step"]) * np.array(sp["n"])
    covered = (ox > o[0]).all() and (ox < o[0] + width[0]).all() and (oy > o[1]).all() and (oy < o[1] + width[1]).all()
    assert covered if full else (oy < o[1]).sum() >= 8, "the grid does not cover the outer ring" if full else "the eastern half's border does not cut the ring"
    w_out, d_out = winding_number(px, py, ox, oy)
    w_in, d_in = winding_number(px, py, ix, iy)
    assert set(np.abs(w_out)) <= {0, 1} and set(np.abs(w_in)) <= {0, 1}
    want = (np.abs(w_out) - np.abs(w_in)).reshape(n0, n1)
    keep = ((d_out > MARGIN_CELLS * sp["step"][0]) & (d_in > MARGIN_CELLS * sp["step"][0])).reshape(n0, n1)
    count = np.asarray(count).astype(np.int64)
    out = dict(left_out_share=float(1.0 - keep.mean()), cells_count_1=float((want[keep] == 1).sum()), cells_count_0=float((want[keep] == 0).sum()),
               nearest_centre_cells=float(min(d_out.min(), d_in.min()) / sp["step"][0]))
    assert out["left_out_share"] <= 0.01 and out["cells_count_1"] >= 500 and out["cells_count_0"] >= 500, out
    assert (want >= 0).all()
    bad = keep & (count != want)
    assert not bad.any(), f"{int(bad.sum())} cell centres: COUNT {count[bad][:8].tolist()} where the ring polygons say {want[bad][:8].tolist()}, first at {tuple(np.argwhere(bad)[0])}"
    if eq == H.EQ_GLOBAL and full:                                                  # the date line passes through the ring: centres on both sides are counted
        lon = cen[:, 1].reshape(n0, n1)
        assert ((want == 1) & keep & (lon > 180.0)).sum() >= 100 and ((want == 1) & keep & (lon < 180.0)).sum() >= 100
    return out


def station_cells(eq, sp, sta, count):
    """twelve cells counted once (flat indices): for each ground station the nearest such centre - the stations of the TTIME_MIN check"""
    cen = cell_centres(sp)
    px, py = _rule_coordinates(eq, cen[:, 0], cen[:, 1])
    sx, sy = _rule_coordinates(eq, sta[:, 0], sta[:, 1])
    d = np.hypot(px[None, :] - sx[:, None], py[None, :] - sy[:, None])
    d = np.where(np.asarray(count).reshape(-1)[None, :] == 1, d, np.inf)
    flat = d.argmin(axis=1)
    assert np.isfinite(d[np.arange(len(sta)), flat]).all() and len(set(flat.tolist())) >= 10
    return flat


def check_ttime_min_at_centres(ttime_min, flat, hits, rows):
    """d. TTIME_MIN of a cell whose centre is a station equals that station's row TTIME, bit for bit (hits [12], rows [12][cap][16] of stations at the centres)"""
    assert (hits == 1).all(), hits
    assert np.array_equal(SR.bits(np.asarray(ttime_min).reshape(-1)[flat]), SR.bits(rows[:, 0, STA["TTIME"]]))


BORDER_CELLS = 1e-6                                  # landing points stay this far from every cell border (plus the last step, DS_MIN)


def check_arrival_map(eq, layers, rec, sp):
    """d. the arrival map of the lattice records: the sum of COUNT is the number of arrivals.  Cartesian sets: every arrival falls in the cell its closed-form
    landing point (on z = z_grnd) names - those points lie BORDER_CELLS of a cell plus DS_MIN from every border, so the record's own end row, at most
    DS_MIN along the ray from it, is in the same cell; TTIME_MIN of a cell holding one arrival is the travel time to that row's own height, to 1e-9, and
    CEL_MAX its distance from the ORIGIN over that time."""
    th, ph, nt, nph = lattice()
    count = np.asarray(layers["count"][0]).astype(np.int64)
    assert int(count.sum()) == len(th) and int(layers["outside"][0]) == 0
    out = {}
    if eq in CARTESIAN:
        o, st = np.array(sp["origin"]), np.array(sp["step"])
        u = (landing_xy(eq, th, ph) - o) / st
        out["border_margin_cells"] = float(np.minimum(u - np.floor(u), np.ceil(u) - u).min())
        assert out["border_margin_cells"] >= BORDER_CELLS + K.DS_MIN / st[0], out
        q = np.floor(u).astype(int)
        flat = q[:, 0] * N_CELLS + q[:, 1]
        want = np.bincount(flat, minlength=N_CELLS * N_CELLS).reshape(N_CELLS, N_CELLS)
        assert np.array_equal(count, want)
        one = want.reshape(-1)[flat] == 1
        assert one.sum() >= 200
        down = Z_SRC - rec[:, 0, S0 + 2]
        t = travel_time(th, down)
        xy = landing_xy(eq, th, ph, down)
        out["ttime_min"] = float(np.abs(layers["ttime_min"][0].reshape(-1)[flat[one]] / t[one] - 1.0).max())
        out["cel_max"] = float(np.abs(layers["cel_max"][0].reshape(-1)[flat[one]] / (np.hypot(xy[:, 0], xy[:, 1])[one] / t[one]) - 1.0).max())
        assert out["ttime_min"] <= 1e-9 and out["cel_max"] <= 1e-9, out
    return out


# ---- e. levels, level stations and level refinement under a raised ground (Cartesian sets) ----
# One bounce.  The reflected ray never comes down again; the vertical limit ends it above the levels (25 km), so that leg 1 is as short as leg 0.
LEVEL_PARAMS = dict(bounces=1, vert_limit=25.0)
LEVEL_SPEC = dict(tol=TOL, step_max_deg=1.0, probe_deg=0.02, max_iter=12)
# Where leg 1 starts.  The reference finds the ground intercept from the last three rows with a quadratic term (ApproximateIntercept,
# 3DStratified.cpp:136-186): on a straight ray the second difference of those rows is the direction times the CHANGE of the step, not zero, so the
# intercept - and with it the mirror plane - lies off z_grnd along the ray by e = (ds_k - ds_{k-1}) / 2 x (dz_grnd / dz_k)^2 <= |ds_k - ds_{k-1}| / 2.
# GeoAc_Set_ds: ds(h) = 0.05 - 0.049 exp(-h / 0.75), |ds'| <= 0.0653 per km; the last rows lie within 2.2e-3 km of the ground where ds <= 1.15e-3, so
# |ds_k - ds_{k-1}| <= 0.0653 x 1.15e-3 = 7.5e-5 and e <= REFLECT_E = 3.8e-5 km.  What that does to a passage of the reflected branch depends on the set:
# - GEOAC_EQ_3D starts leg 1 at the intercept as it is, height included (SetReflectionConditions): the start point and the mirror plane both lie off by e,
#   so a passage moves by at most 2 e, and the path from the start to the level is e shorter or longer: position and distance to 2 e, path (time x c) to e
#   [km] (measured on the oracle: 3.3e-5 and 2.9e-5).
# - GEOAC_EQ_3D_RNGDEP puts the start's height ON the ground (3D.RngDep: the z component is set to z_grnd) and keeps the intercept's x, y: the mirror plane is
#   the ground, the times hold to 1e-9 of the path as on leg 0, and the passages lie e along the track: position and distance to e [km] (measured: 1.6e-5).
REFLECT_E = 3.8e-5
LEG1_GATES = {H.EQ_3D: dict(position_km=2.0 * REFLECT_E, distance_km=2.0 * REFLECT_E, time_km=REFLECT_E),
              H.EQ_3D_RNGDEP: dict(position_km=REFLECT_E, distance_km=REFLECT_E, time=1e-9)}
BRANCHES = (dict(leg=0, direction=-1.0, lsta=dict(leg_max=0)), dict(leg=1, direction=1.0, lsta=dict(leg_min=1)))


def branch_height(branch, z_l):
    """the height a ray has covered, at constant |sin|, when it passes level z_l on a branch: downward on leg 0 z_src - z_l, upward on leg 1 (the mirror
    image of the source lies h below the ground) h + z_l - z_grnd"""
    z_l = np.asarray(z_l, dtype=np.float64)
    return Z_SRC - z_l if branch["leg"] == 0 else HGT + z_l - Z_GRND


def check_levels(eq, rec, count, lrec):
    """e. crossing tables count [360][2], lrec [360][2][cap][12] and records rec [360][2][32] of the lattice launch with LEVEL_PARAMS: every ray passes each
    level twice - downward on leg 0, upward on leg 1 - and nothing else; positions on the launch line and on its mirror image, horizontal distances
    branch_height / tan a from the source, times path / c - to 1e-9 on leg 0, to LEG1_GATES on leg 1 (above).  The reference carries leg 0's travel time to its end row, DS_MIN at most below the
    ground, and starts leg 1 from the intercept ON the ground: the piece below the ground is in leg 1's times, so the reflected branch's path is
    (z_src - z_end) + (z_l - z_grnd) over sin a, z_end the height of the ray's own leg-0 arrival record."""
    from levels_reference import LVL
    th, ph, nt, nph = lattice()
    assert (rec[:, 0, H.REC["VALID"]] == 1.0).all() and (rec[:, 1, H.REC["VALID"]] == 0.0).all()          # leg 1 has passages and no arrival
    assert (count == 2).all(), np.unique(count)
    assert (lrec[:, :, 2:] == 0.0).all()
    a, az = np.radians(-th)[:, None], np.radians(ph)[:, None]
    zl = np.array(LEVELS)[None, :]
    out = {}
    for k, br in enumerate(BRANCHES):
        X = lrec[:, :, k]
        assert (X[..., LVL["LEG"]] == br["leg"]).all() and (X[..., LVL["DIR"]] == br["direction"]).all()
        hgt = branch_height(br, zl)
        d = hgt / np.tan(a)
        want = np.stack([SRC[eq][0] + d * np.sin(az), SRC[eq][1] + d * np.cos(az), zl + 0.0 * d], axis=-1)
        L = hgt / np.sin(a)
        path = L if br["leg"] == 0 else L + ((Z_GRND - rec[:, 0, S0 + 2])[:, None]) / np.sin(a)
        P = X[..., LVL["P0"]:LVL["P0"] + 3]
        gates = dict(position=1e-9, distance=1e-9, time=1e-9) if br["leg"] == 0 else LEG1_GATES[eq]
        err = dict(position=np.linalg.norm(P - want, axis=-1), distance=np.abs(np.hypot(P[..., 0] - SRC[eq][0], P[..., 1] - SRC[eq][1]) - d),
                   time=np.abs(X[..., LVL["TTIME"]] * C - path))
        scale = dict(position=L, distance=d, time=path)
        for name, gate in gates.items():                                            # "<quantity>": relative to the path; "<quantity>_km": kilometres
            q = name[:-3] if name.endswith("_km") else name
            out[f"leg{br['leg']}_{name}"] = float((err[q] / (1.0 if name.endswith("_km") else scale[q])).max())
            assert out[f"leg{br['leg']}_{name}"] <= gate, (name, gate, out)
    return out


def level_stations_of(eq, branch):
    """the 24 stations of a branch: the passage points of (theta*, phi*) on the two levels; sta [24][2], level_of [24]"""
    zl = np.repeat(LEVELS, 12)
    th, ph = np.tile(THETA_STAR, 2), np.tile(PHI_STAR, 2)
    return landing_xy(eq, th, ph, branch_height(branch, zl)), np.repeat([0, 1], 12)


def check_level_station_lists(branch, hits, rows):
    """e. hits [24], rows [24][cap][16] of a branch's stations searched on that branch's leg: one hit each, LEG, DIR as the branch says, ordinal 0"""
    from lstation_reference import LSTA
    assert (hits == 1).all(), hits
    r = rows[:, 0]
    assert (r[:, LSTA["LEG"]] == branch["leg"]).all() and (r[:, LSTA["DIR"]] == branch["direction"]).all() and (r[:, LSTA["ORD"]] == 0).all()
    i, j, cell = cell_of(np.tile(THETA_STAR, 2), np.tile(PHI_STAR, 2))
    tri = r[:, LSTA["TRI"]].astype(int)
    assert ((tri == 2 * cell) | (tri == 2 * cell + 1)).all(), (tri, cell)


def check_level_refined(eq, branch, rows, sta):
    """e. rows [24][16] of level_refine with LEVEL_SPEC on a branch's lists: all converge, within the bounds of test_closed_form
    (tests/test_gpu_level_refine.py) at the branch's height z: |theta - theta*| <= tol sin^2 a / z, |phi - phi*| <= tol tan a / z,
    |TTIME - z / (c sin a)| <= tol / c + 1e-6 TTIME; CELERITY bit for bit the station's distance from the SOURCE POINT over the row's TTIME - another
    number than the distance from the origin, which the ground products divide."""
    import level_refine_reference as LR
    R = LR.LRF
    assert len(rows) == 24 and (rows[:, R["STATUS"]] == LR.CONVERGED).all(), rows[:, R["STATUS"]]
    assert (rows[:, R["LEG"]] == branch["leg"]).all() and (rows[:, R["DIR"]] == branch["direction"]).all() and (rows[:, R["ORD"]] == 0).all()
    assert np.array_equal(rows[:, R["STATION"]], np.arange(24.0)) and (rows[:, R["MISS"]] <= TOL).all()
    th_s, ph_s = np.tile(THETA_STAR, 2), np.tile(PHI_STAR, 2)
    a = np.radians(-th_s)
    z = branch_height(branch, np.repeat(LEVELS, 12))
    e_th, e_ph = np.abs(rows[:, R["THETA"]] - th_s), np.abs(SR._wrap180(rows[:, R["PHI"]] - ph_s))
    e_t = np.abs(rows[:, R["TTIME"]] - z / (C * np.sin(a)))
    b_th, b_ph, b_t = np.degrees(TOL * np.sin(a) ** 2 / z), np.degrees(TOL * np.tan(a) / z), TOL / C + 1e-6 * rows[:, R["TTIME"]]
    out = dict(theta_of_bound=float((e_th / b_th).max()), phi_of_bound=float((e_ph / b_ph).max()), ttime_of_bound=float((e_t / b_t).max()),
               miss_km=float(rows[:, R["MISS"]].max()))
    assert (e_th <= b_th).all() and (e_ph <= b_ph).all() and (e_t <= b_t).all(), out
    dx, dy = sta[:, 0] - SRC[eq][0], sta[:, 1] - SRC[eq][1]
    cel = np.sqrt(dx * dx + dy * dy) / rows[:, R["TTIME"]]
    assert np.array_equal(SR.bits(rows[:, R["CELERITY"]]), SR.bits(cel))
    origin = np.sqrt(sta[:, 0] * sta[:, 0] + sta[:, 1] * sta[:, 1]) / rows[:, R["TTIME"]]
    out["origin_form_differs_by"] = float(np.abs(origin / cel - 1.0).min())
    assert out["origin_form_differs_by"] >= 1e-2, out                                # measured from the origin it is another number, in the second digit
    return out
