"""Deterministic synthetic range-dependent atmosphere for the 3D.RngDep tests: a grid of perturbed, vertically thinned
copies of ToyAtmo.met written as <prefix><n>.met (n = ix*ny + iy, the reference's file index, G2S_MultiDimSpline3D.cpp:154)
plus loc_x.dat / loc_y.dat.  Non-square cells (dx != dy) so that quirk Q11 matters."""
import os

import numpy as np

import harness as H

X_NODES = np.array([-1000.0, -500.0, 0.0, 500.0, 1000.0])
Y_NODES = np.array([-800.0, -400.0, 0.0, 400.0, 800.0])
THIN = 4                      # keep every 4th ToyAtmo row: 350 nodes, dz = 0.4 km


def grid_columns(thin=THIN):
    """returns z [nz], and T, u, v, rho as [nx][ny][nz] (raw .met units: K, m/s, m/s, g/cm^3)"""
    raw = np.loadtxt(H.TOYATMO)[::thin]
    z = raw[:, 0]
    nx, ny = len(X_NODES), len(Y_NODES)
    T = np.zeros((nx, ny, len(z))); u = np.zeros_like(T); v = np.zeros_like(T); rho = np.zeros_like(T)
    for i, x in enumerate(X_NODES):
        for j, y in enumerate(Y_NODES):
            bump = np.exp(-((z - 45.0) / 25.0) ** 2)
            T[i, j] = raw[:, 1] * (1.0 + 0.015 * np.sin(x / 700.0 + y / 900.0) * bump + 0.004 * np.cos(x / 450.0) * np.sin(y / 380.0))
            u[i, j] = raw[:, 2] + 12.0 * (x / 1000.0) * bump + 3.0 * np.sin(y / 500.0)
            v[i, j] = raw[:, 3] + 8.0 * (y / 800.0) * bump - 2.5 * np.cos(x / 600.0) * np.exp(-z / 60.0)
            rho[i, j] = raw[:, 4] * (1.0 + 0.01 * np.cos(x / 800.0 - y / 650.0))
    return z, T, u, v, rho, raw[:, 5]


GRID_NPZ = os.path.join(H.GOLDEN_DIR, "rngdep_grid.npz")
GRID_NPZ_FULL = os.path.join(H.GOLDEN_DIR, "rngdep_grid_1400.npz")       # thin = 1: the 5x5x1400 grid of BASELINE config 4


def _grid_npz(thin):
    assert thin in (THIN, 1)
    return GRID_NPZ if thin == THIN else GRID_NPZ_FULL


def save_grid_npz(thin=THIN):
    """(make_golden.py) evaluates the analytic perturbation once and stores the columns, so that the files written at
    test time are the same bytes on every machine"""
    z, T, u, v, rho, p = grid_columns(thin)
    np.savez_compressed(_grid_npz(thin), z=z, T=T, u=u, v=v, rho=rho, p=p, x=X_NODES, y=Y_NODES)


def load_grid_columns(thin=THIN):
    g = np.load(_grid_npz(thin))
    return g["z"], g["T"], g["u"], g["v"], g["rho"], g["p"]


def write_grid(dirpath, short_paths=True, thin=THIN):
    """writes the files; returns (prefix, locx, locy).  Paths must stay short: the reference formats file names into a
    50-byte buffer (G2S_MultiDimSpline3D.cpp:112,154)."""
    os.makedirs(dirpath, exist_ok=True)
    z, T, u, v, rho, p = load_grid_columns(thin)
    prefix = os.path.join(dirpath, "p")
    assert len(prefix) < 40 or not short_paths     # only the reference needs short names
    for i in range(len(X_NODES)):
        for j in range(len(Y_NODES)):
            n = i * len(Y_NODES) + j
            with open(f"{prefix}{n}.met", "w") as fh:
                for k in range(len(z)):
                    fh.write(f"{z[k]:.10g} {T[i, j, k]:.12g} {u[i, j, k]:.12g} {v[i, j, k]:.12g} {rho[i, j, k]:.12g} {p[k]:.10g}\n")
    locx, locy = os.path.join(dirpath, "loc_x.dat"), os.path.join(dirpath, "loc_y.dat")
    with open(locx, "w") as fh:
        fh.write("".join(f"{x:.10g}\n" for x in X_NODES))
    with open(locy, "w") as fh:
        fh.write("".join(f"{y:.10g}\n" for y in Y_NODES))
    return prefix, locx, locy


# ---- Global.RngDep: grid in latitude / longitude (degrees in the loc files), file index n = ilat*nlon + ilon
#      (G2S_GlobalMultiDimSpline3D.cpp:159); cells of 3 x 4 degrees so that lat and lon scalings differ ----
LAT_NODES = np.array([25.0, 28.0, 31.0, 34.0, 37.0])
LON_NODES = np.array([-8.0, -4.0, 0.0, 4.0, 8.0])
GRID_GLOBAL_NPZ = os.path.join(H.GOLDEN_DIR, "globalrd_grid.npz")
# the same columns around another centre latitude: the perturbation depends on a node's INDEX offset from the centre ((lat - 31) / 6 = -1 .. 1 above), so a grid
# whose rows are `lat_step` apart around `centre_lat` holds the committed columns and differs in loc_lat.dat alone.  POLAR_GRID: 82 .. 89.5 N, where the
# 4-degree longitude cells shrink from 62 km to 3.9 km (tests/golden/globalrd_polar.npz, tests/test_gpu_globalrd.py)
CENTRE_LAT, LAT_STEP, LON_STEP = 31.0, 3.0, 4.0
POLAR_GRID = dict(centre_lat=85.75, lat_step=1.875, lon_step=15.0)


def lat_nodes_global(centre_lat=CENTRE_LAT, lat_step=LAT_STEP):
    return centre_lat + lat_step * np.arange(-2.0, 3.0)


def lon_nodes_global(lon_step=LON_STEP):
    return lon_step * np.arange(-2.0, 3.0)


def grid_columns_global():
    raw = np.loadtxt(H.TOYATMO)[::THIN]
    z = raw[:, 0]
    nt, npn = len(LAT_NODES), len(LON_NODES)
    T = np.zeros((nt, npn, len(z))); u = np.zeros_like(T); v = np.zeros_like(T); rho = np.zeros_like(T)
    for i, la in enumerate(LAT_NODES):
        for j, lo in enumerate(LON_NODES):
            bump = np.exp(-((z - 45.0) / 25.0) ** 2)
            a, b = (la - 31.0) / 6.0, lo / 8.0
            T[i, j] = raw[:, 1] * (1.0 + 0.015 * np.sin(1.3 * a + 0.9 * b) * bump + 0.004 * np.cos(2.1 * a) * np.sin(2.4 * b))
            u[i, j] = raw[:, 2] + 12.0 * a * bump + 3.0 * np.sin(1.7 * b)
            v[i, j] = raw[:, 3] + 8.0 * b * bump - 2.5 * np.cos(1.6 * a) * np.exp(-z / 60.0)
            rho[i, j] = raw[:, 4] * (1.0 + 0.01 * np.cos(1.2 * a - 1.4 * b))
    return z, T, u, v, rho, raw[:, 5]


def save_grid_global_npz():
    z, T, u, v, rho, p = grid_columns_global()
    np.savez_compressed(GRID_GLOBAL_NPZ, z=z, T=T, u=u, v=v, rho=rho, p=p, lat=LAT_NODES, lon=LON_NODES)


def write_grid_global(dirpath, short_paths=True, centre_lat=CENTRE_LAT, lat_step=LAT_STEP, lon_step=LON_STEP):
    """writes g<n>.met, loc_lat.dat, loc_lon.dat; returns (prefix, loclat, loclon).  centre_lat, lat_step: the latitudes of the five rows (the default:
    LAT_NODES, the files the fixtures of the mid-latitude grid were made from)"""
    lat_nodes = lat_nodes_global(centre_lat, lat_step)
    lon_nodes = lon_nodes_global(lon_step)
    assert (centre_lat, lat_step, lon_step) != (CENTRE_LAT, LAT_STEP, LON_STEP) or (np.array_equal(lat_nodes, LAT_NODES) and np.array_equal(lon_nodes, LON_NODES))
    assert np.abs(lat_nodes).max() < 90.0
    os.makedirs(dirpath, exist_ok=True)
    g = np.load(GRID_GLOBAL_NPZ)
    z, T, u, v, rho, p = g["z"], g["T"], g["u"], g["v"], g["rho"], g["p"]
    prefix = os.path.join(dirpath, "g")
    assert len(prefix) < 40 or not short_paths
    for i in range(len(LAT_NODES)):
        for j in range(len(LON_NODES)):
            n = i * len(LON_NODES) + j
            with open(f"{prefix}{n}.met", "w") as fh:
                for k in range(len(z)):
                    fh.write(f"{z[k]:.10g} {T[i, j, k]:.12g} {u[i, j, k]:.12g} {v[i, j, k]:.12g} {rho[i, j, k]:.12g} {p[k]:.10g}\n")
    loclat, loclon = os.path.join(dirpath, "loc_lat.dat"), os.path.join(dirpath, "loc_lon.dat")
    with open(loclat, "w") as fh:
        fh.write("".join(f"{x:.10g}\n" for x in lat_nodes))
    with open(loclon, "w") as fh:
        fh.write("".join(f"{y:.10g}\n" for y in lon_nodes))
    return prefix, loclat, loclon


# ---- a ragged 7 x 4 grid for both sets: unequal node spacing on both horizontal axes (nx != ny), irregular heights, a jet with meridional wind.
#      tests/golden/rngdep_ragged.npz holds the columns (make_golden.py ragged3d / raggedglobal; fixtures rngdep_ragged_{3drd,globalrd}.npz).  The columns are
#      JetAtmo.met's (tests/jet_data.py) on a subset of its own irregular nodes, modulated across the grid by the node's position a, b in [-0.5, 0.5] along the
#      Cartesian axes; the spherical grid holds the same columns on its own nodes.  File index n = i * 4 + j.
#      Heights (ragged_heights): every third node (segments of 0.2 .. 0.8 km, neighbours up to 1 : 10), and around every ninth of the profile's 3.3 m segments all
#      eight of its nodes: 328 heights, six 3.3 m segments whose neighbours are 71 .. 379 m long.  No more and no closer: the spherical reference's slope systems (quirk Q12a)
#      take the right-hand side of a node from the segment ABOVE it on both sides, which multiplies the slope there by about hr / hl.  With both ends of a 3.3 m
#      segment put back between two 0.6 km ones (1 : 200) the reference's own rays turn chaotic - theta (1 + 1e-12) moved its arrivals by 1e-3 and its step counts -
#      and no arithmetic but its own bit pattern follows it; with the profile's own nodes around a short segment its answer stays below 1e-7 on all but one ray. ----
RAGGED_X = np.array([-900.0, -650.0, -300.0, -120.0, 150.0, 520.0, 1000.0])
RAGGED_Y = np.array([-700.0, -250.0, 180.0, 800.0])
RAGGED_LAT = np.array([24.0, 26.5, 28.0, 31.5, 33.0, 36.0, 38.5])
RAGGED_LON = np.array([-9.0, -3.5, 1.0, 8.0])
RAGGED_NPZ = os.path.join(H.GOLDEN_DIR, "rngdep_ragged.npz")
RAGGED_SHORT = 0.03           # km: segments below this count as short


def ragged_heights(zj):
    """indices of the JetAtmo nodes the ragged grid keeps"""
    keep = set(range(0, len(zj), 3)) | {len(zj) - 1}
    short = np.flatnonzero(np.diff(zj) < RAGGED_SHORT)
    for k in short[::9]:
        keep |= set(range(int(k) - 3, int(k) + 5))
    return np.array(sorted(keep))


def grid_columns_ragged():
    """z [nz], T, u, v, rho [7][4][nz], p [nz] (raw .met units)"""
    import jet_data as JD
    c = JD.load_columns()
    k = ragged_heights(c["z"])
    z, T0, u0, v0, rho0, p = (c[q][k] for q in ("z", "T", "u", "v", "rho", "p"))
    nx, ny = len(RAGGED_X), len(RAGGED_Y)
    T = np.zeros((nx, ny, len(z))); u = np.zeros_like(T); v = np.zeros_like(T); rho = np.zeros_like(T)
    for i in range(nx):
        for j in range(ny):
            a = (RAGGED_X[i] - RAGGED_X[0]) / (RAGGED_X[-1] - RAGGED_X[0]) - 0.5
            b = (RAGGED_Y[j] - RAGGED_Y[0]) / (RAGGED_Y[-1] - RAGGED_Y[0]) - 0.5
            T[i, j] = T0 * (1.0 + 0.02 * np.sin(2.3 * a + 1.1 * b) * np.exp(-((z - 50.0) / 20.0) ** 2))
            u[i, j] = u0 * (1.0 + 0.3 * a) + 6.0 * np.sin(3.0 * b)
            v[i, j] = v0 * (1.0 - 0.4 * b) + 5.0 * np.cos(2.5 * a) * np.exp(-z / 60.0)
            rho[i, j] = rho0 * (1.0 + 0.01 * np.cos(1.7 * a - 2.2 * b))
    return z, T, u, v, rho, p


def save_grid_ragged_npz():
    z, T, u, v, rho, p = grid_columns_ragged()
    np.savez_compressed(RAGGED_NPZ, z=z, T=T, u=u, v=v, rho=rho, p=p, x=RAGGED_X, y=RAGGED_Y, lat=RAGGED_LAT, lon=RAGGED_LON)


def ragged_nodes(glob):
    return (RAGGED_LAT, RAGGED_LON) if glob else (RAGGED_X, RAGGED_Y)


def write_grid_ragged(dirpath, glob, short_paths=True):
    """writes r<n>.met (`zTuvdp`: the reference's range-dependent loaders take six-column files only) and the two node files (km, or degrees for the
    spherical set); returns (prefix, loc_a, loc_b)"""
    os.makedirs(dirpath, exist_ok=True)
    g = np.load(RAGGED_NPZ)
    z, T, u, v, rho, p = g["z"], g["T"], g["u"], g["v"], g["rho"], g["p"]
    na, nb = ragged_nodes(glob)
    prefix = os.path.join(dirpath, "r")
    assert len(prefix) < 40 or not short_paths
    for i in range(len(na)):
        for j in range(len(nb)):
            with open(f"{prefix}{i * len(nb) + j}.met", "w") as fh:
                for k in range(len(z)):
                    fh.write(f"{z[k]:.10g} {T[i, j, k]:.12g} {u[i, j, k]:.12g} {v[i, j, k]:.12g} {rho[i, j, k]:.12g} {p[k]:.10g}\n")
    loc_a, loc_b = os.path.join(dirpath, "loc_a.dat"), os.path.join(dirpath, "loc_b.dat")
    with open(loc_a, "w") as fh:
        fh.write("".join(f"{x:.10g}\n" for x in na))
    with open(loc_b, "w") as fh:
        fh.write("".join(f"{y:.10g}\n" for y in nb))
    return prefix, loc_a, loc_b


# ---- tests/golden/rngdep_ragged_{3drd,globalrd}.npz (make_golden.py ragged3d / raggedglobal): what the tables were made with, and how to read them ----
RAGGED_ZG = 0.3               # z_grnd of every table; the Cartesian main also LOADS with it (wind taper), the spherical -prop loads with 0
# table -> (fan, parameters besides src and z_grnd); fan a: ground source off every node, fan b: source at 12 km, rays below the horizontal included
RAGGED_TABLES = {"a_amp1": ("a", dict(bounces=2, calc_amp=1)), "a_amp0": ("a", dict(bounces=2, calc_amp=0)),
                 "b_amp1": ("b", dict(bounces=2, calc_amp=1, freq=10.0, tweak_abs=0.6)), "b_amp0": ("b", dict(bounces=2, calc_amp=0, freq=10.0, tweak_abs=0.6)),
                 "b_f001": ("b", dict(bounces=2, calc_amp=1, freq=0.01, tweak_abs=0.6))}


def ragged_fixture(glob):
    return np.load(os.path.join(H.GOLDEN_DIR, f"rngdep_ragged_{'globalrd' if glob else '3drd'}.npz"))


def ragged_load_z_grnd(glob):
    return 0.0 if glob else RAGGED_ZG


def ragged_table(g, tag):
    """(theta, phi, parameters, records, step total, sens) of a table.  b_f001 is stored as its ATTEN column: the generator asserted every other column equal to b_amp1's"""
    fan, kw = RAGGED_TABLES[tag]
    if f"{tag}_rec" in g.files:
        rec = g[f"{tag}_rec"]
    else:
        rec = g["b_amp1_rec"].copy()
        rec[..., H.REC["ATTEN"]] = g[f"{tag}_atten"]
    params = dict(kw, src=tuple(g[f"{fan}_src"]), z_grnd=float(g["z_grnd"]))
    return g[f"{fan}_theta"], g[f"{fan}_phi"], params, rec, int(g[f"{tag}_steps"]), g[f"{tag}_sens"]
