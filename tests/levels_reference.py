"""Level crossings (include/geoac_levels.h) restated in numpy from the full rows of one leg: the half-open crossing rule of k_levels
(geoac_amd/csrc/geoac_levels.hip), FRAC and the interpolated row with the kernel's operations one by one (a subtract, a divide, a multiply,
an add - no fused multiply-add in numpy either).  Shared by tests/golden/make_golden_levels.py, tests/test_levels_host.py and
tests/test_gpu_levels.py."""
import os

import numpy as np

from harness import EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP, GOLDEN_DIR

FIXTURE = os.path.join(GOLDEN_DIR, "levels_small.npz")
THETAS = np.array([3.0, 10.0, 18.0, 25.0, 33.0, 41.0])      # the fixture's rays, azimuth -90
PHI = -90.0
R_EARTH = 6370.0
LVL = dict(LEG=0, DIR=1, FRAC=2, TTIME=3, ATTEN=4, P0=5)
LVL_STRIDE = 12

SPHERICAL = (EQ_GLOBAL, EQ_GLOBAL_RNGDEP)
PATHW = {EQ_3D: 4, EQ_GLOBAL: 6, EQ_3D_RNGDEP: 6, EQ_GLOBAL_RNGDEP: 6}


def hidx(eq):
    """height component of a path row"""
    return 0 if eq in SPHERICAL else 2


def level_values(eq, z_km, r_earth=R_EARTH):
    """the levels in the units of the height component: z_km, or r_earth + z_km (one addition, as the library forms it)"""
    z = np.asarray(z_km, dtype=np.float64)
    return r_earth + z if eq in SPHERICAL else z.copy()


def crossings(eq, rows, z_km, r_earth=R_EARTH):
    """rows [k + 1][>= pathw] of one leg -> the leg's crossings in path order (segment by segment, within a segment by level): a list of dicts
    level (index into z_km), dir (+1 / -1), seg (i of the segment (i, i + 1)), frac, row (the pathw interpolated components)"""
    pw, hi = PATHW[eq], hidx(eq)
    lev = level_values(eq, z_km, r_earth)
    h = rows[:, hi]
    out = []
    for l, L in enumerate(lev):
        up = (h[:-1] < L) & (L <= h[1:])
        down = (h[:-1] >= L) & (L > h[1:])
        for i in np.nonzero(up | down)[0]:
            ha, hb = h[i], h[i + 1]
            f = (L - ha) / (hb - ha)
            a, b = rows[i, :pw], rows[i + 1, :pw]
            out.append(dict(level=l, dir=1 if up[i] else -1, seg=int(i), frac=f, row=a + f * (b - a), a=a.copy(), b=b.copy()))
    out.sort(key=lambda c: (c["seg"], c["level"]))
    return out


def per_level(cr, n_levels):
    """the crossings of crossings() grouped by level, each in path order - the order of a ray's record slots"""
    return [[c for c in cr if c["level"] == l] for l in range(n_levels)]


def position_errors(eq, got, want):
    """relative error of crossing positions got, want [n][>= 3] (the first three path components), one figure per crossing.
    Cartesian sets: |got - want| / |want| of the position vector (x, y, z) - a ray launched along an axis has a coordinate that is zero up to
    rounding (y ~ 1e-14 km at azimuth -90), and such a component has no relative error of its own.  Spherical sets: r, lat, lon are no vector;
    each is judged as tests/parity.py judges a state component, |got - want| / max(|want|, 1e-6 x the column's largest |want|), the worst of the three."""
    got, want = np.asarray(got)[:, :3], np.asarray(want)[:, :3]
    if eq in SPHERICAL:
        floor = 1e-6 * np.abs(want).max(axis=0, keepdims=True)
        return (np.abs(got - want) / np.maximum(np.abs(want), floor)).max(axis=1)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def fixture_rays(g, name):
    """the fixture's crossings of one set, per ray and level in path order: {(ray, level): [index into the fixture's flat arrays, ...]}"""
    out = {}
    for j, (r, l) in enumerate(zip(g[f"{name}_ray"], g[f"{name}_level"])):
        out.setdefault((int(r), int(l)), []).append(j)
    return out


def turning_height(eq, rows, r_earth=R_EARTH):
    """largest height above sea level of a leg's rows [km]"""
    h = rows[:, hidx(eq)].max()
    return h - r_earth if eq in SPHERICAL else h
