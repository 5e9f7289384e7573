"""Cases that the CPU and the GPU tests of the level loudness maps share (tests/test_lampmap_host.py, tests/test_gpu_lampmap.py) - pure numpy
and imports; nothing here runs the code under test.

1. The closed form.  The isothermal windless medium of tests/raised_ground.py on the Cartesian sets: a source 20 km above a raised ground, straight
rays launched downward, the downward passage of leg 0 through the levels 8 and 15 km.  Ray (theta, phi), a = |theta|, passes level z_l at
X = src + rho(a) (sin phi, cos phi), rho(a) = dz / tan a, dz = z_src - z_l; the exact amplitude at a point of the level is exp(dz / 2H) / (4 pi L),
L its distance from the source.

The bound between the map's first-order amplitude and the exact one, derived here and not measured.  In this medium c = c_s, nu = nu_s = 1 and
G |TZ| = c |nz| on both Cartesian sets (geoac_level_amp.h, step 3: GEOAC_EQ_3D has g = c (cos THETA sin PHI, cos THETA cos PHI, nz), TZ = g2 / G;
GEOAC_EQ_3D_RNGDEP has G = c |n|, TZ = n2 / |n|), Q = c_s, so the header's AMP is
    AMP^2 = K^2 cos THETA / (|nz| DET_rad),    K = exp(dz / 2H) / (4 pi),   DET_rad = |DET| (180 / pi)^2
with THETA and nz = sum Wk sin theta_k interpolated at the centre.  A lattice triangle of the cell theta_i .. theta_i+1 (a_lo <= a <= a_hi),
phi_j .. phi_j + h_phi has the corners rho_1 or rho_2 times (sin phi, cos phi): its area is |rho_2 - rho_1| rho_k sin(h_phi) / 2 with rho_k one of
the two radii, the launch-angle triangle's h_theta h_phi / 2.  By the mean-value theorem |rho_2 - rho_1| / h_theta = dz / sin^2 xi for some xi in the
cell.  Every factor is monotone in a, and the weights are in 0 .. 1, so each lies between its values at the cell's two inclinations:
    cos a_hi <= cos THETA <= cos a_lo,   sin a_lo <= |nz| <= sin a_hi,   dz / sin^2 a_hi <= |drho| / h_theta <= dz / sin^2 a_lo,
    dz / tan a_hi <= rho_k <= dz / tan a_lo,   sin(h_phi) / h_phi <= 1.
AMP therefore lies between K sqrt(lo) and K sqrt(hi),
    lo = cos a_hi / (sin a_hi (dz / sin^2 a_lo) (dz / tan a_lo)),   hi = cos a_lo / (sin a_lo (dz / sin^2 a_hi) (dz / tan a_hi) (sin h_phi / h_phi)),
and the exact amplitude at the centre is known, so the bound on |AMP / exact - 1| is the larger of the two ends' distances from it.  It is first
order in the lattice step: DET is the mean of the ray map's determinant over the triangle, and the determinant changes by O(h) across it.  On top
of it SLACK for what is not the lattice: crossing points within STRAIGHT of their path length of the straight line (tests/level_amp_cases.py), which
DET takes as a difference of two radii, and 1e-9 for the spline's density and the rounding of a few dozen operations.

2. The reference's Jacobian amplitude.  tests/golden/level_amp.npz holds, per crossing of the compiled reference's own rays, the crossing point,
the branch, the travel time, the attenuation and the amplitude of the reference's Jacobian.  A 2 x 2 lattice about each fixture ray (one lattice cell
that holds the ray strictly inside, off its middle) is launched, and a one-cell map is centred on each crossing point.  GAP_MEASURED holds the worst
gaps of the CPU chain (the oracle's paths, the restated k_levels, tests/lampmap_reference.py) per set and lattice step; the caps are twice that."""
import numpy as np

import harness as H
import lampmap_reference as LM
import level_amp_cases as LAC
import raised_ground as RG
import station_cases as SC
import station_reference as SR
from levels_reference import LVL, LVL_STRIDE

P0 = LVL["P0"]

# ---------------------------------------------------------------- 1. the closed form
RG_CELLS = (31, 45)
RG_SPAN = 150.0
RHO0 = 1.2e-3


def rg_lattice(halvings=0, sector=None):
    """the downward lattice of tests/raised_ground.py with its steps halved `halvings` times; sector = (phi_min, phi_max): that many azimuths only"""
    f = 2.0 ** halvings
    lat = dict(RG.LATTICE, theta_step=RG.LATTICE["theta_step"] / f, phi_step=RG.LATTICE["phi_step"] / f)
    if sector is None:
        lat["phi_max"] = 360.0 - lat["phi_step"]
    else:
        lat["phi_min"], lat["phi_max"] = sector
    return SC.lattice(**lat)


def rg_spec(eq, nt, nph, periodic=True, **kw):
    step = (RG_SPAN / RG_CELLS[0], RG_SPAN / RG_CELLS[1])
    origin = tuple(RG.SRC[eq][k] - RG_SPAN / 2 + RG.FRAC[k] * step[k] for k in (0, 1))
    return LM.spec(origin=origin, step=step, n=RG_CELLS, n_theta=nt, n_phi=nph, edge_max=60.0, level_mask=0b11, phi_periodic=periodic, leg_max=0, dir_mask=2, **kw)


def rg_medium(hc, a, b):
    z = np.asarray(hc, dtype=np.float64)
    return np.full_like(z, RG.C), np.zeros_like(z), np.zeros_like(z), RHO0 * np.exp(-z / RG.SCALE_HEIGHT)


def rg_tables(eq, th, ph, atten_per_km=0.0):
    """synthetic crossing tables count [1][n][2], lrec [1][n][2][1][12] of straight rays from RG.SRC[eq] through RG.LEVELS: leg 0, downward"""
    n = len(th)
    a, az = np.radians(-th), np.radians(ph)
    count = np.ones((1, n, len(RG.LEVELS)), dtype=np.int32)
    lrec = np.zeros((1, n, len(RG.LEVELS), 1, LVL_STRIDE))
    for l, z in enumerate(RG.LEVELS):
        dz = RG.Z_SRC - z
        rho, path = dz / np.tan(a), dz / np.sin(a)
        r = lrec[0, :, l, 0]
        r[:, LVL["LEG"]], r[:, LVL["DIR"]] = 0.0, -1.0
        r[:, P0], r[:, P0 + 1], r[:, P0 + 2] = RG.SRC[eq][0] + rho * np.sin(az), RG.SRC[eq][1] + rho * np.cos(az), z
        if eq == H.EQ_3D:
            r[:, P0 + 3] = -np.sin(a)                                                   # (the stratified set keeps nz alone)
        else:
            r[:, P0 + 3], r[:, P0 + 4], r[:, P0 + 5] = np.cos(a) * np.sin(az), np.cos(a) * np.cos(az), -np.sin(a)
        r[:, LVL["TTIME"]], r[:, LVL["ATTEN"]] = path / RG.C, atten_per_km * path
    return count, lrec


def check_closed_form(eq, layers, sp, th, ph, nt):
    """layers of rg_spec on the lattice th, ph whose inclination axis is th[:nt].  Every cell with one usable hit: AMP_MAX against exp(dz / 2H) / (4 pi L) under
    the bound derived above.  Returns per level (cells checked, worst error, median error, largest share of the bound used)."""
    axis = np.abs(np.asarray(th[:nt], dtype=np.float64))
    n_tri = 2 * (nt - 1) * (sp["n_phi"] if sp["phi_periodic"] else sp["n_phi"] - 1)
    hp = np.radians(abs(float(ph[nt]) - float(ph[0])))                                   # the azimuth step
    cen = LM.LT.centres(sp)
    src = np.array(RG.SRC[eq])
    out = {}
    for ls, z in enumerate(RG.LEVELS):
        dz = RG.Z_SRC - z
        one = np.flatnonzero((layers["count"][0, ls].reshape(-1) == 1) & (layers["weak"][0, ls].reshape(-1) == 0))
        assert one.size >= 100, (z, one.size)
        amp = layers["amp_max"][0, ls].reshape(-1)[one]
        key = layers["loudest"][0, ls].reshape(-1)[one]
        assert (key // n_tri == 1).all()                                                # b = ((0 - 0) * 2 + 1) * 1 + 0: leg 0, downward, ordinal 0
        i = ((key % n_tri) // 2) % (nt - 1)
        a_lo, a_hi = np.radians(np.minimum(axis[i], axis[i + 1])), np.radians(np.maximum(axis[i], axis[i + 1]))
        K = np.exp(0.5 * dz / RG.SCALE_HEIGHT) / (4.0 * np.pi)
        lo = np.cos(a_hi) / (np.sin(a_hi) * (dz / np.sin(a_lo) ** 2) * (dz / np.tan(a_lo)))
        hi = np.cos(a_lo) / (np.sin(a_lo) * (dz / np.sin(a_hi) ** 2) * (dz / np.tan(a_hi)) * (np.sin(hp) / hp))
        L = np.sqrt(((cen[one] - src[:2]) ** 2).sum(axis=1) + dz * dz)
        exact = K / L
        # SLACK: the two radii of DET's difference each within STRAIGHT of the path length of its place, halved by the root; TZ's; the density and rounding
        d_rho = dz / np.tan(a_lo) - dz / np.tan(a_hi)
        slack = LAC.STRAIGHT * (dz / np.sin(a_lo)) / d_rho + 0.5 * LAC.STRAIGHT / np.sin(a_lo) + 1e-9
        bound = np.maximum(K * np.sqrt(hi) / exact - 1.0, 1.0 - K * np.sqrt(lo) / exact) + slack
        err = np.abs(amp / exact - 1.0)
        out[z] = (int(one.size), float(err.max()), float(np.median(err)), float((err / bound).max()))
        assert (bound > 0).all() and (err <= bound).all(), (z, out[z], int(one[np.argmax(err / bound)]))
    return out


def cf_figures(out):
    return ", ".join(f"level {z} km: {n} cells, worst |AMP_MAX / exact - 1| {w:.3e}, median {m:.3e}, largest share of the bound used {s:.3f}" for z, (n, w, m, s) in out.items())


# ---------------------------------------------------------------- 2. the reference's Jacobian amplitude
FIX_SETS = (("3d", H.EQ_3D), ("global", H.EQ_GLOBAL), ("3drd", H.EQ_3D_RNGDEP))
FIX_STEPS = (2.0, 1.0)                                  # lattice steps [deg], the second half the first
FIX_OFF = 0.4                                           # the fixture ray lies this share of a step above the cell's lower node, on both axes
FIX_CELL = {H.EQ_3D: 1.0, H.EQ_3D_RNGDEP: 1.0, H.EQ_GLOBAL: 0.01}          # the one-cell map's cell size [km | deg]
FIX_EDGE = {H.EQ_3D: 250.0, H.EQ_3D_RNGDEP: 250.0, H.EQ_GLOBAL: 2.5}         # edge_max: removes no triangle of a 2-degree cell (span 503 x 503 centres)


def fix_lattice(theta, phi, h):
    """the 2 x 2 lattice about a fixture ray: rays (a, b, d, c) = (lo, lo), (hi, lo), (lo, hi), (hi, hi) in the order ray = j * 2 + i"""
    t = np.array([theta - FIX_OFF * h, theta + (1.0 - FIX_OFF) * h])
    p = np.array([phi - FIX_OFF * h, phi + (1.0 - FIX_OFF) * h])
    return np.tile(t, 2), np.repeat(p, 2)


def fix_spec(eq, point, leg, direction, level, **kw):
    """the one-cell map centred on a crossing point, restricted to the crossing's branch"""
    c = FIX_CELL[eq]
    return LM.spec(origin=(point[0] - c / 2, point[1] - c / 2), step=(c, c), n=(1, 1), n_theta=2, n_phi=2, edge_max=FIX_EDGE[eq], level_mask=1 << int(level),
                   leg_min=int(leg), leg_max=int(leg), ord_max=1, dir_mask=1 if direction > 0 else 2, **kw)


def fix_crossings(g, name):
    """per fixture ray of set `name`: (ray index, theta, phi, [crossing indices])"""
    ray = g[f"{name}_ray"]
    return [(int(r), float(g[f"{name}_theta"][r]), float(g[f"{name}_phi"][r]), np.flatnonzero(ray == r)) for r in np.unique(ray)]


def fix_amp(g, name):
    return g[f"{name}_amp_jac_cos"] if f"{name}_amp_jac_cos" in g.files else g[f"{name}_amp_jac"]


# worst gaps of the CPU chain per (set, lattice step): (|AMP / amp_jac - 1|, |TTIME / ttime - 1|, |ATTEN - atten| / max(atten, 1e-3 dB)), and the crossings
# the chain leaves out (no hit or WEAK), measured by tests/test_lampmap_host.py::test_gap_to_the_references_jacobian_amplitude, which prints them
GAP_MEASURED = {
    ("3d", 2.0): (0.3594, 2.439e-4, 0.1356), ("3d", 1.0): (0.1671, 6.106e-5, 0.02496),
    ("global", 2.0): (0.1493, 3.584e-4, 0.02095), ("global", 1.0): (0.09584, 8.971e-5, 5.088e-3),
    ("3drd", 2.0): (0.4693, 2.063e-4, 7.121e-3), ("3drd", 1.0): (0.1573, 5.157e-5, 1.742e-3),
}
GAP_LEFT_OUT = {key: [] for key in GAP_MEASURED}          # the CPU chain leaves no fixture crossing out: every one-cell map has one usable hit
GAP_FACTOR = 2.0


def gap_caps(name, h):
    return tuple(GAP_FACTOR * v for v in GAP_MEASURED[(name, h)][:3])


def fix_gaps(name, eq, g, h, tables_of, hit_of):
    """the chain of part 2 at lattice step h.  tables_of(theta [4], phi [4]) launches the 2 x 2 lattice and returns whatever hit_of needs;
    hit_of(tables, sp) returns None (no hit, or the only hit is WEAK) or (AMP_MAX, TTIME, ATTEN) of the one-cell map sp.  Returns the gaps [n][3] per
    fixture crossing (NaN rows: left out) as GAP_MEASURED states them"""
    amp, tt, at = fix_amp(g, name), g[f"{name}_ttime"], g[f"{name}_atten"]
    out = np.full((len(amp), 3), np.nan)
    for r, theta, phi, idx in fix_crossings(g, name):
        tables = tables_of(*fix_lattice(theta, phi, h))
        for k in idx:
            sp = fix_spec(eq, g[f"{name}_points"][k, 0], g[f"{name}_leg"][k], g[f"{name}_dir"][k], g[f"{name}_level"][k])
            got = hit_of(tables, sp)
            if got is not None:
                out[k] = abs(got[0] / amp[k] - 1.0), abs(got[1] / tt[k] - 1.0), abs(got[2] - at[k]) / max(at[k], 1e-3)
    return out


def fix_summary(name, h, gaps):
    left = np.flatnonzero(np.isnan(gaps[:, 0]))
    kept = gaps[~np.isnan(gaps[:, 0])]
    return (f"{name} step {h:g} deg: {len(kept)} of {len(gaps)} crossings, worst gaps AMP {kept[:, 0].max():.3e} TTIME {kept[:, 1].max():.3e} ATTEN {kept[:, 2].max():.3e}, "
            f"median AMP gap {np.median(kept[:, 0]):.3e}, left out {left.tolist()}")
