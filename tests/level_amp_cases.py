"""Cases that the CPU and the GPU tests of the level amplitudes share (tests/test_level_amp_host.py, tests/test_gpu_level_amp.py) - pure numpy.

The closed form: the isothermal windless medium of tests/raised_ground.py (source 20 km above a raised ground, rays launched downward), Cartesian
sets, the downward passage of leg 0 through the levels 8 and 15 km.  The rays are straight lines: ray (theta, phi), a = |theta|, passes level z_l at
the horizontal distance rho(theta) = dz / tan a from the source, dz = z_src - z_l, on the bearing phi.  The forward-difference matrix of
include/geoac_level_amp.h is then known without any ray: its columns are (rho(theta + h) - rho(theta)) / h (sin phi, cos phi) and
rho(theta) / h (sin(phi + h) - sin phi, cos(phi + h) - cos phi), so |DET| = |rho(theta + h) - rho(theta)| rho(theta) sin(h) / h^2 (h in degrees, the sine
of h degrees).  The amplitude of a point source in this medium is spherical spreading times the density factor, 1 / (4 pi L) sqrt(rho_air / rho_air,0)
with L = dz / sin a."""
import numpy as np

import raised_ground as RG
from level_amp_reference import LAMP, OK

THETA, PHI = RG.THETA_STAR, RG.PHI_STAR                # twelve rays, none on an axis
LEVELS = RG.LEVELS
PARAMS = RG.LEVEL_PARAMS                               # one bounce, the reflected ray ended above the levels
H_DEG = 0.02
BRANCH = dict(leg=0, dir=-1, ord=0)
STRAIGHT = 1e-9                                        # a passage lies within this much of its path length of the straight line (tests/raised_ground.py check_levels)


def rays():
    """theta, phi, level_of [24]: the twelve rays on each of the two levels"""
    return np.tile(THETA, 2), np.tile(PHI, 2), np.repeat([0, 1], len(THETA))


def rho_of(theta_deg, dz):
    return dz / np.tan(np.radians(np.abs(theta_deg)))


def check_closed_form(rows, h=H_DEG):
    """rows [24][16] of the rays() at probe step h, all on BRANCH.  Returns the worst figures; raises on the first rule broken."""
    th, ph, lv = rays()
    assert rows.shape == (24, 16) and (rows[:, LAMP["STATUS"]] == OK).all(), rows[:, LAMP["STATUS"]]
    assert (rows[:, LAMP["LEG"]] == 0).all() and (rows[:, LAMP["DIR"]] == -1.0).all() and (rows[:, LAMP["ORD"]] == 0).all()
    dz = RG.Z_SRC - np.asarray(LEVELS)[lv]
    a = np.radians(-th)
    rho, rho_h = rho_of(th, dz), rho_of(th + h, dz)
    path = dz / np.sin(a)
    # 1. DET: three crossing points, each within STRAIGHT x path of its place; the difference rho(theta + h) - rho(theta) carries two of them
    det_cf = np.abs(rho_h - rho) * rho * np.sin(np.radians(h)) / (h * h)
    e_det = np.abs(np.abs(rows[:, LAMP["DET"]]) / det_cf - 1.0)
    b_det = 2.0 * STRAIGHT * path / np.abs(rho_h - rho)
    # 2. TZ = -sin a (the group velocity is the launch direction), C, and the records' own travel time
    e_tz = np.abs(rows[:, LAMP["TZ"]] + np.sin(a))
    # 3. AMP against spherical spreading x the density factor.  What separates the forward tube from the exact spreading is known in closed form too:
    #    D_exact = sin a rho |rho'| with rho' = dz / sin^2 a per radian, D_tube = sin a x det_cf (180 / pi)^2, AMP ~ D^-1/2.  On top of it the error of DET
    #    above, halved by the root, TZ's, and 1e-9 for the spline's density between nodes and the rounding of a dozen operations.
    d_exact = np.sin(a) * rho * dz / np.sin(a) ** 2
    d_tube = np.sin(a) * det_cf * (180.0 / np.pi) ** 2
    trunc = np.abs(np.sqrt(d_exact / d_tube) - 1.0)
    amp_cf = np.exp(0.5 * dz / RG.SCALE_HEIGHT) / (4.0 * np.pi * path)
    e_amp = np.abs(rows[:, LAMP["AMP"]] / amp_cf - 1.0)
    b_fd = 0.5 * b_det + 0.5 * STRAIGHT / np.sin(a) + 1e-9
    b_amp = trunc + b_fd
    e_fd = np.abs(rows[:, LAMP["AMP"]] / (amp_cf * np.sqrt(d_exact / d_tube)) - 1.0)          # ... and against the closed form of the forward tube itself
    out = dict(det_of_bound=float((e_det / b_det).max()), det_err=float(e_det.max()), tz_err=float(e_tz.max()), amp_err=float(e_amp.max()),
               amp_of_bound=float((e_amp / b_amp).max()), truncation=float(trunc.max()), amp_fd_err=float(e_fd.max()), amp_fd_of_bound=float((e_fd / b_fd).max()))
    assert (e_det <= b_det).all(), out
    assert (e_tz <= STRAIGHT).all(), out
    assert (e_amp <= b_amp).all() and (e_fd <= b_fd).all(), out
    assert np.allclose(rows[:, LAMP["C"]], RG.C, rtol=1e-12, atol=0.0) and np.allclose(rows[:, LAMP["TTIME"]], path / RG.C, rtol=1e-9, atol=0.0), out
    return out
