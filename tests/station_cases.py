"""Shared pieces of the station tests (tests/test_gpu_stations.py, tools/perf_stations.py): lattice fans, stations drawn from a launch's own landing
points, and the re-launch check of an estimate - all of it independent of where the records come from (the device or the plain-C oracle)."""
import numpy as np

import harness as H
import station_reference as SR

S = SR.STA

# the lattice of the bit-identity cases: 13 inclinations x 9 azimuths around the westward direction the stratified test fans look in
PARITY_LATTICE = dict(theta_min=3.0, theta_max=39.0, theta_step=3.0, phi_min=-122.0, phi_max=-58.0, phi_step=8.0)
# the range-dependent cases run over the small synthetic grid of profiles: a narrower fan that stays inside it
PARITY_LATTICE_RD = dict(theta_min=4.0, theta_max=28.0, theta_step=3.0, phi_min=-120.0, phi_max=-64.0, phi_step=8.0)

# physics cases: GEOAC_EQ_GLOBAL, ToyAtmo, source (0, 30, 0), one bounce; 16 stations of the 2.5-degree, 64-position ring of config 5 around the source
PHYS_SRC = (0.0, 30.0, 0.0)
PHYS_FAN = dict(theta_min=0.5, theta_max=45.0, theta_step=0.5, phi_min=-180.0, phi_max=179.0, phi_step=1.0)
PHYS_FAN_HALF = dict(theta_min=0.5, theta_max=45.0, theta_step=0.25, phi_min=-180.0, phi_max=179.5, phi_step=0.5)


def lattice(**kw):
    """theta, phi, n_theta, n_phi of the reference's double loop (phi outer, theta inner, repeated addition)"""
    th, ph = H.fan_angles(**kw)
    n_theta = int(np.flatnonzero(ph != ph[0])[0]) if (ph != ph[0]).any() else th.size
    return th, ph, n_theta, th.size // n_theta


def draw_stations(eqset, rec, n_near=190, n_far=10, seed=5, jitter=0.35):
    """about 200 stations for a launch: VALID landing points of member 0 (any leg), each moved by a fixed-seed jitter of `jitter` times the spread
    of the landing points divided by 10, so that most stations lie inside some landing triangle; and n_far stations far outside every one"""
    rec = np.asarray(rec)
    c0, c1 = SR.landing(eqset, rec)
    ok = rec[0, :, :, 0] != 0.0
    p = np.stack([c0[0][ok], c1[0][ok]], axis=1)
    assert len(p) >= 20
    rng = np.random.default_rng(seed)
    pick = p[rng.integers(0, len(p), n_near)]
    scale = (p.max(axis=0) - p.min(axis=0)) / 10.0
    near = pick + rng.uniform(-jitter, jitter, pick.shape) * scale
    far = p.max(axis=0) + scale * 10.0 * (2.0 + rng.uniform(0.0, 1.0, (n_far, 2)))
    return np.concatenate([near, far])


PHYS_POSITIONS = list(range(40, 56))       # 16 neighbouring positions of the 64-ring, south-west to north-west of the source: where ToyAtmo's westward duct lands


def ring_stations(positions=None, lat0=30.0, lon0=0.0, radius_deg=2.5):
    """stations of the 64-position ring of config 5 around (lat0, lon0); the physics cases take PHYS_POSITIONS"""
    from parity import ring_receivers
    return ring_receivers(n=64, lat0=lat0, lon0=lon0, radius_deg=radius_deg)[PHYS_POSITIONS if positions is None else positions]


def relaunch_misses(eqset, hits, rows, rec, sp, sta, fan):
    """every kept estimate of member 0 integrated again: fan(theta, phi) -> records [n][legs][32].  Returns per estimate (miss, longest side of its
    landing triangle, valid): miss = distance of the re-launched ray's landing point on the estimate's leg from the station, in axis units"""
    est = [(r, k) for r in range(len(sta)) for k in range(min(int(hits[0, r]), sp["cap"]))]
    if not est:
        return np.zeros((0, 3))
    th = np.array([rows[0, r, k, S["THETA"]] for r, k in est])
    ph = np.array([rows[0, r, k, S["PHI"]] for r, k in est])
    again = np.asarray(fan(th, ph))
    c0, c1 = SR.landing(eqset, again[None])
    out = np.zeros((len(est), 3))
    for n, (r, k) in enumerate(est):
        leg = int(rows[0, r, k, S["LEG"]])
        _, side = SR.landing_triangle(eqset, rec, sp, 0, rows[0, r, k], sta[r])
        dx, dy = c0[0, n, leg] - sta[r, 0], c1[0, n, leg] - sta[r, 1]
        if eqset in (H.EQ_GLOBAL, H.EQ_GLOBAL_RNGDEP):
            dy = dy - 360.0 * np.floor((dy + 180.0) / 360.0)
        out[n] = (np.hypot(dx, dy), side, again[n, leg, 0] != 0.0)
    return out
