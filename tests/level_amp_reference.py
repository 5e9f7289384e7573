"""Plain numpy restatement of the level amplitudes (include/geoac_level_amp.h), written from its definition - TEST-ONLY, nothing under geoac_amd/
imports it.

The round's fan, BRANCH of the three rays, the finite-difference determinant, TZ, D and AMP, operation for operation in unfused float64, given
crossing tables (a FanContext's fetch_levels(), the restated k_levels of the oracle's paths, or synthetic ones) and a callable for the medium
(the public probe calls of the same context, the oracle's probes, or a made-up medium).  The elementary functions are those of
tests/refine_reference.py, the branch walk is branch_of_ray of tests/lstation_reference.py; both are imported, not edited."""
import os

import numpy as np

import lstation_reference as LS
from harness import GOLDEN_DIR
from levels_reference import LVL
from refine_reference import COS, SINCOSD, WRAP, PI, CONVERGED, spherical, bits  # noqa: F401
from station_reference import EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP  # noqa: F401

LAMP = dict(MEMBER=0, INDEX=1, LEG=2, DIR=3, ORD=4, STATUS=5, THETA=6, PHI=7, DET=8, TZ=9, D=10, AMP=11, C=12, RHO=13, TTIME=14, ATTEN=15)
LAMP_STRIDE = 16
OK, ABSENT, NO_PROBE, SINGULAR, SKIPPED = 1, 2, 3, 4, 5
STATUS_NAMES = {OK: "OK", ABSENT: "ABSENT", NO_PROBE: "NO_PROBE", SINGULAR: "SINGULAR", SKIPPED: "SKIPPED"}
P0 = LVL["P0"]
FIXTURE = os.path.join(GOLDEN_DIR, "level_amp.npz")          # tests/golden/make_level_amp.py


def fan_angles(th, ph, h):
    """the fan of 3 n rays: ray j * n + i is ray i at the trial (j = 0), at theta + h (1), at phi + h (2)"""
    th, ph = np.asarray(th, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    return np.concatenate([th, th + h, th]), np.concatenate([ph, ph, ph + h])


def source_points(eqset, src3, z_grnd=0.0, r_earth=6370.0):
    """the members' source points as the launch places them, src3 [M][3] in the layout of Params.src: (hc, a, b) [M] each - the height coordinate and the
    two horizontal abscissae in table order ((x, y) / (lat, lon) [rad])"""
    s = np.atleast_2d(np.asarray(src3, dtype=np.float64))
    if spherical(eqset):
        z = np.where(s[:, 0] < z_grnd, z_grnd, s[:, 0])
        return z + r_earth, s[:, 1] * PI / 180.0, s[:, 2] * PI / 180.0
    return np.where(z_grnd < s[:, 2], s[:, 2], z_grnd), s[:, 0].copy(), s[:, 1].copy()


def crossing_abscissae(eqset, rec):
    """(hc, a, b) of base crossing records rec [n][12], as source_points gives them"""
    if spherical(eqset):
        return rec[:, P0].copy(), rec[:, P0 + 1].copy(), rec[:, P0 + 2].copy()
    return rec[:, P0 + 2].copy(), rec[:, P0].copy(), rec[:, P0 + 1].copy()


def medium_of_context(ctx):
    """medium(hc, a, b) -> (c, u, v, rho) through the public probe calls of a FanContext after a launch: the bits the device rows are made of"""
    grid = ctx.eqset in (EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP)

    def medium(hc, a, b):
        if grid:
            _, a7 = ctx.probe_grid(a, b, hc, coop=False)
            return a7[:, 0].copy(), a7[:, 2].copy(), a7[:, 3].copy(), a7[:, 1].copy()
        o9, rho = ctx.probe_atmo_1d(hc)
        return o9[:, 0].copy(), o9[:, 3].copy(), o9[:, 6].copy(), rho
    return medium


def medium_of_oracle(O):
    """the same through the plain-C oracle's probes (tests/harness.py, Oracle or RefShim)"""
    grid = O.eqset in (EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP)

    def medium(hc, a, b):
        if grid:
            _, a8 = O.grid_probe(hc, a, b) if spherical(O.eqset) else O.grid_probe(a, b, hc)          # (the oracle's spherical grid takes r, lat, lon)
            return a8[:, 0].copy(), a8[:, 2].copy(), a8[:, 3].copy(), a8[:, 1].copy()
        o9, rho = O.atmo_probe(hc)
        return o9[:, 0].copy(), o9[:, 3].copy(), o9[:, 6].copy(), rho
    return medium


def branch_records(count, lrec, member, level, leg, direction, ordinal, index, n, j):
    """rec [R][12] and present [R] of BRANCH(ray j * n + index) for every row of crossing tables count [M][3 n][L], lrec [M][3 n][L][capL][12]"""
    R = len(member)
    rec, present = np.zeros((R, lrec.shape[-1])), np.zeros(R, dtype=bool)
    for t in range(R):
        ray = j * n + int(index[t])
        k = LS.branch_of_ray(count[member[t], ray, level[t]], lrec[member[t], ray, level[t]], int(leg[t]), direction[t], int(ordinal[t]))
        if k >= 0:
            rec[t], present[t] = lrec[member[t], ray, level[t], k], True
    return rec, present


def tube(eqset, rec, rec_t, rec_p, th, ph, h, r_level, m, s, parts=False):
    """DET, TZ, D, AMP [n] of the header's steps 1 .. 5 from the three crossing records [n][12], the base rays' launch angles th, ph [n], the level radii
    r_level [n] (spherical sets) and the medium m = (c, u, v, rho) at the crossing, s = the same at the member's source, [n] each.  parts: also num and
    den / D, so that a caller can put another D in its place (tests/golden/make_level_amp.py: the Jacobian's)"""
    c, ct, cp = (LS.crossing_points(eqset, r) for r in (rec, rec_t, rec_p))
    c_, u, v, rho = m
    cs, us, vs, rhos = s
    with np.errstate(all="ignore"):
        a00, a01 = (ct[0] - c[0]) / h, (cp[0] - c[0]) / h
        if spherical(eqset):
            a10, a11 = WRAP(ct[1] - c[1]) / h, WRAP(cp[1] - c[1]) / h
        else:
            a10, a11 = (ct[1] - c[1]) / h, (cp[1] - c[1]) / h
        det = a00 * a11 - a01 * a10
        sth, cth = SINCOSD(th)
        sph, cph = SINCOSD(ph)
        n0, n1, n2 = rec[:, P0 + 3], rec[:, P0 + 4], rec[:, P0 + 5]
        c3, cs3 = c_ * c_ * c_, cs * cs * cs
        if eqset == EQ_3D:
            e0, e1 = cth * sph, cth * cph
            MS = 1.0 + (e0 * (us / cs) + e1 * (vs / cs))
            nx, ny, nz = e0 / MS, e1 / MS, n0
            nu = (cs - nx * u - ny * v) / c_
            nu_s = 1.0 - (nx * us - ny * vs) / cs
            g0, g1, g2 = c_ * nx / nu + u, c_ * ny / nu + v, c_ * nz / nu
            G = np.sqrt(g0 * g0 + g1 * g1 + g2 * g2)
            tz = g2 / G
            q0, q1, qx, qy = cs * nx / nu_s + us, cs * ny / nu_s + vs, nx / nu_s, ny / nu_s
            q2 = cs * np.sqrt(1.0 - qx * qx - qy * qy)
            Q = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2)
        elif eqset == EQ_3D_RNGDEP:
            nm = np.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
            j0, j1, j2 = c_ * n0 / nm + u, c_ * n1 / nm + v, c_ * n2 / nm
            J = np.sqrt(j0 * j0 + j1 * j1 + j2 * j2)
            tz = j2 / J
            nu = (cs - n0 * u - n1 * v) / c_
            nu_s = 1.0 - n0 * us / cs - n1 * vs / cs
            g0, g1, g2 = c_ * n0 / nu + u, c_ * n1 / nu + v, c_ * n2 / nu
            G = np.sqrt(g0 * g0 + g1 * g1 + g2 * g2)
            q0, q1, q2 = cs * cth * sph + us, cs * cth * cph + vs, cs * sth
            Q = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2)
        else:
            nm = np.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
            j0, j1, j2 = c_ * n0 / nm, c_ * n1 / nm + v, c_ * n2 / nm + u
            J = np.sqrt(j0 * j0 + j1 * j1 + j2 * j2)
            tz = j0 / J
            e1, e2 = cth * cph, cth * sph
            MS = 1.0 + (e1 * (vs / cs) + e2 * (us / cs))
            nu_s = 1.0 / MS
            nu = (cs - n1 * v - n2 * u) / c_
            g0, g1, g2 = c_ * n0 / nu, c_ * n1 / nu + v, c_ * n2 / nu + u
            G = np.sqrt(g0 * g0 + g1 * g1 + g2 * g2)
            q0, q1, q2 = cs * sth / nu_s, cs * e1 / nu + vs, cs * e2 / nu + us
            Q = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2)
        if spherical(eqset):
            D = r_level * r_level * COS(c[0] * PI / 180.0) * np.abs(tz * det)
        else:
            D = np.abs(tz * det) * (180.0 / PI) * (180.0 / PI)
        num = rho * nu * c3 * Q * cth
        den0 = rhos * nu_s * cs3 * G
        den = den0 * D
        amp = 1.0 / (4.0 * PI) * np.sqrt(np.abs(num / den))
    return (det, tz, D, amp, num, den0) if parts else (det, tz, D, amp)


def reference_rows(eqset, count, lrec, th, ph, h, member, index, level, leg, direction, ordinal, z_km, medium, src3, z_grnd=0.0, r_earth=6370.0, refine_status=None):
    """rows [R][16] of crossing tables count [M][3 n][L], lrec [M][3 n][L][capL][12] of the fan fan_angles(th, ph, h): row t is ray index[t] of member
    member[t] on level level[t], branch (leg, direction +1 / -1, ordinal)[t].  medium(hc, a, b) -> (c, u, v, rho); src3 [M][3]; refine_status [R]: the
    refinement's statuses (rows that are not CONVERGED are SKIPPED), or None"""
    th, ph = np.asarray(th, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    n = len(th)
    member, index, level, leg, ordinal = (np.asarray(a, dtype=np.int64) for a in (member, index, level, leg, ordinal))
    direction = np.where(np.asarray(direction, dtype=np.float64) > 0.0, 1.0, -1.0)
    R = len(member)
    count, lrec = np.asarray(count), np.asarray(lrec)
    count = count.reshape((-1, 3 * n, count.shape[-1]))
    lrec = lrec.reshape((count.shape[0], 3 * n) + lrec.shape[-3:])
    rec, has = branch_records(count, lrec, member, level, leg, direction, ordinal, index, n, 0)
    rec_t, has_t = branch_records(count, lrec, member, level, leg, direction, ordinal, index, n, 1)
    rec_p, has_p = branch_records(count, lrec, member, level, leg, direction, ordinal, index, n, 2)
    status = np.full(R, OK)
    status[~(has_t & has_p)] = NO_PROBE
    status[~has] = ABSENT
    if refine_status is not None:
        status[np.asarray(refine_status) != CONVERGED] = SKIPPED
    out = np.zeros((R, LAMP_STRIDE))
    out[:, LAMP["MEMBER"]], out[:, LAMP["INDEX"]], out[:, LAMP["LEG"]], out[:, LAMP["DIR"]], out[:, LAMP["ORD"]] = member, index, leg, direction, ordinal
    out[:, LAMP["THETA"]], out[:, LAMP["PHI"]] = th[index], ph[index]
    ok = status == OK
    if ok.any():
        hc, a, b = crossing_abscissae(eqset, rec[ok])
        shc, sa, sb = source_points(eqset, src3, z_grnd, r_earth)
        m = medium(hc, a, b)
        s = tuple(v[member[ok]] for v in medium(shc, sa, sb))
        r_level = r_earth + np.asarray(z_km, dtype=np.float64)[level[ok]]
        det, tz, D, amp = tube(eqset, rec[ok], rec_t[ok], rec_p[ok], th[index[ok]], ph[index[ok]], h, r_level, m, s)
        bad = (det == 0.0) | ~np.isfinite(det) | (D == 0.0) | ~np.isfinite(D) | (amp == 0.0) | ~np.isfinite(amp)
        vals = np.stack([det, tz, D, amp, m[0], m[3], rec[ok][:, LVL["TTIME"]], rec[ok][:, LVL["ATTEN"]]], axis=1)
        vals[bad] = 0.0
        out[ok, LAMP["DET"]:] = vals
        st = status[ok]
        st[bad] = SINGULAR
        status[ok] = st
    out[:, LAMP["STATUS"]] = status
    return out


def rows_at(eqset, count, lrec, th, ph, level_of, leg, direction, ordinal, h, z_km, medium, src3, **kw):
    """the rows [M][n][16] of level_amp_at: every member, every ray"""
    n = len(th)
    M = np.asarray(count).reshape((-1, 3 * n, np.asarray(count).shape[-1])).shape[0]
    rep = lambda a: np.tile(np.broadcast_to(np.asarray(a), (n,)), M)          # noqa: E731
    out = reference_rows(eqset, count, lrec, th, ph, h, np.repeat(np.arange(M), n), np.tile(np.arange(n), M), rep(level_of), rep(leg), rep(direction), rep(ordinal),
                         z_km, medium, src3, **kw)
    return out.reshape(M, n, LAMP_STRIDE)


def assert_equal_bits(got, want, name="rows"):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    diff = bits(g) != bits(w)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.size} entries differ, first at {at}: {g[at]!r} vs {w[at]!r}")
