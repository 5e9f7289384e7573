"""Plain numpy restatement of the level refinement (include/geoac_level_refine.h), written from its definition - TEST-ONLY, nothing under
geoac_amd/ imports it.

Seeds, the three rays of a round, BRANCH, miss, the finite-difference Newton step, the step rule and the rows, operation for operation in unfused
float64, given a callable that integrates launch angles to crossing counts and records: a second FanContext (run + fetch_levels: the device's own
launches, so rows compare bit for bit).  The elementary functions are those of tests/refine_reference.py, the branch walk is branch_of_ray of
tests/lstation_reference.py; both are imported, not edited."""
import numpy as np

import lstation_reference as LS
from levels_reference import LVL
from refine_reference import DIST, WRAP, CONVERGED, ITER_LIMIT, STALLED, LOST, SINGULAR, MAX_RAY_MEMBERS, spherical, bits, start, step_rule, tally  # noqa: F401

LRF = dict(MEMBER=0, STATION=1, LEG=2, DIR=3, ORD=4, STATUS=5, ITER=6, THETA=7, PHI=8, MISS=9, TTIME=10, CELERITY=11, ATTEN=12, N0=13)
LRF_STRIDE = 16
S, P0 = LS.LSTA, LVL["P0"]


def spec(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2, probe_deg=0.02):
    return dict(max_iter=int(max_iter), max_shrink=int(max_shrink), tol=float(tol), step_max_deg=float(step_max_deg), probe_deg=float(probe_deg))


def seeds(hits, rows):
    """member, station, leg, ord [n] int, dir [n] (+1 / -1) and theta, phi [n] of the kept rows of level-station lists hits [M][R], rows [M][R][cap][16],
    in list order"""
    M, R, cap = rows.shape[:3]
    out = [(m, r, k) for m in range(M) for r in range(R) for k in range(min(int(hits[m, r]), cap))]
    if not out:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, np.zeros(0), np.zeros(0), np.zeros(0)
    m, r, k = (np.array(v, dtype=np.int64) for v in zip(*out))
    sel = rows[m, r, k]
    return (m, r, sel[:, S["LEG"]].astype(np.int64), sel[:, S["ORD"]].astype(np.int64), np.where(sel[:, S["DIR"]] > 0.0, 1.0, -1.0),
            sel[:, S["THETA"]].copy(), sel[:, S["PHI"]].copy())


def fan_angles(th, ph, h):
    """the round's fan of 3 n rays: ray j * n + i is seed i at the trial (j = 0), at theta + h (1), at phi + h (2)"""
    return np.concatenate([th, th + h, th]), np.concatenate([ph, ph, ph + h])


def branch_records(count, lrec, sm, sl, leg, direction, ordinal, j):
    """rec [n][12] and present [n] of BRANCH(ray j * n + i) for every seed i of crossing tables count [M][3 n][L], lrec [M][3 n][L][capL][12]"""
    n = len(sm)
    rec, present = np.zeros((n, lrec.shape[-1])), np.zeros(n, dtype=bool)
    for i in range(n):
        ray = j * n + i
        k = LS.branch_of_ray(count[sm[i], ray, sl[i]], lrec[sm[i], ray, sl[i]], int(leg[i]), direction[i], int(ordinal[i]))
        if k >= 0:
            rec[i], present[i] = lrec[sm[i], ray, sl[i], k], True
    return rec, present


def miss_of(eqset, c0, c1, present, s0, s1, r_level):
    """miss [n] of crossing points (c0, c1) [n] against stations (s0, s1) [n] on spheres of radius r_level [n]"""
    with np.errstate(all="ignore"):
        if spherical(eqset):
            miss = DIST(c0, c1, s0, s1, r_level)
        else:
            dx, dy = s0 - c0, s1 - c1
            miss = np.sqrt(dx * dx + dy * dy)
    miss = np.where(miss == miss, miss, np.inf)
    return np.where(present, miss, np.inf)


def newton(eqset, c, ct, cp, ok_probes, s0, s1, h, step_max):
    """d_th, d_ph, ok [n] from the crossing points c, ct, cp (each a pair of [n]) of the base ray and the two probes"""
    with np.errstate(all="ignore"):
        e0, a00, a01 = s0 - c[0], (ct[0] - c[0]) / h, (cp[0] - c[0]) / h
        if spherical(eqset):
            e1, a10, a11 = WRAP(s1 - c[1]), WRAP(ct[1] - c[1]) / h, WRAP(cp[1] - c[1]) / h
        else:
            e1, a10, a11 = s1 - c[1], (ct[1] - c[1]) / h, (cp[1] - c[1]) / h
        det = a00 * a11 - a01 * a10
        dt = (a11 * e0 - a01 * e1) / det
        dp = (a00 * e1 - a10 * e0) / det
    ok = ok_probes & (det != 0.0) & np.isfinite(det) & np.isfinite(dt) & np.isfinite(dp)
    dt = np.where(dt > step_max, step_max, dt)
    dt = np.where(dt < -step_max, -step_max, dt)
    dp = np.where(dp > step_max, step_max, dp)
    dp = np.where(dp < -step_max, -step_max, dp)
    return np.where(ok, dt, 0.0), np.where(ok, dp, 0.0), ok


def sources(eqset, src):
    """[M][2]: the members' source points in the stations' axes; src [M][3] in the layout of Params.src"""
    src = np.atleast_2d(np.asarray(src, dtype=np.float64))
    return np.ascontiguousarray(src[:, 1:3] if spherical(eqset) else src[:, 0:2])


def reference_level_refine(eqset, hits, rows, sta, level_of, z_km, sp, integrate, src, r_earth=6370.0):
    """rows [n][16], stats dict and the final (count, lrec) of the refinement of level-station lists (hits, rows) at stations sta on levels level_of of the
    level list z_km [km] under spec dict sp.  integrate(theta, phi) -> (count [M][3 n][L], lrec [M][3 n][L][capL][12]) of a launch of these angles;
    src [M][2] from sources()"""
    sta, level_of = np.ascontiguousarray(sta, dtype=np.float64), np.asarray(level_of, dtype=np.int64)
    M = rows.shape[0]
    sm, ss, leg, ordinal, direction, th, ph = seeds(hits, rows)
    n = len(sm)
    assert 3 * n * M <= MAX_RAY_MEMBERS
    stats = dict(launches=0, ray_members=0, seeds=n, converged=0, stalled_or_limit=0, lost_or_singular=0)
    if n == 0:
        return np.zeros((0, LRF_STRIDE)), stats, None
    sl = level_of[ss]
    s0, s1 = sta[ss, 0], sta[ss, 1]
    r_level = r_earth + np.asarray(z_km, dtype=np.float64)[sl]
    h = sp["probe_deg"]
    run = start(n)
    count = lrec = None
    for rnd in range(1, sp["max_iter"] + 1):
        if not (run[5] == 0).any():
            break
        count, lrec = integrate(*fan_angles(th, ph, h))
        count, lrec = np.asarray(count).reshape((M, 3 * n, -1)), np.asarray(lrec)
        lrec = lrec.reshape((M, 3 * n) + lrec.shape[-3:])
        stats["launches"] = rnd
        stats["ray_members"] += 3 * n * M
        R, present = branch_records(count, lrec, sm, sl, leg, direction, ordinal, 0)
        Rt, has_t = branch_records(count, lrec, sm, sl, leg, direction, ordinal, 1)
        Rp, has_p = branch_records(count, lrec, sm, sl, leg, direction, ordinal, 2)
        c, ct, cp = (LS.crossing_points(eqset, r) for r in (R, Rt, Rp))
        run, th, ph = step_rule(sp, rnd, th, ph, miss_of(eqset, c[0], c[1], present, s0, s1, r_level),
                                newton(eqset, c, ct, cp, has_t & has_p, s0, s1, h, sp["step_max_deg"]), run)
    b_th, b_ph, b_miss, _, _, status, _, used = run
    status = np.where(status == 0, ITER_LIMIT, status)
    out = np.zeros((n, LRF_STRIDE))
    out[:, LRF["MEMBER"]], out[:, LRF["STATION"]], out[:, LRF["LEG"]], out[:, LRF["DIR"]], out[:, LRF["ORD"]] = sm, ss, leg, direction, ordinal
    out[:, LRF["STATUS"]], out[:, LRF["ITER"]] = status, used
    out[:, LRF["THETA"]], out[:, LRF["PHI"]] = b_th, b_ph
    out[:, LRF["MISS"]] = np.where(status == LOST, -1.0, b_miss)
    R, present = branch_records(count, lrec, sm, sl, leg, direction, ordinal, 0)
    c = (status == CONVERGED) & present
    src = np.asarray(src, dtype=np.float64)
    with np.errstate(all="ignore"):
        if spherical(eqset):
            rng = DIST(src[sm, 0], src[sm, 1], s0, s1, r_earth)
        else:
            dx, dy = s0 - src[sm, 0], s1 - src[sm, 1]
            rng = np.sqrt(dx * dx + dy * dy)
        cel = rng / R[:, LVL["TTIME"]]
    for name, v in (("TTIME", R[:, LVL["TTIME"]]), ("CELERITY", cel), ("ATTEN", R[:, LVL["ATTEN"]])):
        out[:, LRF[name]] = np.where(c, v, 0.0)
    for q in range(3):
        out[:, LRF["N0"] + q] = np.where(c, R[:, P0 + 3 + q], 0.0)
    return out, tally(stats, status), (count, lrec)


def assert_equal_bits(got, want, name="rows"):
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    diff = bits(g) != bits(w)
    if diff.any():
        at = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.size} entries differ, first at {at}: {g[at]!r} vs {w[at]!r}")
