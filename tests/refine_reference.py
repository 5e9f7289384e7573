"""Plain numpy restatement of the station refinement (include/geoac_refine.h), written from its definition - TEST-ONLY, nothing under geoac_amd/
imports it.

Seeds, the step rule, the rows and the elementary functions of the header, operation for operation in unfused float64, given a callable that
integrates launch angles to records: a FanContext (the device's own launches: rows compare bit for bit) or the plain-C oracle (the CPU tests)."""
import numpy as np

from station_reference import REC, STA, EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP

RFN = dict(MEMBER=0, STATION=1, LEG=2, TRI=3, STATUS=4, ITER=5, THETA=6, PHI=7, MISS=8, TTIME=9, CELERITY=10, TURN=11, INCL=12, BACKAZ=13, AMP=14, JACOB=15)
RFN_STRIDE = 16
CONVERGED, ITER_LIMIT, STALLED, LOST, SINGULAR = 1, 2, 3, 4, 5
MAX_RAY_MEMBERS = 1 << 20
PI = 3.141592653589793238462643
S0 = REC["STATE"]


def spec(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2):
    return dict(max_iter=int(max_iter), max_shrink=int(max_shrink), tol=float(tol), step_max_deg=float(step_max_deg))


# ---- the header's elementary functions ----
def SIN(x):
    x = np.asarray(x, dtype=np.float64)
    x2 = x * x
    t, s = x.copy(), x.copy()
    for k in range(1, 15):
        t = -(t * x2) / float((2 * k) * (2 * k + 1))
        s = s + t
    return s


def COS(x):
    x = np.asarray(x, dtype=np.float64)
    x2 = x * x
    t, s = np.ones_like(x), np.ones_like(x)
    for k in range(1, 15):
        t = -(t * x2) / float((2 * k - 1) * (2 * k))
        s = s + t
    return s


def SINCOSD(a):
    a = np.asarray(a, dtype=np.float64)
    q = np.floor(a / 90.0 + 0.5)
    r = (a - 90.0 * q) * PI / 180.0
    n = q - 4.0 * np.floor(q / 4.0)
    s, c = SIN(r), COS(r)
    sn = np.where(n == 0.0, s, np.where(n == 1.0, c, np.where(n == 2.0, -s, -c)))
    cs = np.where(n == 0.0, c, np.where(n == 1.0, -s, np.where(n == 2.0, -c, s)))
    return sn, cs


def ASIN(s):
    s = np.asarray(s, dtype=np.float64)
    low = s <= 0.5
    u = np.where(low, s, np.sqrt((1.0 - s) / 2.0))
    x2 = u * u
    t, a = u.copy(), u.copy()
    for k in range(1, 31):
        t = ((t * x2) * float((2 * k - 1) * (2 * k - 1))) / float((2 * k) * (2 * k + 1))
        a = a + t
    return np.where(low, a, PI / 2.0 - 2.0 * a)


def WRAP(d):
    return d - 360.0 * np.floor((d + 180.0) / 360.0)


def DIST(lat1, lon1, lat2, lon2, R):
    a = SIN(((lat2 - lat1) * PI / 180.0) / 2.0)
    b = SIN((WRAP(lon2 - lon1) * PI / 180.0) / 2.0)
    h = a * a + (COS(lat1 * PI / 180.0) * COS(lat2 * PI / 180.0)) * (b * b)
    h = np.where(h > 1.0, 1.0, h)
    return (2.0 * R) * ASIN(np.sqrt(h))


def spherical(eqset):
    return eqset in (EQ_GLOBAL, EQ_GLOBAL_RNGDEP)


def seeds(hits, rows):
    """member, station, leg, tri [n] int and theta, phi [n] of the kept rows of station lists hits [M][R], rows [M][R][cap][16], in list order"""
    M, R, cap = rows.shape[:3]
    out = [(m, r, k) for m in range(M) for r in range(R) for k in range(min(int(hits[m, r]), cap))]
    if not out:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, np.zeros(0), np.zeros(0)
    m, r, k = (np.array(v, dtype=np.int64) for v in zip(*out))
    sel = rows[m, r, k]
    return m, r, sel[:, STA["LEG"]].astype(np.int64), sel[:, STA["TRI"]].astype(np.int64), sel[:, STA["THETA"]].copy(), sel[:, STA["PHI"]].copy()


def miss_of(eqset, R, s0, s1, rg):
    """miss [n] of records R [n][32] against stations (s0, s1) [n]"""
    S = R[:, S0:]
    with np.errstate(all="ignore"):
        if spherical(eqset):
            miss = DIST(S[:, 1] * 180.0 / PI, S[:, 2] * 180.0 / PI, s0, s1, rg)
        else:
            dx, dy = s0 - S[:, 0], s1 - S[:, 1]
            miss = np.sqrt(dx * dx + dy * dy)
    miss = np.where(miss == miss, miss, np.inf)
    return np.where(R[:, REC["VALID"]] == 0.0, np.inf, miss)


def newton(eqset, R, s0, s1, th, ph, mem, rg, step_max):
    """d_th, d_ph, ok [n]"""
    S = R[:, S0:]
    with np.errstate(all="ignore"):
        if spherical(eqset):
            e0 = s0 * PI / 180.0 - S[:, 1]
            e1 = WRAP(s1 - S[:, 2] * 180.0 / PI) * PI / 180.0
            q, qc = 1.0 / rg, 1.0 / (rg * COS(S[:, 1]))
            a00 = S[:, 7] - ((q * S[:, 4]) / S[:, 3]) * S[:, 6]
            a01 = S[:, 13] - ((q * S[:, 4]) / S[:, 3]) * S[:, 12]
            a10 = S[:, 8] - ((qc * S[:, 5]) / S[:, 3]) * S[:, 6]
            a11 = S[:, 14] - ((qc * S[:, 5]) / S[:, 3]) * S[:, 12]
        elif eqset == EQ_3D:
            e0, e1 = s0 - S[:, 0], s1 - S[:, 1]
            st, ct = SINCOSD(th)
            sp, cp = SINCOSD(90.0 - ph)
            n0, n1 = ct * cp, ct * sp
            m = 1.0 + (n0 * mem[:, 2] + n1 * mem[:, 3])
            g0, g1 = (n0 / m) / S[:, 3], (n1 / m) / S[:, 3]
            a00, a01 = S[:, 4] - g0 * S[:, 6], S[:, 8] - g0 * S[:, 10]
            a10, a11 = S[:, 5] - g1 * S[:, 6], S[:, 9] - g1 * S[:, 10]
        else:
            e0, e1 = s0 - S[:, 0], s1 - S[:, 1]
            g0, g1 = S[:, 3] / S[:, 5], S[:, 4] / S[:, 5]
            a00, a01 = S[:, 6] - g0 * S[:, 8], S[:, 12] - g0 * S[:, 14]
            a10, a11 = S[:, 7] - g1 * S[:, 8], S[:, 13] - g1 * S[:, 14]
        det = a00 * a11 - a01 * a10
        dlt = (((a11 * e0 - a01 * e1) / det) * 180.0) / PI
        dlp = (((a00 * e1 - a10 * e0) / det) * 180.0) / PI
    ok = (det != 0.0) & np.isfinite(det) & np.isfinite(dlt) & np.isfinite(dlp)
    dlt = np.where(dlt > step_max, step_max, dlt)
    dlt = np.where(dlt < -step_max, -step_max, dlt)
    dlp = np.where(dlp > step_max, step_max, dlp)
    dlp = np.where(dlp < -step_max, -step_max, dlp)
    return np.where(ok, dlt, 0.0), np.where(ok, -dlp, 0.0), ok


def members(eqset, sources, mach=None):
    """mem [M][4]: the members' source in the map's axes and (EQ_3D) u / c, v / c at the source; sources [M][3] in the layout of Params.src"""
    sources = np.atleast_2d(np.asarray(sources, dtype=np.float64))
    mem = np.zeros((len(sources), 4))
    mem[:, 0:2] = sources[:, 1:3] if spherical(eqset) else sources[:, 0:2]
    if mach is not None:
        mem[:, 2:4] = np.atleast_2d(mach)
    return mem


def start(n):
    """the running arrays of n seeds before their first round: b_th, b_ph, b_miss, d_th, d_ph, status, shrink, used"""
    return (np.zeros(n), np.zeros(n), np.full(n, np.inf), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64),
            np.zeros(n, dtype=np.int64))


def step_rule(sp, rnd, th, ph, miss, step, run):
    """the header's step rule after the launch of round rnd at trials (th, ph): miss [n] (inf: no record), step = (n_th, n_ph, ok) the Newton step
    of every seed, run the running arrays of start().  Returns the updated arrays and the next trials."""
    b_th, b_ph, b_miss, d_th, d_ph, status, shrink, used = run
    n_th, n_ph, ok = step
    act = status == 0
    used = np.where(act, rnd, used)
    conv = act & (miss <= sp["tol"])
    lost = act & ~conv & (rnd == 1) & (miss == np.inf)
    acc = act & ~conv & ~lost & ((rnd == 1) | (miss < b_miss))
    rej = act & ~conv & ~lost & ~acc
    take = conv | lost | acc
    b_th, b_ph = np.where(take, th, b_th), np.where(take, ph, b_ph)
    b_miss = np.where(conv | acc, miss, b_miss)
    d_th, d_ph = np.where(acc, n_th, d_th), np.where(acc, n_ph, d_ph)
    shrink = np.where(acc, 0, shrink)
    d_th, d_ph = np.where(rej, d_th / 2.0, d_th), np.where(rej, d_ph / 2.0, d_ph)
    shrink = np.where(rej, shrink + 1, shrink)
    status = np.where(conv, CONVERGED, status)
    status = np.where(lost, LOST, status)
    status = np.where(acc & ~ok, SINGULAR, status)
    status = np.where(rej & (shrink > sp["max_shrink"]), STALLED, status)
    live = status == 0
    return (b_th, b_ph, b_miss, d_th, d_ph, status, shrink, used), np.where(live, b_th + d_th, b_th), np.where(live, b_ph + d_ph, b_ph)


def tally(stats, status):
    """the statuses of finished seeds into the stats dict"""
    stats["converged"] = int((status == CONVERGED).sum())
    stats["stalled_or_limit"] = int(((status == STALLED) | (status == ITER_LIMIT)).sum())
    stats["lost_or_singular"] = int(((status == LOST) | (status == SINGULAR)).sum())
    return stats


def reference_refine(eqset, hits, rows, sta, sp, integrate, mem, r_earth=6370.0, z_grnd=0.0, level_of=None):
    """rows [n][16], level [n][F], stats dict and the final records of the refinement of station lists (hits, rows) at stations sta under spec dict sp.
    integrate(theta, phi) -> records [M][n][legs][32] of a launch of these angles; level_of() -> level table [M][F][n][legs] of the last launch
    (None: one frequency, formed here as 20 log10(AMP) - ATTEN, NaN where the leg is not VALID)"""
    sta = np.ascontiguousarray(sta, dtype=np.float64)
    M = rows.shape[0]
    sm, ss, sl, stri, th, ph = seeds(hits, rows)
    n = len(sm)
    assert n * M <= MAX_RAY_MEMBERS
    stats = dict(launches=0, ray_members=0, seeds=n, converged=0, stalled_or_limit=0, lost_or_singular=0)
    if n == 0:
        return np.zeros((0, RFN_STRIDE)), np.zeros((0, 1)), stats, None
    s0, s1 = sta[ss, 0], sta[ss, 1]
    rg = r_earth + z_grnd
    run = start(n)
    idx = np.arange(n)
    rec = None
    for rnd in range(1, sp["max_iter"] + 1):
        if not (run[5] == 0).any():
            break
        rec = np.asarray(integrate(th.copy(), ph.copy()))
        rec = rec.reshape((M, n) + rec.shape[-2:])
        stats["launches"] = rnd
        stats["ray_members"] += n * M
        R = rec[sm, idx, sl]
        run, th, ph = step_rule(sp, rnd, th, ph, miss_of(eqset, R, s0, s1, rg), newton(eqset, R, s0, s1, th, ph, mem[sm], rg, sp["step_max_deg"]), run)
    b_th, b_ph, b_miss, _, _, status, _, used = run
    status = np.where(status == 0, ITER_LIMIT, status)
    if level_of is None:
        with np.errstate(all="ignore"):
            level = (20.0 * np.log10(rec[..., REC["AMP"]]) - rec[..., REC["ATTEN"]])[:, None]
        level = np.where(rec[..., REC["VALID"]][:, None] != 0.0, level, np.nan)
    else:
        level = np.asarray(level_of())
    F = level.shape[1]
    out, lvl = np.zeros((n, RFN_STRIDE)), np.zeros((n, F))
    out[:, RFN["MEMBER"]], out[:, RFN["STATION"]], out[:, RFN["LEG"]], out[:, RFN["TRI"]] = sm, ss, sl, stri
    out[:, RFN["STATUS"]], out[:, RFN["ITER"]] = status, used
    out[:, RFN["THETA"]], out[:, RFN["PHI"]] = b_th, b_ph
    out[:, RFN["MISS"]] = np.where(status == LOST, -1.0, b_miss)
    c = status == CONVERGED
    R = rec[sm, idx, sl]
    with np.errstate(all="ignore"):
        rng = DIST(mem[sm, 0], mem[sm, 1], s0, s1, r_earth) if spherical(eqset) else np.sqrt(s0 * s0 + s1 * s1)
        cel = rng / R[:, REC["TTIME"]]
    for name, v in (("TTIME", R[:, REC["TTIME"]]), ("CELERITY", cel), ("TURN", R[:, REC["TURN"]]), ("INCL", R[:, REC["INCL"]]), ("BACKAZ", R[:, REC["BACKAZ"]]),
                    ("AMP", R[:, REC["AMP"]]), ("JACOB", R[:, REC["JACOB"]])):
        out[:, RFN[name]] = np.where(c, v, 0.0)
    for f in range(F):
        lvl[:, f] = np.where(c, level[sm, f, idx, sl], 0.0)
    return out, lvl, tally(stats, status), rec


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_equal_bits(got, want, names=("rows", "level")):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        diff = bits(g) != bits(w)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} entries differ, first at {tuple(np.argwhere(diff)[0])}: {g[tuple(np.argwhere(diff)[0])]!r} vs {w[tuple(np.argwhere(diff)[0])]!r}"
