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


# ---------------------------------------------------------------- every leg: k_levels restated, and the comparison with tests/golden/levels_legs.npz
LEGS_FIXTURE = os.path.join(GOLDEN_DIR, "levels_legs.npz")
LEGS_SETS = {"3d": EQ_3D, "global": EQ_GLOBAL, "3drd": EQ_3D_RNGDEP, "globalrd": EQ_GLOBAL_RNGDEP}
MUTATIONS = ("lat_dropped", "f_dropped", "leg_not_advanced", "pair_is_a_segment", "up_rule_swapped")


def restate_k_levels(eq, legs, z_km, cap, r_earth=R_EARTH, mutate=None):
    """k_levels for one ray, from its legs [(k, rows [k + 1][>= 3], sums [k + 1][2]), ...]: rows as the path chunk holds them, sums = the running
    travel time and attenuation at each row in the arrivals-only form (segments 0 .. m - 1 of the leg at row m, on top of the legs before).  Returns
    (count [L], lrec [L][cap][LVL_STRIDE]) in the library's layout: the count runs past cap, the first cap crossings are kept.

    The kernel's walk: every segment (i, i + 1) of the concatenated rows except the pair (a leg's last row, the next leg's first row); per segment the
    half-open rules for every level, FRAC = (lev - ha) / (hb - ha), component = pa + f (pb - pa), TTIME = (tt + ltt) + f c_tt with tt the sum at the leg's
    first row, ltt the leg's partial sum at row i and c_tt the segment's contribution - here T_i + f (T_{i+1} - T_i), which is the same number up to the
    rounding of the sums; the leg number goes up at a leg end.

    mutate: one of MUTATIONS, a deliberately wrong kernel (tests/test_levels_host.py proves that compare_with_fixture refuses each)."""
    assert mutate is None or mutate in MUTATIONS
    pw, hi = PATHW[eq], hidx(eq)
    lev = level_values(eq, z_km, r_earth)
    count = np.zeros(len(lev), dtype=np.int32)
    lrec = np.zeros((len(lev), cap, LVL_STRIDE))
    leg = 0
    prev = None                                                 # the leg before: its last row, last sums and last segment
    for k, rows, sums in legs:
        w = min(pw, rows.shape[1])
        rows, sums = rows[:, :w], np.asarray(sums)
        if prev is not None and mutate == "pair_is_a_segment":
            # (leg-end row -> this leg's first row) taken for a segment: the post-pass would price it as it prices its neighbour, by its length
            pa, pb, sa, sb = prev
            extra = (sb - sa) * (np.linalg.norm(rows[0, :3] - pb[:3]) / np.linalg.norm(pb[:3] - pa[:3]))
            rows, sums = np.vstack([pb[None, :], rows]), np.vstack([sums[:1], sums + extra])
        base = sums[0]                                          # tt, at: the sums at the leg's first row
        h = rows[:, hi]
        hits = []
        for l, z in enumerate(lev):
            up = ((h[:-1] <= z) & (z < h[1:])) if mutate == "up_rule_swapped" else ((h[:-1] < z) & (z <= h[1:]))
            down = (h[:-1] >= z) & (z > h[1:])
            hits += [(int(i), l, bool(up[i])) for i in np.flatnonzero(up | down)]
        for i, l, up in sorted(hits):                           # segment by segment, within a segment by level
            n = count[l]
            count[l] += 1
            if n >= cap:
                continue
            f = (lev[l] - h[i]) / (h[i + 1] - h[i])
            R = lrec[l, n]
            R[LVL["LEG"]], R[LVL["DIR"]], R[LVL["FRAC"]] = leg, 1.0 if up else -1.0, f
            R[LVL["TTIME"]] = sums[i, 0] + (1.0 if mutate == "f_dropped" else f) * (sums[i + 1, 0] - sums[i, 0])
            R[LVL["ATTEN"]] = (base[1] if mutate == "lat_dropped" else sums[i, 1]) + f * (sums[i + 1, 1] - sums[i, 1])
            R[LVL["P0"]:LVL["P0"] + w] = rows[i] + f * (rows[i + 1] - rows[i])
        prev = (rows[-2], rows[-1], sums[-2], sums[-1])
        if mutate != "leg_not_advanced":
            leg += 1
    return count, lrec


def restate_fan(eq, paths, z_km, cap, r_earth=R_EARTH, mutate=None):
    """restate_k_levels for every ray of a fan: (count [n_rays][L], lrec [n_rays][L][cap][LVL_STRIDE])"""
    out = [restate_k_levels(eq, legs, z_km, cap, r_earth, mutate) for legs in paths]
    return np.stack([c for c, _ in out]), np.stack([r for _, r in out])


def compare_with_fixture(eq, count, lrec, fixture, name=None, rtol=1e-6):
    """crossing records count [n_rays][L], lrec [n_rays][L][cap][LVL_STRIDE] of the fixture's fan against the crossings of the compiled reference's own
    rows and running sums (tests/golden/levels_legs.npz; name: the fixture's set, the equation set's own by default).  Exact: the count of every
    (ray, level), and LEG and DIR of every crossing in path order - so the count per (ray, level, leg) too.  Within rtol = 1e-6 relative, the project's
    rule for values against the reference (tests/parity.py): TTIME and ATTEN; the position (position_errors); the components P0 + 3 .. of the
    interpolated row, each as parity.py judges a state component (|got - want| / max(|want|, 1e-6 x the column's largest |want|)); FRAC, by the
    distance that its error moves the crossing along its segment, measured as position_errors measures a position.  Prints and returns the worst
    error per column; raises AssertionError on the first rule broken."""
    name = name or {v: k for k, v in LEGS_SETS.items()}[eq]
    g, pw, P0 = fixture, PATHW[eq], LVL["P0"]
    n_rays, L = count.shape
    assert (n_rays, L) == (len(g[f"{name}_theta"]), len(g[f"{name}_levels"])) and lrec.shape[:2] == (n_rays, L), (count.shape, lrec.shape)
    cap = lrec.shape[2]
    assert count.max() <= cap, (name, "raise cap: a count beyond it leaves crossings unseen")
    by = fixture_rays(g, name)
    got = np.zeros((len(g[f"{name}_ray"]), LVL_STRIDE))
    for r in range(n_rays):
        for l in range(L):
            idx = by.get((r, l), [])
            assert count[r, l] == len(idx), (name, "count", r, l, int(count[r, l]), len(idx))
            got[idx] = lrec[r, l, :len(idx)]
            assert (lrec[r, l, len(idx):] == 0.0).all(), (name, "slots past the count are not zero", r, l)
    assert np.array_equal(got[:, LVL["LEG"]], g[f"{name}_leg"].astype(np.float64)), (name, "LEG")
    assert np.array_equal(got[:, LVL["DIR"]], g[f"{name}_dir"].astype(np.float64)), (name, "DIR")
    want, dab = g[f"{name}_row"], np.abs(g[f"{name}_dab"].astype(np.float64))
    err = {}
    df = np.abs(got[:, LVL["FRAC"]] - g[f"{name}_frac"])
    if eq in SPHERICAL:
        floor = 1e-6 * np.abs(want[:, :3]).max(axis=0, keepdims=True)
        err["FRAC"] = (df[:, None] * dab / np.maximum(np.abs(want[:, :3]), floor)).max(axis=1)
    else:
        err["FRAC"] = df * np.linalg.norm(dab, axis=1) / np.linalg.norm(want[:, :3], axis=1)
    err["P0..2"] = position_errors(eq, got[:, P0:P0 + 3], want)
    floor = 1e-6 * np.abs(want[:, 3:pw]).max(axis=0, keepdims=True)
    err["P3.."] = (np.abs(got[:, P0 + 3:P0 + pw] - want[:, 3:pw]) / np.maximum(np.abs(want[:, 3:pw]), floor)).max(axis=1)
    assert (got[:, P0 + pw:] == 0.0).all(), (name, "columns past the path width are not zero")
    for col in ("TTIME", "ATTEN"):
        w = g[f"{name}_{col.lower()}"]
        err[col] = np.abs(got[:, LVL[col]] - w) / np.abs(w)
    worst = {k: float(v.max()) for k, v in err.items()}
    print(f"{name}: {len(got)} crossings ({int((g[f'{name}_leg'] >= 1).sum())} behind a bounce) against the reference's rows and sums, worst error "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in err.items():
        j = int(np.argmax(v))
        assert v[j] <= rtol, (name, k, float(v[j]), "ray", int(g[f"{name}_ray"][j]), "level", int(g[f"{name}_level"][j]), "leg", int(g[f"{name}_leg"][j]))
    return worst


# ---------------------------------------------------------------- the same launch's path, from sample capture at stride 1
REC_STEPS, REC_BROKE, REC_TTIME, REC_ATTEN, REC_STATE = 1, 2, 3, 4, 12      # include/geoac_hip.h


def rows_from_samples(eq, smp, rec, src, params, rec_arrivals):
    """every leg's rows and running sums of every ray of a fan, rebuilt from a run with mode = MODE_WRITE_RAYS and sample_stride = 1 (smp: fetch_samples(),
    rec: its records) and from the records rec_arrivals of the same fan run without sample capture.  src: the source as set_params takes it, params:
    dict(z_grnd=, r_earth=).  Returns (paths, n_rows): paths[ray] = [(k, rows [.][3], sums [.][2]), ...] for restate_k_levels, in the units of the path chunk
    (spherical sets: r = r_earth + the sample's height, an exact inverse of the sample's r - r_earth for r_earth = 6370 and r below 8192 km, both being
    multiples of 2^-40; latitude and longitude back from degrees, within 4 roundings); n_rows[ray] = the rows of the ray.

    Row m = 1 .. k - 1 of a leg: the sample (ray, leg, m) - asserted to be there, exactly once each.  Row k: GEOAC_REC_STATE of the leg's record.  A leg that
    ended by the break check has no record of its last row: its rows stop at k - 1 and its last segment is not restated - a crossing in it would show as a
    count one short.  Row 0 of leg 0: the source, (x, y, max(z, z_grnd)) or (r_earth + max(z, z_grnd), lat pi / 180, lon pi / 180), the operations of the
    kernels' start.  Row 0 of a later leg is what EQ::reflect leaves (geoac_kernels.hip): the height component is set to the ground's, z_grnd or
    r_earth + z_grnd, exactly; the horizontal ones are rows k - 1, k (and k - 2, Cartesian sets) of the leg before extrapolated back to the ground, which is
    not re-done here - they are taken from row k, and the caller asserts that row 1 lies below the lowest level, so that no crossing lies in the segment
    (0, 1) and they enter no record.

    Sums: the sample rows' are in the sample-capture form of quirk Q7, every finished leg lacking its last segment; the arrivals-only form at row m of leg j
    is the sample's plus D_{j-1}, D_j = rec_arrivals TTIME[j] - rec TTIME[j] (ATTEN alike; D_{-1} = 0).  Row 0 of leg j carries rec_arrivals' sums of leg
    j - 1, row k those of leg j."""
    sph = eq in SPHERICAL
    zg, re = float(params.get("z_grnd", 0.0)), float(params.get("r_earth", R_EARTH))
    smp = smp[smp[:, 3] == 0.0]
    n_rays, legs = rec.shape[0], rec.shape[1]
    order = np.lexsort((smp[:, 2], smp[:, 1], smp[:, 0]))
    smp = smp[order]
    key = smp[:, 0].astype(np.int64) * legs + smp[:, 1].astype(np.int64)
    first = np.searchsorted(key, np.arange(n_rays * legs + 1))

    def units(v):
        v = np.array(v, dtype=np.float64)
        if sph:
            v[..., 0] = v[..., 0] + re
            v[..., 1:3] = v[..., 1:3] * np.pi / 180.0
        return v
    if sph:
        z_src = max(float(src[0]), zg)
        source = np.array([re + z_src, float(src[1]) * np.pi / 180.0, float(src[2]) * np.pi / 180.0])
        ground = re + zg
    else:
        source = np.array([float(src[0]), float(src[1]), max(float(src[2]), zg)])
        ground = zg
    hi = hidx(eq)
    paths, n_rows = [], []
    for r in range(n_rays):
        out, carry, total, row0 = [], np.zeros(2), 0, source
        for j in range(legs):
            k = int(rec[r, j, REC_STEPS])
            if k == 0:
                break
            mine = smp[first[r * legs + j]:first[r * legs + j + 1]]
            assert np.array_equal(mine[:, 2], np.arange(1, k, dtype=np.float64)), (r, j, k, len(mine), "raypath rows 1 .. k - 1, once each")
            broke = rec[r, j, REC_BROKE] > 0
            D = (rec_arrivals[r, j - 1, [REC_TTIME, REC_ATTEN]] - rec[r, j - 1, [REC_TTIME, REC_ATTEN]]) if j else np.zeros(2)
            rows = [row0[None, :], units(mine[:, 4:7])]
            sums = [carry[None, :], np.stack([mine[:, 9], -mine[:, 8]], axis=1) + D[None, :]]
            end = rec_arrivals[r, j, [REC_TTIME, REC_ATTEN]]
            if not broke:
                rows.append(rec[r, j, REC_STATE:REC_STATE + 3][None, :])
                sums.append(end[None, :])
            rows, sums = np.vstack(rows), np.vstack(sums)
            out.append((-k if broke else k, rows, sums))
            total += k + 1
            carry = end
            row0 = rows[-1].copy()
            row0[hi] = ground
        paths.append(out)
        n_rows.append(total)
    return paths, np.array(n_rows)
