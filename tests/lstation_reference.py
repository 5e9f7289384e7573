"""Plain numpy restatement of the level-station search (include/geoac_lstations.h), written from its definition - TEST-ONLY, nothing under
geoac_amd/ imports it.

Given the crossing records and counts of a launch as fetched from the device (geoac_fan_fetch_levels), its launch angles and a spec it forms the
branch table, the hits and the rows of every (member, station) list with the device's operations in the device's order, in unfused float64: the
lists can be compared bit for bit.  Triangles, the lattice check and the hit rule are those of tests/station_reference.py, imported and not
edited: a branch-table plane is handed to its hit_tests as a landing table whose `valid` is the plane's `present` and whose turning heights are
all zero under turn_tol = +inf, which is the ground rule minus its two filters."""
import numpy as np

import station_reference as SR
from levels_reference import LVL, LVL_STRIDE

LSTA = dict(LEG=0, DIR=1, ORD=2, TRI=3, RAY0=4, ORIENT=5, W0=6, W1=7, W2=8, THETA=9, PHI=10, TTIME=11, ATTEN=12, N0=13)
LSTA_STRIDE = 16
LEG_ALL = SR.LEG_ALL
P0 = LVL["P0"]


def spec(n_theta, n_phi, phi_periodic=False, leg_min=0, leg_max=LEG_ALL, ord_max=1, edge_max=np.inf, cap=16):
    """the arguments of geoac_amd.lstation_spec as a plain dict"""
    return dict(n_theta=int(n_theta), n_phi=int(n_phi), phi_periodic=bool(phi_periodic), leg_min=int(leg_min), leg_max=int(leg_max),
                ord_max=int(ord_max), edge_max=float(edge_max), cap=int(cap))


def extent(sp, legs):
    """leg0, n_legs of a spec on a launch of `legs` legs (geoac_lattice_extent)"""
    last = min(sp["leg_max"], legs - 1)
    return sp["leg_min"], (last - sp["leg_min"] + 1 if last >= sp["leg_min"] else 0)


def crossing_points(eqset, lrec):
    """c0, c1 of crossing records [...][12] in the map's coordinates"""
    if eqset in (SR.EQ_GLOBAL, SR.EQ_GLOBAL_RNGDEP):
        return lrec[..., P0 + 1] * 180.0 / np.pi, lrec[..., P0 + 2] * 180.0 / np.pi
    if eqset in (SR.EQ_3D, SR.EQ_3D_RNGDEP):
        return lrec[..., P0 + 0], lrec[..., P0 + 1]
    raise ValueError("the level-station search is not defined for the 2-D set")


def branch_table(eqset, count, lrec, sp, legs):
    """count [M][n_rays][L], lrec [M][n_rays][L][capL][12] -> c0, c1 [M][L][B][n_rays] float64, slot [M][L][B][n_rays] int64, present the same
    shape, bool: the kept crossings of every (member, ray, level) walked once in path order with two ordinal counters that reset when the leg changes"""
    M, n_rays, L, capL = lrec.shape[:4]
    leg0, n_legs = extent(sp, legs)
    om = sp["ord_max"]
    B = n_legs * 2 * om
    c0, c1 = np.zeros((M, L, B, n_rays)), np.zeros((M, L, B, n_rays))
    slot, present = np.zeros((M, L, B, n_rays), dtype=np.int64), np.zeros((M, L, B, n_rays), dtype=bool)
    p0, p1 = crossing_points(eqset, lrec)
    for m in range(M):
        for ray in range(n_rays):
            for l in range(L):
                leg_now, o = -1, [0, 0]
                for k in range(min(int(count[m, ray, l]), capL)):
                    leg = int(lrec[m, ray, l, k, LVL["LEG"]])
                    if leg != leg_now:
                        leg_now, o = leg, [0, 0]
                    d = 0 if lrec[m, ray, l, k, LVL["DIR"]] > 0.0 else 1
                    ordinal = o[d]
                    o[d] += 1
                    li = leg - leg0
                    if li < 0 or li >= n_legs or ordinal >= om:
                        continue
                    b = (li * 2 + d) * om + ordinal
                    c0[m, l, b, ray], c1[m, l, b, ray] = p0[m, ray, l, k], p1[m, ray, l, k]
                    slot[m, l, b, ray], present[m, l, b, ray] = k, True
    return c0, c1, slot, present


def reference_level_stations(eqset, count, lrec, theta, phi, legs, sp, sta, level_of, block=64):
    """hits [M][n_sta] u32 and rows [M][n_sta][cap][16] of crossing counts [M][n_rays][L] and records [M][n_rays][L][capL][12], launch angles theta,
    phi [n_rays], the launch's number of legs, stations sta [n_sta][2] on the levels level_of [n_sta] under spec dict sp"""
    count, lrec = np.asarray(count), np.asarray(lrec)
    sta, level_of = np.ascontiguousarray(sta, dtype=np.float64), np.asarray(level_of, dtype=np.int64)
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    M, n_rays, L, capL = lrec.shape[:4]
    assert lrec.shape[4] == LVL_STRIDE and count.shape == (M, n_rays, L)
    assert SR.is_lattice(theta, phi, sp["n_theta"], sp["n_phi"]), "the launch angles are not the lattice the spec names"
    assert len(level_of) == len(sta) and (level_of >= 0).all() and (level_of < L).all()
    R, cap, om = len(sta), sp["cap"], sp["ord_max"]
    leg0, n_legs = extent(sp, legs)
    B = n_legs * 2 * om
    tri = SR.triangles(sp)
    c0, c1, slot, present = branch_table(eqset, count, lrec, sp, legs)
    ground = dict(turn_tol=np.inf, edge_max=sp["edge_max"])
    hits = np.zeros((M, R), dtype=np.uint32)
    rows = np.zeros((M, R, cap, LSTA_STRIDE))
    filled = np.zeros((M, R), dtype=np.int64)
    zero = np.zeros(n_rays)
    for m in range(M):
        for b in range(B):                                                                       # (ascending b, then ascending triangle: key order)
            for l in np.unique(level_of):
                on = np.flatnonzero(level_of == l)
                if not present[m, l, b].any():
                    continue
                for lo in range(0, len(on), block):
                    idx = on[lo:lo + block]
                    hit, w, s = SR.hit_tests(eqset, c0[m, l, b], c1[m, l, b], zero, present[m, l, b].astype(np.float64), tri, sta[idx], ground)
                    si, ti = np.nonzero(hit)
                    for q in np.unique(si):
                        r = int(idx[q])
                        t = ti[si == q]
                        hits[m, r] += np.uint32(t.size)
                        t = t[:max(0, cap - int(filled[m, r]))]
                        if t.size == 0:
                            continue
                        at = slice(int(filled[m, r]), int(filled[m, r]) + t.size)
                        filled[m, r] += t.size
                        sv = s[q, t]
                        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                            W = [w[k][q, t] / sv for k in range(3)]
                            r0, r1, r2 = tri[t, 0], tri[t, 1], tri[t, 2]
                            R0, R1, R2 = (lrec[m, rk, l, slot[m, l, b, rk]] for rk in (r0, r1, r2))
                            out = rows[m, r, at]
                            out[:, LSTA["LEG"]] = leg0 + (b // om) // 2
                            out[:, LSTA["DIR"]] = -1.0 if (b // om) % 2 else 1.0
                            out[:, LSTA["ORD"]] = b % om
                            out[:, LSTA["TRI"]] = t
                            out[:, LSTA["RAY0"]] = r0
                            out[:, LSTA["ORIENT"]] = np.where(sv > 0.0, 1.0, -1.0)
                            out[:, LSTA["W0"]], out[:, LSTA["W1"]], out[:, LSTA["W2"]] = W
                            out[:, LSTA["THETA"]] = SR._interp(W, theta[r0], theta[r1], theta[r2])
                            p0, p1, p2 = phi[r0], phi[r1], phi[r2]
                            if sp["phi_periodic"]:
                                p1, p2 = SR._near(p0, p1), SR._near(p0, p2)
                            out[:, LSTA["PHI"]] = SR._interp(W, p0, p1, p2)
                            for name, col in (("TTIME", LVL["TTIME"]), ("ATTEN", LVL["ATTEN"])):
                                out[:, LSTA[name]] = SR._interp(W, R0[:, col], R1[:, col], R2[:, col])
                            for q3 in range(3):
                                out[:, LSTA["N0"] + q3] = SR._interp(W, R0[:, P0 + 3 + q3], R1[:, P0 + 3 + q3], R2[:, P0 + 3 + q3])
    # the rows were appended station by station within a (member, branch): across levels nothing interleaves, a station has one level
    return hits, rows


def assert_lists_equal(got, want):
    """hits and rows bit for bit (floats compared as their uint64 views)"""
    for name, g, w in zip(("hits", "rows"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        diff = SR.bits(g) != SR.bits(w)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} entries differ, first at {tuple(np.argwhere(diff)[0])}"


def crossing_triangle(eqset, count, lrec, legs, sp, m, row, station, level):
    """corner offsets [3][2] of a row's crossing triangle relative to its station (the device's x, y), its longest side, and the corners' records [3][12]"""
    leg0, _ = extent(sp, legs)
    om = sp["ord_max"]
    b = ((int(row[LSTA["LEG"]]) - leg0) * 2 + (0 if row[LSTA["DIR"]] > 0 else 1)) * om + int(row[LSTA["ORD"]])
    tri = SR.triangles(sp)[int(row[LSTA["TRI"]])]
    c0, c1, slot, present = branch_table(eqset, count[m:m + 1, tri], lrec[m:m + 1, tri], sp, legs)
    assert present[0, level, b].all()
    x, y = c0[0, level, b] - station[0], c1[0, level, b] - station[1]
    if eqset in (SR.EQ_GLOBAL, SR.EQ_GLOBAL_RNGDEP):
        y = SR._wrap180(y)
    p = np.stack([x, y], axis=1)
    side = max(float(np.hypot(*(p[a] - p[c]))) for a, c in ((0, 1), (1, 2), (2, 0)))
    recs = np.stack([lrec[m, tri[k], level, slot[0, level, b, k]] for k in range(3)])
    return p, side, recs


def branch_of_ray(count_rl, lrec_rl, leg, direction, ordinal):
    """slot k of the (leg, direction, ordinal) passage among one (ray, level)'s kept crossings, or -1"""
    seen = 0
    for k in range(min(int(count_rl), lrec_rl.shape[0])):
        if int(lrec_rl[k, LVL["LEG"]]) == leg and (lrec_rl[k, LVL["DIR"]] > 0) == (direction > 0):
            if seen == ordinal:
                return k
            seen += 1
    return -1
