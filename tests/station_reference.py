"""Plain numpy restatement of the station search (include/geoac_stations.h), written from its definition - TEST-ONLY, nothing under geoac_amd/
imports it.

Given the records of a launch, its launch angles, its level table as fetched from the device (so that log10 differences stay out, as in the map
tests) and a spec it forms hits, rows and level of every (member, station) list with the device's operations in the device's order, in unfused
float64: the lists can be compared bit for bit.  Every product below is rounded before it is added (numpy never fuses)."""
import numpy as np

REC = dict(VALID=0, STEPS=1, BROKE=2, TTIME=3, ATTEN=4, TURN=5, INCL=6, BACKAZ=7, AMP=8, RANGE=9, JACOB=10, STATE=12)
STA = dict(LEG=0, TRI=1, RAY0=2, ORIENT=3, W0=4, W1=5, W2=6, THETA=7, PHI=8, TTIME=9, CELERITY=10, TURN=11, INCL=12, BACKAZ=13)
STA_STRIDE = 16
EQ_2D, EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP = 0, 1, 2, 3, 4
LEG_ALL = 2**31 - 1


def spec(n_theta, n_phi, phi_periodic=False, leg_min=0, leg_max=LEG_ALL, turn_tol=np.inf, edge_max=np.inf, cap=16):
    """the arguments of geoac_amd.station_spec as a plain dict"""
    return dict(n_theta=int(n_theta), n_phi=int(n_phi), phi_periodic=bool(phi_periodic), leg_min=int(leg_min), leg_max=int(leg_max),
                turn_tol=float(turn_tol), edge_max=float(edge_max), cap=int(cap))


def is_lattice(theta, phi, n_theta, n_phi):
    """the host check of geoac_fan_stations: every ray of row i the same theta, every ray of column j the same phi, bit for bit"""
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    if theta.size != n_theta * n_phi or phi.size != theta.size:
        return False
    t, p = theta.reshape(n_phi, n_theta).view(np.uint64), phi.reshape(n_phi, n_theta).view(np.uint64)
    return bool((t == t[:1]).all() and (p == p[:, :1]).all())


def triangles(sp):
    """ray indices [n_tri][3] of the lattice triangles in key order: triangle 2 * cell = (a, b, c), 2 * cell + 1 = (a, c, d)"""
    nt, nph = sp["n_theta"], sp["n_phi"]
    ncol = nph if sp["phi_periodic"] else nph - 1
    cell = np.arange((nt - 1) * ncol)
    i, j = cell % (nt - 1), cell // (nt - 1)
    jn = np.where(j + 1 == nph, 0, j + 1)
    a, d = j * nt + i, jn * nt + i
    b, c = a + 1, d + 1
    tri = np.empty((2 * cell.size, 3), dtype=np.int64)
    tri[0::2] = np.stack([a, b, c], axis=1)
    tri[1::2] = np.stack([a, c, d], axis=1)
    return tri


def landing(eqset, rec):
    """c0, c1 [M][n_rays][legs] in the map's coordinates"""
    S = REC["STATE"]
    if eqset in (EQ_GLOBAL, EQ_GLOBAL_RNGDEP):
        return rec[..., S + 1] * 180.0 / np.pi, rec[..., S + 2] * 180.0 / np.pi
    if eqset in (EQ_3D, EQ_3D_RNGDEP):
        return rec[..., S + 0], rec[..., S + 1]
    raise ValueError("the station search is not defined for the 2-D set")


def _wrap180(d):
    return d - 360.0 * np.floor((d + 180.0) / 360.0)


def _near(v0, vk):
    return v0 + _wrap180(vk - v0)


def _max(a, b):
    return np.where(a > b, a, b)


def _min(a, b):
    return np.where(a < b, a, b)


def _len2(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return dx * dx + dy * dy


def _interp(W, v0, v1, v2):
    return ((W[0] * v0) + (W[1] * v1)) + (W[2] * v2)


def hit_tests(eqset, c0, c1, turn, valid, tri, sta, sp):
    """one member, one leg: c0, c1, turn, valid [n_rays]; sta [B][2] -> hit [B][n_tri] bool, w [3][B][n_tri], s [B][n_tri]"""
    spherical = eqset in (EQ_GLOBAL, EQ_GLOBAL_RNGDEP)
    k0, k1, k2 = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (valid[k0] != 0.0) & (valid[k1] != 0.0) & (valid[k2] != 0.0)
        tmx = _max(_max(turn[k0], turn[k1]), turn[k2])
        tmn = _min(_min(turn[k0], turn[k1]), turn[k2])
        ok = ok & (tmx - tmn <= sp["turn_tol"])
        s0, s1 = sta[:, 0][:, None], sta[:, 1][:, None]
        x = [c0[k][None, :] - s0 for k in (k0, k1, k2)]
        y = [c1[k][None, :] - s1 for k in (k0, k1, k2)]
        if spherical:
            y = [_wrap180(v) for v in y]
        e2 = _max(_max(_len2(x[0], y[0], x[1], y[1]), _len2(x[1], y[1], x[2], y[2])), _len2(x[2], y[2], x[0], y[0]))
        ok = ok[None, :] & (e2 <= sp["edge_max"] * sp["edge_max"])
        w0 = x[1] * y[2] - y[1] * x[2]
        w1 = x[2] * y[0] - y[2] * x[0]
        w2 = x[0] * y[1] - y[0] * x[1]
        s = (w0 + w1) + w2
        hit = ok & (s != 0.0) & (((w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)) | ((w0 <= 0.0) & (w1 <= 0.0) & (w2 <= 0.0)))
    return hit, (w0, w1, w2), s


def reference_stations(eqset, rec, theta, phi, level, sp, sta, block=64):
    """hits [M][n_sta] u32, rows [M][n_sta][cap][16], level [M][n_sta][cap][F] of records rec [M][n_rays][legs][32], launch angles theta, phi
    [n_rays], level table [M][F][n_rays][legs] and stations sta [n_sta][2] under spec dict sp"""
    rec, level, sta = np.asarray(rec), np.asarray(level), np.ascontiguousarray(sta, dtype=np.float64)
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    M, n_rays, legs = rec.shape[:3]
    F = level.shape[1]
    assert level.shape == (M, F, n_rays, legs)
    assert is_lattice(theta, phi, sp["n_theta"], sp["n_phi"]), "the launch angles are not the lattice the spec names"
    R, cap = len(sta), sp["cap"]
    tri = triangles(sp)
    n_tri = len(tri)
    c0, c1 = landing(eqset, rec)
    hits = np.zeros((M, R), dtype=np.uint32)
    rows = np.zeros((M, R, cap, STA_STRIDE))
    lvl = np.zeros((M, R, cap, F))
    filled = np.zeros((M, R), dtype=np.int64)
    col = lambda name: rec[..., REC[name]]                                                      # noqa: E731
    for m in range(M):
        for leg in range(sp["leg_min"], min(sp["leg_max"], legs - 1) + 1):
            for lo in range(0, R, block):
                hit, w, s = hit_tests(eqset, c0[m, :, leg], c1[m, :, leg], col("TURN")[m, :, leg], col("VALID")[m, :, leg], tri, sta[lo:lo + block], sp)
                si, ti = np.nonzero(hit)                                                        # (row-major: per station ascending triangle = key order)
                for b in np.unique(si):
                    r = lo + int(b)
                    t = ti[si == b]
                    hits[m, r] += np.uint32(t.size)
                    t = t[:max(0, cap - int(filled[m, r]))]
                    if t.size == 0:
                        continue
                    at = slice(int(filled[m, r]), int(filled[m, r]) + t.size)
                    filled[m, r] += t.size
                    sv = s[b, t]
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        W = [w[k][b, t] / sv for k in range(3)]
                        r0, r1, r2 = tri[t, 0], tri[t, 1], tri[t, 2]
                        out = rows[m, r, at]
                        out[:, STA["LEG"]] = leg
                        out[:, STA["TRI"]] = t
                        out[:, STA["RAY0"]] = r0
                        out[:, STA["ORIENT"]] = np.where(sv > 0.0, 1.0, -1.0)
                        out[:, STA["W0"]], out[:, STA["W1"]], out[:, STA["W2"]] = W
                        out[:, STA["THETA"]] = _interp(W, theta[r0], theta[r1], theta[r2])
                        p0, p1, p2 = phi[r0], phi[r1], phi[r2]
                        if sp["phi_periodic"]:
                            p1, p2 = _near(p0, p1), _near(p0, p2)
                        out[:, STA["PHI"]] = _interp(W, p0, p1, p2)
                        g = lambda name: (col(name)[m, r0, leg], col(name)[m, r1, leg], col(name)[m, r2, leg])      # noqa: E731
                        tt = _interp(W, *g("TTIME"))
                        out[:, STA["TTIME"]] = tt
                        out[:, STA["CELERITY"]] = _interp(W, *g("RANGE")) / tt
                        out[:, STA["TURN"]] = _interp(W, *g("TURN"))
                        out[:, STA["INCL"]] = _interp(W, *g("INCL"))
                        b0, b1, b2 = g("BACKAZ")
                        out[:, STA["BACKAZ"]] = _interp(W, b0, _near(b0, b1), _near(b0, b2))
                        for f in range(F):
                            lvl[m, r, at, f] = _interp(W, level[m, f, r0, leg], level[m, f, r1, leg], level[m, f, r2, leg])
    return hits, rows, lvl


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def assert_lists_equal(got, want):
    """hits, rows and level bit for bit (floats compared as their bit patterns)"""
    for name, g, w in zip(("hits", "rows", "level"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        diff = bits(g) != bits(w)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} entries differ, first at {tuple(np.argwhere(diff)[0])}"


def landing_triangle(eqset, rec, sp, m, row, station):
    """corner offsets [3][2] of a row's landing triangle relative to its station (the device's x, y) and its longest side"""
    tri = triangles(sp)[int(row[STA["TRI"]])]
    leg = int(row[STA["LEG"]])
    c0, c1 = landing(eqset, rec[m:m + 1, tri, leg])
    x, y = c0[0] - station[0], c1[0] - station[1]
    if eqset in (EQ_GLOBAL, EQ_GLOBAL_RNGDEP):
        y = _wrap180(y)
    p = np.stack([x, y], axis=1)
    side = max(float(np.hypot(*(p[a] - p[b]))) for a, b in ((0, 1), (1, 2), (2, 0)))
    return p, side
