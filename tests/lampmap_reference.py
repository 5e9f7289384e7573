"""Plain numpy restatement of the level loudness map (include/geoac_lampmap.h), written from its definition - TEST-ONLY, nothing under geoac_amd/
imports it.

A hit of the map is a row of the level-station search at a cell centre (tests/ltubemap_reference.py, tests/lstation_reference.py); its crossing and
launch-angle areas come from the branch table's corners, steps 3 to 5 of the amplitude are tube() of tests/level_amp_reference.py, the elementary
functions are those of tests/refine_reference.py - all imported, none edited.  EXP is restated here.  Crossing tables come from a FanContext's
fetch_levels(), from the restated k_levels of the oracle's paths, or are synthetic; the medium is a list of callables, one per profile, as
level_amp_reference.reference_rows takes one."""
import numpy as np

import level_amp_reference as LA
import lstation_reference as LS
import ltubemap_reference as LT
import map_reference as MR
import station_reference as SR
from levels_reference import LVL_STRIDE
from refine_reference import COS, WRAP, PI, spherical

S = LS.LSTA
P0 = LS.P0
LAYERS = ("count", "weak", "amp_max", "ramp_max", "loudest", "detect")
LN10 = 2.302585092994045684
LN2, LN2_HI, LN2_LO = 0.693147180559945309417, 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_TERMS, EXP_CUT = 14, -700.0


def EXP(x):
    """the series of the header, operation for operation: NaN -> NaN, x < -700 -> 0, x > 700 -> +inf"""
    x = np.asarray(x, dtype=np.float64)
    inside = np.where(np.isfinite(x) & (x >= EXP_CUT) & (x <= -EXP_CUT), x, 0.0)
    q = np.floor(inside / LN2 + 0.5)
    r = (inside - q * LN2_HI) - q * LN2_LO
    s = np.ones_like(inside)
    for k in range(EXP_TERMS, 0, -1):
        s = 1.0 + (r * s) / float(k)
    out = s * np.ldexp(1.0, q.astype(np.int64))
    with np.errstate(invalid="ignore"):
        out = np.where(x < EXP_CUT, 0.0, np.where(x > -EXP_CUT, np.inf, out))
    return np.where(np.isnan(x), x, out)


def spec(det_floor=0.0, detect_amp=float("nan"), **kw):
    """the arguments of geoac_amd.lampmap_spec as a plain dict"""
    return dict(LT.spec(**kw), det_floor=float(det_floor), detect_amp=float(detect_amp))


def ltube_spec_of(sp):
    return {k: v for k, v in sp.items() if k not in ("det_floor", "detect_amp")}


def hits_of_lists(eqset, hits, rows, count, lrec, theta, phi, legs, sp, z_km, media, src3, z_grnd=0.0, r_earth=6370.0):
    """every hit of the map from level-station lists at LT.stations_of(sp) (cap = LT.CAP): a dict of arrays [n] - member, selected level ls, cell, key
    b * n_tri + tri, DET, TZ, D, AMP, RAMP, TTIME, ATTEN, usable.  media: one callable medium(hc, a, b) -> (c, u, v, rho) per profile, member m
    reads media[m % len(media)]; src3 [M][3] in the layout of Params.src."""
    count, lrec = np.asarray(count), np.asarray(lrec)
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    z_km = np.asarray(z_km, dtype=np.float64)
    n0, n1 = sp["n"]
    cells, sel = n0 * n1, np.asarray(LT.selected(sp))
    M, R = hits.shape
    K = len(media)
    assert R == len(sel) * cells and rows.shape == (M, R, LT.CAP, LS.LSTA_STRIDE) and lrec.shape[-1] == LVL_STRIDE
    assert int(hits.max(initial=0)) <= LT.CAP, f"a cell centre has {int(hits.max())} hits: the lists are truncated at {LT.CAP}"
    lsp = LT.lstation_spec_of(sp)
    tri = SR.triangles(lsp)
    n_tri = len(tri)
    c0, c1, slot, present = LS.branch_table(eqset, count, lrec, lsp, legs)
    down = rows[..., S["DIR"]] < 0.0
    wanted = np.where(down, bool(sp["dir_mask"] & 2), bool(sp["dir_mask"] & 1))
    keep = (np.arange(LT.CAP)[None, None, :] < hits[..., None]) & wanted
    m, r, q = np.nonzero(keep)
    row = rows[m, r, q]
    ls, cell = r // cells, r % cells
    l = sel[ls]
    b = (((row[:, S["LEG"]] - sp["leg_min"]) * 2 + (row[:, S["DIR"]] < 0.0)) * sp["ord_max"] + row[:, S["ORD"]]).astype(np.int64)
    t = row[:, S["TRI"]].astype(np.int64)
    corners = tri[t]                                                                   # [n][3] rays, corner order 0, 1, 2
    cx, cy = c0[m[:, None], l[:, None], b[:, None], corners], c1[m[:, None], l[:, None], b[:, None], corners]
    assert present[m[:, None], l[:, None], b[:, None], corners].all()
    cen = LT.centres(sp)[cell]
    with np.errstate(all="ignore"):
        # 1. the crossing area, 2. the launch-angle area
        ex1, ex2 = cx[:, 1] - cx[:, 0], cx[:, 2] - cx[:, 0]
        ey1, ey2 = cy[:, 1] - cy[:, 0], cy[:, 2] - cy[:, 0]
        if spherical(eqset):
            ey1, ey2 = WRAP(ey1), WRAP(ey2)
        AX = ex1 * ey2 - ex2 * ey1
        th, ph = theta[corners], phi[corners]
        at1, at2 = th[:, 1] - th[:, 0], th[:, 2] - th[:, 0]
        ap1, ap2 = WRAP(ph[:, 1] - ph[:, 0]), WRAP(ph[:, 2] - ph[:, 0])
        AA = at1 * ap2 - at2 * ap1
        det = AX / AA
        # 3. the row's own values
        THETA, PHI, tt, at = row[:, S["THETA"]], row[:, S["PHI"]], row[:, S["TTIME"]], row[:, S["ATTEN"]]
        fake = np.zeros((len(m), LVL_STRIDE))
        fake[:, P0 + 3:P0 + 6] = row[:, S["N0"]:S["N0"] + 3]
        # 4. the medium, profile by profile
        zl = z_km[l]
        hc = r_earth + zl if spherical(eqset) else zl
        med, src = np.zeros((4, len(m))), np.zeros((4, len(m)))
        shc, sa, sb = LA.source_points(eqset, src3, z_grnd, r_earth)
        assert len(shc) == M
        for k in range(K):
            on = np.flatnonzero(m % K == k)
            if on.size == 0:
                continue
            med[:, on] = np.stack(media[k](hc[on], cen[on, 0], cen[on, 1]))
            src[:, on] = np.stack(media[k](shc, sa, sb))[:, m[on]]
        # 5. steps 3 to 5 of geoac_level_amp.h: TZ and the factors of num and den from tube(), D and AMP with this DET and the centre's latitude
        _, tz, _, _, num, den0 = LA.tube(eqset, fake, fake, fake, THETA, PHI, 1.0, hc, tuple(med), tuple(src), parts=True)
        if spherical(eqset):
            D = hc * hc * COS(cen[:, 0] * PI / 180.0) * np.abs(tz * det)
        else:
            D = np.abs(tz * det) * (180.0 / PI) * (180.0 / PI)
        amp = 1.0 / (4.0 * PI) * np.sqrt(np.abs(num / (den0 * D)))
        # 6. the received amplitude
        ramp = amp * EXP(-(at * (LN10 / 20.0)))
        fin = np.isfinite
        usable = (AA != 0.0) & (np.abs(det) > sp["det_floor"]) & fin(det) & (det != 0.0) & fin(D) & (D != 0.0) & fin(amp) & (amp != 0.0) & fin(tt) & fin(at) & fin(ramp)
    return dict(member=m, ls=ls, cell=cell, key=b * n_tri + t, det=det, tz=tz, D=D, amp=amp, ramp=ramp, ttime=tt, atten=at, usable=usable, theta=THETA, phi=PHI,
                row=row, shape=(M, len(sel), n0, n1))


def reduce_hits(h, sp):
    """the layers of the hits of hits_of_lists"""
    shape = h["shape"]
    W = int(np.prod(shape))
    word = (h["member"] * shape[1] + h["ls"]) * (shape[2] * shape[3]) + h["cell"]
    u = h["usable"]
    count, weak = np.zeros(W, dtype=np.uint64), np.zeros(W, dtype=np.uint64)
    np.add.at(count, word[u], np.uint64(1))
    np.add.at(weak, word[~u], np.uint64(1))
    kamp, kramp = np.zeros(W, dtype=np.uint64), np.zeros(W, dtype=np.uint64)
    np.maximum.at(kamp, word[u], MR.key(h["amp"][u]))
    np.maximum.at(kramp, word[u], MR.key(h["ramp"][u]))
    loud = np.full(W, np.iinfo(np.int64).max)
    holder = u & (MR.key(h["ramp"]) == kramp[word])
    np.minimum.at(loud, word[holder], h["key"][holder])
    some = count > 0
    out = dict(count=count.reshape(shape), weak=weak.reshape(shape),
               amp_max=np.where(some, MR.unkey(np.where(some, kamp, MR.key(np.zeros(W)))), -np.inf).reshape(shape),
               ramp_max=np.where(some, MR.unkey(np.where(some, kramp, MR.key(np.zeros(W)))), -np.inf).reshape(shape),
               loudest=np.where(some, loud, -1).astype(np.int64).reshape(shape))
    out["detect"] = None if np.isnan(sp["detect_amp"]) else (out["ramp_max"] >= sp["detect_amp"]).sum(axis=0).astype(np.uint32)
    return out


def reduce_lists(eqset, hits, rows, count, lrec, theta, phi, legs, sp, z_km, media, src3, **kw):
    return reduce_hits(hits_of_lists(eqset, hits, rows, count, lrec, theta, phi, legs, sp, z_km, media, src3, **kw), sp)


def reference_level_ampmap(eqset, count, lrec, theta, phi, legs, sp, z_km, media, src3, hits_too=False, **kw):
    """the loudness map of crossing counts [M][n_rays][L] and records [M][n_rays][L][capL][12], launch angles theta, phi [n_rays] and the launch's
    number of legs under spec dict sp; z_km the launch's level list"""
    sta, level_of = LT.stations_of(sp)
    assert max(LT.selected(sp)) < np.asarray(count).shape[2] and sp["level_mask"] > 0
    hits, rows = LS.reference_level_stations(eqset, count, lrec, theta, phi, legs, LT.lstation_spec_of(sp), sta, level_of)
    h = hits_of_lists(eqset, hits, rows, count, lrec, theta, phi, legs, sp, z_km, media, src3, **kw)
    out = reduce_hits(h, sp)
    return (out, h) if hits_too else out


def media_of_contexts(ctxs):
    """one medium callable per profile from FanContexts after a launch (the public probe calls: the bits the device layers are made of)"""
    return [LA.medium_of_context(c) for c in ctxs]


def assert_layers_equal(got, want, what=""):
    """every layer bit for bit (floats compared as their bit patterns)"""
    assert set(got) == set(want) == set(LAYERS), (what, sorted(got), sorted(want))
    for name in LAYERS:
        g, w = got[name], want[name]
        if g is None or w is None:
            assert g is None and w is None, (what, name)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = SR.bits(g) != SR.bits(w)
        if diff.any():
            at = tuple(np.argwhere(diff)[0])
            raise AssertionError(f"{what} {name}: {int(diff.sum())} of {diff.size} cells differ, first at {at}: {g[at]!r} vs {w[at]!r}")
