"""Plain numpy restatement of the level tube map (include/geoac_ltubemap.h), built on the level-station restatement (tests/lstation_reference.py,
imported, not copied) - TEST-ONLY, nothing under geoac_amd/ imports it.

The header defines a level tube map as what the level-station search returns with one station per cell centre and selected level, reduced:
stations at the centres, lists at cap = 256, rows filtered by their direction, reduction to the layers with the keys of the arrival map
(tests/map_reference.py).  reduce_lists() does the last two steps for any level-station lists - the restatement's or the device's own
(FanContext.level_stations) - so both can be compared bit for bit with FanContext.level_tubemap."""
import numpy as np

import lstation_reference as LS
import map_reference as MR
import station_reference as SR

S = LS.LSTA
CAP = 256                                   # GEOAC_STA_MAX_CAP: the lists the reduction is taken from hold every hit only while hits <= CAP
LEG_ALL = LS.LEG_ALL
LAYERS = ("count", "ttime_min", "atten_min", "first", "reach")


def spec(origin, step, n, n_theta, n_phi, edge_max, level_mask, wrap_lon=False, phi_periodic=False, leg_min=0, leg_max=LEG_ALL, ord_max=1, dir_mask=3):
    """the arguments of geoac_amd.ltube_spec as a plain dict"""
    return dict(origin=tuple(float(v) for v in origin), step=tuple(float(v) for v in step), n=tuple(int(v) for v in n), n_theta=int(n_theta), n_phi=int(n_phi),
                edge_max=float(edge_max), level_mask=int(level_mask), wrap_lon=bool(wrap_lon), phi_periodic=bool(phi_periodic), leg_min=int(leg_min),
                leg_max=int(leg_max), ord_max=int(ord_max), dir_mask=int(dir_mask))


def lstation_spec_of(sp):
    """the level-station spec whose lists hold a level tube map's hits (and those of the directions it leaves out)"""
    return LS.spec(sp["n_theta"], sp["n_phi"], phi_periodic=sp["phi_periodic"], leg_min=sp["leg_min"], leg_max=sp["leg_max"], ord_max=sp["ord_max"],
                   edge_max=sp["edge_max"], cap=CAP)


def selected(sp):
    """the selected levels in ascending level index"""
    return [l for l in range(31) if (sp["level_mask"] >> l) & 1]


def centres(sp):
    """cell centres [n0 * n1][2], row-major: s_a = origin[a] + (i_a + 0.5) * step[a], the product rounded before the sum"""
    s0 = sp["origin"][0] + (np.arange(sp["n"][0]) + 0.5) * sp["step"][0]
    s1 = sp["origin"][1] + (np.arange(sp["n"][1]) + 0.5) * sp["step"][1]
    return np.stack([np.repeat(s0, sp["n"][1]), np.tile(s1, sp["n"][0])], axis=1)


def stations_of(sp):
    """the stations of the definition: the centres once per selected level, level after level; sta [Ls * cells][2], level_of [Ls * cells]"""
    c, sel = centres(sp), selected(sp)
    return np.tile(c, (len(sel), 1)), np.repeat(sel, len(c))


def reduce_lists(hits, rows, sp):
    """level-station lists at stations_of(sp) (cap = CAP) -> the layers of the level tube map.  Asserts that no list overflowed: that is the
    condition under which the list reduction is the definition."""
    n0, n1 = sp["n"]
    Ls = len(selected(sp))
    M, R = hits.shape
    assert R == Ls * n0 * n1 and rows.shape == (M, R, CAP, LS.LSTA_STRIDE)
    assert int(hits.max(initial=0)) <= CAP, f"a cell centre has {int(hits.max())} hits: the lists are truncated at {CAP}"
    n_tri = 2 * (sp["n_theta"] - 1) * (sp["n_phi"] if sp["phi_periodic"] else sp["n_phi"] - 1)
    down = rows[..., S["DIR"]] < 0.0
    wanted = np.where(down, bool(sp["dir_mask"] & 2), bool(sp["dir_mask"] & 1))
    keep = (np.arange(CAP)[None, None, :] < hits[..., None]) & wanted
    shape = (M, Ls, n0, n1)
    out = {}
    count = keep.sum(axis=-1).astype(np.uint64)
    out["count"] = count.reshape(shape)
    tt, at = rows[..., S["TTIME"]], rows[..., S["ATTEN"]]
    fin = keep & np.isfinite(tt) & np.isfinite(at)                                    # a hit whose TTIME or ATTEN is not finite counts in COUNT only
    some = fin.any(axis=-1)
    top = np.uint64(0xffffffffffffffff)
    kt = np.where(fin, MR.key(tt), top).min(axis=-1)
    ka = np.where(fin, MR.key(at), top).min(axis=-1)
    out["ttime_min"] = np.where(some, MR.unkey(kt), np.inf).reshape(shape)
    out["atten_min"] = np.where(some, MR.unkey(ka), np.inf).reshape(shape)
    b = ((rows[..., S["LEG"]] - sp["leg_min"]) * 2 + down) * sp["ord_max"] + rows[..., S["ORD"]]
    hit_key = (b * n_tri + rows[..., S["TRI"]]).astype(np.int64)
    holder = fin & (MR.key(tt) == kt[..., None])
    first = np.where(holder, hit_key, np.iinfo(np.int64).max).min(axis=-1)
    out["first"] = np.where(some, first, -1).astype(np.int64).reshape(shape)
    out["reach"] = (out["count"] > 0).sum(axis=0).astype(np.uint32)
    return out


def reference_level_tubemap(eqset, count, lrec, theta, phi, legs, sp):
    """the level tube map of crossing counts [M][n_rays][L] and records [M][n_rays][L][capL][12], launch angles theta, phi [n_rays] and the launch's
    number of legs under spec dict sp"""
    sta, level_of = stations_of(sp)
    assert max(selected(sp)) < np.asarray(count).shape[2] and sp["level_mask"] > 0
    hits, rows = LS.reference_level_stations(eqset, count, lrec, theta, phi, legs, lstation_spec_of(sp), sta, level_of)
    return reduce_lists(hits, rows, sp)


def counts_per_level(layers, m=0):
    """per selected level of member m: the cells with COUNT 0, 1 and >= 2"""
    c = layers["count"][m]
    return [(int((c[ls] == 0).sum()), int((c[ls] == 1).sum()), int((c[ls] >= 2).sum())) for ls in range(c.shape[0])]


def assert_layers_equal(got, want, what=""):
    """every layer bit for bit (floats compared as their bit patterns)"""
    assert set(got) == set(want) == set(LAYERS), (what, sorted(got), sorted(want))
    for name in LAYERS:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = SR.bits(g) != SR.bits(w)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {diff.size} cells differ, first at {tuple(np.argwhere(diff)[0])}: {g[tuple(np.argwhere(diff)[0])]} vs {w[tuple(np.argwhere(diff)[0])]}"
