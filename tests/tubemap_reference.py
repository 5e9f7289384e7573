"""Plain numpy restatement of the tube map (include/geoac_tubemap.h), built on the station restatement (tests/station_reference.py, imported, not
copied) - TEST-ONLY, nothing under geoac_amd/ imports it.

The header defines a tube map as what the station search returns at every cell centre, reduced: stations at the centres, rows filtered by the
band on the interpolated turning height, reduction to the layers with the keys of the arrival map (tests/map_reference.py).  reduce_lists() does
the last two steps for any station lists - the restatement's or the device's own (FanContext.stations) - so both can be compared bit for bit
with FanContext.tubemap."""
import numpy as np

import map_reference as MR
import station_reference as SR

S = SR.STA
CAP = 256                                   # GEOAC_STA_MAX_CAP: the lists the reduction is taken from hold every hit only while hits <= CAP
LEG_ALL = SR.LEG_ALL


def spec(origin, step, n, n_theta, n_phi, edge_max, wrap_lon=False, phi_periodic=False, leg_min=0, leg_max=LEG_ALL, turn_tol=np.inf,
         turn_min=-np.inf, turn_max=np.inf, detect_db=np.nan):
    """the arguments of geoac_amd.tube_spec as a plain dict"""
    return dict(origin=tuple(float(v) for v in origin), step=tuple(float(v) for v in step), n=tuple(int(v) for v in n), n_theta=int(n_theta), n_phi=int(n_phi),
                edge_max=float(edge_max), wrap_lon=bool(wrap_lon), phi_periodic=bool(phi_periodic), leg_min=int(leg_min), leg_max=int(leg_max),
                turn_tol=float(turn_tol), turn_min=float(turn_min), turn_max=float(turn_max), detect_db=float(detect_db))


def station_spec_of(sp):
    """the station spec whose lists hold a tube map's hits"""
    return SR.spec(sp["n_theta"], sp["n_phi"], phi_periodic=sp["phi_periodic"], leg_min=sp["leg_min"], leg_max=sp["leg_max"], turn_tol=sp["turn_tol"],
                   edge_max=sp["edge_max"], cap=CAP)


def centres(sp):
    """cell centres [n0 * n1][2], row-major: s_a = origin[a] + (i_a + 0.5) * step[a], the product rounded before the sum"""
    s0 = sp["origin"][0] + (np.arange(sp["n"][0]) + 0.5) * sp["step"][0]
    s1 = sp["origin"][1] + (np.arange(sp["n"][1]) + 0.5) * sp["step"][1]
    return np.stack([np.repeat(s0, sp["n"][1]), np.tile(s1, sp["n"][0])], axis=1)


def reduce_lists(hits, rows, level, sp):
    """station lists at the cell centres (cap = CAP) -> the layers of the tube map.  Asserts that no list overflowed."""
    n0, n1 = sp["n"]
    M, R = hits.shape
    F = level.shape[-1]
    assert R == n0 * n1 and rows.shape == (M, R, CAP, SR.STA_STRIDE) and level.shape == (M, R, CAP, F)
    assert int(hits.max(initial=0)) <= CAP, f"a cell centre has {int(hits.max())} hits: the lists are truncated at {CAP}"
    n_tri = 2 * (sp["n_theta"] - 1) * (sp["n_phi"] if sp["phi_periodic"] else sp["n_phi"] - 1)
    turn = rows[..., S["TURN"]]
    with np.errstate(invalid="ignore"):
        keep = (np.arange(CAP)[None, None, :] < hits[..., None]) & (turn >= sp["turn_min"]) & (turn < sp["turn_max"])
    out = {}
    count = keep.sum(axis=-1).astype(np.uint64)
    out["count"] = count.reshape(M, n0, n1)
    any_ = count > 0
    kt = np.where(keep, MR.key(rows[..., S["TTIME"]]), np.uint64(0xffffffffffffffff)).min(axis=-1)
    kc = np.where(keep, MR.key(rows[..., S["CELERITY"]]), np.uint64(0)).max(axis=-1)
    out["ttime_min"] = np.where(any_, MR.unkey(kt), np.inf).reshape(M, n0, n1)
    out["cel_max"] = np.where(any_, MR.unkey(kc), -np.inf).reshape(M, n0, n1)
    hit_key = (rows[..., S["LEG"]] * n_tri + rows[..., S["TRI"]]).astype(np.int64)
    lvl = np.moveaxis(level, -1, 1)                                                   # [M][F][R][CAP]
    ok = keep[:, None] & np.isfinite(lvl)
    kl = np.where(ok, MR.key(lvl), np.uint64(0))
    top = kl.max(axis=-1)
    some = ok.any(axis=-1)
    out["level_max"] = np.where(some, MR.unkey(top), -np.inf).reshape(M, F, n0, n1)
    holder = ok & (kl == top[..., None])
    best = np.where(holder, hit_key[:, None], np.iinfo(np.int64).max).min(axis=-1)
    out["best"] = np.where(some, best, -1).astype(np.int64).reshape(M, F, n0, n1)
    if sp["detect_db"] == sp["detect_db"]:
        out["detect"] = (out["level_max"] >= sp["detect_db"]).sum(axis=0).astype(np.uint32)
    return out


def reference_tubemap(eqset, rec, theta, phi, level, sp):
    """the tube map of records rec [M][n_rays][legs][32], launch angles theta, phi [n_rays] and level table [M][F][n_rays][legs] under spec dict sp"""
    lists = SR.reference_stations(eqset, rec, theta, phi, level, station_spec_of(sp), centres(sp))
    return reduce_lists(*lists, sp)


def check_non_vacuity(ref, what=""):
    """the conditions every GPU case asserts of member 0 of its reference tube map (conditions, not measurements): empty cells, single-path cells
    and multipath cells all occur, at least a quarter of the cells is reached, and no centre has more hits than a station list holds"""
    c = ref["count"][0]
    n0, n1, n2 = int((c == 0).sum()), int((c == 1).sum()), int((c >= 2).sum())
    assert n0 > 0 and n1 > 0 and n2 > 0, f"{what}: cells with COUNT 0 / 1 / >= 2: {n0} / {n1} / {n2}"
    assert 4 * (n1 + n2) >= c.size, f"{what}: only {n1 + n2} of {c.size} cells are reached"
    assert int(ref["count"].max()) <= CAP, f"{what}: a centre has {int(ref['count'].max())} hits"
    return n0, n1, n2


def assert_layers_equal(got, want, what=""):
    """every layer bit for bit (floats compared as their bit patterns)"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in sorted(want):
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = SR.bits(g) != SR.bits(w)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {diff.size} cells differ, first at {tuple(np.argwhere(diff)[0])}: {g[tuple(np.argwhere(diff)[0])]} vs {w[tuple(np.argwhere(diff)[0])]}"
