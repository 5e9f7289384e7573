"""Plain numpy restatement of the arrival map (include/geoac_map.h), written from its definition - TEST-ONLY, nothing under geoac_amd/ imports it.

Given the records of a launch, its attenuation table and its level table it forms every layer the device forms, reducing by the same
order-preserving integer keys of the doubles, so that ties, signed zeros and NaNs resolve as they do there: the layers can be compared bit for bit.
The cell arithmetic is the device's, operation for operation: degrees = rad * 180.0 / pi, q = floor((c - origin) / step)."""
import numpy as np

REC = dict(VALID=0, STEPS=1, BROKE=2, TTIME=3, ATTEN=4, TURN=5, INCL=6, BACKAZ=7, AMP=8, RANGE=9, JACOB=10, STATE=12)
EQ_2D, EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP = 0, 1, 2, 3, 4
SIGN = np.uint64(1 << 63)
LEG_ALL = 2**31 - 1


def key(x):
    """order-preserving u64 key of float64 values: all bits flipped for a negative value, otherwise the sign bit set"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | SIGN)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k & ~SIGN, ~k).view(np.float64)


def spec(origin, step, n, wrap_lon=False, leg_min=0, leg_max=LEG_ALL, turn_min=-np.inf, turn_max=np.inf, detect_db=np.nan):
    """the arguments of geoac_amd.map_spec as a plain dict (scalars for a one-axis grid)"""
    origin, step, n = (list(np.atleast_1d(a)) for a in (origin, step, n))
    if len(origin) == 1:
        origin, step, n = origin + [0.0], step + [1.0], n + [1]
    return dict(origin=[float(v) for v in origin], step=[float(v) for v in step], n=[int(v) for v in n], wrap_lon=bool(wrap_lon),
                leg_min=int(leg_min), leg_max=int(leg_max), turn_min=float(turn_min), turn_max=float(turn_max), detect_db=float(detect_db))


def level_numpy(rec, atten, calc_amp):
    """host restatement of the level table: rec [M][n_rays][legs][32], atten [F][n_rays][legs] (F > 1 needs M == 1) -> [M][F][n_rays][legs].
    numpy's log10 against the device's: agreement to rounding, not bit for bit."""
    rec = np.asarray(rec)
    M, n_rays, legs = rec.shape[:3]
    atten = np.asarray(atten).reshape(-1, n_rays, legs)
    F = atten.shape[0]
    assert M == 1 or F == 1
    out = np.full((M, F, n_rays, legs), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(M):
            amp_db = 20.0 * np.log10(rec[m, :, :, REC["AMP"]]) if calc_amp else np.zeros((n_rays, legs))
            for f in range(F):
                att = atten[f] if F > 1 else rec[m, :, :, REC["ATTEN"]]
                out[m, f] = np.where(rec[m, :, :, REC["VALID"]] != 0.0, amp_db - att, np.nan)
    return out


def passes(rec, sp):
    """[M][n_rays][legs] bool: VALID records inside the leg range and the turning-height band"""
    rec = np.asarray(rec)
    legs = rec.shape[2]
    leg = np.arange(legs)[None, None, :]
    turn = rec[..., REC["TURN"]]
    with np.errstate(invalid="ignore"):
        return (rec[..., REC["VALID"]] != 0.0) & (leg >= sp["leg_min"]) & (leg <= sp["leg_max"]) & (turn >= sp["turn_min"]) & (turn < sp["turn_max"])


def cells(eqset, rec, sp):
    """[M][n_rays][legs] int64: flat cell n1 * q0 + q1 of every record by its coordinates alone (filters not applied), -1 off the grid"""
    rec = np.asarray(rec)
    S = REC["STATE"]
    o, st, n = sp["origin"], sp["step"], sp["n"]
    with np.errstate(invalid="ignore", over="ignore"):
        if eqset in (EQ_GLOBAL, EQ_GLOBAL_RNGDEP):
            c0 = rec[..., S + 1] * 180.0 / np.pi
            c1 = rec[..., S + 2] * 180.0 / np.pi
            if sp["wrap_lon"]:
                c1 = c1 - 360.0 * np.floor((c1 - o[1]) / 360.0)
        elif eqset in (EQ_3D, EQ_3D_RNGDEP):
            c0, c1 = rec[..., S + 0], rec[..., S + 1]
        else:
            c0, c1 = rec[..., S + 0], None
        q0 = np.floor((c0 - o[0]) / st[0])
        q1 = np.zeros_like(q0) if c1 is None else np.floor((c1 - o[1]) / st[1])
        inside = (q0 >= 0.0) & (q0 < float(n[0])) & (q1 >= 0.0) & (q1 < float(n[1]))
    q0i = np.where(inside, q0, 0.0).astype(np.int64)
    q1i = np.where(inside, q1, 0.0).astype(np.int64)
    return np.where(inside, q0i * n[1] + q1i, -1)


def reference_map(eqset, rec, level, sp):
    """the map of records rec [M][n_rays][legs][32] with level table [M][F][n_rays][legs] under spec dict sp: dict of count, ttime_min, cel_max
    [M][n0][n1], level_max, best [M][F][n0][n1], outside [M], detect [F][n0][n1] (when detect_db is not NaN) and n_pass (filtered VALID arrivals)"""
    rec = np.asarray(rec)
    level = np.asarray(level)
    M, n_rays, legs = rec.shape[:3]
    F = level.shape[1]
    assert level.shape == (M, F, n_rays, legs)
    n0, n1 = sp["n"]
    nc = n0 * n1
    ok = passes(rec, sp)
    cell = cells(eqset, rec, sp)
    binned = ok & (cell >= 0)
    outside = (ok & (cell < 0)).reshape(M, -1).sum(axis=1).astype(np.uint64)
    count = np.zeros((M, nc), dtype=np.uint64)
    tkey = np.full((M, nc), ~np.uint64(0), dtype=np.uint64)
    ckey = np.zeros((M, nc), dtype=np.uint64)
    lkey = np.zeros((M, F, nc), dtype=np.uint64)
    best = np.full((M, F, nc), np.iinfo(np.int64).max, dtype=np.int64)
    index = (np.arange(n_rays)[:, None] * legs + np.arange(legs)[None, :]).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cel = rec[..., REC["RANGE"]] / rec[..., REC["TTIME"]]
    for m in range(M):
        sel = binned[m]
        c = cell[m][sel]
        np.add.at(count[m], c, np.uint64(1))
        np.minimum.at(tkey[m], c, key(rec[m, :, :, REC["TTIME"]][sel]))
        np.maximum.at(ckey[m], c, key(cel[m][sel]))
        for f in range(F):
            lv = level[m, f]
            fin = sel & np.isfinite(lv)
            cf = cell[m][fin]
            kf = key(lv[fin])
            np.maximum.at(lkey[m, f], cf, kf)
            holds = kf == lkey[m, f][cf]
            np.minimum.at(best[m, f], cf[holds], index[fin][holds])
    any_ = count != 0
    empty_l = lkey == 0
    out = dict(count=count.reshape(M, n0, n1),
               ttime_min=np.where(any_, unkey(tkey), np.inf).reshape(M, n0, n1),
               cel_max=np.where(any_, unkey(ckey), -np.inf).reshape(M, n0, n1),
               level_max=np.where(empty_l, -np.inf, unkey(lkey)).reshape(M, F, n0, n1),
               best=np.where(empty_l, np.int64(-1), best).reshape(M, F, n0, n1),
               outside=outside, n_pass=int(ok.sum()))
    if sp["detect_db"] == sp["detect_db"]:
        out["detect"] = (out["level_max"] >= sp["detect_db"]).sum(axis=0).astype(np.uint32)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def assert_maps_equal(got, want):
    """every layer bit for bit (floats compared as their bit patterns)"""
    for name in ("count", "ttime_min", "cel_max", "level_max", "best", "outside"):
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (name, got[name].shape, want[name].shape, got[name].dtype, want[name].dtype)
        diff = bits(got[name]) != bits(want[name])
        assert not diff.any(), f"layer {name}: {int(diff.sum())} of {diff.size} entries differ, first at {tuple(np.argwhere(diff)[0])}"
    assert ("detect" in got) == ("detect" in want)
    if "detect" in want:
        assert got["detect"].dtype == np.uint32 and np.array_equal(got["detect"], want["detect"]), "layer detect differs"


def check_non_vacuity(ref, sp, M):
    """the conditions every parity case asserts of its reference map (conditions, not measurements)"""
    inside = int(ref["count"].sum())
    assert ref["n_pass"] > 0 and inside >= 0.9 * ref["n_pass"], f"only {inside} of {ref['n_pass']} filtered arrivals fall inside the grid"
    assert int(ref["count"].max()) >= 2, "no cell holds two arrivals"
    if "detect" in ref:
        d = ref["detect"]
        assert (d == 0).any() and (d != 0).any(), "DETECT is all zero or nowhere zero"
        if M > 1:
            assert ((d > 0) & (d < M)).any(), "no cell is detected by some members and not by others"
