"""Station refinement without a GPU (include/geoac_refine.h): geoac_refine_check on the host, the header's elementary functions against numpy's,
and the numpy restatement (tests/refine_reference.py) driven by the plain-C oracle: every seed of a small lattice converges and lands on its
station, and a station on a fold ends every seed in a defined status."""
import ctypes

import numpy as np
import pytest

import harness as H
import refine_reference as RR
import station_cases as SC
import station_reference as SR

R, S = RR.RFN, SR.STA


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def test_refine_check_accepts_and_refuses(G):
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        G.refine_check(eq, G.refine_spec())
        G.refine_check(eq, G.refine_spec(max_iter=1, max_shrink=0, tol=1e-9, step_max_deg=1e-6))
        G.refine_check(eq, G.refine_spec(max_iter=32, max_shrink=16, tol=50.0, step_max_deg=5.0))
    bad = [(dict(max_iter=0), "max_iter"), (dict(max_iter=33), "max_iter"), (dict(max_shrink=-1), "max_shrink"), (dict(max_shrink=17), "max_shrink"),
           (dict(tol=0.0), "tol"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
           (dict(step_max_deg=0.0), "step_max_deg"), (dict(step_max_deg=-0.2), "step_max_deg"), (dict(step_max_deg=float("nan")), "step_max_deg"),
           (dict(step_max_deg=float("inf")), "step_max_deg")]
    for kw, word in bad:
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            G.refine_check(G.EQ_GLOBAL, G.refine_spec(**kw))
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.refine_check(G.EQ_2D, G.refine_spec())
    lib = G.load_library()
    assert lib.geoac_refine_check(G.EQ_2D, ctypes.byref(G.refine_spec())) == -4
    assert lib.geoac_refine_check(G.EQ_GLOBAL, None) == -1
    assert lib.geoac_refine_check(7, ctypes.byref(G.refine_spec())) == -1


def test_python_names_mirror_the_restatement(G):
    assert G.RFN == RR.RFN and G.RFN_STRIDE == RR.RFN_STRIDE and G.RFN_MAX_RAY_MEMBERS == RR.MAX_RAY_MEMBERS
    assert G.RFN_STATUS == dict(CONVERGED=RR.CONVERGED, ITER_LIMIT=RR.ITER_LIMIT, STALLED=RR.STALLED, LOST=RR.LOST, SINGULAR=RR.SINGULAR)
    sp = G.refine_spec(max_iter=5, max_shrink=3, tol=0.25, step_max_deg=0.1)
    assert {k: getattr(sp, k) for k in ("max_iter", "max_shrink", "tol", "step_max_deg")} == RR.spec(5, 3, 0.25, 0.1)


def test_header_symbols_exist_in_the_built_library(G):
    lib = G.load_library()
    for name in ("geoac_refine_check", "geoac_refine_fault", "geoac_fan_refine", "geoac_fan_refine_shape", "geoac_fan_refine_fetch", "geoac_fan_refine_dev",
                 "geoac_fan_refine_timing", "geoac_fan_refine_stats"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    assert hasattr(G.FanContext, "refine") and hasattr(G.FanContext, "refine_timing")


def test_elementary_functions_agree_with_numpy():
    """the header's SIN, COS, ASIN, SINCOSD and DIST are series in plain arithmetic: within a few ulp of numpy's over the ranges the header gives"""
    x = np.linspace(-np.pi / 2.0, np.pi / 2.0, 20001)
    assert np.abs(RR.SIN(x) - np.sin(x)).max() < 4e-16 and np.abs(RR.COS(x) - np.cos(x)).max() < 4e-16
    s = np.concatenate([np.linspace(0.0, 1.0, 20001), 10.0 ** np.linspace(-12.0, -1.0, 500)])
    err = np.abs(RR.ASIN(s) - np.arcsin(s))
    # recursive summation of 31 terms: at most 31 u relative to the sum (u = 2^-53); the complement form above 0.5 doubles it and works at the scale of Pi / 2
    u = 2.0 ** -53
    assert (err <= 64.0 * u * np.where(s > 0.5, np.pi / 2.0, np.arcsin(s))).all()
    a = np.linspace(-720.0, 720.0, 28801)
    sn, cs = RR.SINCOSD(a)
    assert np.abs(sn - np.sin(np.radians(a))).max() < 2e-15 and np.abs(cs - np.cos(np.radians(a))).max() < 2e-15
    assert RR.SINCOSD(np.array([0.0, 90.0, 180.0, -90.0]))[0].tolist() == [0.0, 1.0, 0.0, -1.0]
    rng = np.random.default_rng(3)
    lat1, lat2 = rng.uniform(-89.0, 89.0, 4000), rng.uniform(-89.0, 89.0, 4000)
    lon1, lon2 = rng.uniform(-180.0, 180.0, 4000), rng.uniform(-180.0, 540.0, 4000)
    h = np.sin(np.radians(lat2 - lat1) / 2.0) ** 2 + np.cos(np.radians(lat1)) * np.cos(np.radians(lat2)) * np.sin(np.radians(lon2 - lon1) / 2.0) ** 2
    want = 2.0 * 6370.0 * np.arcsin(np.sqrt(h))
    assert np.allclose(RR.DIST(lat1, lon1, lat2, lon2, 6370.0), want, rtol=1e-12, atol=1e-9)
    assert RR.DIST(np.array([30.0]), np.array([179.5]), np.array([30.0]), np.array([-179.5]), 6370.0)[0] < 100.0          # across the antimeridian: 1 degree, not 359


# ---- the algorithm, integrated by the plain-C oracle ----
# lattices of 0.5 x 1 degrees over the sector where ToyAtmo's westward stratospheric duct lands at 2.5 degrees (278 km), one bounce; the oracle
# integrates about 15 rays a second with amplitudes, so the sectors are small
CASES = {
    "global": dict(eq=H.EQ_GLOBAL, src=(0.0, 30.0, 0.0), fan=dict(theta_min=25.0, theta_max=28.0, theta_step=0.5, phi_min=-102.0, phi_max=-88.0, phi_step=1.0)),
    "3d": dict(eq=H.EQ_3D, src=(0.0, 0.0, 0.0), fan=dict(theta_min=23.5, theta_max=26.0, theta_step=0.5, phi_min=-102.0, phi_max=-88.0, phi_step=1.0)),
}


def _stations(name):
    if name == "global":
        return SC.ring_stations([46, 47, 48])                                      # three neighbours of the 2.5-degree, 64-position ring
    az = np.radians(np.array([-99.0, -95.0, -91.0]))
    return np.stack([278.0 * np.sin(az), 278.0 * np.cos(az)], axis=1)              # the same distance from the Cartesian source [km]


class _OracleRun:
    """a lattice launch by the oracle, its station lists (the restatement of geoac_fan_stations) and what the refinement needs"""

    def __init__(self, eq, src, fan, sta, cap=8):
        self.eq, self.sta = eq, np.ascontiguousarray(sta)
        self.O = H.Oracle(eq)
        self.cfg = H.make_cfg(eq, bounces=1, calc_amp=True, src=src)
        th, ph, nt, nph = SC.lattice(**fan)
        self.rec = self.O.fan(self.cfg, th, ph)[1][None]
        level = np.zeros((1, 1) + self.rec.shape[1:3])
        self.hits, self.rows, _ = SR.reference_stations(eq, self.rec, th, ph, level, SR.spec(nt, nph, cap=cap), self.sta)
        o9, _ = self.O.atmo_probe(np.array([max(src[2], 0.0)]))
        self.mem = RR.members(eq, [src], (o9[0, 3] / o9[0, 0], o9[0, 6] / o9[0, 0]) if eq == H.EQ_3D else None)
        self.launches = 0

    def integrate(self, th, ph):
        self.launches += 1
        return self.O.fan(self.cfg, th, ph)[1][None]

    def refine(self, **kw):
        return RR.reference_refine(self.eq, self.hits, self.rows, self.sta, RR.spec(**kw), self.integrate, self.mem)


@pytest.fixture(scope="module")
def runs():
    return {name: _OracleRun(c["eq"], c["src"], c["fan"], _stations(name)) for name, c in CASES.items()}


def _independent_miss(eq, rec_row, station):
    """distance of a record's landing point from a station with numpy's own functions (not the header's series) [km]"""
    st = rec_row[H.REC["STATE"]:]
    if eq == H.EQ_GLOBAL:
        lat, lon, la2, lo2 = st[1], st[2], np.radians(station[0]), np.radians(station[1])
        h = np.sin((la2 - lat) / 2.0) ** 2 + np.cos(lat) * np.cos(la2) * np.sin((lo2 - lon) / 2.0) ** 2
        return 2.0 * 6370.0 * np.arcsin(np.sqrt(h))
    return float(np.hypot(station[0] - st[0], station[1] - st[1]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_seed_converges_and_lands_on_its_station(runs, name):
    run = runs[name]
    eq = run.eq
    assert (run.hits[0] >= 1).all(), run.hits                                       # every station has an estimate
    rows, level, stats, fin = run.refine(max_iter=8, tol=0.1)
    n = int(np.minimum(run.hits, 8).sum())
    print(name, stats, "rounds per seed", rows[:, R["ITER"]].tolist(), "miss", rows[:, R["MISS"]].tolist())
    assert rows.shape == (n, 16) and level.shape == (n, 1) and stats["seeds"] == n
    assert (rows[:, R["STATUS"]] == RR.CONVERGED).all() and stats["converged"] == n and stats["launches"] <= 8
    assert (rows[:, R["MISS"]] <= 0.1).all() and (rows[:, R["ITER"]] >= 1).all() and (rows[:, R["ITER"]] <= stats["launches"]).all()
    assert stats["ray_members"] == stats["launches"] * n
    # list order, and the seeds' own columns
    key = rows[:, R["STATION"]] * 1e6 + rows[:, R["LEG"]] * 1e5 + rows[:, R["TRI"]]
    assert (np.diff(key) > 0).all() and (rows[:, R["MEMBER"]] == 0).all()
    # the final landing, recomputed from a fresh oracle launch at the rows' angles with numpy's own functions
    again = run.O.fan(run.cfg, rows[:, R["THETA"]].copy(), rows[:, R["PHI"]].copy())[1]
    for i, row in enumerate(rows):
        leg, sta = int(row[R["LEG"]]), run.sta[int(row[R["STATION"]])]
        rec = again[i, leg]
        assert rec[H.REC["VALID"]] == 1.0
        miss = _independent_miss(eq, rec, sta)
        assert miss <= 0.1 and abs(miss - row[R["MISS"]]) <= 1e-9 * max(1.0, miss) + 1e-7, (i, miss, row[R["MISS"]])
        assert np.array_equal(rec, fin[0, i, leg])                                  # a frozen seed is integrated at the same angles: the same record
        for col, field in (("TTIME", "TTIME"), ("TURN", "TURN"), ("INCL", "INCL"), ("BACKAZ", "BACKAZ"), ("AMP", "AMP"), ("JACOB", "JACOB")):
            assert row[R[col]] == rec[H.REC[field]]
        rng = RR.DIST(np.array([30.0]), np.array([0.0]), sta[:1], sta[1:], 6370.0)[0] if eq == H.EQ_GLOBAL else float(np.sqrt(sta[0] * sta[0] + sta[1] * sta[1]))
        assert row[R["CELERITY"]] == rng / rec[H.REC["TTIME"]] and 0.2 < row[R["CELERITY"]] < 0.36
        assert level[i, 0] == 20.0 * np.log10(rec[H.REC["AMP"]]) - rec[H.REC["ATTEN"]]
    # the refined angles stay inside the seed's lattice cell neighbourhood (one lattice step in both angles)
    m, r, l, t, th0, ph0 = RR.seeds(run.hits, run.rows)
    assert (np.abs(rows[:, R["THETA"]] - th0) <= 0.5).all() and (np.abs(rows[:, R["PHI"]] - ph0) <= 1.0).all()


def test_one_launch_is_not_enough_and_the_limit_is_reported(runs):
    """max_iter = 1: the seeds' own rays miss by more than a tight tolerance, so every seed ends ITER_LIMIT with its first miss and no eigenray columns"""
    run = runs["global"]
    rows, level, stats, _ = run.refine(max_iter=1, tol=1e-6)
    assert stats["launches"] == 1 and (rows[:, R["STATUS"]] == RR.ITER_LIMIT).all() and stats["stalled_or_limit"] == len(rows)
    assert (rows[:, R["MISS"]] > 1e-6).all() and np.isfinite(rows).all() and (rows[:, R["TTIME"]:] == 0).all() and (level == 0).all()
    m, r, l, t, th0, ph0 = RR.seeds(run.hits, run.rows)
    assert np.array_equal(rows[:, R["THETA"]], th0) and np.array_equal(rows[:, R["PHI"]], ph0) and (rows[:, R["ITER"]] == 1).all()


def test_a_seed_whose_ray_is_lost_or_never_improves_ends_in_a_defined_status(runs):
    """synthetic integrators on the oracle's lists: every leg not VALID -> LOST in one launch; records that never move -> STALLED after max_shrink + 1
    rejected trials; a record with zero derivatives -> SINGULAR"""
    run = runs["global"]
    n = int(np.minimum(run.hits, 8).sum())
    legs = run.rec.shape[2]
    rows, _, stats, _ = RR.reference_refine(run.eq, run.hits, run.rows, run.sta, RR.spec(), lambda a, b: np.zeros((1, len(a), legs, 32)), run.mem)
    assert stats["launches"] == 1 and (rows[:, R["STATUS"]] == RR.LOST).all() and (rows[:, R["MISS"]] == -1.0).all() and stats["lost_or_singular"] == n
    first = run.O.fan(run.cfg, *RR.seeds(run.hits, run.rows)[4:6])[1][None]
    rows, _, stats, _ = RR.reference_refine(run.eq, run.hits, run.rows, run.sta, RR.spec(max_iter=12, max_shrink=3, tol=1e-6), lambda a, b: first, run.mem)
    assert (rows[:, R["STATUS"]] == RR.STALLED).all() and stats["launches"] == 5 and (rows[:, R["ITER"]] == 5).all() and np.isfinite(rows).all()
    flat = first.copy()
    flat[..., H.REC["STATE"] + 6:] = 0.0
    rows, _, stats, _ = RR.reference_refine(run.eq, run.hits, run.rows, run.sta, RR.spec(tol=1e-6), lambda a, b: flat, run.mem)
    assert (rows[:, R["STATUS"]] == RR.SINGULAR).all() and stats["launches"] == 1 and np.isfinite(rows).all()


def test_station_on_a_fold_ends_every_seed_in_a_defined_status():
    """ToyAtmo's stratospheric branch has its shortest range (221.0 km) near 19.5 degrees: a station just beyond it, between the landing points of
    the 19 and 19.5 degree rays, lies inside landing triangles of both sheets - seeds of opposite ORIENT in neighbouring cells.  The landing Jacobian
    is close to singular there: convergence is not required, a defined status and finite rows are."""
    fan = dict(theta_min=18.0, theta_max=21.0, theta_step=0.5, phi_min=-92.0, phi_max=-88.0, phi_step=1.0)
    th, ph, nt, nph = SC.lattice(**fan)
    probe = _OracleRun(H.EQ_GLOBAL, (0.0, 30.0, 0.0), fan, np.zeros((1, 2)))
    c0, c1 = SR.landing(H.EQ_GLOBAL, probe.rec)
    pick = [j * nt + i for j in (2, 3) for i in (2, 3)]                                # theta 19 and 19.5 (the fold's own ray) at phi -90 and -89
    assert th[pick].tolist() == [19.0, 19.5, 19.0, 19.5]
    sta = np.array([[c0[0, pick, 0].mean(), c1[0, pick, 0].mean()]])
    run = probe
    run.sta = sta
    run.hits, run.rows, _ = SR.reference_stations(H.EQ_GLOBAL, run.rec, th, ph, np.zeros((1, 1) + run.rec.shape[1:3]), SR.spec(nt, nph, cap=8, leg_max=0), sta)
    kept = run.rows[0, 0, :int(run.hits[0, 0])]
    print("fold: hits", run.hits.tolist(), "orient", kept[:, S["ORIENT"]].tolist(), "theta", kept[:, S["THETA"]].tolist())
    assert len(kept) >= 2 and {-1.0, 1.0} <= set(kept[:, S["ORIENT"]])
    plus, minus = kept[kept[:, S["ORIENT"]] > 0], kept[kept[:, S["ORIENT"]] < 0]
    cells = lambda r: r[:, S["TRI"]].astype(int) // 2                               # noqa: E731
    assert min(abs(int(a) - int(b)) for a in cells(plus) for b in cells(minus)) <= 1        # neighbouring cells of one lattice column
    rows, level, stats, _ = run.refine(max_iter=8, tol=0.1)
    print("fold:", stats, "status", rows[:, R["STATUS"]].tolist(), "miss", rows[:, R["MISS"]].tolist(), "theta", rows[:, R["THETA"]].tolist())
    assert len(rows) == len(kept) and np.isfinite(rows).all() and np.isfinite(level).all()
    assert set(rows[:, R["STATUS"]]) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    assert stats["converged"] + stats["stalled_or_limit"] + stats["lost_or_singular"] == len(rows)
    done = rows[:, R["STATUS"]] != RR.CONVERGED
    assert (rows[done, R["TTIME"]:] == 0).all() and (level[done] == 0).all()
