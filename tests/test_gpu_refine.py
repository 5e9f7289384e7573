"""Station refinement on the device (include/geoac_refine.h, FanContext.refine): rows, level and counters against the numpy restatement
(tests/refine_reference.py) driven by a second context's launches, bit for bit; members of an ensemble, a source set and a frequency set against
plain contexts; the landing condition from a fresh launch; the call's lifecycle; a station on a fold; and the reference's own config-5 eigenrays.
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import map_cases as MC
import refine_reference as RR
import station_cases as SC
import station_reference as SR
import test_gpu_globalrd as TGG
import test_gpu_rngdep as TGR
from parity import parse_eig_results, ring_golden_name, ring_receivers
from test_gpu_ensemble import _device_arrays, _raw_members
from test_gpu_sources import SOURCES, _toy, _upload

pytestmark = pytest.mark.gpu
R, S = RR.RFN, SR.STA
STEP_LIMIT_S = 300
GRID_KINDS = ("3drd", "globalrd")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _context(G, case, tmpdir, params=None):
    """a context set up as the map case says (atmosphere, parameters, sources, frequencies), nothing launched"""
    eq, kind, prm = case["eq"], case["kind"], dict(case["params"], **(params or {}))
    if kind in GRID_KINDS:
        return (TGR if kind == "3drd" else TGG)._ctx(MC.write_grid(kind, str(tmpdir)), **prm)
    ctx = G.FanContext(eq, device=0)
    if kind == "ensemble" or (kind == "sources" and case["n_prof"] > 1):
        _upload(ctx, [_device_arrays(eq, *r) for r in _raw_members()])
    else:
        _upload(ctx, [_toy(eq)])
    ctx.set_params(**prm)
    if kind == "sources":
        ctx.set_sources(SOURCES[eq][:case["n_src"]])
    if kind == "freqs":
        ctx.set_frequencies(case["freqs"])
    return ctx


def _sources_of(ctx, case):
    """[M][3] source rows of the launch's members, m = source * K + profile"""
    if case["kind"] == "sources":
        return np.repeat(SOURCES[case["eq"]][:case["n_src"]], case["n_prof"], axis=0)
    return np.repeat(np.array([list(ctx.params.src)]), ctx.n_members, axis=0)


def _mach(ctx, z):
    """u / c, v / c of the context's (single) profile at height z, as the library evaluates them (geoac_medium_1d)"""
    out = (ctypes.c_double * 4)()
    ctx.lib.geoac_medium_1d.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    assert ctx.lib.geoac_medium_1d(ctx._h, float(z), out) == 0
    return out[1] / out[0], out[2] / out[0]


def _members(ctx, case):
    src = _sources_of(ctx, case)
    mach = None
    if case["eq"] == H.EQ_3D:
        assert ctx.n_members == 1                                                   # (the restatement's Mach numbers come from the one profile on the host)
        mach = [_mach(ctx, max(s[2], ctx.params.z_grnd)) for s in src]
    return RR.members(case["eq"], src, mach)


def _lattice_launch(ctx, case, lattice=None):
    th, ph, nt, nph = SC.lattice(**(lattice or (SC.PARITY_LATTICE_RD if case["kind"] in GRID_KINDS else SC.PARITY_LATTICE)))
    rec = ctx.run(th, ph)[0]
    return rec.reshape((-1,) + rec.shape[-3:]), th, ph, nt, nph


def _refine_both(G, case, tmpdir, sta_of, spec_kw, sta_kw=None, lattice=None, params=None):
    """refine on one context; restate with a second context of the same set-up as the integrator.  Returns the device result and the lists."""
    ctx = _context(G, case, tmpdir, params)
    rec, th, ph, nt, nph = _lattice_launch(ctx, case, lattice)
    sta = sta_of(rec, th, nt)
    hits, rows, _ = ctx.stations(sta=sta, n_theta=nt, n_phi=nph, **(sta_kw or dict(cap=4)))
    mem = _members(ctx, case)
    got = ctx.refine(**spec_kw)
    other = _context(G, case, tmpdir, params)
    want = RR.reference_refine(case["eq"], hits, rows, sta, RR.spec(**spec_kw), lambda a, b: other.run(a, b)[0], mem, r_earth=ctx.params.r_earth, z_grnd=ctx.params.z_grnd,
                               level_of=other.fetch_level)
    RR.assert_equal_bits(got[:2], want[:2])
    assert got[2] == want[2], (got[2], want[2])
    other.close()
    return ctx, got, (hits, rows, sta)


# the four 3-D-capable sets, an ensemble, a source set and a frequency set
RESTATED = ["plain-global-amp1-b2", "plain-3d-amp1-b2", "3drd", "globalrd", "ensemble3-global", "sources2-3d", "freqs4-global"]
CASES = dict(MC.CASES, **{"sources2-3d": dict(MC.CASES["sources4-3d"], n_src=2, params=dict(bounces=1, calc_amp=1))})          # sources (0, 0, 0) and (100, -50, 20): two heights, two pairs of Mach numbers; one bounce keeps it short


@pytest.mark.parametrize("name", RESTATED)
def test_rows_equal_restatement(G, name, tmp_path):
    """the coarse lattices of the station tests (3 x 8 degrees): the estimates are far from their eigenrays, so the rounds are cut steps, rejected
    trials and every final status - the step rule's branches, not its convergence"""
    case = CASES[name]
    spec_kw = dict(max_iter=6, max_shrink=2, tol=0.5, step_max_deg=1.0)
    ctx, (rows, level, stats), (hits, srows, sta) = _refine_both(G, case, tmp_path, lambda rec, th, nt: SC.draw_stations(case["eq"], rec, n_near=24, n_far=3), spec_kw)
    M, F = hits.shape[0], len(case.get("freqs", [0]))
    n = int(np.minimum(hits, 4).sum())
    status = rows[:, R["STATUS"]].astype(int)
    print(f"{name}: M {M} F {F} seeds {n} launches {stats['launches']} status counts {np.bincount(status, minlength=6)[1:].tolist()} (converged, limit, stalled, lost, singular)")
    assert rows.shape == (n, 16) and level.shape == (n, F) and stats["seeds"] == n and n >= 8
    assert stats["ray_members"] == stats["launches"] * n * M and 1 <= stats["launches"] <= 6
    assert n % 64 != 0                                                              # a part-filled last wave
    assert set(status) <= {1, 2, 3, 4, 5} and len(set(rows[:, R["MEMBER"]])) == M
    assert np.isfinite(rows).all()
    done = status != RR.CONVERGED
    assert (rows[done, R["TTIME"]:] == 0).all() and (level[done] == 0).all() and (rows[~done, R["MISS"]] <= 0.5).all()
    # the launch's own records are those of the last round: n rays per member
    assert ctx.fetch()[0].reshape(M, -1, case["params"]["bounces"] + 1, 32).shape[1] == n
    ctx.close()


def test_single_seed(G):
    case = MC.CASES["plain-global-amp1-b2"]

    def one(rec, th, nt):
        sta = SC.draw_stations(case["eq"], rec, n_near=40, n_far=0)
        return sta[:1]

    ctx, (rows, level, stats), (hits, _, _) = _refine_both(G, case, None, one, dict(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=1.0), sta_kw=dict(cap=1))
    assert hits[0, 0] >= 1 and rows.shape == (1, 16) and stats["seeds"] == 1 and stats["ray_members"] == stats["launches"]
    ctx.close()


# ---- members against plain contexts ----
FINE = dict(theta_min=20.0, theta_max=30.0, theta_step=0.5, phi_min=-140.0, phi_max=-40.0, phi_step=1.0)          # 21 x 101 rays around ToyAtmo's westward duct
SPEC = dict(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2)


def _fine_stations(eq, src):
    """13 stations 2.5 degrees (278 km) from a source, south-west to north-west of it (positions 42 .. 54 of the 64-ring), in the axes of the set"""
    if eq == H.EQ_GLOBAL:
        return ring_receivers(n=64, lat0=src[1], lon0=src[2], radius_deg=2.5)[42:55]
    az = np.radians(-123.75 + 5.625 * np.arange(13))
    return np.stack([src[0] + 278.0 * np.sin(az), src[1] + 278.0 * np.cos(az)], axis=1)


def _plain_refine(G, eq, prof, src, sta, freq=None, bounces=1):
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(bounces=bounces, calc_amp=1, src=tuple(src), **({} if freq is None else dict(freq=freq)))
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    out = ctx.refine(**SPEC)
    ctx.close()
    return out


def _member_rows(rows, level, m):
    sel = rows[:, R["MEMBER"]] == m
    r = rows[sel].copy()
    r[:, R["MEMBER"]] = 0.0
    return r, level[sel]


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_ensemble_member_equals_plain_context(G, eq):
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    src = SOURCES[eq][0]
    sta = _fine_stations(eq, src)
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(src))
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    rows, level, stats = ctx.refine(**SPEC)
    ctx.close()
    print(f"ensemble {H.EQ_NAMES[eq]}: {stats}")
    per_member = [int(((rows[:, R["MEMBER"]] == m) & (rows[:, R["STATUS"]] == RR.CONVERGED)).sum()) for m in range(3)]
    print("converged per member", per_member)
    assert sum(c > 0 for c in per_member) >= 2                                      # (a member with weaker winds may have no stratospheric return here: its lists are empty in both)
    for m, prof in enumerate(profs):
        pr, pl, pst = _plain_refine(G, eq, prof, src, sta)
        RR.assert_equal_bits(_member_rows(rows, level, m), (pr, pl))


def test_source_set_member_equals_plain_context(G):
    eq = H.EQ_GLOBAL
    profs = [_device_arrays(eq, *r) for r in _raw_members()[:2]]
    srcs = np.array([[0.0, 30.0, 0.0], [0.0, 30.5, 0.4]])                            # two candidate sources half a degree apart: the same stations serve both
    sta = _fine_stations(eq, srcs[0])
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(bounces=1, calc_amp=1)
    ctx.set_sources(srcs)
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    rows, level, stats = ctx.refine(**SPEC)
    ctx.close()
    print(f"sources 2 x 2: {stats}")
    per_member = [int(((rows[:, R["MEMBER"]] == m) & (rows[:, R["STATUS"]] == RR.CONVERGED)).sum()) for m in range(4)]
    print("converged per member", per_member)
    assert sum(c > 0 for c in per_member) >= 2
    for s, src in enumerate(srcs):
        for k, prof in enumerate(profs):
            pr, pl, _ = _plain_refine(G, eq, prof, src, sta)
            RR.assert_equal_bits(_member_rows(rows, level, s * 2 + k), (pr, pl))


def test_frequency_set_equals_plain_contexts(G):
    eq, freqs = H.EQ_GLOBAL, [0.1, 0.5, 2.0]
    prof, src = _toy(eq), SOURCES[eq][0]
    sta = _fine_stations(eq, src)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(src))
    ctx.set_frequencies(freqs)
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    rows, level, stats = ctx.refine(**SPEC)
    ctx.close()
    assert level.shape == (len(rows), 3) and stats["converged"] >= 1
    for f, freq in enumerate(freqs):
        pr, pl, _ = _plain_refine(G, eq, prof, src, sta, freq=freq)
        if f == 0:
            RR.assert_equal_bits((rows,), (pr,), names=("rows",))
        RR.assert_equal_bits((level[:, f:f + 1],), (pl,), names=(f"level[:, {f}]",))
    conv = rows[:, R["STATUS"]] == RR.CONVERGED
    assert (level[conv, 0] > level[conv, 2]).all()                                  # more absorption at 2 Hz than at 0.1 Hz


# ---- the landing condition ----
@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_converged_rows_land_on_their_station(G, eq):
    prof, src = _toy(eq), SOURCES[eq][0]
    sta = _fine_stations(eq, src)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(src))
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx.run(th, ph)
    hits, srows, _ = ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    rows, level, stats = ctx.refine(**SPEC)
    ctx.close()
    print(f"landing {H.EQ_NAMES[eq]}: hits {hits[0].tolist()} {stats} rounds {rows[:, R['ITER']].tolist()}")
    conv = rows[rows[:, R["STATUS"]] == RR.CONVERGED]
    assert len(conv) >= 3
    fresh = G.FanContext(eq, device=0)
    fresh.upload_atmo_1d(*prof)
    fresh.set_params(bounces=1, calc_amp=1, src=tuple(src))
    again = fresh.run(conv[:, R["THETA"]].copy(), conv[:, R["PHI"]].copy())[0]
    lv = fresh.fetch_level()
    fresh.close()
    for i, row in enumerate(conv):
        leg, st = int(row[R["LEG"]]), sta[int(row[R["STATION"]])]
        rec = again[i, leg]
        state = rec[H.REC["STATE"]:]
        assert rec[H.REC["VALID"]] == 1.0
        if eq == H.EQ_GLOBAL:
            la2, lo2 = np.radians(st[0]), np.radians(st[1])
            h = np.sin((la2 - state[1]) / 2.0) ** 2 + np.cos(state[1]) * np.cos(la2) * np.sin((lo2 - state[2]) / 2.0) ** 2
            miss = 2.0 * 6370.0 * np.arcsin(np.sqrt(h))
        else:
            miss = float(np.hypot(st[0] - state[0], st[1] - state[1]))
        assert miss <= 0.1 and abs(miss - row[R["MISS"]]) <= 1e-9 * max(1.0, miss) + 1e-7, (i, miss, row[R["MISS"]])
        for col in ("TTIME", "TURN", "INCL", "BACKAZ", "AMP", "JACOB"):
            assert SR.bits(np.array([row[R[col]]]))[0] == SR.bits(np.array([rec[H.REC[col]]]))[0], col
    sel = np.flatnonzero(rows[:, R["STATUS"]] == RR.CONVERGED)
    assert np.array_equal(SR.bits(level[sel, 0]), SR.bits(np.array([lv[0, 0, i, int(conv[i, R["LEG"]])] for i in range(len(conv))])))


# ---- lifecycle ----
def test_lifecycle(G):
    eq = H.EQ_GLOBAL
    prof, src = _toy(eq), SOURCES[eq][0]
    sta = _fine_stations(eq, src)
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(src))
    lib = ctx.lib
    buf = np.zeros((64, 16))

    def fetch_rc():
        return lib.geoac_fan_refine_fetch(ctx._h, buf.ctypes.data_as(ctypes.c_void_p), None)

    with pytest.raises(G.GeoAcError, match="invalid.*no station lists"):
        ctx.refine(**SPEC)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*no station lists"):             # a launch alone makes no lists
        ctx.refine(**SPEC)
    assert fetch_rc() == -1
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    first = ctx.refine(**SPEC)
    assert first[2]["seeds"] >= 3 and fetch_rc() == 0 and ctx.refine_timing()["launch_ms"] > 0.0
    # the lattice's lists, maps and tube maps went with the refinement's launches
    hits = np.zeros((1, len(sta)), dtype=np.uint32)
    assert lib.geoac_fan_stations_fetch(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), None, None) == -1
    cnt = np.zeros((4, 4), dtype=np.uint64)
    assert lib.geoac_fan_map_fetch(ctx._h, 0, cnt.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.geoac_fan_tubemap_fetch(ctx._h, 0, cnt.ctypes.data_as(ctypes.c_void_p)) == -1
    with pytest.raises(G.GeoAcError, match="invalid.*no station lists"):
        ctx.refine(**SPEC)
    assert fetch_rc() == 0                                                          # a refused call leaves the result alone
    # lattice launch, stations, refine: works again, and gives the same bits
    ctx.run(th, ph)
    assert fetch_rc() == -1                                                         # a launch invalidates the result
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    second = ctx.refine(**SPEC)
    RR.assert_equal_bits(second[:2], first[:2])
    assert second[2] == first[2]
    for what, act in (("set_angles", lambda: ctx.set_angles(th, ph)), ("set_frequencies", lambda: ctx.set_frequencies([0.1])),
                      ("set_sources", lambda: ctx.set_sources(np.array([list(src)]))), ("upload", lambda: ctx.upload_atmo_1d(*prof))):
        assert fetch_rc() == 0, what
        act()
        assert fetch_rc() == -1 and "fan_refine_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        ctx.run(th, ph)
        ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
        RR.assert_equal_bits(ctx.refine(**SPEC)[:2], first[:2])
    # bad specs name their fault and leave the lists alone
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    for bad, word in ((dict(SPEC, max_iter=0), "max_iter"), (dict(SPEC, max_shrink=17), "max_shrink"), (dict(SPEC, tol=0.0), "tol"), (dict(SPEC, step_max_deg=float("nan")), "step_max_deg")):
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            ctx.refine(**bad)
    assert lib.geoac_fan_stations_fetch(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), None, None) == 0
    # zero seeds: an empty result, nothing launched
    far = np.array([[-60.0, 100.0], [-61.0, 101.0]])
    ctx.stations(sta=far, n_theta=nt, n_phi=nph, cap=4)
    rows, level, stats = ctx.refine(**SPEC)
    assert rows.shape == (0, 16) and level.shape == (0, 1) and stats == dict(launches=0, ray_members=0, seeds=0, converged=0, stalled_or_limit=0, lost_or_singular=0)
    assert ctx.n_rays == len(th)
    # sample capture, and calc_amp = 0 now or at the lattice launch
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    ctx.set_params(mode=H.MODE_WRITE_RAYS)
    with pytest.raises(G.GeoAcError, match="invalid.*sample capture"):
        ctx.refine(**SPEC)
    ctx.set_params(mode=0, calc_amp=0)
    with pytest.raises(G.GeoAcError, match="invalid.*calc_amp"):
        ctx.refine(**SPEC)
    ctx.run(th, ph)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)
    with pytest.raises(G.GeoAcError, match="invalid.*calc_amp"):
        ctx.refine(**SPEC)
    ctx.set_params(calc_amp=1)
    with pytest.raises(G.GeoAcError, match="invalid.*calc_amp"):                    # the lattice launch ran without amplitudes
        ctx.refine(**SPEC)
    ctx.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=1)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        c2.refine(**SPEC)
    c2.close()


def test_ray_member_cap(G):
    """more than GEOAC_RFN_MAX_RAY_MEMBERS = 2^20 seeds x members: one station with an estimate, repeated; refused before anything is launched"""
    eq = H.EQ_GLOBAL
    prof, src = _toy(eq), SOURCES[eq][0]
    th, ph, nt, nph = SC.lattice(**FINE)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(bounces=1, calc_amp=1, src=tuple(src))
    ctx.run(th, ph)
    one = _fine_stations(eq, src)[6:7]                                              # due west
    hits, _, _ = ctx.stations(sta=one, n_theta=nt, n_phi=nph, cap=1)
    assert hits[0, 0] >= 1
    many = np.ascontiguousarray(np.repeat(one, G.RFN_MAX_RAY_MEMBERS + 1, axis=0))
    spec = G.station_spec(n_theta=nt, n_phi=nph, cap=1)
    assert ctx.lib.geoac_fan_stations(ctx._h, ctypes.byref(spec), len(many), many.ctypes.data_as(ctypes.c_void_p)) == 0
    with pytest.raises(G.GeoAcError, match="capacity.*ray-members"):
        ctx.refine(**SPEC)
    hits = np.zeros((1, len(many)), dtype=np.uint32)
    assert ctx.lib.geoac_fan_stations_fetch(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), None, None) == 0 and (hits == hits[0, 0]).all()          # the lists stay
    ctx.stations(sta=one, n_theta=nt, n_phi=nph, cap=1)
    assert ctx.refine(**SPEC)[2]["seeds"] == 1
    ctx.close()


# ---- a station on a fold ----
def test_fold_case_equals_restatement(G):
    """the CPU fold case (tests/test_refine_host.py) on the device: a station between the landing points of the 19 and 19.5 degree rays, where
    ToyAtmo's stratospheric branch has its shortest range"""
    case = dict(kind="plain", eq=H.EQ_GLOBAL, params=dict(bounces=1, calc_amp=1, src=(0.0, 30.0, 0.0)))
    fan = dict(theta_min=18.0, theta_max=21.0, theta_step=0.5, phi_min=-92.0, phi_max=-88.0, phi_step=1.0)

    def fold_station(rec, th, nt):
        c0, c1 = SR.landing(H.EQ_GLOBAL, rec)
        pick = [j * nt + i for j in (2, 3) for i in (2, 3)]
        assert th[pick].tolist() == [19.0, 19.5, 19.0, 19.5]
        return np.array([[c0[0, pick, 0].mean(), c1[0, pick, 0].mean()]])

    ctx, (rows, level, stats), (hits, srows, sta) = _refine_both(G, case, None, fold_station, SPEC, sta_kw=dict(cap=8, leg_max=0), lattice=fan)
    kept = srows[0, 0, :int(hits[0, 0])]
    print("fold:", stats, "orient", kept[:, S["ORIENT"]].tolist(), "status", rows[:, R["STATUS"]].tolist(), "miss", rows[:, R["MISS"]].tolist())
    assert len(kept) >= 2 and {-1.0, 1.0} <= set(kept[:, S["ORIENT"]])
    assert len(rows) == len(kept) and np.isfinite(rows).all() and np.isfinite(level).all() and set(rows[:, R["STATUS"]]) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    ctx.close()


# ---- the reference's own eigenrays (config 5) ----
EIG_POSITIONS = [42, 44, 45, 46, 47, 48, 49, 50, 52, 53, 54, 55, 56, 57, 58]          # as tests/test_gpu_stations.py: the ring positions that have reference eigenrays
EIG_FAN = dict(theta_min=0.5, theta_max=45.0, theta_step=0.5, phi_min=-150.0, phi_max=-28.0, phi_step=1.0)


def test_reference_eigenrays_have_a_converged_row(G, tmp_path):
    """the receivers of the golden config-5 eigenray fixtures (GeoAcGlobal.RngDep -eig_search): every eigenray the reference found inside the fan's
    inclination range has a CONVERGED row on its leg within one lattice step in both angles.  The travel times are compared and the largest
    differences written out (profiles/refine_accuracy.txt); they are not gated: both routines stop at a miss of 0.1 km, anywhere inside that
    circle, so the two travel times differ by up to the time sound takes to cross it (0.2 km / 0.3 km/s, about 0.7 s), far above parity.RTOL."""
    import rngdep_data as RD
    ctx = G.FanContext(G.EQ_GLOBAL_RNGDEP, device=0)
    ctx.load_grid(*RD.write_grid_global(str(tmp_path), short_paths=False))
    ctx.set_params(src=(0.0, 31.0, 0.0), bounces=2, calc_amp=1)
    th, ph, nt, nph = SC.lattice(**EIG_FAN)
    ctx.run(th, ph)
    rc = ring_receivers()
    ctx.stations(sta=rc[EIG_POSITIONS], n_theta=nt, n_phi=nph, cap=32)
    rows, level, stats = ctx.refine(**SPEC)
    ms = ctx.refine_timing()
    ctx.close()
    conv = rows[rows[:, R["STATUS"]] == RR.CONVERGED]
    n_eig, unmatched, d_th, d_ph, d_tt = 0, [], [], [], []
    for k, p in enumerate(EIG_POSITIONS):
        for e in parse_eig_results(os.path.join(H.GOLDEN_DIR, "cli", ring_golden_name(p), "g_results.dat")):
            if not (th.min() <= e["theta"] <= th.max()):
                continue
            n_eig += 1
            r = conv[(conv[:, R["STATION"]] == k) & (conv[:, R["LEG"]] == e["bounces"])]
            ok = (np.abs(r[:, R["THETA"]] - e["theta"]) <= EIG_FAN["theta_step"]) & (np.abs(r[:, R["PHI"]] - e["phi"]) <= EIG_FAN["phi_step"])
            if not ok.any():
                unmatched.append((p, e["theta"]))
                continue
            best = r[ok][np.argmin(np.abs(r[ok][:, R["THETA"]] - e["theta"]))]
            d_th.append(abs(best[R["THETA"]] - e["theta"])); d_ph.append(abs(best[R["PHI"]] - e["phi"]))
            if "ttime" in e:
                d_tt.append(abs(best[R["TTIME"]] - e["ttime"]))
    line = (f"config-5 ring, {len(EIG_POSITIONS)} receivers: {n_eig} reference eigenrays, unmatched {unmatched}; seeds {stats['seeds']}, converged {stats['converged']}, "
            f"stalled or limit {stats['stalled_or_limit']}, lost or singular {stats['lost_or_singular']}, launches {stats['launches']}, ray-members {stats['ray_members']}; "
            f"largest |theta - theta_ref| {max(d_th):.3e} deg, |phi - phi_ref| {max(d_ph):.3e} deg" + (f", |TTIME - ttime_ref| {max(d_tt):.3e} s" if d_tt else ", no travel time in the fixtures") +
            f"; launches {ms['launch_ms']:.1f} ms, refine kernels {ms['kernel_ms']:.3f} ms")
    print(line)
    out = os.environ.get("GEOAC_REFINE_ACCURACY_OUT")
    if out:
        open(out, "a").write(line + "\n")
    assert n_eig >= 15 and not unmatched
    assert (conv[:, R["MISS"]] <= 0.1).all()
