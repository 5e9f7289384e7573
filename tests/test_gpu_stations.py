"""Station arrivals on the device (include/geoac_stations.h, FanContext.stations): hits, rows and level against the numpy restatement
(tests/station_reference.py) of the same launch's fetched records, angles and level table, bit for bit; overflow, repeatability, contention,
repeated calls, invalidation, isolation from the launch; and three physics checks of the estimates themselves (re-launch, convergence, the
reference's own eigenrays).  Launch set-ups are those of the map cases (tests/map_cases.py) with lattice fans in place of their 97-ray fan.
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import map_cases as MC
import station_cases as SC
import station_reference as SR
import tubemap_cases as TC
import test_gpu_globalrd as TGG
import test_gpu_rngdep as TGR
from parity import compare_records, parse_eig_results, ring_golden_name, ring_receivers
from test_gpu_ensemble import _device_arrays, _raw_members
from test_gpu_sources import SOURCES, _toy, _upload

pytestmark = pytest.mark.gpu
S = SR.STA
STEP_LIMIT_S = 300


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


def _lattice_of(case):
    return SC.lattice(**(SC.PARITY_LATTICE_RD if case["kind"] in ("3drd", "globalrd") else SC.PARITY_LATTICE))


def _context(G, case, tmpdir, params=None):
    """the map case's context (left open), set up and not launched"""
    eq, kind, prm = case["eq"], case["kind"], dict(case["params"], **(params or {}))
    if kind in ("3drd", "globalrd"):
        ctx = (TGR if kind == "3drd" else TGG)._ctx(MC.write_grid(kind, str(tmpdir)), **prm)
    else:
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


def _launch(G, case, tmpdir, params=None):
    """the map case's launch over the lattice fan: context (left open), records [M][n_rays][legs][32], angles, lattice shape"""
    ctx = _context(G, case, tmpdir, params)
    th, ph, nt, nph = _lattice_of(case)
    rec, _ = ctx.run(th, ph)
    return ctx, rec.reshape((-1,) + rec.shape[-3:]), th, ph, nt, nph


def _stations_and_reference(ctx, eq, rec, th, ph, sta, **spec_kw):
    level = ctx.fetch_level()
    got = ctx.stations(sta=sta, **spec_kw)
    want = SR.reference_stations(eq, rec, th, ph, level, SR.spec(**spec_kw), sta)
    SR.assert_lists_equal(got, want)
    return got


# the launches the issue names: the 3-D-capable stratified sets x calc_amp 0 / 1 x legs 1 / 3, and the member / frequency / grid cases of the maps
PARITY = [n for n in sorted(MC.CASES) if MC.CASES[n]["eq"] != H.EQ_2D]


@pytest.mark.parametrize("name", PARITY)
def test_lists_equal_reference(G, name, tmp_path):
    case = MC.CASES[name]
    ctx, rec, th, ph, nt, nph = _launch(G, case, tmp_path)
    M, legs = rec.shape[0], rec.shape[2]
    F = len(case.get("freqs", [0]))
    sta = SC.draw_stations(case["eq"], rec)
    hits, rows, level = _stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=12)
    assert hits.shape == (M, len(sta)) and rows.shape == (M, len(sta), 12, 16) and level.shape == (M, len(sta), 12, F)
    with_hits = int((hits[0] > 0).sum())
    print(f"{name}: M {M} F {F} legs {legs} stations {len(sta)} with hits (member 0) {with_hits}, most hits {int(hits.max())}, hits in all {int(hits.sum())}")
    assert with_hits >= len(sta) // 2 and (hits[0, -10:] == 0).all()              # most stations have hits, the far ones none
    if legs > 1:
        assert len(set(rows[hits > 0][:, 0, S["LEG"]])) > 1 or (rows[..., S["LEG"]] > 0).any()          # more than one leg takes part
    if F > 1:
        kept = rows[0, :, 0, S["W0"]] != 0
        assert not np.array_equal(level[0, kept, 0, 0], level[0, kept, 0, F - 1])
    # filters on the same launch: bit-identical too, and they only ever remove hits
    tight = _stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=12, leg_min=0, leg_max=0, turn_tol=25.0,
                                    edge_max=float(np.median(np.abs(sta[:-10] - sta[:-10].mean(axis=0)))))
    assert (tight[0] <= hits).all() and int(tight[0].sum()) < int(hits.sum())
    ctx.close()


def test_overflow_keeps_the_first_rows(G):
    case = MC.CASES["plain-global-amp1-b2"]
    ctx, rec, th, ph, nt, nph = _launch(G, case, None)
    sta = SC.draw_stations(case["eq"], rec)
    full = _stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=32)
    assert int(full[0].max()) >= 3 and int(full[0].max()) <= 32
    for cap in (1, 2):
        h, r, lv = _stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=cap)
        assert np.array_equal(h, full[0])
        assert np.array_equal(SR.bits(r), SR.bits(full[1][:, :, :cap])) and np.array_equal(SR.bits(lv), SR.bits(full[2][:, :, :cap]))
    ctx.close()


def test_two_chunks_and_the_periodic_seam(G):
    """the case level stations have (tests/test_gpu_lstations.py), on the ground lists that run the same walk: GEOAC_EQ_GLOBAL, ToyAtmo, source (0, 30, 0), one
    bounce, 30 inclinations x 72 azimuths over the whole circle: 29 x 72 = 2 088 cells, one full chunk of 2 048 and a tail of 40 (a partial trip).  Every
    station is a convex blend of the four leg-0 landing points of one lattice cell (from the fetched records), so it lies inside the cell's image where that
    is convex; four cells are in the seam column 71 -> 0, which is also the second chunk.  With tests/station_reference.py on the plain-C oracle's records of
    this fan every corner of the 16 cells is VALID on leg 0 and every station has a row of its own cell: the own-cell assertion is dropped for 0 of 16"""
    eq = H.EQ_GLOBAL
    th, ph, nt, nph = SC.lattice(theta_min=10.0, theta_max=39.0, theta_step=1.0, phi_min=-180.0, phi_max=175.0, phi_step=5.0)
    assert (nt, nph) == (30, 72)
    ctx = _phys_ctx(G)
    rec = ctx.run(th, ph)[0][None]
    sp = SR.spec(nt, nph, phi_periodic=True, cap=6)
    tri = SR.triangles(sp)
    c0, c1 = (c[0, :, 0] for c in SR.landing(eq, rec))
    cells = [(i, 71) for i in (2, 9, 17, 26)] + [(i, j) for i, j in zip((0, 5, 11, 14, 19, 23, 28, 7, 13, 21, 4, 16), (0, 6, 13, 21, 29, 36, 44, 52, 59, 66, 70, 33))]
    sta = []
    for i, j in cells:
        a, b, c = tri[2 * (j * (nt - 1) + i)]
        d = tri[2 * (j * (nt - 1) + i) + 1][2]
        assert (rec[0, [a, b, c, d], 0, SR.REC["VALID"]] != 0).all(), (i, j)           # (an unsuitable fan fails here, loudly)
        w = np.array([0.35, 0.3, 0.25, 0.1])                                       # (off the diagonal a - c: inside triangle (a, b, c) of a near-parallelogram)
        lon = c1[[a, b, c, d]]
        lon = lon[0] + SR._wrap180(lon - lon[0])
        sta.append([float(w @ c0[[a, b, c, d]]), float(w @ lon)])
    hits, rows, _ = _stations_and_reference(ctx, eq, rec, th, ph, np.array(sta), **sp)
    kept = rows[0][rows[0][..., S["W0"]] != 0]
    print(f"2 088 cells: hits {hits[0].tolist()}, triangles {sorted(set(kept[:, S['TRI']].astype(int)))}")
    assert (hits[0] >= 1).all()
    own = [any(int(t) // 2 == j * (nt - 1) + i for t in rows[0, k, :min(int(hits[0, k]), 6), S["TRI"]]) for k, (i, j) in enumerate(cells)]
    assert all(own), own
    assert (kept[:, S["TRI"]] >= 2 * 71 * (nt - 1)).any() and (kept[:, S["TRI"]] >= 2 * 2048).any()          # the seam column; the second chunk
    seam = rows[0, :4, 0]
    assert ((seam[:, S["PHI"]] > 175.0) & (seam[:, S["PHI"]] < 180.0)).all()            # continuous with corner 0 (175), not an average of 175 and -180
    ctx.close()


def test_repeatable_and_contention(G):
    case = MC.CASES["ensemble3-global"]
    ctx, rec, th, ph, nt, nph = _launch(G, case, None)
    sta = SC.draw_stations(case["eq"], rec)
    kw = dict(n_theta=nt, n_phi=nph, cap=8)
    a = ctx.stations(sta=sta, **kw)
    b = ctx.stations(sta=sta, **kw)
    SR.assert_lists_equal(a, b)
    busiest = int(np.argmax(a[0][0]))
    assert a[0][0, busiest] >= 2
    same = np.repeat(sta[busiest:busiest + 1], 512, axis=0)
    h, r, lv = _stations_and_reference(ctx, case["eq"], rec, th, ph, same, **kw)
    for got, one in ((h, a[0][:, busiest]), (r, a[1][:, busiest]), (lv, a[2][:, busiest])):
        assert (SR.bits(got) == SR.bits(np.ascontiguousarray(one))[:, None]).all()
    ctx.close()


def test_repeated_calls_leave_the_launch_alone(G):
    case = MC.CASES["sources2x3-global"]
    ctx, rec, th, ph, nt, nph = _launch(G, case, None)
    before, steps = ctx.fetch()
    epochs = ctx.timing()["epochs"]
    sta = SC.draw_stations(case["eq"], rec)
    first = _stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=6)
    _stations_and_reference(ctx, case["eq"], rec, th, ph, sta[::3], n_theta=nt, n_phi=nph, cap=3, leg_min=1, leg_max=1, turn_tol=40.0)
    SR.assert_lists_equal(_stations_and_reference(ctx, case["eq"], rec, th, ph, sta, n_theta=nt, n_phi=nph, cap=6), first)
    ctx.map(**case["spec"])                                                         # maps and station lists share the level table
    SR.assert_lists_equal(ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=6), first)
    after, steps2 = ctx.fetch()
    assert steps2 == steps and ctx.timing()["epochs"] == epochs
    assert np.array_equal(SR.bits(after), SR.bits(before))
    assert ctx.stations_timing() > 0.0
    # the landing table is shared with tubemap(): a smaller lattice, either module asking first, then the 13 x 9 launch again
    (hits, _, _), small = TC.small_lattice_step(ctx, lambda: _context(G, case, None), "stations")
    print(f"7 x 5 lattice, {hits.shape[0]} members: station hits {hits.sum(axis=0).tolist()}, hits on the grid {int(small['count'].sum())}")
    SR.assert_lists_equal(ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=6), first)
    after, steps2 = ctx.fetch()
    assert steps2 == steps and np.array_equal(SR.bits(after), SR.bits(before))      # (the same launch again: the same records)
    ctx.close()


def test_refusals(G):
    import ctypes
    th, ph, nt, nph = SC.lattice(**SC.PARITY_LATTICE)
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(bounces=1, calc_amp=1)
    lib = ctx.lib
    sta = np.array([[30.0, -2.0], [31.0, -3.0]])
    kw = dict(n_theta=nt, n_phi=nph, cap=4)
    hits = np.zeros((1, 2), dtype=np.uint32)

    def fetch_rc():
        return lib.geoac_fan_stations_fetch(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), None, None)

    with pytest.raises(G.GeoAcError, match="invalid.*no completed launch"):
        ctx.stations(sta=sta, **kw)
    ctx.set_angles(th, ph)
    ctx.launch()
    assert fetch_rc() == -1                                                         # a launch alone makes no lists
    want = ctx.stations(sta=sta, **kw)
    assert fetch_rc() == 0
    invalidators = [("launch", ctx.launch), ("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: _upload(ctx, [_toy(H.EQ_GLOBAL)])),
                    ("set_sources", lambda: ctx.set_sources(np.array([[0.0, 30.0, 0.0]]))), ("set_frequencies", lambda: ctx.set_frequencies([0.1]))]
    for what, act in invalidators:
        act()
        assert fetch_rc() == -1, what
        assert "invalid" in lib.geoac_strerror(-1).decode() and "fan_stations_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        if what != "launch":
            with pytest.raises(G.GeoAcError, match="invalid.*launch again"):
                ctx.stations(sta=sta, **kw)
            ctx.launch()
            assert fetch_rc() == -1, what
        SR.assert_lists_equal(ctx.stations(sta=sta, **kw), want)
    # bad specs name their fault and leave the current lists alone
    for bad, word in ((dict(kw, n_theta=nt + 1), "n_theta \\* n_phi"), (dict(kw, cap=0), "cap"), (dict(kw, cap=257), "cap"), (dict(kw, turn_tol=float("nan")), "turn_tol"),
                      (dict(kw, leg_min=2, leg_max=1), "leg_min"), (dict(kw, edge_max=-1.0), "edge_max")):
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            ctx.stations(sta=sta, **bad)
        assert fetch_rc() == 0
    # the same number of rays, not a lattice: one inclination off by an ulp; then the transposed shape
    th2 = th.copy()
    th2[nt + 2] = np.nextafter(th2[nt + 2], 90.0)
    ctx.run(th2, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*not an n_theta x n_phi lattice"):
        ctx.stations(sta=sta, **kw)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*not an n_theta x n_phi lattice"):
        ctx.stations(sta=sta, **dict(kw, n_theta=nph, n_phi=nt))
    SR.assert_lists_equal(ctx.stations(sta=sta, **kw), want)
    ctx.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        c2.stations(sta=sta, **kw)
    c2.close()


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_a_plain_context_does_not_change(G, golden, eq):
    """run() on a context that never calls the header: the golden parity records of tests/test_gpu_parity.py, under its comparison"""
    g = golden(eq)
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1, mode=0)
    rec, steps = ctx.run(g["theta"], g["phi"])
    assert steps == int(g["steps_amp1_mode0"])
    compare_records(rec, g["rec_amp1_mode0"], E=18 if eq == H.EQ_GLOBAL else 12, hidx=None if eq == H.EQ_GLOBAL else 2)
    ctx.close()


# ---- physics ----
def _phys_ctx(G):
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1, src=SC.PHYS_SRC)
    return ctx


def _phys_estimates(G, fan_kw):
    ctx = _phys_ctx(G)
    th, ph, nt, nph = SC.lattice(**fan_kw)
    rec = ctx.run(th, ph)[0][None]
    sta = SC.ring_stations()
    sp = SR.spec(nt, nph, phi_periodic=True, cap=16)
    hits, rows, _ = ctx.stations(sta=sta, **sp)
    mis = SC.relaunch_misses(H.EQ_GLOBAL, hits, rows, rec, sp, sta, lambda a, b: ctx.run(a, b)[0])
    ctx.close()
    return hits, rows, mis


def test_physics_relaunch_lands_inside_the_triangle(G):
    """GEOAC_EQ_GLOBAL, ToyAtmo, source (0, 30, 0), one bounce, the 0.5 x 1 degree fan over the whole azimuth circle (phi_periodic), 16 neighbouring
    stations of the 2.5-degree, 64-position ring (positions 40 .. 55, where ToyAtmo's westward duct lands).  Every estimate's (THETA, PHI) is integrated as a second fan: on the estimate's leg the re-launched ray must land no farther
    from the station than the longest side of the estimate's landing triangle (a worse miss means the interpolation left its own triangle); a
    re-launched ray whose leg is not VALID is left out, at most 1 estimate in 10.
    Fan and stations were fixed after running this fan on the CPU with the plain-C oracle and tests/station_reference.py for all 64 ring positions:
    positions 38 .. 58 have estimates (25 in all, 15 of them at the stations taken here), every one re-launched VALID in the oracle, and the
    largest miss at these stations was 0.135 of the longest side (profiles/stations_accuracy.txt)."""
    hits, rows, mis = _phys_estimates(G, SC.PHYS_FAN)
    assert len(mis) >= 8, "too few estimates for the check to mean anything"
    valid = mis[:, 2] != 0
    worst = float((mis[valid, 0] / mis[valid, 1]).max())
    print(f"re-launch: {len(mis)} estimates at {int((hits[0] > 0).sum())} of 16 stations, {int((~valid).sum())} not VALID again, largest miss / longest side {worst:.4f}, "
          f"median miss {np.median(mis[valid, 0]):.3e} deg")
    assert int((~valid).sum()) * 10 <= len(mis)
    assert (mis[valid, 0] <= mis[valid, 1]).all()


def test_physics_convergence_with_both_steps_halved(G):
    """the same case with both lattice steps halved: the median re-launch miss must fall by at least 2x (a second-order interpolant predicts 4x; the
    margin is for triangles near caustics).  On the CPU oracle with tests/station_reference.py the medians at these stations were 1.792e-2 and 3.81e-3 degrees,
    a ratio of 4.70 (5.5 over all 64 ring positions), before the stations were fixed (profiles/stations_accuracy.txt)."""
    _, _, coarse = _phys_estimates(G, SC.PHYS_FAN)
    _, _, fine = _phys_estimates(G, SC.PHYS_FAN_HALF)
    mc, mf = (float(np.median(m[m[:, 2] != 0, 0])) for m in (coarse, fine))
    line = f"median re-launch miss [deg]: 0.5 x 1 deg fan {mc:.6e} ({len(coarse)} estimates), 0.25 x 0.5 deg fan {mf:.6e} ({len(fine)} estimates), ratio {mc / mf:.3f}"
    print(line)
    out = os.environ.get("GEOAC_STATIONS_ACCURACY_OUT")
    if out:
        open(out, "a").write(line + "\n")
    assert mc / mf >= 2.0


# ring positions of config 5 whose reference eigenrays are taken (tests/golden/cli/, GeoAcGlobal.RngDep -eig_search): the positions 42 .. 58 that
# have any.  Positions 38 .. 41 are left out: each holds a pair of eigenrays 0.002 - 0.01 degrees apart in inclination, a fold inside one
# lattice cell, which a first-order estimate from the cell's corners cannot resolve.
EIG_POSITIONS = [42, 44, 45, 46, 47, 48, 49, 50, 52, 53, 54, 55, 56, 57, 58]
EIG_FAN = dict(theta_min=0.5, theta_max=45.0, theta_step=0.5, phi_min=-150.0, phi_max=-28.0, phi_step=1.0)
EIG_UNMATCHED = []                                                                # (position, theta) of eigenrays known to go unmatched: none


def test_physics_reference_eigenrays_have_a_station_row(G, tmp_path):
    """the receivers of the golden config-5 eigenray fixtures: for every eigenray the reference found whose inclination lies inside the fan's range
    there must be a station row on the same leg with |THETA - theta_eig| <= one inclination step and |PHI - phi_eig| <= one azimuth step (both lie in
    the same lattice triangle).  turn_tol = edge_max = +inf.  At most 1 eigenray in 10 may go unmatched (folds inside a cell)."""
    import rngdep_data as RD
    ctx = G.FanContext(G.EQ_GLOBAL_RNGDEP, device=0)
    ctx.load_grid(*RD.write_grid_global(str(tmp_path), short_paths=False))
    ctx.set_params(src=(0.0, 31.0, 0.0), bounces=2, calc_amp=1)
    th, ph, nt, nph = SC.lattice(**EIG_FAN)
    ctx.run(th, ph)
    rc = ring_receivers()
    hits, rows, _ = ctx.stations(sta=rc[EIG_POSITIONS], n_theta=nt, n_phi=nph, cap=32)
    n_eig, unmatched = 0, []
    for k, p in enumerate(EIG_POSITIONS):
        for e in parse_eig_results(os.path.join(H.GOLDEN_DIR, "cli", ring_golden_name(p), "g_results.dat")):
            if not (th.min() <= e["theta"] <= th.max()):
                continue
            n_eig += 1
            r = rows[0, k, :min(int(hits[0, k]), 32)]
            ok = (r[:, S["LEG"]] == e["bounces"]) & (np.abs(r[:, S["THETA"]] - e["theta"]) <= EIG_FAN["theta_step"]) & (np.abs(r[:, S["PHI"]] - e["phi"]) <= EIG_FAN["phi_step"])
            if not ok.any():
                unmatched.append((p, e["theta"]))
    print(f"{n_eig} reference eigenrays at {len(EIG_POSITIONS)} receivers, unmatched: {unmatched}")
    assert n_eig >= 15
    assert len(unmatched) * 10 <= n_eig
    assert sorted(unmatched) == sorted(EIG_UNMATCHED)
    ctx.close()
