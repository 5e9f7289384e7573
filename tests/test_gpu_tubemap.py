"""Tube maps on the device (include/geoac_tubemap.h, FanContext.tubemap).  The main check is equivalence with merged code: every layer equals,
bit for bit, the reduction (tests/tubemap_reference.py) of FanContext.stations at the cell centres with cap = 256, and the numpy restatement on
the fetched records.  Then repeated calls, invalidation and refusals, and what the map is for: coverage against the point-binned map, and the
one-cell maps at the ring stations.  Cases and grids: tests/tubemap_cases.py (proved non-vacuous on the CPU oracle in tests/test_tubemap_host.py).
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import map_cases as MC
import map_reference as MR
import station_cases as SC
import station_reference as SR
import test_gpu_globalrd as TGG
import test_gpu_rngdep as TGR
import tubemap_cases as TC
import tubemap_reference as TR
from test_gpu_ensemble import _device_arrays
from test_gpu_sources import _toy, _upload

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


def _launch(G, L, tmpdir):
    """a launch of tests/tubemap_cases.py: context (left open), records [M][n_rays][legs][32], angles, lattice shape"""
    eq, kind, prm = L["eq"], L["kind"], L["params"]
    th, ph, nt, nph = TC.lattice_of(L)
    if kind in ("3drd", "globalrd"):
        ctx = (TGR if kind == "3drd" else TGG)._ctx(MC.write_grid(kind, str(tmpdir)), **prm)
    elif kind == "gridens":
        ctx = G.FanContext(eq, device=0)
        ctx.member_files = TC.write_grid_members(str(tmpdir))                        # (kept for the per-member check: written once)
        ctx.load_grid_ensemble(ctx.member_files)
        ctx.set_params(**prm)
    else:
        ctx = G.FanContext(eq, device=0)
        _upload(ctx, [_toy(eq) if raw is None else _device_arrays(eq, *raw) for raw in TC.profiles_of(L)])
        ctx.set_params(**prm)
        if kind == "sources":
            ctx.set_sources(L["sources"])
        if kind == "freqs":
            ctx.set_frequencies(L["freqs"])
    rec, _ = ctx.run(th, ph)
    return ctx, rec.reshape((-1,) + rec.shape[-3:]), th, ph, nt, nph


@pytest.fixture(scope="module")
def launches(G, tmp_path_factory):
    """every launch once, shared by the cases that rasterise it (a tube map does not change its launch)"""
    made = {}

    def get(name):
        if name not in made:
            ctx, rec, th, ph, nt, nph = _launch(G, TC.LAUNCHES[name], tmp_path_factory.mktemp(name))
            made[name] = (ctx, rec, th, ph, nt, nph, ctx.fetch_level())
        return made[name]

    yield get
    for v in made.values():
        v[0].close()


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_layers_equal_the_station_lists_at_the_centres(G, launches, name):
    case = TC.CASES[name]
    eq = TC.LAUNCHES[case["launch"]]["eq"]
    ctx, rec, th, ph, nt, nph, level = launches(case["launch"])
    sp = TC.spec_of(case, nt, nph)
    got = ctx.tubemap(**sp)
    stats = ctx.tubemap_stats()
    M, F = rec.shape[0], level.shape[1]
    assert got["count"].shape == (M,) + sp["n"] and got["best"].shape == (M, F) + sp["n"]
    # the merged station code at the cell centres, every hit kept
    hits, rows, lvl = ctx.stations(sta=TR.centres(sp), **TR.station_spec_of(sp))
    most = int(hits.max())
    print(f"{name}: M {M} F {F} cells {sp['n']} hits in all {int(got['count'].sum())}, most at one centre {most}, walk {stats}")
    assert most <= TR.CAP                                                           # (so the cap cannot hide a difference)
    TR.assert_layers_equal(got, TR.reduce_lists(hits, rows, lvl, sp), name + " against stations()")
    TR.assert_layers_equal(got, TR.reference_tubemap(eq, rec, th, ph, level, sp), name + " against the restatement")
    TR.check_non_vacuity(got, name)
    assert stats["triangles"] > 0 and stats["candidates"] >= int(got["count"].sum())
    if case.get("cooperative"):
        assert stats["cooperative"] > 0 and stats["candidates"] > G.TUBE_COOP_MIN * stats["cooperative"]
    if F > 1:
        assert not np.array_equal(got["level_max"][0, 0], got["level_max"][0, F - 1])
    if "detect" in got:
        assert got["detect"].max() >= 1
    if TC.LAUNCHES[case["launch"]]["kind"] == "gridens":
        _members_equal_plain_contexts(G, case, ctx.member_files, got, th, ph, sp)


def _members_equal_plain_contexts(G, case, files, got, th, ph, sp):
    """a grid ensemble: every member's layers are those of a plain context holding that member's grid (one lane per ray, as the ensemble integrates)"""
    L = TC.LAUNCHES[case["launch"]]
    assert got["count"].shape[0] == len(files) == 2
    for m, f in enumerate(files):
        with G.options(GRID_LANES="1"):
            ctx = G.FanContext(L["eq"], device=0)
        ctx.load_grid(*f)
        ctx.set_params(**L["params"])
        ctx.run(th, ph)
        want = ctx.tubemap(**dict(sp, detect_db=np.nan))
        ctx.close()
        for name in want:
            assert np.array_equal(SR.bits(got[name][m]), SR.bits(want[name][0])), (m, name)
    assert not np.array_equal(SR.bits(got["ttime_min"][0]), SR.bits(got["ttime_min"][1]))          # (the members are different atmospheres)


def test_filters_only_remove_hits(G, launches):
    ctx, rec, th, ph, nt, nph, level = launches("global")
    full = ctx.tubemap(**TC.spec_of(TC.CASES["global"], nt, nph))["count"]
    for name in ("leg-band", "turn-band", "edge-max"):
        part = ctx.tubemap(**TC.spec_of(TC.CASES[name], nt, nph))["count"]
        assert (part <= full).all() and int(part.sum()) < int(full.sum()), name
    lo = ctx.tubemap(**TC.spec_of(TC.CASES["global"], nt, nph, turn_min=-np.inf, turn_max=60.0))["count"]
    hi = ctx.tubemap(**TC.spec_of(TC.CASES["turn-band"], nt, nph))["count"]
    assert np.array_equal(lo + hi, full) and int(lo.sum()) > 0 and int(hi.sum()) > 0    # the band separates the two families, every hit is in one


def test_repeated_calls_invalidation_and_refusals(G):
    L = TC.LAUNCHES["global"]
    th, ph, nt, nph = TC.lattice_of(L)
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(**L["params"])
    lib = ctx.lib
    sp = TC.spec_of(TC.CASES["global"], nt, nph)
    count = np.zeros(sp["n"], dtype=np.uint64)

    def fetch_rc():
        return lib.geoac_fan_tubemap_fetch(ctx._h, 0, count.ctypes.data_as(ctypes.c_void_p))

    with pytest.raises(G.GeoAcError, match="invalid.*no completed launch"):
        ctx.tubemap(**sp)
    ctx.set_angles(th, ph)
    ctx.launch()
    before, steps = ctx.fetch()
    assert fetch_rc() == -1                                                         # a launch alone makes no tube map
    want = ctx.tubemap(**sp)
    assert fetch_rc() == 0 and ctx.tubemap_timing() > 0.0
    TR.assert_layers_equal(ctx.tubemap(**sp), want, "second call")                  # two calls, identical bits
    other = ctx.tubemap(**TC.spec_of(TC.CASES["coarse"], nt, nph))                  # a second spec replaces the first
    assert other["count"].shape == (1,) + TC.GRID_COARSE["n"] and "detect" not in other
    M, F, n0, n1 = (ctypes.c_int(0) for _ in range(4))
    assert lib.geoac_fan_tubemap_shape(ctx._h, *[ctypes.byref(v) for v in (M, F, n0, n1)]) == 0 and (n0.value, n1.value) == TC.GRID_COARSE["n"]
    assert lib.geoac_fan_tubemap_fetch_detect(ctx._h, count.ctypes.data_as(ctypes.c_void_p)) == -1
    TR.assert_layers_equal(ctx.tubemap(**sp), want, "back to the first spec")
    ctx.map(origin=sp["origin"], step=sp["step"], n=sp["n"])                        # the arrival map and the station lists stay their own
    ctx.stations(sta=TR.centres(sp)[:5], n_theta=nt, n_phi=nph)
    assert fetch_rc() == 0
    after, steps2 = ctx.fetch()
    assert steps2 == steps and np.array_equal(SR.bits(after), SR.bits(before))      # the launch is left alone
    invalidators = [("launch", ctx.launch), ("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: _upload(ctx, [_toy(H.EQ_GLOBAL)])),
                    ("set_sources", lambda: ctx.set_sources(np.array([[0.0, 30.0, 0.0]]))), ("set_frequencies", lambda: ctx.set_frequencies([0.1]))]
    for what, act in invalidators:
        act()
        assert fetch_rc() == -1, what
        assert "fan_tubemap_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        if what != "launch":
            with pytest.raises(G.GeoAcError, match="invalid.*launch again"):
                ctx.tubemap(**sp)
            ctx.launch()
            assert fetch_rc() == -1, what
        TR.assert_layers_equal(ctx.tubemap(**sp), want, "after " + what)
    # bad specs name their fault and leave the current map alone
    for bad, word in ((dict(sp, n_theta=nt + 1), "n_theta \\* n_phi"), (dict(sp, edge_max=float("inf")), "edge_max must be finite"), (dict(sp, edge_max=180.0), "below 180"),
                      (dict(sp, step=(0.375, 10.0)), "360 degrees"), (dict(sp, step=(0.001, 0.001)), "GEOAC_TUBE_MAX_SPAN"), (dict(sp, turn_min=5.0, turn_max=5.0), "turn_min < turn_max"),
                      (dict(sp, n=(0, 4)), "at least 1"), (dict(sp, leg_min=2, leg_max=1), "leg_min")):
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            ctx.tubemap(**bad)
        assert fetch_rc() == 0
    # the same number of rays, not a lattice: one inclination off by an ulp; then the transposed shape
    th2 = th.copy()
    th2[nt + 2] = np.nextafter(th2[nt + 2], 90.0)
    ctx.run(th2, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*not an n_theta x n_phi lattice"):
        ctx.tubemap(**sp)
    assert lib.geoac_fan_tubemap(ctx._h, ctypes.byref(G.tube_spec(**sp))) == -1
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*not an n_theta x n_phi lattice"):
        ctx.tubemap(**dict(sp, n_theta=nph, n_phi=nt))
    TR.assert_layers_equal(ctx.tubemap(**sp), want, "after the refusals")

    # the landing table is shared with stations(): a smaller lattice, either module asking first, then the 13 x 9 launch again
    def make_ctx():
        c = G.FanContext(H.EQ_GLOBAL, device=0)
        _upload(c, [_toy(H.EQ_GLOBAL)])
        c.set_params(**L["params"])
        return c

    (hits, _, _), small = TC.small_lattice_step(ctx, make_ctx, "tubemap")
    print(f"7 x 5 lattice: hits on the grid {int(small['count'].sum())}, station hits {hits[0].tolist()}")
    assert small["count"].sum() > 0 and (hits > 0).any()                            # (tests/test_tubemap_host.py: so it is on the oracle's records)
    TR.assert_layers_equal(ctx.tubemap(**sp), want, "after the small lattice")
    ctx.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        c2.tubemap(**sp)
    assert c2.lib.geoac_fan_tubemap(c2._h, ctypes.byref(G.tube_spec(**sp))) == -4
    c2.close()


# ---- what the map is for ----
ANNULUS = dict(origin=(27.0, -3.0), step=(0.1, 0.1), n=(60, 60))                  # the 2.5-degree ring around (30, 0) and what it encloses
PHYS_EDGE = 2.0


def _one_cell(s):
    """origin and step of a cell whose centre is s, bit for bit: origin = s - 0.5 * step with step a power of two small enough that neither the
    subtraction nor the centre's sum rounds"""
    for k in range(4, 40):
        step = 2.0 ** -k
        origin = s - 0.5 * step
        if origin + (0 + 0.5) * step == s:
            return origin, step
    raise AssertionError(f"no power-of-two cell is centred on {s!r}")


def test_what_the_map_is_for(G):
    """GeoAcGlobal, ToyAtmo, source (0, 30, 0), one bounce (tests/station_cases.py PHYS_FAN, and PHYS_FAN_HALF with both lattice steps halved).
    Measured and recorded, not gated: the share of the cells of a 0.1-degree grid over the 2.5-degree ring's annulus with COUNT >= 1 in the tube
    map and in the point-binned arrival map on the same grid (profiles/tubemap_accuracy.txt).  Gated, exactly: a one-cell tube map whose centre
    is a ring station has that station's hits as COUNT and its smallest row TTIME as TTIME_MIN, at each of the 16 stations."""
    lines = []
    for label, fan in (("0.5 x 1 deg fan", SC.PHYS_FAN), ("0.25 x 0.5 deg fan", SC.PHYS_FAN_HALF)):
        ctx = G.FanContext(H.EQ_GLOBAL, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=1, calc_amp=1, src=SC.PHYS_SRC)
        th, ph, nt, nph = SC.lattice(**fan)
        ctx.run(th, ph)
        tube = ctx.tubemap(n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=PHYS_EDGE, **ANNULUS)["count"][0]
        binned = ctx.map(**ANNULUS)["count"][0]
        lines.append(f"{label} ({th.size} rays), {ANNULUS['n'][0]} x {ANNULUS['n'][1]} cells of {ANNULUS['step'][0]} deg: share of cells with COUNT >= 1: tube map "
                     f"{(tube >= 1).mean():.4f} (multipath cells, COUNT >= 2: {(tube >= 2).mean():.4f}), point-binned map {(binned >= 1).mean():.4f}")
        if fan is SC.PHYS_FAN:
            sta = SC.ring_stations()
            hits, rows, _ = ctx.stations(sta=sta, n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=PHYS_EDGE, cap=TR.CAP)
            assert len(sta) == 16 and int(hits.sum()) >= 8 and int(hits.max()) <= TR.CAP
            for r, s in enumerate(sta):
                (o0, s0), (o1, s1) = _one_cell(float(s[0])), _one_cell(float(s[1]))
                one = ctx.tubemap(origin=(o0, o1), step=(s0, s1), n=(1, 1), n_theta=nt, n_phi=nph, phi_periodic=True, edge_max=PHYS_EDGE)
                n = int(hits[0, r])
                assert int(one["count"][0, 0, 0]) == n, (r, s, int(one["count"][0, 0, 0]), n)
                want = MR.unkey(MR.key(rows[0, r, :n, S["TTIME"]]).min(keepdims=True))[0] if n else np.inf
                assert SR.bits(one["ttime_min"])[0, 0, 0] == SR.bits(np.array([want]))[0], (r, s, float(one["ttime_min"][0, 0, 0]), want)
            lines.append(f"{label}: one-cell tube maps at the 16 ring stations: COUNT = hits and TTIME_MIN = smallest row TTIME at all 16 ({int(hits.sum())} hits at "
                         f"{int((hits[0] > 0).sum())} stations)")
        ctx.close()
    print("\n".join(lines))
    out = os.environ.get("GEOAC_TUBEMAP_ACCURACY_OUT")
    if out:
        open(out, "a").write("\n".join(lines) + "\n")
