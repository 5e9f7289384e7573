"""Arrival maps on the device (include/geoac_map.h, FanContext.map): every layer against the numpy restatement (tests/map_reference.py) of the
same launch's fetched records, attenuation table and level table, bit for bit; the level table against numpy's log10 under the project's value
rule; filters, wrap, contention, determinism, isolation from the launch, refusals and clones.  Launch helpers, sources, frequencies and profile
members are those of the ensemble, source-set and frequency-set tests; the range-dependent cases build their grids of profiles as
test_gpu_rngdep / test_gpu_globalrd do (rngdep_data) and use their context builders."""
import numpy as np
import pytest

import harness as H
import map_cases as MC
import map_reference as MR
import test_gpu_globalrd as TGG
import test_gpu_rngdep as TGR
from parity import RTOL
from test_gpu_ensemble import _angles, _device_arrays, _raw_members
from test_gpu_sources import SOURCES, _toy, _upload

pytestmark = pytest.mark.gpu

LEVEL_FLOOR_DB = 1e-9                 # absolute floor of the level comparison, for levels near zero


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _launch(G, case, tmpdir):
    """the case's launch: context (left open), records as [M][n_rays][legs][32], attenuation table [F][n_rays][legs]"""
    eq, kind, prm = case["eq"], case["kind"], case["params"]
    th, ph = MC.case_angles(case)
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
    rec, _ = ctx.run(th, ph)
    rec = rec.reshape((-1,) + rec.shape[-3:])
    atten = ctx.fetch_atten() if rec.shape[0] == 1 else rec[0, :, :, H.REC["ATTEN"]][None]
    return ctx, rec, atten


def _map_and_reference(G, ctx, eq, rec, spec_kw):
    """device map and reference map of the same launch under one spec"""
    level = ctx.fetch_level()
    got = ctx.map(**spec_kw)
    sp = MR.spec(**spec_kw)
    ref = MR.reference_map(eq, rec, level, sp)
    MR.assert_maps_equal(got, ref)
    return got, ref, sp, level


def _check_level(level, rec, atten, calc_amp):
    """NaN exactly where VALID is 0; elsewhere numpy's (calc_amp ? 20 log10(AMP) : 0) - atten[f] to RTOL with a 1e-9 dB floor; returns the worst difference"""
    valid = rec[..., H.REC["VALID"]] != 0.0
    want = MR.level_numpy(rec, atten, calc_amp)
    assert level.shape == want.shape
    worst = 0.0
    for f in range(level.shape[1]):
        got_f, want_f = level[:, f], want[:, f]
        assert np.array_equal(np.isnan(got_f), ~valid), "level is not NaN exactly where VALID is 0"
        fin = valid & np.isfinite(want_f)
        assert np.array_equal(got_f[valid & ~fin].view(np.uint64), want_f[valid & ~fin].view(np.uint64))        # (-inf for a zero amplitude)
        d = np.abs(got_f[fin] - want_f[fin])
        worst = max(worst, float(d.max()) if d.size else 0.0)
        assert (d <= np.maximum(RTOL * np.abs(want_f[fin]), LEVEL_FLOOR_DB)).all(), f"frequency {f}: level off by up to {d.max()} dB"
    return worst


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_map_equals_reference(G, name, tmp_path):
    case = MC.CASES[name]
    ctx, rec, atten = _launch(G, case, tmp_path)
    M = rec.shape[0]
    got, ref, sp, level = _map_and_reference(G, ctx, case["eq"], rec, case["spec"])
    F = len(case.get("freqs", [0]))
    assert got["level_max"].shape == (M, F) + tuple(sp["n"]) and got["detect"].shape == (F,) + tuple(sp["n"])
    MR.check_non_vacuity(ref, sp, M)
    # bookkeeping: every filtered VALID arrival is in a cell or in `outside`
    assert int(got["count"].sum()) + int(got["outside"].sum()) == int((rec[..., 0] != 0).sum()) == ref["n_pass"]
    worst = _check_level(level, rec, atten, case["params"]["calc_amp"])
    print(f"{name}: M {M} F {F} arrivals {ref['n_pass']} inside {int(got['count'].sum())} fullest cell {int(got['count'].max())} "
          f"worst level difference to numpy {worst:.3e} dB")
    if F > 1:
        # column f of the level table is built from row f of the attenuation table (_check_level), and the rows differ
        assert all(not np.array_equal(atten[f], atten[0]) for f in range(1, F))
        assert not np.array_equal(got["level_max"][0, 0], got["level_max"][0, F - 1])
    ctx.close()


def test_turning_height_bands_partition_the_count(G):
    case = MC.CASES["plain-global-amp1-b2"]
    ctx, rec, _ = _launch(G, case, None)
    grid = {k: v for k, v in case["spec"].items() if k != "detect_db"}
    whole, _, _, _ = _map_and_reference(G, ctx, case["eq"], rec, grid)
    bands = [(-np.inf, 60.0), (60.0, 125.0), (125.0, np.inf)]          # stratospheric, mesospheric and thermospheric returns
    parts = [_map_and_reference(G, ctx, case["eq"], rec, dict(grid, turn_min=a, turn_max=b))[0] for a, b in bands]
    assert all(int(p["count"].sum()) > 0 for p in parts)
    assert np.array_equal(sum(p["count"] for p in parts), whole["count"])
    assert sum(int(p["outside"][0]) for p in parts) == int(whole["outside"][0])
    ctx.close()


def test_leg_filters_and_best(G):
    case = MC.CASES["plain-3d-amp1-b2"]
    ctx, rec, _ = _launch(G, case, None)
    legs = rec.shape[2]
    grid = {k: v for k, v in case["spec"].items() if k != "detect_db"}
    total = 0
    for leg in range(legs):
        got, ref, sp, level = _map_and_reference(G, ctx, case["eq"], rec, dict(grid, leg_min=leg, leg_max=leg))
        only = np.zeros_like(rec)
        only[:, :, leg] = rec[:, :, leg]                                # the same launch with every other leg blanked out
        lv_only = np.full_like(level, np.nan)
        lv_only[..., leg] = level[..., leg]
        MR.assert_maps_equal(got, MR.reference_map(case["eq"], only, lv_only, MR.spec(**grid)))
        assert int(got["count"].sum()) + int(got["outside"][0]) == int((rec[0, :, leg, 0] != 0).sum())
        total += int(got["count"].sum())
        # BEST names a record of this leg whose level is the cell's LEVEL_MAX and whose cell is that cell
        cell = MR.cells(case["eq"], rec, sp)[0].reshape(-1)
        best, lmax = got["best"][0, 0].reshape(-1), got["level_max"][0, 0].reshape(-1)
        filled = np.flatnonzero(best >= 0)
        assert filled.size > 0 and np.array_equal(best < 0, np.isneginf(lmax))
        assert (best[filled] % legs == leg).all()
        assert np.array_equal(level[0, 0].reshape(-1)[best[filled]].view(np.uint64), lmax[filled].view(np.uint64))
        assert np.array_equal(cell[best[filled]], filled)
    whole = ctx.map(**grid)
    assert total == int(whole["count"].sum())
    ctx.close()


def test_wrap_lon(G):
    """a fan from lon 179.5 whose eastbound rays cross the date line.  The state's longitude is continuous (the arrivals lie at 164 .. 190 deg), so on
    a grid with origin[1] = 0 the wrap has nothing to move - map and reference agree, nothing is outside with or without it; on the grid from -180
    the arrivals beyond 180 deg are inside with wrap_lon and counted in `outside` without it."""
    th, ph = _angles()
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(bounces=2, calc_amp=1, src=MC.WRAP_SRC)
    rec = ctx.run(th, ph)[0][None]
    lon = np.degrees(rec[0, :, :, 14])
    beyond = int(((lon >= 180.0) & (rec[0, :, :, 0] != 0)).sum())
    assert beyond >= 10
    for grid in (MC.WRAP_GRID_0, MC.WRAP_GRID_180):
        got, ref, sp, _ = _map_and_reference(G, ctx, H.EQ_GLOBAL, rec, dict(grid, wrap_lon=True))
        MR.check_non_vacuity(ref, sp, 1)
        assert got["outside"].tolist() == [0]
    got, _, _, _ = _map_and_reference(G, ctx, H.EQ_GLOBAL, rec, dict(MC.WRAP_GRID_180))
    assert got["outside"].tolist() == [beyond]
    wrapped = ctx.map(wrap_lon=True, **MC.WRAP_GRID_180)
    assert int(wrapped["count"].sum()) == int(got["count"].sum()) + beyond
    assert int(wrapped["count"][0, :, :20].sum()) == beyond            # they land in lon -180 .. -170
    ctx.close()


def test_contention_one_cell(G):
    """4 096 identical rays: every arrival of a leg competes for one cell"""
    n = 4096
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(bounces=0, calc_amp=1)
    rec = ctx.run(np.full(n, 12.0), np.full(n, -90.0))[0][None]
    assert (rec[0, :, 0, 0] != 0).all()
    assert (rec[0].view(np.uint64) == rec[0, :1].view(np.uint64)).all()
    got, ref, sp, _ = _map_and_reference(G, ctx, H.EQ_GLOBAL, rec, dict(MC.GRID_GLOBAL, detect_db=-200.0))
    assert int((got["count"] != 0).sum()) == 1 and int(got["count"].max()) == n and got["outside"].tolist() == [0]
    assert got["best"][got["best"] >= 0].tolist() == [0] and int(got["detect"].sum()) == 1
    ctx.close()


def test_determinism_and_isolation(G):
    case = MC.CASES["ensemble3-global"]
    ctx, rec, _ = _launch(G, case, None)
    epochs, steps = ctx.timing()["epochs"], ctx.total_steps()
    a = ctx.map(**case["spec"])
    b = ctx.map(**case["spec"])
    MR.assert_maps_equal(a, b)
    assert np.array_equal(a["detect"], b["detect"])
    # another spec on the same launch: no new integration
    other = dict(origin=(25.0, -10.0), step=(1.0, 2.0), n=(12, 8), turn_min=60.0, turn_max=np.inf, detect_db=-75.0)
    _map_and_reference(G, ctx, case["eq"], rec, other)
    assert ctx.timing()["epochs"] == epochs and ctx.total_steps() == steps
    MR.assert_maps_equal(ctx.map(**case["spec"]), a)
    # the records are untouched
    again, steps2 = ctx.fetch()
    assert steps2 == steps and np.array_equal(again.reshape(rec.shape).view(np.uint64), rec.view(np.uint64))
    # a second launch gives the same map bits
    rec2 = ctx.run(*_angles())[0]
    assert np.array_equal(rec2.reshape(rec.shape).view(np.uint64), rec.view(np.uint64))
    MR.assert_maps_equal(ctx.map(**case["spec"]), a)
    ctx.close()


def test_refusals(G):
    import ctypes
    th, ph = _angles()
    spec = dict(MC.GRID_GLOBAL)
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(bounces=1, calc_amp=1)
    lib, buf = ctx.lib, np.zeros(44 * 54, dtype=np.uint64)

    def fetch_rc():
        return lib.geoac_fan_map_fetch(ctx._h, G.MAP_COUNT, buf.ctypes.data_as(ctypes.c_void_p))

    with pytest.raises(G.GeoAcError, match="no completed launch"):
        ctx.map(**spec)                                                 # before any launch
    with pytest.raises(G.GeoAcError, match="no completed launch"):
        ctx.fetch_level()
    ctx.set_angles(th, ph)
    with pytest.raises(G.GeoAcError, match="no completed launch"):
        ctx.map(**spec)                                                 # angles alone are not a launch
    ctx.launch()
    want = ctx.map(**spec)
    assert fetch_rc() == 0
    # each of these invalidates the map; the context maps again after the next launch
    invalidators = [("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: _upload(ctx, [_toy(H.EQ_GLOBAL)])),
                    ("set_sources", lambda: ctx.set_sources(np.array([[0.0, 30.0, 0.0]]))), ("set_frequencies", lambda: ctx.set_frequencies([0.1]))]
    for what, act in invalidators:
        act()
        assert fetch_rc() == -1, what
        msg = lib.geoac_last_error(ctx._h).decode()
        assert "no completed launch" in msg and "launch again" in msg, (what, msg)
        with pytest.raises(G.GeoAcError, match="launch again"):
            ctx.map(**spec)
        ctx.launch()
        assert fetch_rc() == -1, what                                   # (a new launch: the old map is gone until geoac_fan_map runs again)
        MR.assert_maps_equal(ctx.map(**spec), want)
    # bad specs name their fault and leave the current map alone
    for bad, word in ((dict(spec, step=(0.0, 0.5)), "step"), (dict(spec, n=(0, 5)), "n must be"), (dict(spec, n=(4096, 4097)), "2\\^24"),
                      (dict(spec, leg_min=3, leg_max=1), "leg_min"), (dict(spec, turn_min=float("nan")), "turn")):
        with pytest.raises(G.GeoAcError, match=word):
            ctx.map(**bad)
        assert fetch_rc() == 0
    ctx.map(**spec)                                                     # made without a threshold: there is no detection map to fetch
    assert lib.geoac_fan_map_fetch_detect(ctx._h, buf.ctypes.data_as(ctypes.c_void_p)) == -1
    assert "detect_db" in lib.geoac_last_error(ctx._h).decode()
    assert fetch_rc() == 0
    ctx.close()
    c3 = G.FanContext(H.EQ_3D, device=0)
    _upload(c3, [_toy(H.EQ_3D)])
    c3.set_params(bounces=1, calc_amp=1)
    c3.run(th, ph)
    with pytest.raises(G.GeoAcError, match="wrap_lon"):
        c3.map(wrap_lon=True, **MC.GRID_3D)
    assert int(c3.map(**MC.GRID_3D)["count"].sum()) > 0                 # still usable
    c3.close()


def test_clone_maps_its_own_launch(G):
    th, ph = _angles()
    ctx = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ctx, [_toy(H.EQ_GLOBAL)])
    ctx.set_params(bounces=2, calc_amp=1)
    rec = ctx.run(th, ph)[0][None]
    clone = ctx.clone()
    with pytest.raises(G.GeoAcError, match="no completed launch"):
        clone.map(**MC.GRID_GLOBAL)
    rec_c = clone.run(th[:40], ph[:40])[0][None]
    _map_and_reference(G, clone, H.EQ_GLOBAL, rec_c, dict(MC.GRID_GLOBAL, detect_db=-70.0))
    got, _, _, _ = _map_and_reference(G, ctx, H.EQ_GLOBAL, rec, dict(MC.GRID_GLOBAL, detect_db=-70.0))
    assert int(got["count"].sum()) > int(clone.map(**MC.GRID_GLOBAL)["count"].sum()) > 0
    clone.close()
    ctx.close()
