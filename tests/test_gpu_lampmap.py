"""Level loudness maps on the device (include/geoac_lampmap.h, FanContext.level_ampmap).  The main check is bit equality with the numpy
restatement (tests/lampmap_reference.py) - on the device's own level-station lists at the cell centres and on the fetched crossing records alone, the
medium taken through the public probe calls.  Then the layers' own rules, the closed form and the reference's Jacobian amplitude (bounds and caps:
tests/lampmap_cases.py, proved and measured on the CPU in tests/test_lampmap_host.py), members, det_floor, launch plans, lifecycle and refusals.
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried).

Measured on an MI355X: see the figures each test prints."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import lampmap_cases as LC
import lampmap_reference as LM
import level_amp_reference as LA
import lstation_reference as LS
import ltubemap_cases as LTC
import ltubemap_reference as LT
import raised_ground as RGD
import rngdep_data as RD
import station_reference as SR
import test_gpu_ltubemap as TGL
from test_gpu_ensemble import _device_arrays, _raw_members
from test_gpu_sources import _toy, _upload

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 300
ALL = dict(level_mask=0b111, ord_max=2)
# a 9 x 7 cell grid over the crossings of the 12 x 8 (6 x 5) lattices of tests/ltubemap_cases.py, and a grid whose cells are several times smaller than
# the crossing triangles (31 x 29: odd sizes), so that triangles take the cooperative walk
GRIDS = {
    "3d": (dict(origin=(-312.0, -180.0), step=(34.0, 51.0), n=(9, 7), edge_max=120.0), dict(origin=(-300.0, -100.0), step=(6.5, 6.5), n=(31, 29), edge_max=120.0)),
    "global": (dict(origin=(28.2, -3.3), step=(0.4, 0.49), n=(9, 7), edge_max=1.2), dict(origin=(29.0, -3.2), step=(0.0625, 0.0625), n=(31, 29), edge_max=1.2)),
    "3drd": (dict(origin=(-312.0, -180.0), step=(34.0, 51.0), n=(9, 7), edge_max=160.0), dict(origin=(-300.0, -100.0), step=(6.5, 6.5), n=(31, 29), edge_max=160.0)),
}


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


@pytest.fixture(scope="module")
def launches(G, tmp_path_factory):
    """every launch of tests/ltubemap_cases.py once, shared by the cases that map it (a loudness map does not change its launch)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = TGL._launch(G, LTC.LAUNCHES[name], tmp_path_factory.mktemp(name))
        return made[name]

    yield get
    for v in made.values():
        v[0].close()


def _spec(name, which, nt, nph, **kw):
    return LM.spec(n_theta=nt, n_phi=nph, **dict(GRIDS[name][which], **dict(ALL, **kw)))


def _lists_at_centres(ctx, sp):
    sta, lv = LT.stations_of(sp)
    return ctx.level_stations(sta=sta, level_of=lv, **LT.lstation_spec_of(sp))


def _src3(ctx):
    return [list(ctx.params.src)]


def _with_detect(ctx, sp):
    """the map once without a DETECT layer, then again with detect_amp at the median RAMP_MAX of the reached cells: (spec, layers)"""
    first = ctx.level_ampmap(**dict(sp, detect_amp=float("nan")))
    assert first["detect"] is None and int((first["count"] > 0).sum()) >= 10
    sp2 = dict(sp, detect_amp=float(np.median(first["ramp_max"][first["count"] > 0])))
    got = ctx.level_ampmap(**sp2)
    for name in ("count", "weak", "amp_max", "ramp_max", "loudest"):
        assert _same_bits(got[name], first[name]), name
    return sp2, got


def _same_bits(a, b):
    return np.array_equal(SR.bits(a), SR.bits(b))


# ---------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("name", ["3d", "global", "3drd"])
@pytest.mark.parametrize("which", [0, 1], ids=["9x7", "fine"])
def test_layers_equal_the_restatement(G, launches, name, which):
    eq = LTC.LAUNCHES[name]["eq"]
    ctx, count, lrec, th, ph, nt, nph, legs = launches(name)
    n_cells = (nt - 1) * (nph - 1)
    assert (count.shape[0] * 3 * (legs * 2 * 2) * n_cells) % 64 != 0                  # the walk's items do not fill its last wave
    sp, got = _with_detect(ctx, _spec(name, which, nt, nph))
    stats = ctx.level_ampmap_stats()
    assert got["count"].shape == (1, 3) + sp["n"] and got["detect"].shape == (3,) + sp["n"] and ctx.level_ampmap_timing() > 0.0
    media = [LA.medium_of_context(ctx)]
    levels = LTC.LAUNCHES[name].get("levels", LTC.LEVELS)
    hits, rows = _lists_at_centres(ctx, sp)
    assert int(hits.max()) <= LT.CAP
    want = LM.reduce_lists(eq, hits, rows, count, lrec, th, ph, legs, sp, levels, media, _src3(ctx))
    print(f"{name} {sp['n']}: usable hits {int(got['count'].sum())}, weak {int(got['weak'].sum())}, cells reached {int((got['count'] > 0).sum())}, DETECT cells "
          f"{int(got['detect'].sum())}, AMP_MAX {got['amp_max'][got['count'] > 0].min():.3e} .. {got['amp_max'].max():.3e}, walk {stats}")
    LM.assert_layers_equal(got, want, f"{name} against the restatement on level_stations()")
    LM.assert_layers_equal(got, LM.reference_level_ampmap(eq, count, lrec, th, ph, legs, sp, levels, media, _src3(ctx)), f"{name} against the restatement")
    assert int(got["count"].sum()) >= 20 and int((got["count"] == 0).sum()) > 0 and 0 < int(got["detect"].sum()) <= int((got["count"] > 0).sum())
    assert stats["triangles"] > 0 and stats["candidates"] >= int(got["count"].sum() + got["weak"].sum())
    if which == 1:
        assert stats["cooperative"] > 0 and stats["candidates"] > G.TUBE_COOP_MIN * stats["cooperative"]
        seen = {}
        try:
            for t in (0, 2**31 - 1):
                os.environ["GEOAC_LTUBE_COOP"] = str(t)
                LM.assert_layers_equal(ctx.level_ampmap(**sp), got, f"{name} threshold {t}")
                seen[t] = ctx.level_ampmap_stats()
        finally:
            os.environ.pop("GEOAC_LTUBE_COOP", None)
        assert seen[0]["cooperative"] == seen[0]["triangles"] and seen[2**31 - 1]["cooperative"] == 0 and seen[0]["candidates"] == seen[2**31 - 1]["candidates"]


# ---------------------------------------------------------------- 2. the layers' own rules
@pytest.mark.parametrize("name", ["global", "3drd"])
def test_count_weak_loudest_and_the_station_rows(G, launches, name):
    eq = LTC.LAUNCHES[name]["eq"]
    ctx, count, lrec, th, ph, nt, nph, legs = launches(name)
    sp = _spec(name, 0, nt, nph)
    got = ctx.level_ampmap(**sp)
    tube = ctx.level_tubemap(**LM.ltube_spec_of(sp))
    assert np.array_equal(got["count"] + got["weak"], tube["count"]) and got["detect"] is None
    hits, rows = _lists_at_centres(ctx, sp)
    h = LM.hits_of_lists(eq, hits, rows, count, lrec, th, ph, legs, sp, LTC.LAUNCHES[name].get("levels", LTC.LEVELS), [LA.medium_of_context(ctx)], _src3(ctx))
    cells = sp["n"][0] * sp["n"][1]
    word = (h["member"] * 3 + h["ls"]) * cells + h["cell"]
    loud = got["loudest"].reshape(-1)
    n = 0
    for w in np.flatnonzero(loud >= 0):
        at = np.flatnonzero((word == w) & (h["key"] == loud[w]))                        # the hit LOUDEST names is a row level_stations returns at that centre
        assert len(at) == 1 and h["usable"][at[0]], (w, loud[w])
        assert SR.bits(np.float64(got["ramp_max"].reshape(-1)[w])) == SR.bits(np.float64(h["ramp"][at[0]]))
        mine = (word == w) & h["usable"]
        assert got["amp_max"].reshape(-1)[w] == h["amp"][mine].max() and got["ramp_max"].reshape(-1)[w] == h["ramp"][mine].max()
        n += 1
    assert n >= 10 and n == int((got["count"] > 0).sum())
    assert (got["ramp_max"] <= got["amp_max"]).all() and (got["amp_max"][got["count"] == 0] == -np.inf).all() and (loud[got["count"].reshape(-1) == 0] == -1).all()


# ---------------------------------------------------------------- 3. closed form
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form_under_a_raised_ground(G, eq, tmp_path):
    """the medium of tests/raised_ground.py, levels 8 and 15 km, leg 0 downward: AMP_MAX of every cell with one hit against exp(dz / 2H) / (4 pi L) under the
    bound derived in tests/lampmap_cases.py, the one the CPU test holds the restatement to on straight-ray tables"""
    th, ph, nt, nph = RGD.lattice()
    ctx = G.FanContext(eq, device=0)
    if eq == H.EQ_3D_RNGDEP:
        ctx.load_grid(*RGD.write_uniform_grid(eq, str(tmp_path)), z_grnd=RGD.Z_GRND)
    else:
        ctx.upload_atmo_1d(*RGD.profile())
    ctx.set_params(**dict(RGD.params(eq), **RGD.LEVEL_PARAMS))
    ctx.set_levels(RGD.LEVELS)
    ctx.run(th, ph)
    sp = LC.rg_spec(eq, nt, nph)
    got = ctx.level_ampmap(**sp)
    ctx.close()
    assert int(got["weak"].sum()) == 0
    print(f"raised ground, device, {H.EQ_NAMES[eq]}, loudness map: " + LC.cf_figures(LC.check_closed_form(eq, got, sp, th, ph, nt)))


# ---------------------------------------------------------------- 4. the reference's Jacobian amplitude
@pytest.mark.parametrize("name,eq", LC.FIX_SETS)
@pytest.mark.parametrize("step", LC.FIX_STEPS)
def test_against_the_references_jacobian_amplitude(G, name, eq, step, tmp_path):
    """tests/golden/level_amp.npz: a 2 x 2 lattice about every fixture ray, a one-cell map centred on every crossing point of the compiled reference's own ray,
    restricted to the crossing's branch.  AMP_MAX against amp_jac (the cos form on the spherical set), TTIME and ATTEN of the enclosing hit's level-station row
    against the fixture's, each within twice the worst gap of the CPU chain (LC.GAP_MEASURED; the factor covers the difference between oracle and device paths
    and a lattice origin shifted within a cell); at most one eighth of the crossings left out."""
    g = np.load(LA.FIXTURE)
    ctx = G.FanContext(eq, device=0)
    if eq == H.EQ_3D_RNGDEP:
        ctx.load_grid(*RD.write_grid_ragged(str(tmp_path), False, short_paths=False), z_grnd=RD.ragged_load_z_grnd(False))
    else:
        ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=0, mode=0, src=tuple(g[f"{name}_src"]), z_grnd=float(g[f"{name}_z_grnd"]))
    ctx.set_levels(g[f"{name}_levels"], cap=16)

    def tables_of(th, ph):
        ctx.run(th, ph)
        return None

    def hit_of(_, sp):
        m = ctx.level_ampmap(**sp)
        if m["count"][0, 0, 0, 0] == 0:
            return None
        assert m["count"][0, 0, 0, 0] == 1
        sta, lv = LT.stations_of(sp)
        hits, rows = ctx.level_stations(sta=sta, level_of=lv, **LT.lstation_spec_of(sp))
        row = [r for r in rows[0, 0, :int(hits[0, 0])] if (r[LS.LSTA["DIR"]] > 0) == (sp["dir_mask"] == 1) and int(r[LS.LSTA["TRI"]]) == int(m["loudest"][0, 0, 0, 0]) % 2]
        assert len(row) == 1
        return m["amp_max"][0, 0, 0, 0], row[0][LS.LSTA["TTIME"]], row[0][LS.LSTA["ATTEN"]]

    gaps = LC.fix_gaps(name, eq, g, step, tables_of, hit_of)
    ctx.close()
    print("device, " + LC.fix_summary(name, step, gaps))
    left = np.flatnonzero(np.isnan(gaps[:, 0]))
    kept = gaps[~np.isnan(gaps[:, 0])]
    assert len(left) * 8 <= len(gaps), left
    assert (kept.max(axis=0) <= np.array(LC.gap_caps(name, step))).all(), (kept.max(axis=0), LC.gap_caps(name, step))


# ---------------------------------------------------------------- 5. members
def _plain_layers(G, L, sp, th, ph, tmpdir, **over):
    ctx = TGL._context(G, dict(L, **over), tmpdir)
    ctx.run(th, ph)
    out = ctx.level_ampmap(**sp)
    ctx.close()
    return out


def _check_members(got, plain, sp, what):
    """member m's layers equal those of the plain context m, bit for bit; DETECT is the count formed from the members' RAMP_MAX"""
    for m, want in enumerate(plain):
        for name in ("count", "weak", "amp_max", "ramp_max", "loudest"):
            assert _same_bits(got[name][m], want[name][0]), (what, m, name)
    assert np.array_equal(got["detect"], (got["ramp_max"] >= sp["detect_amp"]).sum(axis=0).astype(np.uint32))
    assert int(got["detect"].max()) >= 2 and int((got["detect"] == 1).sum()) > 0, what
    assert not _same_bits(got["amp_max"][0], got["amp_max"][1]), what                  # (the members are different launches)


def test_a_source_set_and_an_ensemble_against_plain_contexts(G, launches, tmp_path):
    # two sources x two profiles: member m = s * 2 + k is the plain context of profile k at source s
    L = LTC.LAUNCHES["sources2x2"]
    ctx, count, lrec, th, ph, nt, nph, legs = launches("sources2x2")
    sp, got = _with_detect(ctx, LM.spec(n_theta=nt, n_phi=nph, **dict(LTC.GRID_2SRC, **ALL)))
    raw = _raw_members()[:2]
    plain = []
    for s in range(2):
        for k in range(2):
            c = G.FanContext(L["eq"], device=0)
            _upload(c, [_device_arrays(L["eq"], *raw[k])])
            c.set_params(**dict(L["params"], src=tuple(L["sources"][s])))
            c.set_levels(LTC.LEVELS)
            c.run(th, ph)
            plain.append(c.level_ampmap(**sp))
            c.close()
    _check_members(got, plain, sp, "sources2x2")
    # a 1-D ensemble, K = 2
    ens = G.FanContext(H.EQ_GLOBAL, device=0)
    _upload(ens, [_device_arrays(H.EQ_GLOBAL, *r) for r in raw])
    ens.set_params(**LTC.TOY)
    ens.set_levels(LTC.LEVELS)
    ens.run(th, ph)
    sp1, got = _with_detect(ens, _spec("global", 0, nt, nph))
    ens.close()
    singles = []
    for k in range(2):
        c = G.FanContext(H.EQ_GLOBAL, device=0)
        _upload(c, [_device_arrays(H.EQ_GLOBAL, *raw[k])])
        c.set_params(**LTC.TOY)
        c.set_levels(LTC.LEVELS)
        c.run(th, ph)
        singles.append(c.level_ampmap(**sp1))
        c.close()
    _check_members(got, singles, sp1, "ensemble")


def test_a_grid_ensemble_against_plain_contexts(G, tmp_path):
    eq = H.EQ_3D_RNGDEP
    th, ph, nt, nph = LTC.lattice_of(LTC.LAUNCHES["3drd"])
    base = G.FanContext(eq, device=0)
    g = base.load_grid(*RD.write_grid(str(tmp_path), short_paths=False))
    base.close()
    members = [{k: g[k] * (1.0 if (k == "rho" or m == 0) else 0.9) for k in ("T", "u", "v", "rho")} for m in range(2)]
    prm = dict(LTC.TOY, src=(0.0, 0.0, 0.0))
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([mem[k] for mem in members]) for k in ("T", "u", "v", "rho")])
    ctx.set_params(**prm); ctx.set_levels(LTC.LEVELS)
    ctx.run(th, ph)
    sp, got = _with_detect(ctx, _spec("3drd", 0, nt, nph))
    ctx.close()
    plain = []
    for mem in members:
        with G.options(GRID_LANES="1"):          # (a grid ensemble integrates one lane per ray: the plain context whose records are the member's bits, tests/test_gpu_grid_ensemble.py)
            c = G.FanContext(eq, device=0)
            c.upload_atmo_3d(g["x"], g["y"], g["z"], mem["T"], mem["u"], mem["v"], mem["rho"])
            c.set_params(**prm); c.set_levels(LTC.LEVELS)
            c.run(th, ph)
            plain.append(c.level_ampmap(**sp))
            c.close()
    assert got["count"].shape[0] == 2 and int(got["count"][1].sum()) >= 10
    _check_members(got, plain, sp, "grid ensemble")


def test_a_frequency_set_gives_the_map_of_frequency_0(G, launches, tmp_path):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("freqs2")
    sp = _spec("global", 0, nt, nph, detect_amp=1e-4)
    got = ctx.level_ampmap(**sp)
    for freq, same in ((LTC.FREQS[0], True), (0.1, False)):
        want = _plain_layers(G, LTC.LAUNCHES["global"], sp, th, ph, tmp_path, params=dict(LTC.TOY, freq=freq))
        if same:
            LM.assert_layers_equal(got, want, "the plain context at frequency 0")
        else:                                                                       # (RAMP carries the attenuation at that frequency; AMP does not depend on it)
            assert np.array_equal(got["count"], want["count"]) and _same_bits(got["amp_max"], want["amp_max"]) and not _same_bits(got["ramp_max"], want["ramp_max"])


# ---------------------------------------------------------------- 6. det_floor
def test_det_floor_moves_hits_to_weak_and_never_back(G, launches):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("global")
    base = ctx.level_ampmap(**_spec("global", 1, nt, nph))
    total, last = base["count"] + base["weak"], base["count"]
    hits, rows = _lists_at_centres(ctx, _spec("global", 1, nt, nph))
    h = LM.hits_of_lists(H.EQ_GLOBAL, hits, rows, count, lrec, th, ph, legs, _spec("global", 1, nt, nph), LTC.LEVELS, [LA.medium_of_context(ctx)], _src3(ctx))
    # with +0.0 only singular hits are WEAK
    assert int(base["weak"].sum()) == int((~h["usable"]).sum()) and ((np.abs(h["det"][~h["usable"]]) == 0.0) | ~np.isfinite(h["det"][~h["usable"]]) | ~np.isfinite(h["ramp"][~h["usable"]])).all()
    det = np.abs(h["det"][h["usable"]])
    for floor in (float(np.quantile(det, 0.25)), float(np.median(det)), float(det.max())):
        m = ctx.level_ampmap(**_spec("global", 1, nt, nph, det_floor=floor))
        assert np.array_equal(m["count"] + m["weak"], total) and (m["count"] <= last).all() and int(m["count"].sum()) == int((det > floor).sum())
        assert (m["amp_max"] <= base["amp_max"]).all()
        last = m["count"]
    assert int(last.sum()) == 0 and (m["loudest"] == -1).all() and (m["ramp_max"] == -np.inf).all()


# ---------------------------------------------------------------- 7. launch plans
def test_layers_do_not_depend_on_the_launch_plan(G, launches, tmp_path):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("global")
    sp = _spec("global", 0, nt, nph, detect_amp=1e-4)
    want = ctx.level_ampmap(**sp)
    for opts in ({"NO_OVERLAP": "1"}, {"COMPACT": "0"}):
        with G.options(**opts):
            one = TGL._context(G, LTC.LAUNCHES["global"], tmp_path)
            one.run(th, ph)
            LM.assert_layers_equal(one.level_ampmap(**sp), want, str(opts))
            one.close()


# ---------------------------------------------------------------- 8. lifecycle and refusals
def test_lifecycle_and_refusals(G, tmp_path):
    L = LTC.LAUNCHES["global"]
    th, ph, nt, nph = LTC.lattice_of(L)
    sp = _spec("global", 0, nt, nph, detect_amp=1e-4)
    ctx = TGL._context(G, L, tmp_path, levels=None)
    lib = ctx.lib
    word = np.zeros((3,) + sp["n"], dtype=np.uint64)

    def fetch_rc():
        return lib.geoac_fan_level_ampmap_fetch(ctx._h, 0, word.ctypes.data_as(ctypes.c_void_p))

    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_ampmap: no completed launch"):
        ctx.level_ampmap(**sp)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_ampmap.*no levels set"):
        ctx.level_ampmap(**sp)
    ctx.set_levels(LTC.LEVELS)
    ctx.launch()
    before, steps = ctx.fetch()
    assert fetch_rc() == -1                                                         # a launch alone makes no map; a refused call has made nothing
    want = ctx.level_ampmap(**sp)
    assert ctx.level_ampmap_stats()["table_formed"]
    assert fetch_rc() == 0 and np.array_equal(word, want["count"][0])
    after, steps2 = ctx.fetch()
    assert steps2 == steps and _same_bits(after, before)                            # the launch is left alone
    # the shared branch table is formed once across this call, level_tubemap and level_stations
    ctx.level_tubemap(**LM.ltube_spec_of(sp))
    assert not ctx.level_tubemap_stats()["table_formed"]
    _lists_at_centres(ctx, sp)
    LM.assert_layers_equal(ctx.level_ampmap(**sp), want, "second call")
    assert not ctx.level_ampmap_stats()["table_formed"]
    # set_params ends nothing, and the source point and ground stay the launch's
    ctx.set_params(src=(3.0, 31.0, 0.5), z_grnd=0.2)
    assert fetch_rc() == 0
    LM.assert_layers_equal(ctx.level_ampmap(**sp), want, "after set_params")
    ctx.set_params(src=(0.0, 30.0, 0.0), z_grnd=0.0)
    src = list(ctx.params.src)
    invalidators = [("launch", ctx.launch), ("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: _upload(ctx, [_toy(H.EQ_GLOBAL)])),
                    ("set_levels", lambda: ctx.set_levels(LTC.LEVELS)), ("set_sources", lambda: ctx.set_sources(np.array([src]))),
                    ("set_frequencies", lambda: ctx.set_frequencies([0.1]))]
    for what, act in invalidators:
        assert fetch_rc() == 0, what
        act()
        assert fetch_rc() == -1 and "fan_level_ampmap_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        if what != "launch":
            with pytest.raises(G.GeoAcError, match="invalid.*fan_level_ampmap"):
                ctx.level_ampmap(**sp)
            ctx.launch()
        LM.assert_layers_equal(ctx.level_ampmap(**sp), want, "after " + what)
    # bad specs name their fault and leave the current map alone
    for bad, word_ in ((dict(sp, n_theta=nt + 1), "n_theta \\* n_phi"), (dict(sp, edge_max=float("inf")), "edge_max must be finite"), (dict(sp, edge_max=180.0), "below 180"),
                       (dict(sp, step=(0.375, 60.0)), "360 degrees"), (dict(sp, step=(0.0005, 0.0005)), "GEOAC_TUBE_MAX_SPAN"), (dict(sp, n=(0, 4)), "at least 1"),
                       (dict(sp, leg_min=2, leg_max=1), "leg_min"), (dict(sp, ord_max=0), "ord_max"), (dict(sp, dir_mask=0), "dir_mask"), (dict(sp, level_mask=0), "level_mask"),
                       (dict(sp, level_mask=0b1000), "level_mask has a bit"), (dict(sp, det_floor=-1.0), "det_floor"), (dict(sp, det_floor=float("nan")), "det_floor"),
                       (dict(sp, detect_amp=0.0), "detect_amp"), (dict(sp, detect_amp=float("inf")), "detect_amp")):
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_ampmap: .*" + word_):
            ctx.level_ampmap(**bad)
        assert fetch_rc() == 0
    nodet = ctx.level_ampmap(**dict(sp, detect_amp=float("nan")))
    assert nodet["detect"] is None and lib.geoac_fan_level_ampmap_fetch_detect(ctx._h, word.ctypes.data_as(ctypes.c_void_p)) == -1
    # sample capture
    ctx.set_params(mode=H.MODE_WRITE_RAYS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_ampmap: not available with sample capture"):
        ctx.level_ampmap(**sp)
    ctx.set_params(mode=0)
    # a leg band beyond the launch's legs is an empty map, not an error
    none = ctx.level_ampmap(**dict(sp, leg_min=5, leg_max=7))
    assert (none["count"] == 0).all() and (none["weak"] == 0).all() and (none["amp_max"] == -np.inf).all() and (none["loudest"] == -1).all() and (none["detect"] == 0).all()
    ctx.close()
    # calc_amp = 0 gives the same layers: the crossing records do not depend on it
    c0 = TGL._context(G, dict(L, params=dict(LTC.TOY, calc_amp=0)), tmp_path)
    c0.run(th, ph)
    LM.assert_layers_equal(c0.level_ampmap(**sp), want, "calc_amp = 0")
    c0.close()
    # the sets that are refused: nothing is made
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_ampmap: .*2-D set"):
        c2.level_ampmap(**sp)
    assert c2.lib.geoac_fan_level_ampmap_fetch(c2._h, 0, word.ctypes.data_as(ctypes.c_void_p)) == -1
    c2.close()
    Lg = LTC.LAUNCHES["globalrd"]
    tg, pg, ntg, npg = LTC.lattice_of(Lg)
    c3 = TGL._context(G, Lg, tmp_path)
    c3.run(tg, pg)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_ampmap: not available for GEOAC_EQ_GLOBAL_RNGDEP"):
        c3.level_ampmap(**LM.spec(n_theta=ntg, n_phi=npg, **dict(LTC.GRID_GLOBALRD, **ALL)))
    assert c3.lib.geoac_fan_level_ampmap_fetch(c3._h, 0, word.ctypes.data_as(ctypes.c_void_p)) == -1
    c3.level_tubemap(**LT.spec(n_theta=ntg, n_phi=npg, **dict(LTC.GRID_GLOBALRD, **ALL)))          # (the level tube map serves that set as before)
    c3.close()
