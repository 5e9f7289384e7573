"""Level tube maps on the device (include/geoac_ltubemap.h, FanContext.level_tubemap).  The main check is equivalence with merged code: every
layer equals, bit for bit, the reduction (tests/ltubemap_reference.py) of FanContext.level_stations at the cell centres with cap = 256, and the
numpy restatement on the fetched crossing records.  Then what the masks and filters do, the frequency set, the cooperative threshold and the
single-stream launch, the shared branch table, invalidation and refusals, and a closed form that owes nothing to the code: the raised-ground
medium of tests/raised_ground.py.  Cases and grids: tests/ltubemap_cases.py (proved non-vacuous on the CPU oracle in tests/test_ltubemap_host.py).
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import lstation_reference as LS
import ltubemap_cases as LC
import ltubemap_reference as LT
import map_cases as MC
import raised_ground as RGD
import station_reference as SR
import test_gpu_globalrd as TGG
import test_gpu_rngdep as TGR
import tubemap_cases as TC
from test_gpu_ensemble import _device_arrays
from test_gpu_sources import _toy, _upload

pytestmark = pytest.mark.gpu
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


def _members(a, tail):
    """a fetched table with its member axes merged into one: [M] + the last `tail` axes"""
    return a.reshape((-1,) + a.shape[-tail:])


def _context(G, L, tmpdir, levels=LC.LEVELS):
    """a context of tests/ltubemap_cases.py with its levels set (the launch's own list where it names one), nothing launched"""
    if levels is not None:
        levels = L.get("levels", levels)
    eq, kind, prm = L["eq"], L["kind"], L["params"]
    if kind in ("3drd", "globalrd"):
        ctx = (TGR if kind == "3drd" else TGG)._ctx(MC.write_grid(kind, str(tmpdir)), **prm)
    elif kind == "gridens":
        ctx = G.FanContext(eq, device=0)
        ctx.load_grid_ensemble(TC.write_grid_members(str(tmpdir)))
        ctx.set_params(**prm)
    else:
        ctx = G.FanContext(eq, device=0)
        _upload(ctx, [_toy(eq) if raw is None else _device_arrays(eq, *raw) for raw in TC.profiles_of(L)])
        ctx.set_params(**prm)
        if kind == "sources":
            ctx.set_sources(L["sources"])
        if kind == "freqs":
            ctx.set_frequencies(L["freqs"])
    if levels is not None:
        ctx.set_levels(levels)
    return ctx


def _launch(G, L, tmpdir):
    """a launch of tests/ltubemap_cases.py: context (left open), crossing counts [M][n_rays][L] and records [M][n_rays][L][cap][12], angles, lattice
    shape, legs"""
    th, ph, nt, nph = LC.lattice_of(L)
    ctx = _context(G, L, tmpdir)
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    return ctx, _members(count, 2), _members(lrec, 4), th, ph, nt, nph, rec.shape[-2]


@pytest.fixture(scope="module")
def launches(G, tmp_path_factory):
    """every launch once, shared by the cases that rasterise it (a level tube map does not change its launch)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _launch(G, LC.LAUNCHES[name], tmp_path_factory.mktemp(name))
        return made[name]

    yield get
    for v in made.values():
        v[0].close()


def _lists_at_centres(ctx, sp):
    """the merged level-station code at the cell centres of every selected level, every hit kept"""
    sta, lv = LT.stations_of(sp)
    return ctx.level_stations(sta=sta, level_of=lv, **LT.lstation_spec_of(sp))


# ---------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_layers_equal_the_level_station_lists_at_the_centres(G, launches, name):
    case = LC.CASES[name]
    eq = LC.LAUNCHES[case["launch"]]["eq"]
    ctx, count, lrec, th, ph, nt, nph, legs = launches(case["launch"])
    sp = LC.spec_of(case, nt, nph)
    got = ctx.level_tubemap(**sp)
    stats = ctx.level_tubemap_stats()
    M, Ls = count.shape[0], len(LT.selected(sp))
    assert got["count"].shape == (M, Ls) + sp["n"] and got["reach"].shape == (Ls,) + sp["n"]
    hits, rows = _lists_at_centres(ctx, sp)
    most = int(hits.max())
    print(f"{name}: M {M} Ls {Ls} cells {sp['n']} hits in all {int(got['count'].sum())}, most at one centre {most}, walk {stats}, "
          f"cells with COUNT 0 / 1 / >= 2 per selected level {LT.counts_per_level(got)}")
    assert most <= LT.CAP                                                           # (so the cap cannot hide a difference)
    LT.assert_layers_equal(got, LT.reduce_lists(hits, rows, sp), name + " against level_stations()")
    LT.assert_layers_equal(got, LT.reference_level_tubemap(eq, count, lrec, th, ph, legs, sp), name + " against the restatement")
    LC.check_non_vacuity(got, name)
    assert stats["triangles"] > 0 and stats["candidates"] >= int(got["count"].sum())
    if case.get("cooperative"):
        assert stats["cooperative"] > 0 and stats["candidates"] > G.TUBE_COOP_MIN * stats["cooperative"]
    if M > 1:
        assert not np.array_equal(SR.bits(got["ttime_min"][0]), SR.bits(got["ttime_min"][1]))          # (the members are different launches)
        assert int(got["reach"].max()) >= 2 and np.array_equal(got["reach"], (got["count"] > 0).sum(axis=0).astype(np.uint32))
    if name == "slot-mix":
        # neighbours whose leg-0 passages differ: some hits' corners hold their branch in different record slots (a build that read every corner's
        # record through corner 0's slot passed every other case of this file and fails this one: DESIGN 8o)
        assert LC.mixed_slot_hits(eq, count, lrec, th, ph, legs, sp) >= 3
    if name == "circle-wrap":
        # the grid's longitudes are -180 .. -177 and the crossings' 176 .. 182 (the state's longitude is continuous, tests/ltubemap_cases.py): every
        # reached centre is reached through a column run taken modulo 360, and the oracle's own map reaches more than 300 of them
        assert float(LT.centres(sp)[:, 1].max()) < -177.0 and int((got["count"] > 0).sum()) >= 300


def test_masks_and_filters(G, launches):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("global")
    m = {n: ctx.level_tubemap(**LC.spec_of(LC.CASES[n], nt, nph)) for n in ("global", "dir-up", "dir-down", "level-1", "levels-0-2", "leg-min-1", "ord-1", "edge-max")}
    full = m["global"]
    assert np.array_equal(m["dir-up"]["count"] + m["dir-down"]["count"], full["count"])
    assert int(m["dir-up"]["count"].sum()) > 0 and int(m["dir-down"]["count"].sum()) > 0
    # each level's layers equal its single-bit map, wherever it stands in the mask
    for name in ("count", "ttime_min", "atten_min", "first"):
        assert np.array_equal(SR.bits(m["level-1"][name][:, 0]), SR.bits(full[name][:, 1])), name
        assert np.array_equal(SR.bits(m["levels-0-2"][name]), SR.bits(full[name][:, [0, 2]])), name
        for ls, bit in enumerate((0b001, 0b100)):
            one = ctx.level_tubemap(**LC.spec_of(LC.CASES["global"], nt, nph, level_mask=bit))
            assert np.array_equal(SR.bits(one[name][:, 0]), SR.bits(m["levels-0-2"][name][:, ls])), (name, bit)
    assert np.array_equal(m["level-1"]["reach"][0], full["reach"][1])
    assert (m["leg-min-1"]["count"] <= full["count"][:, :2]).all() and 0 < int(m["leg-min-1"]["count"].sum()) < int(full["count"][:, :2].sum())
    assert (m["edge-max"]["count"] <= full["count"]).all() and int(m["edge-max"]["count"].sum()) < int(full["count"].sum())
    # ord_max changes the branch index a hit is filed under: b = ((leg - leg_min) * 2 + d) * ord_max + o
    n_tri = 2 * (nt - 1) * (nph - 1)
    f1, f2 = m["ord-1"]["first"], full["first"]
    some = f1 >= 0
    assert np.array_equal(m["ord-1"]["count"], full["count"]) and some.any()         # (no ray of this fan passes a level twice in one direction on one leg)
    assert np.array_equal(f2[some] % n_tri, f1[some] % n_tri) and np.array_equal(f2[some] // n_tri, 2 * (f1[some] // n_tri))


def test_a_frequency_set_gives_the_map_of_frequency_0(G, launches, tmp_path):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("freqs2")
    sp = LC.spec_of(LC.CASES["freqs2"], nt, nph)
    got = ctx.level_tubemap(**sp)
    for freq, same in ((LC.FREQS[0], True), (0.1, False)):
        L = dict(LC.LAUNCHES["global"], params=dict(LC.TOY, freq=freq))
        plain = _context(G, L, tmp_path)
        plain.run(th, ph)
        want = plain.level_tubemap(**sp)
        plain.close()
        if same:
            LT.assert_layers_equal(got, want, "the plain context at frequency 0")
        else:                                                                       # (ATTEN is the attenuation at that frequency, not at the default 0.1 Hz)
            assert np.array_equal(got["count"], want["count"]) and not np.array_equal(SR.bits(got["atten_min"]), SR.bits(want["atten_min"]))


def test_the_cooperative_threshold_does_not_change_the_layers(G, launches):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("global")
    sp = LC.spec_of(LC.CASES["fine"], nt, nph)
    want, coop = ctx.level_tubemap(**sp), ctx.level_tubemap_stats()["cooperative"]
    seen = {}
    try:
        for t in (0, 32, 2**31 - 1):
            os.environ["GEOAC_LTUBE_COOP"] = str(t)
            LT.assert_layers_equal(ctx.level_tubemap(**sp), want, f"threshold {t}")
            seen[t] = ctx.level_tubemap_stats()
    finally:
        os.environ.pop("GEOAC_LTUBE_COOP", None)
    print("cooperative walks by threshold:", {t: s["cooperative"] for t, s in seen.items()})
    assert seen[0]["cooperative"] == seen[0]["triangles"] and seen[32]["cooperative"] == coop > 0 and seen[2**31 - 1]["cooperative"] == 0
    assert len({s["candidates"] for s in seen.values()}) == 1


def test_a_single_stream_launch_gives_the_same_layers(G, launches, tmp_path):
    ctx, count, lrec, th, ph, nt, nph, legs = launches("global")
    sp = LC.spec_of(LC.CASES["global"], nt, nph)
    want = ctx.level_tubemap(**sp)
    with G.options(NO_OVERLAP="1"):
        one = _context(G, LC.LAUNCHES["global"], tmp_path)
        one.run(th, ph)
        LT.assert_layers_equal(one.level_tubemap(**sp), want, "NO_OVERLAP=1")
        one.close()


# ---------------------------------------------------------------- 2. lifecycle
def test_the_branch_table_is_shared_and_formed_once(G, tmp_path):
    L = LC.LAUNCHES["global"]
    th, ph, nt, nph = LC.lattice_of(L)
    sp = LC.spec_of(LC.CASES["global"], nt, nph)
    sta, lv = LT.stations_of(sp)
    sta, lv = sta[::7], lv[::7]
    ls_kw = dict(LT.lstation_spec_of(sp), cap=8)
    ctx = _context(G, L, tmp_path)
    ctx.run(th, ph)
    count, lrec = (_members(a, t) for a, t in zip(ctx.fetch_levels(), (2, 4)))
    lists = ctx.level_stations(sta=sta, level_of=lv, **ls_kw)                        # forms the table
    first = ctx.level_tubemap(**sp)
    assert not ctx.level_tubemap_stats()["table_formed"] and ctx.level_tubemap_timing() > 0.0
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, **ls_kw), lists)  # both results stay valid
    LT.assert_layers_equal(ctx.level_tubemap(**sp), first, "second call")
    assert not ctx.level_tubemap_stats()["table_formed"]
    # another ord_max is another table; back again it is formed again, by whichever module asks first
    other = ctx.level_tubemap(**dict(sp, ord_max=1))
    assert ctx.level_tubemap_stats()["table_formed"] and np.array_equal(other["count"], first["count"])
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, **ls_kw), lists)
    LT.assert_layers_equal(ctx.level_tubemap(**sp), first, "after the other table")
    assert not ctx.level_tubemap_stats()["table_formed"]
    ctx.launch()                                                                    # a new launch: the tube map asks first
    LT.assert_layers_equal(ctx.level_tubemap(**sp), first, "after a launch")
    assert ctx.level_tubemap_stats()["table_formed"]
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, **ls_kw), lists)
    LS.assert_lists_equal(lists, LS.reference_level_stations(L["eq"], count, lrec, th, ph, 2, LS.spec(**ls_kw), sta, lv))
    ctx.close()


def test_invalidation_and_refusals(G, tmp_path):
    L = LC.LAUNCHES["global"]
    th, ph, nt, nph = LC.lattice_of(L)
    sp = LC.spec_of(LC.CASES["global"], nt, nph)
    ctx = _context(G, L, tmp_path, levels=None)
    lib = ctx.lib
    word = np.zeros((3,) + sp["n"], dtype=np.uint64)

    def fetch_rc():
        return lib.geoac_fan_level_tubemap_fetch(ctx._h, 0, word.ctypes.data_as(ctypes.c_void_p))

    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap: no completed launch"):
        ctx.level_tubemap(**sp)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap.*no levels set"):
        ctx.level_tubemap(**sp)
    ctx.set_levels(LC.LEVELS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap.*no levels set"):             # (set, but not launched with)
        ctx.level_tubemap(**sp)
    ctx.launch()
    before, steps = ctx.fetch()
    assert fetch_rc() == -1                                                         # a launch alone makes no map
    want = ctx.level_tubemap(**sp)
    assert fetch_rc() == 0 and np.array_equal(word, want["count"][0])
    after, steps2 = ctx.fetch()
    assert steps2 == steps and np.array_equal(SR.bits(after), SR.bits(before))      # the launch is left alone
    invalidators = [("launch", ctx.launch), ("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: _upload(ctx, [_toy(H.EQ_GLOBAL)])),
                    ("set_levels", lambda: ctx.set_levels(LC.LEVELS))]
    for what, act in invalidators:
        act()
        assert fetch_rc() == -1, what
        assert "fan_level_tubemap_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        if what != "launch":
            with pytest.raises(G.GeoAcError, match="invalid.*(launch again|level list has changed)"):
                ctx.level_tubemap(**sp)
            ctx.launch()
            assert fetch_rc() == -1, what
        LT.assert_layers_equal(ctx.level_tubemap(**sp), want, "after " + what)
    # bad specs name their fault and leave the current map alone
    for bad, word_ in ((dict(sp, n_theta=nt + 1), "n_theta \\* n_phi"), (dict(sp, edge_max=float("inf")), "edge_max must be finite"), (dict(sp, edge_max=180.0), "below 180"),
                       (dict(sp, step=(0.375, 10.0)), "360 degrees"), (dict(sp, step=(0.0005, 0.0005)), "GEOAC_TUBE_MAX_SPAN"), (dict(sp, n=(0, 4)), "at least 1"),
                       (dict(sp, leg_min=2, leg_max=1), "leg_min"), (dict(sp, ord_max=0), "ord_max"), (dict(sp, dir_mask=0), "dir_mask"), (dict(sp, level_mask=0), "level_mask"),
                       (dict(sp, level_mask=0b1000), "level_mask has a bit")):
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap: .*" + word_):
            ctx.level_tubemap(**bad)
        assert fetch_rc() == 0
    # the same number of rays, not a lattice: one inclination off by an ulp; then the transposed shape
    th2 = th.copy()
    th2[nt + 2] = np.nextafter(th2[nt + 2], 90.0)
    ctx.run(th2, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap: .*not an n_theta x n_phi lattice"):
        ctx.level_tubemap(**sp)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_tubemap: .*not an n_theta x n_phi lattice"):
        ctx.level_tubemap(**dict(sp, n_theta=nph, n_phi=nt))
    LT.assert_layers_equal(ctx.level_tubemap(**sp), want, "after the refusals")
    # a leg band beyond the launch's legs is an empty map, not an error
    none = ctx.level_tubemap(**dict(sp, leg_min=5, leg_max=7))
    assert (none["count"] == 0).all() and (none["ttime_min"] == np.inf).all() and (none["first"] == -1).all() and (none["reach"] == 0).all()
    ctx.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_tubemap: .*2-D set"):
        c2.level_tubemap(**sp)
    assert c2.lib.geoac_fan_level_tubemap(c2._h, ctypes.byref(G.ltube_spec(**sp))) == -4
    c2.close()


# ---------------------------------------------------------------- 3. closed form
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form_under_a_raised_ground(G, eq, tmp_path):
    """the medium of tests/raised_ground.py, levels 8 and 15 km, leg 0 downward: COUNT against the winding numbers of the two ring polygons, TTIME_MIN
    against |X - s| / c and the bound e^2 / (2 c h) of a linear interpolant (LC.check_raised_ground; tests/test_ltubemap_host.py holds the
    restatement on the oracle's paths to the same).  The largest share of the bound used is printed (profiles/ltubemap_known_answers.txt keeps it)."""
    th, ph, nt, nph = RGD.lattice()
    ctx = G.FanContext(eq, device=0)
    if eq == H.EQ_3D_RNGDEP:
        ctx.load_grid(*RGD.write_uniform_grid(eq, str(tmp_path)), z_grnd=RGD.Z_GRND)
    else:
        ctx.upload_atmo_1d(*RGD.profile())
    ctx.set_params(**dict(RGD.params(eq), **RGD.LEVEL_PARAMS))
    ctx.set_levels(RGD.LEVELS)
    ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    got = ctx.level_tubemap(**LC.rg_spec(eq))
    ctx.close()
    worst = LC.check_raised_ground(eq, got, count, lrec)
    print(f"raised ground, device, {H.EQ_NAMES[eq]}, level tube map: " + LC.rg_figures(worst))
