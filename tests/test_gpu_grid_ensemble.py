"""Grid ensembles (geoac_upload_atmo_3d_ensemble): one launch integrates one set of launch angles through K range-dependent atmospheres - grids of profiles on
shared nodes - for both grid sets.  Member m's records must be the very bits a plain context that uploaded grid m alone returns with one lane per ray
(GRID_LANES=1: the ensemble's launch plan is one lane per ray), under every launch plan, and member 0 - the unperturbed grid - must match the compiled reference's fixture.

Inputs: the ragged 7 x 4 jet grid (tests/rngdep_data.py) in its Cartesian and spherical forms, and fan b of its fixture (25 rays = 5 inclinations x 5 azimuths from 12 km
inside the jet, rays below the horizontal, raised ground, legs past 15 000 steps).  Members: the grid as load_grid returns it, winds scaled by 1.0 / 0.85 / 1.15 and T
shifted by 0 / +3 / -3 K.  With these factors the plain-C oracle, run on met files written for each member, finds 17 / 16 / 18 arrivals (Cartesian) and 22 / 19 / 24
(spherical) with two bounces, 8 / 8 / 9 and 10 / 9 / 11 with none: no milder factors were needed."""
import ctypes

import numpy as np
import pytest

import harness as H
import rngdep_data as RD
from parity import compare_records

pytestmark = pytest.mark.gpu

SETS = [H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP]
HIDX = {H.EQ_3D_RNGDEP: 2, H.EQ_GLOBAL_RNGDEP: 0}
FACTORS = [(1.0, 0.0), (0.85, 3.0), (1.15, -3.0)]             # (wind scale, T shift [K]) per member
K = len(FACTORS)
STEP_LIMIT_S = 120
VALID, STEPS, BROKE = H.REC["VALID"], H.REC["STEPS"], H.REC["BROKE"]


@pytest.fixture
def time_limit():
    import faulthandler
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


@pytest.fixture(scope="module")
def grids(G, tmp_path_factory):
    """per set: the grid files, the arrays load_grid returns for them, the K members derived from those, fan b and its parameters, the reference's records"""
    out = {}
    for eq in SETS:
        glob = eq == H.EQ_GLOBAL_RNGDEP
        files = RD.write_grid_ragged(str(tmp_path_factory.mktemp("ge")), glob, short_paths=False)
        ctx = G.FanContext(eq, device=0)
        g = ctx.load_grid(*files, z_grnd=RD.ragged_load_z_grnd(glob))
        ctx.close()
        members = [dict(T=g["T"] + dT, u=g["u"] * w, v=g["v"] * w, rho=g["rho"]) for w, dT in FACTORS]
        th, ph, params, want, steps_want, _ = RD.ragged_table(RD.ragged_fixture(glob), "b_amp1")
        out[eq] = dict(files=files, nodes=(g["x"], g["y"], g["z"]), members=members, th=th, ph=ph, params=params, want=want, steps_want=steps_want)
    return out


def _stack(members):
    return [np.stack([m[k] for m in members]) for k in ("T", "u", "v", "rho")]


def _params(d, **over):
    return dict(d["params"], mode=0, **over)


_plain_runs, _ens_runs = {}, {}


def _plain(G, eq, d, m, th=None, ph=None, opts=None, **over):
    """member m alone on a plain context, one lane per ray"""
    from geoac_amd.api import options
    with options(**dict({"GRID_LANES": "1"}, **(opts or {}))):
        ctx = G.FanContext(eq, device=0)
        ctx.upload_atmo_3d(*d["nodes"], *[d["members"][m][k] for k in ("T", "u", "v", "rho")])
        ctx.set_params(**_params(d, **over))
        rec, steps = ctx.run(d["th"] if th is None else th, d["ph"] if ph is None else ph)
        rec = rec.copy(); ctx.close()
    return rec, steps


def _plain_cached(G, eq, d, m, amp, bounces):
    key = (eq, m, amp, bounces)
    if key not in _plain_runs:
        _plain_runs[key] = _plain(G, eq, d, m, calc_amp=amp, bounces=bounces)
    return _plain_runs[key]


def _ens(G, eq, d, members=None, th=None, ph=None, opts=None, **over):
    from geoac_amd.api import options
    with options(**(opts or {})):
        ctx = G.FanContext(eq, device=0)
        ctx.upload_atmo_3d_ensemble(*d["nodes"], *_stack(d["members"] if members is None else members))
        ctx.set_params(**_params(d, **over))
        rec, steps = ctx.run(d["th"] if th is None else th, d["ph"] if ph is None else ph)
        rec = rec.copy(); ctx.close()
    return rec, steps


def _ens_cached(G, eq, d, amp, bounces):
    key = (eq, amp, bounces)
    if key not in _ens_runs:
        _ens_runs[key] = _ens(G, eq, d, calc_amp=amp, bounces=bounces)
    return _ens_runs[key]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- 1. member equals single context ----
@pytest.mark.parametrize("bounces", [0, 2])
@pytest.mark.parametrize("amp", [0, 1])
@pytest.mark.parametrize("eq", SETS)
def test_member_equals_single_context(G, grids, eq, amp, bounces, time_limit):
    d = grids[eq]
    rec, steps = _ens_cached(G, eq, d, amp, bounces)
    assert rec.shape == (K, len(d["th"]), bounces + 1, 32)
    singles = [_plain_cached(G, eq, d, m, amp, bounces) for m in range(K)]
    print(f"eq {eq} amp {amp} bounces {bounces}: steps {steps}, members {[s for _, s in singles]}, arrivals {[int((r[..., VALID] > 0).sum()) for r, _ in singles]}")
    # no test that passes with every member reading table 0: the members arrive, and differently
    for m in range(K):
        assert (rec[m][..., VALID] > 0).sum() >= 5, m
    for a in range(K):
        for b in range(a + 1, K):
            assert not _same_bits(rec[a], rec[b]), (a, b)
    for m in range(K):
        assert _same_bits(rec[m], singles[m][0]), f"member {m} differs from the plain context that holds grid {m}"
    assert steps == sum(s for _, s in singles)


# ---- 2. member 0 against the reference ----
@pytest.mark.parametrize("eq", SETS)
def test_member_0_vs_reference(G, grids, eq, time_limit):
    d = grids[eq]
    assert d["params"]["calc_amp"] == 1 and d["params"]["bounces"] == 2
    rec, steps = _ens_cached(G, eq, d, 1, 2)
    want = d["want"]
    for f in (VALID, STEPS, BROKE):
        assert np.array_equal(rec[0][..., f], want[..., f])
    # the step total: the reference's for member 0 (= the sum of its STEPS column), the plain contexts' for the others
    assert d["steps_want"] == int(want[..., STEPS].sum()) == int(rec[0][..., STEPS].sum())
    assert steps == d["steps_want"] + sum(_plain_cached(G, eq, d, m, 1, 2)[1] for m in range(1, K))
    compare_records(rec[0], want, E=18, hidx=HIDX[eq])


# ---- 3. schedule independence ----
SCHEDULES = {
    "s_rows512": {"S_ROWS": "512"},                              # some 30 epochs: k_compact_ens runs many times, members finish at different epochs
    "compact0": {"COMPACT": "0"},
    "coop0": {"GRID_COOP": "0"},                                 # per-lane gathers
    "coop1": {"GRID_COOP": "1"},
    "no_overlap": {"NO_OVERLAP": "1"},
    "sub_epochs": {"SUB_MIN_WAVES": "0", "SUB_EPOCHS": "4", "S_ROWS": "512"},      # the cross-wave hand-off of saturated fans
    "grid_lanes4": {"GRID_LANES": "4"},                          # ignored with K > 1
}


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("eq", SETS)
def test_records_do_not_depend_on_the_schedule(G, grids, eq, name, time_limit):
    d = grids[eq]
    want, steps_want = _ens_cached(G, eq, d, 1, 2)
    rec, steps = _ens(G, eq, d, opts=SCHEDULES[name], calc_amp=1, bounces=2)
    assert steps == steps_want and _same_bits(rec, want)


# ---- 4. fans that are no multiple of 64 ----
@pytest.mark.parametrize("eq", SETS)
def test_odd_fan_sizes(G, grids, eq, time_limit):
    d = grids[eq]
    full = [_plain_cached(G, eq, d, m, 1, 2)[0] for m in range(K)]
    # 23 of the 25 rays, K = 2: a ray's records do not depend on the rest of the fan
    rec, _ = _ens(G, eq, d, members=d["members"][:2], th=d["th"][:23], ph=d["ph"][:23], calc_amp=1, bounces=2)
    assert rec.shape == (2, 23, 3, 32)
    for m in range(2):
        assert (rec[m][..., VALID] > 0).sum() >= 5 and _same_bits(rec[m], full[m][:23])
    assert not _same_bits(rec[0], rec[1])
    # one ray, K = 3
    rec, steps = _ens(G, eq, d, th=d["th"][7:8], ph=d["ph"][7:8], calc_amp=1, bounces=2)
    assert rec.shape == (3, 1, 3, 32)
    for m in range(K):
        assert _same_bits(rec[m], full[m][7:8])
    assert steps == sum(int(full[m][7, :, STEPS].sum()) for m in range(K))


# ---- 5. K changes between launches ----
@pytest.mark.parametrize("eq", SETS)
def test_k_changes_between_launches(G, grids, eq, time_limit):
    d = grids[eq]
    want, steps_want = _ens_cached(G, eq, d, 1, 2)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(*d["nodes"], *_stack(d["members"]))
    ctx.set_params(**_params(d))
    assert ctx.n_members == K
    rec, steps = ctx.run(d["th"], d["ph"])
    assert steps == steps_want and _same_bits(rec, want)
    # back to a plain context: the default plan's bits (eight lanes per ray on this fan), as a fresh context gives them
    ctx.upload_atmo_3d(*d["nodes"], *[d["members"][1][k] for k in ("T", "u", "v", "rho")])
    k = ctypes.c_int(0)
    assert ctx.lib.geoac_get_members(ctx._h, ctypes.byref(k)) == 0 and k.value == 1 and ctx.n_members == 1
    rec1, steps1 = ctx.run(d["th"], d["ph"])
    rec1 = rec1.copy()
    fresh = G.FanContext(eq, device=0)
    fresh.upload_atmo_3d(*d["nodes"], *[d["members"][1][k] for k in ("T", "u", "v", "rho")])
    fresh.set_params(**_params(d))
    recf, stepsf = fresh.run(d["th"], d["ph"])
    assert rec1.shape == (len(d["th"]), 3, 32) and steps1 == stepsf and _same_bits(rec1, recf)
    fresh.close()
    # K = 1 through the new call is a plain context too
    ctx.upload_atmo_3d_ensemble(*d["nodes"], *_stack(d["members"][1:2]))
    assert ctx.n_members == 1
    rec1b, steps1b = ctx.run(d["th"], d["ph"])
    assert steps1b == stepsf and _same_bits(rec1b, recf)
    # and an ensemble again
    ctx.upload_atmo_3d_ensemble(*d["nodes"], *_stack(d["members"]))
    assert ctx.lib.geoac_get_members(ctx._h, ctypes.byref(k)) == 0 and k.value == K
    rec, steps = ctx.run(d["th"], d["ph"])
    assert steps == steps_want and _same_bits(rec, want)
    ctx.close()


# ---- 6. refusals ----
@pytest.mark.parametrize("eq", SETS)
def test_refusals(G, grids, eq, time_limit):
    d = grids[eq]
    x, y, z = d["nodes"]
    T, u, v, rho = _stack(d["members"])
    want, steps_want = _ens_cached(G, eq, d, 1, 2)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    f = G.load_library().geoac_upload_atmo_3d_ensemble
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 7
    # a stratified context
    c = G.FanContext(G.EQ_GLOBAL, device=0)
    with pytest.raises(G.GeoAcError, match="not implemented"):
        c.upload_atmo_3d_ensemble(x, y, z, T, u, v, rho)
    c.close()
    ctx = G.FanContext(eq, device=0)
    # K out of range: the message names n_members
    for bad in (0, 65):
        assert f(ctx._h, bad, len(x), len(y), len(z), ptr(x), ptr(y), ptr(z), ptr(T), ptr(u), ptr(v), ptr(rho)) == -1
        assert b"n_members" in ctx.lib.geoac_last_error(ctx._h)
    # shapes
    with pytest.raises(G.GeoAcError, match="must be"):
        ctx.upload_atmo_3d_ensemble(x, y, z, T, u[:2], v, rho)
    with pytest.raises(G.GeoAcError, match="must be"):
        ctx.upload_atmo_3d_ensemble(x, y[:-1], z, T, u, v, rho)
    ctx.upload_atmo_3d_ensemble(x, y, z, T, u, v, rho)
    # the 1-D ensemble, source sets and frequency sets stay refused on a range-dependent context, now with the word for it
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.set_sources(np.array([d["params"]["src"], d["params"]["src"]]))
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.set_frequencies([0.1, 0.2])
    # sample capture
    ctx.set_params(**dict(_params(d), mode=1))
    ctx.set_angles(d["th"], d["ph"])
    with pytest.raises(G.GeoAcError, match="not implemented.*sample capture.*ensemble"):
        ctx.launch()
    ctx.set_params(**_params(d))
    # clone, eigenray searches
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.clone()
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.eig_search(np.array([[31.0, 0.5]]))
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.eig_direct(np.array([[31.0, 0.5]]), [10.0], [-90.0])
    # the pool
    pool = G.FanPool(eq, [0])
    h = ctypes.c_void_p(pool.lib.geoac_pool_ctx(pool._h, 0))
    assert f(h, K, len(x), len(y), len(z), ptr(x), ptr(y), ptr(z), ptr(T), ptr(u), ptr(v), ptr(rho)) == 0
    pool.set_params(**_params(d))
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        pool.run(d["th"], d["ph"])
    pool.close()
    # refinement: the station lists of a grid ensemble exist, their refinement does not
    rec, steps = ctx.run(d["th"], d["ph"])
    assert steps == steps_want and _same_bits(rec, want)
    ctx.stations(sta=np.array([[0.0, 0.0]]) if eq == H.EQ_3D_RNGDEP else np.array([[30.0, 0.0]]), n_theta=5, n_phi=5)
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.refine()
    # the context still launches, and gives the right bits
    rec, steps = ctx.run(d["th"], d["ph"])
    assert steps == steps_want and _same_bits(rec, want)
    ctx.close()


# ---- 7. post-launch modules on members ----
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


@pytest.mark.parametrize("eq", SETS)
def test_map_and_stations_on_members(G, grids, eq, time_limit):
    import station_reference as SR
    from geoac_amd.api import options
    d = grids[eq]
    # one small grid around the arrivals of member 0, and three stations inside landing triangles of member 0's lattice
    rec0 = _plain_cached(G, eq, d, 0, 1, 2)[0]
    c0, c1 = SR.landing(eq, rec0[None])
    ok = rec0[..., VALID] > 0
    lo = np.array([c0[0][ok].min(), c1[0][ok].min()]); hi = np.array([c0[0][ok].max(), c1[0][ok].max()])
    n = (6, 5)
    spec = dict(origin=tuple(lo - 0.01 * (hi - lo)), step=tuple(1.02 * (hi - lo) / np.array(n)), n=n)
    tri = SR.triangles(SR.spec(5, 5))
    sta = []
    for leg in range(3):
        for t in tri:
            if ok[t, leg].all() and len(sta) < 3:
                sta.append([c0[0][t, leg].mean(), c1[0][t, leg].mean()])
    assert len(sta) == 3, "fan b has fewer than three landing triangles with three arrivals on one leg"
    sta = np.array(sta)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(*d["nodes"], *_stack(d["members"]))
    ctx.set_params(**_params(d))
    rec, _ = ctx.run(d["th"], d["ph"])
    got_map = ctx.map(**spec)
    got_hits, got_rows, got_lvl = ctx.stations(sta=sta, n_theta=5, n_phi=5)
    ctx.close()
    assert got_map["count"].shape == (K,) + n and got_hits.shape == (K, 3)
    assert got_hits[0].sum() >= 3 and got_map["count"][0].sum() == ok.sum()
    for m in range(K):
        with options(GRID_LANES="1"):
            c = G.FanContext(eq, device=0)
        c.upload_atmo_3d(*d["nodes"], *[d["members"][m][k] for k in ("T", "u", "v", "rho")])
        c.set_params(**_params(d))
        c.run(d["th"], d["ph"])
        want_map = c.map(**spec)
        hits, rows, lvl = c.stations(sta=sta, n_theta=5, n_phi=5)
        c.close()
        for name in ("count", "ttime_min", "cel_max", "level_max", "best", "outside"):
            assert np.array_equal(_bits(got_map[name][m]), _bits(want_map[name][0])), (m, name)
        assert np.array_equal(got_hits[m], hits[0]), m
        for r in range(3):
            k = min(int(hits[0][r]), rows.shape[2])
            assert np.array_equal(_bits(got_rows[m, r, :k]), _bits(rows[0, r, :k])) and np.array_equal(_bits(got_lvl[m, r, :k]), _bits(lvl[0, r, :k])), (m, r)
    assert any(not np.array_equal(_bits(got_map["ttime_min"][0]), _bits(got_map["ttime_min"][m])) for m in range(1, K))


# ---- 8. load_grid_ensemble ----
@pytest.mark.parametrize("eq", SETS)
def test_load_grid_ensemble(G, grids, eq, tmp_path, time_limit):
    import shutil
    d = grids[eq]
    glob = eq == H.EQ_GLOBAL_RNGDEP
    prefix, loc_a, loc_b = d["files"]
    other = tmp_path / "loc_a_other.dat"
    nodes = np.loadtxt(loc_a); nodes[2] += 0.125
    other.write_text("".join(f"{v:.10g}\n" for v in nodes))
    ctx = G.FanContext(eq, device=0)
    with pytest.raises(G.GeoAcError, match="loc_a_other"):
        ctx.load_grid_ensemble([(prefix, loc_a, loc_b), (prefix, str(other), loc_b)], z_grnd=RD.ragged_load_z_grnd(glob))
    with pytest.raises(G.GeoAcError, match="no grids"):
        ctx.load_grid_ensemble([])
    mem = ctx.load_grid_ensemble([(prefix, loc_a, loc_b)] * 2, z_grnd=RD.ragged_load_z_grnd(glob))
    assert ctx.n_members == 2 and len(mem) == 2
    ctx.set_params(**_params(d))
    rec, steps = ctx.run(d["th"], d["ph"])
    ctx.close()
    want = _plain_cached(G, eq, d, 0, 1, 2)
    assert rec.shape == (2, len(d["th"]), 3, 32) and _same_bits(rec[0], rec[1]) and _same_bits(rec[0], want[0]) and steps == 2 * want[1]
