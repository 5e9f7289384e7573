"""GPU: every post-launch product held to an answer that owes nothing to its restatement - the medium, fans, closed forms and checks of
tests/raised_ground.py (isothermal, windless, a source 20 km above a ground raised to 1.5 km, off the origin / across the date line), applied to the
HIP path.  tests/test_raised_ground_host.py applies the same checks to the plain-C oracle's records and the numpy restatements in the CPU suite:
that is where the forms, the conditions on the inputs and the tolerances are proved.  What a pass here excludes that the bit-for-bit tests cannot:
a radius, an origin or a wrap that kernel and restatement misread alike.
Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import faulthandler

import numpy as np
import pytest

import harness as H
import raised_ground as RGD
import refine_reference as RR

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 120
SETS = RGD.ALL_SETS
GRID_SETS = (H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP)


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
def grids(tmp_path_factory):
    """the uniform grids' files, written once per set"""
    made = {}

    def get(eq):
        if eq not in made:
            made[eq] = RGD.write_uniform_grid(eq, str(tmp_path_factory.mktemp(f"rg{eq}")))
        return made[eq]
    return get


def _ctx(G, grids, eq, **params):
    """a context holding the medium of set eq, nothing launched"""
    ctx = G.FanContext(eq, device=0)
    if eq in GRID_SETS:
        ctx.load_grid(*grids(eq), z_grnd=RGD.Z_GRND)
    else:
        z, T, u, v, rho = RGD.profile()
        ctx.upload_atmo_1d(z + (RGD.R_EARTH if eq == H.EQ_GLOBAL else 0.0), T, u, v, rho)
    ctx.set_params(**dict(RGD.params(eq), **params))
    return ctx


class _Run:
    """the lattice launch of one set on a context of its own, and a second plain context that integrates single fans"""

    def __init__(self, G, grids, eq):
        self.eq = eq
        self.th, self.ph, self.nt, self.nph = RGD.lattice()
        self.ctx, self.other = _ctx(G, grids, eq), _ctx(G, grids, eq)
        self.rec = self.ctx.run(self.th, self.ph)[0].copy()
        assert self.ctx.params.z_grnd == RGD.Z_GRND and (eq in RGD.CARTESIAN or self.ctx.params.r_earth == RGD.R_EARTH)

    def launch(self, th, ph):
        return self.other.run(th, ph)[0].copy()

    def close(self):
        self.ctx.close()
        self.other.close()


def _show(eq, part, figures):
    print(f"raised ground, device, {H.EQ_NAMES[eq]}, {part}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))


# ---------------------------------------------------------------- a. launch records
@pytest.mark.parametrize("eq", SETS)
def test_launch_records(G, grids, eq, tmp_path):
    """the closed forms on the device path; counts, VALID, STEPS and BROKE equal the oracle's.  On the grid sets the oracle integrates the azimuths 0 and
    195 alone (its grid interpolation takes a tenth of a second per ray); the other 22 columns follow: check_launch asserts, here on the device and in
    tests/test_raised_ground_host.py on the oracle's whole fan, that every ray is VALID, none BROKE, and that an inclination's STEPS are the same on
    every azimuth - so the device's STEPS on any azimuth are its column 0's, those are the oracle's column 0's, and those the oracle's on that azimuth"""
    run = _Run(G, grids, eq)
    run.close()
    _show(eq, "launch", RGD.check_launch(eq, run.rec))
    pick = np.arange(len(run.th)) if eq not in GRID_SETS else np.concatenate([np.arange(15), 13 * 15 + np.arange(15)])
    O = RGD.oracle(eq, tmp_path)
    _, ro, _, _ = O.fan(RGD.cfg(eq), run.th[pick], run.ph[pick])
    for f in ("VALID", "STEPS", "BROKE"):
        assert np.array_equal(run.rec[pick][..., H.REC[f]], ro[..., H.REC[f]]), f
    for f in ("TTIME", "AMP", "RANGE"):
        e = np.abs(run.rec[pick][..., H.REC[f]] / ro[..., H.REC[f]] - 1.0)
        assert e.max() <= 1e-6, (f, e.max())


# ---------------------------------------------------------------- b, c. stations and refinement
@pytest.mark.parametrize("eq", SETS)
def test_stations_and_refinement(G, grids, eq):
    run = _Run(G, grids, eq)
    ctx = run.ctx
    lattice_delta = RGD.check_axial_symmetry(eq, run.rec)[0] if eq in RGD.SPHERICAL else None
    sta, t_star, delta = RGD.ground_stations(eq, run.launch)
    hits, srows, _ = ctx.stations(sta=sta, n_theta=run.nt, n_phi=run.nph, phi_periodic=True, cap=4)
    _show(eq, "stations (not gated)", RGD.check_station_lists(hits[0], srows[0], t_star))
    rows, _, stats = ctx.refine(**RGD.GROUND_SPEC)
    print(stats, "rounds", rows[:, RR.RFN["ITER"]].astype(int).tolist())
    _show(eq, "refinement", RGD.check_refined(eq, rows, sta, t_star, delta, lattice_delta))
    _show(eq, "miss, converged rows", RGD.check_miss(eq, rows, sta, run.launch, separated=False))
    # the first misses, kilometres long: where the ground radius and the sphere radius give numbers 1e3 gates apart
    ctx.run(run.th, run.ph)
    ctx.stations(sta=sta, n_theta=run.nt, n_phi=run.nph, phi_periodic=True, cap=4)
    first, _, stats1 = ctx.refine(**dict(RGD.GROUND_SPEC, max_iter=1, tol=1e-9))
    assert stats1["launches"] == 1 and (first[:, RR.RFN["STATUS"]] == RR.ITER_LIMIT).all()
    _show(eq, "miss, first round", RGD.check_miss(eq, first, sta, run.launch, separated=True))
    run.close()


# ---------------------------------------------------------------- d. tube map and arrival map
@pytest.mark.parametrize("eq", SETS)
def test_tube_map_and_arrival_map(G, grids, eq):
    import tubemap_reference as TR
    run = _Run(G, grids, eq)
    ctx = run.ctx
    sp = RGD.tube_spec(eq)
    layers = ctx.tubemap(**sp)
    _show(eq, "tube map", RGD.check_tubemap(eq, layers["count"][0], run.rec, sp))
    half = RGD.tube_spec(eq, east_half=True)
    _show(eq, "tube map, eastern half", RGD.check_tubemap(eq, ctx.tubemap(**half)["count"][0], run.rec, half))
    sta = RGD.ground_stations(eq, run.launch)[0]
    flat = RGD.station_cells(eq, sp, sta, layers["count"][0])
    hits, rows, _ = ctx.stations(sta=TR.centres(sp)[flat], n_theta=run.nt, n_phi=run.nph, phi_periodic=True, edge_max=sp["edge_max"], cap=4)
    RGD.check_ttime_min_at_centres(layers["ttime_min"][0], flat, hits[0], rows[0])
    msp = RGD.map_spec(eq)
    _show(eq, "arrival map", RGD.check_arrival_map(eq, ctx.map(**msp), run.rec, msp))
    run.close()


# ---------------------------------------------------------------- e. levels, level stations, level refinement
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_levels_level_stations_and_level_refinement(G, grids, eq):
    th, ph, nt, nph = RGD.lattice()
    ctx = _ctx(G, grids, eq, **RGD.LEVEL_PARAMS)
    ctx.set_levels(RGD.LEVELS)
    for k, br in enumerate(RGD.BRANCHES):
        rec = ctx.run(th, ph)[0].copy()                                             # (a refinement leaves its own last round behind: launch the lattice again)
        count, lrec = ctx.fetch_levels()
        if k == 0:
            _show(eq, "levels", RGD.check_levels(eq, rec, count, lrec))
        sta, lv = RGD.level_stations_of(eq, br)
        hits, rows = ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, phi_periodic=True, ord_max=2, cap=4, **br["lsta"])
        RGD.check_level_station_lists(br, hits[0], rows[0])
        out, stats = ctx.level_refine(**RGD.LEVEL_SPEC)
        print(stats)
        _show(eq, f"level refinement, leg {br['leg']}", RGD.check_level_refined(eq, br, out, sta))
    ctx.close()
