"""The cases of the tube-map tests: launch set-ups and grid literals, shared by tests/test_tubemap_host.py (which proves on the CPU oracle's
records that every grid meets the non-vacuity conditions) and tests/test_gpu_tubemap.py (which runs them on the device).  Launches are those of
the map cases (tests/map_cases.py) over the 13 x 9 lattice fans of tests/station_cases.py with one bounce.  Grid extents, bands and edge_max were
chosen from the oracle's landing points; they are literals, not derived from the code under test."""
import numpy as np

import harness as H
import map_cases as MC
import map_reference as MR
import rngdep_data as RD
import station_cases as SC
import tubemap_reference as TR
from test_gpu_ensemble import _raw_members
from test_gpu_freqs import FREQS

ONE_BOUNCE = dict(bounces=1, calc_amp=1)
# the full-circle lattice of the column-wrap case: 13 inclinations x 9 azimuths 40 degrees apart, -180 .. 140, the last column neighbours the first
CIRCLE_LATTICE = dict(theta_min=3.0, theta_max=39.0, theta_step=3.0, phi_min=-180.0, phi_max=140.0, phi_step=40.0)
WRAP_SRC = (0.0, 30.0, 179.0)
# two sources whose fans land on one grid: the ground source of the plain cases and one 20 km up, 1.5 degrees north and 2 degrees west of it
TUBE_SOURCES = np.array([[0.0, 30.0, 0.0], [20.0, 31.5, -2.0]])

LAUNCHES = {
    "3d": dict(kind="plain", eq=H.EQ_3D, params=ONE_BOUNCE),
    "global": dict(kind="plain", eq=H.EQ_GLOBAL, params=ONE_BOUNCE),
    "3drd": dict(kind="3drd", eq=H.EQ_3D_RNGDEP, params=dict(bounces=1, calc_amp=1, mode=0, src=(0.0, 0.0, 0.0))),
    "globalrd": dict(kind="globalrd", eq=H.EQ_GLOBAL_RNGDEP, params=dict(bounces=1, calc_amp=1, mode=0, src=(0.0, 31.0, 0.0))),
    "ensemble3": dict(kind="ensemble", eq=H.EQ_GLOBAL, params=ONE_BOUNCE),
    "sources2x2": dict(kind="sources", eq=H.EQ_GLOBAL, sources=TUBE_SOURCES, n_prof=2, params=ONE_BOUNCE),
    "freqs3": dict(kind="freqs", eq=H.EQ_GLOBAL, freqs=FREQS[:3], params=ONE_BOUNCE),
    "circle": dict(kind="plain", eq=H.EQ_GLOBAL, params=dict(ONE_BOUNCE, src=WRAP_SRC), lattice=CIRCLE_LATTICE),
    "gridens2": dict(kind="gridens", eq=H.EQ_3D_RNGDEP, params=dict(bounces=1, calc_amp=1, mode=0, src=(0.0, 0.0, 0.0))),
}
# the K = 2 grid ensemble: the 5 x 5 grid of tests/rngdep_data.py and the same grid with weaker winds and a warmer atmosphere - (wind scale, T shift [K])
GRID_MEMBERS = [(1.0, 0.0), (0.85, 3.0)]

# grids (at most 32 x 48 cells).  The westward fan from (30, 0) lands at lat 27.8 .. 32.1, lon -6.1 .. -2.1 on leg 0 and lat 25.5 .. 34.1,
# lon -12.5 .. -4.1 on leg 1; the Cartesian one at x -540 .. -205, |y| < 309 km and x -1081 .. -410, |y| < 617 km
GRID_GLOBAL = dict(origin=(25.0, -10.0), step=(0.375, 0.25), n=(24, 40), edge_max=3.0)
GRID_3D = dict(origin=(-900.0, -450.0), step=(37.5, 30.0), n=(24, 30), edge_max=300.0)
GRID_3DRD = dict(origin=(-620.0, -300.0), step=(17.5, 25.0), n=(24, 24), edge_max=300.0)
GRID_GLOBALRD = dict(origin=(28.0, -6.0), step=(0.2, 0.16), n=(25, 25), edge_max=3.0)
GRID_2SRC = dict(origin=(25.5, -11.5), step=(0.3, 0.3), n=(28, 32), edge_max=3.0)                       # the two sources of TUBE_SOURCES
# lon -180 .. -168: the fan from lon 179 lands at 169.6 .. 187.3 (the state's longitude is continuous), its part beyond 180 is on the grid modulo 360
GRID_CIRCLE = dict(origin=(20.0, -180.0), step=(0.625, 0.25), n=(32, 48), edge_max=8.0, wrap_lon=True, phi_periodic=True)
GRID_FINE = dict(origin=(28.0, -6.0), step=(0.0625, 0.0625), n=(32, 48), edge_max=3.0)                  # cells several times smaller than the triangles
GRID_COARSE = dict(origin=(25.5, -11.5), step=(1.5, 1.5), n=(6, 7), edge_max=3.0)                       # cells larger than most triangles
GRID_HALF_OFF = dict(origin=(28.0, -5.5), step=(0.25, 0.25), n=(24, 24), edge_max=3.0)                  # the landing area ends inside the grid

# the small-lattice step of the repeated-call tests (small_lattice_step below): every second inclination and azimuth of SC.PARITY_LATTICE, 7 x 5;
# edge_max doubled for the doubled triangles; five stations inside the westward fan's landing area
SMALL_LATTICE = dict(theta_min=3.0, theta_max=39.0, theta_step=6.0, phi_min=-122.0, phi_max=-58.0, phi_step=16.0)
SMALL_GRID = dict(GRID_COARSE, edge_max=6.0)
SMALL_STATIONS = np.array([[30.0, -4.0], [30.5, -5.5], [29.0, -8.0], [31.5, -9.0], [28.5, -3.5]])
SMALL_CAP = 8

CASES = {
    "3d": dict(launch="3d", spec=dict(GRID_3D, detect_db=MC.DETECT_AMP)),
    "global": dict(launch="global", spec=dict(GRID_GLOBAL, detect_db=MC.DETECT_AMP)),
    "3drd": dict(launch="3drd", spec=dict(GRID_3DRD, detect_db=MC.DETECT_AMP)),
    "globalrd": dict(launch="globalrd", spec=dict(GRID_GLOBALRD, detect_db=MC.DETECT_AMP)),
    "ensemble3": dict(launch="ensemble3", spec=dict(GRID_GLOBAL, detect_db=MC.DETECT_AMP)),
    "sources2x2": dict(launch="sources2x2", spec=dict(GRID_2SRC, detect_db=MC.DETECT_AMP)),
    "freqs3": dict(launch="freqs3", spec=dict(GRID_GLOBAL, detect_db=-80.0)),
    "circle-wrap": dict(launch="circle", spec=dict(GRID_CIRCLE)),
    "gridens2": dict(launch="gridens2", spec=dict(GRID_3DRD, detect_db=MC.DETECT_AMP)),
    "fine": dict(launch="global", spec=dict(GRID_FINE), cooperative=True),
    "coarse": dict(launch="global", spec=dict(GRID_COARSE)),
    "half-off": dict(launch="global", spec=dict(GRID_HALF_OFF)),
    "leg-band": dict(launch="global", spec=dict(GRID_GLOBAL, leg_min=1, leg_max=1)),
    "turn-band": dict(launch="global", spec=dict(GRID_GLOBAL, turn_min=60.0, turn_max=np.inf)),      # the thermospheric family alone
    "edge-max": dict(launch="global", spec=dict(GRID_GLOBAL, edge_max=2.0, turn_tol=20.0)),          # removes the long triangles
}


def write_grid_members(dirpath):
    """the files of the grid ensemble's members, one directory each, written as tests/rngdep_data.py writes its grid (member 0: the same bytes);
    returns [(prefix, locx, locy), ...]"""
    import os
    files = [RD.write_grid(os.path.join(dirpath, "m0"), short_paths=False)]
    z, T, u, v, rho, p = RD.load_grid_columns()
    for m, (w, dT) in enumerate(GRID_MEMBERS[1:], start=1):
        prefix, locx, locy = RD.write_grid(os.path.join(dirpath, f"m{m}"), short_paths=False)
        for i in range(len(RD.X_NODES)):
            for j in range(len(RD.Y_NODES)):
                with open(f"{prefix}{i * len(RD.Y_NODES) + j}.met", "w") as fh:
                    for k in range(len(z)):
                        fh.write(f"{z[k]:.10g} {T[i, j, k] + dT:.12g} {w * u[i, j, k]:.12g} {w * v[i, j, k]:.12g} {rho[i, j, k]:.12g} {p[k]:.10g}\n")
        files.append((prefix, locx, locy))
    return files


def lattice_of(launch):
    kw = launch.get("lattice") or (SC.PARITY_LATTICE_RD if launch["kind"] in ("3drd", "globalrd", "gridens") else SC.PARITY_LATTICE)
    return SC.lattice(**kw)


def profiles_of(launch):
    """raw profile columns of the launch's members (None: ToyAtmo itself)"""
    if launch["kind"] == "ensemble":
        return _raw_members()
    if launch["kind"] == "sources" and launch["n_prof"] > 1:
        return _raw_members()[:launch["n_prof"]]
    return [None]


def spec_of(case, nt, nph, **overrides):
    return TR.spec(n_theta=nt, n_phi=nph, **dict(case["spec"], **overrides))


def oracle_tables(launch, tmpdir, member0=None):
    """the launch on the CPU oracle: rec [M][n_rays][legs][32], level [M][F][n_rays][legs] (numpy's log10), angles, lattice shape.  member0: a grid
    ensemble's member 0 is the "3drd" launch itself; a caller that holds those records [n_rays][legs][32] passes them and saves the oracle's minutes"""
    eq, kind, prm = launch["eq"], launch["kind"], launch["params"]
    th, ph, nt, nph = lattice_of(launch)
    cfg = dict(bounces=prm["bounces"], calc_amp=bool(prm["calc_amp"]))
    if "src" in prm:
        cfg["src"] = prm["src"]
    recs, atten = [], None

    def oracle(raw):
        O = H.Oracle(eq, H.TOYATMO if raw is None else None)
        if raw is not None:
            O.load_arrays(*raw)
        return O

    if kind in ("plain", "ensemble"):
        for raw in profiles_of(launch):
            recs.append(oracle(raw).fan(H.make_cfg(eq, **cfg), th, ph)[1])
    elif kind == "sources":
        for src in launch["sources"]:
            for raw in profiles_of(launch):
                recs.append(oracle(raw).fan(H.make_cfg(eq, src=tuple(src), **cfg), th, ph)[1])
    elif kind == "freqs":
        O = oracle(None)
        per_f = [O.fan(H.make_cfg(eq, freq=f, **cfg), th, ph)[1] for f in launch["freqs"]]
        recs.append(per_f[0])
        atten = np.stack([r[:, :, H.REC["ATTEN"]] for r in per_f])
    elif kind == "gridens":
        for m, files in enumerate(write_grid_members(str(tmpdir))):
            if m == 0 and member0 is not None:
                assert LAUNCHES["3drd"]["params"] == prm
                recs.append(np.asarray(member0))
                continue
            O = H.Oracle(eq, met=None)
            O.load_grid(*files)
            recs.append(O.fan(H.make_cfg(eq, **cfg), th, ph)[1])
    else:
        O = H.Oracle(eq, met=None)
        O.load_grid(*MC.write_grid(kind, str(tmpdir)))
        recs.append(O.fan(H.make_cfg(eq, **cfg), th, ph)[1])
    rec = np.stack(recs)
    if atten is None:
        atten = rec[0, :, :, H.REC["ATTEN"]][None]
    return rec, MR.level_numpy(rec, atten, prm["calc_amp"]), th, ph, nt, nph


def stations_and_tubemap(ctx, nt, nph, tube_first):
    """the station lists at SMALL_STATIONS and the tube map on SMALL_GRID of the context's launch, in either order: (hits, rows, level), layers"""
    def lists():
        return ctx.stations(sta=SMALL_STATIONS, n_theta=nt, n_phi=nph, edge_max=SMALL_GRID["edge_max"], cap=SMALL_CAP)

    def layers():
        return ctx.tubemap(**TR.spec(n_theta=nt, n_phi=nph, **SMALL_GRID))

    if tube_first:
        m = layers()
        return lists(), m
    return lists(), layers()


def small_lattice_step(ctx, make_ctx, what=""):
    """The landing table is one table per context, formed by whichever of stations() and tubemap() asks first after a launch (geoac_stations.hip).
    `ctx` holds a completed 13 x 9 launch of SC.PARITY_LATTICE; make_ctx() gives a context set up alike with no launch.  After a 7 x 5 launch on
    `ctx` (a table larger than its launch) the lists and layers are the same bits whichever module asks first - on `ctx` the stations, on a second
    context that saw the same two launches the tube map - and equal those of a context that only ever saw the 7 x 5 launch.  Then the 13 x 9
    launch again: on `ctx` (a stale table) and on the 7 x 5 context (a regrown table, the tube map asking first) the first results come back.
    Returns the 7 x 5 results."""
    import station_reference as SR

    def same(got, want, why):
        SR.assert_lists_equal(got[0], want[0])
        TR.assert_layers_equal(got[1], want[1], what + " " + why)

    th, ph, nt, nph = SC.lattice(**SC.PARITY_LATTICE)
    ths, phs, nts, nphs = SC.lattice(**SMALL_LATTICE)
    assert (nts, nphs) == (7, 5)
    assert np.array_equal(ths.reshape(nphs, nts), th.reshape(nph, nt)[::2, ::2]) and np.array_equal(phs.reshape(nphs, nts), ph.reshape(nph, nt)[::2, ::2])
    second, fresh = make_ctx(), make_ctx()
    first = stations_and_tubemap(ctx, nt, nph, tube_first=False)
    second.run(th, ph)
    same(stations_and_tubemap(second, nt, nph, tube_first=True), first, "13 x 9, the tube map first")
    for c in (ctx, second, fresh):
        c.run(ths, phs)
    small = stations_and_tubemap(ctx, nts, nphs, tube_first=False)
    same(stations_and_tubemap(second, nts, nphs, tube_first=True), small, "7 x 5, the tube map first")
    same(stations_and_tubemap(fresh, nts, nphs, tube_first=False), small, "7 x 5 on a context that saw nothing else")
    assert small[1]["count"].shape != first[1]["count"].shape or not np.array_equal(small[1]["count"], first[1]["count"])      # (another launch, other layers)
    ctx.run(th, ph)
    same(stations_and_tubemap(ctx, nt, nph, tube_first=False), first, "13 x 9 again")
    fresh.run(th, ph)
    same(stations_and_tubemap(fresh, nt, nph, tube_first=True), first, "13 x 9 after 7 x 5, the tube map first")
    second.close()
    fresh.close()
    return small
