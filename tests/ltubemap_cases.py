"""The cases of the level-tube-map tests: launch set-ups, level lists and grid literals, shared by tests/test_ltubemap_host.py (which proves on
the CPU oracle's path rows that every grid meets the non-vacuity conditions) and tests/test_gpu_ltubemap.py (which runs them on the device).
Launches are the small lattices of tests/test_gpu_lstations.py (12 x 8 through ToyAtmo, 6 x 5 on the 5 x 5 grids; one bounce, range limit 300 km)
with the members of tests/tubemap_cases.py, and a 30 x 72 full-circle lattice from a source at longitude 179.  Grid extents, masks and edge_max
were chosen from the oracle's crossing points; they are literals, not derived from the code under test."""
import numpy as np

import harness as H
import ltubemap_reference as LT
import map_cases as MC
import station_cases as SC
import tubemap_cases as TC

LEVELS = [20.0, 35.0, 110.0]
TOY = dict(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
LATTICE_12x8 = dict(theta_min=10.0, theta_max=43.0, theta_step=3.0, phi_min=-125.0, phi_max=-55.0, phi_step=10.0)
LATTICE_6x5 = dict(theta_min=10.0, theta_max=35.0, theta_step=5.0, phi_min=-118.0, phi_max=-62.0, phi_step=14.0)
LATTICE_CIRCLE = dict(theta_min=10.0, theta_max=39.0, theta_step=1.0, phi_min=-180.0, phi_max=175.0, phi_step=5.0)          # 30 x 72, phi_periodic
WRAP_SRC = (0.0, 30.0, 179.0)
FREQS = (0.5, 2.0)
SPHERICAL = (H.EQ_GLOBAL, H.EQ_GLOBAL_RNGDEP)

LAUNCHES = {
    "3d": dict(kind="plain", eq=H.EQ_3D, params=TOY, lattice=LATTICE_12x8),
    "global": dict(kind="plain", eq=H.EQ_GLOBAL, params=TOY, lattice=LATTICE_12x8),
    "3drd": dict(kind="3drd", eq=H.EQ_3D_RNGDEP, params=dict(TOY, src=(0.0, 0.0, 0.0)), lattice=LATTICE_6x5),
    "globalrd": dict(kind="globalrd", eq=H.EQ_GLOBAL_RNGDEP, params=dict(TOY, src=(0.0, 31.0, 0.0)), lattice=LATTICE_6x5),
    "ensemble3": dict(kind="ensemble", eq=H.EQ_GLOBAL, params=TOY, lattice=LATTICE_12x8),
    "sources2x2": dict(kind="sources", eq=H.EQ_GLOBAL, sources=TC.TUBE_SOURCES, n_prof=2, params=TOY, lattice=LATTICE_12x8),
    "gridens2": dict(kind="gridens", eq=H.EQ_3D_RNGDEP, params=dict(TOY, src=(0.0, 0.0, 0.0)), lattice=LATTICE_6x5),
    "freqs2": dict(kind="freqs", eq=H.EQ_GLOBAL, freqs=FREQS, params=TOY, lattice=LATTICE_12x8),
    "circle": dict(kind="plain", eq=H.EQ_GLOBAL, params=dict(TOY, src=WRAP_SRC), lattice=LATTICE_CIRCLE),
    # one level at 46 km on the ragged grid, where a ray turns below it on leg 0 and passes it on leg 1 while its lattice neighbours pass it on both
    "globalrd46": dict(kind="globalrd", eq=H.EQ_GLOBAL_RNGDEP, params=dict(TOY, src=(0.0, 31.0, 0.0), range_limit=600.0), lattice=LATTICE_6x5, levels=[46.0]),
}

# grids (at most 32 x 48 cells).  Within 300 km of the source the 12 x 8 fan passes the three levels at x -300 .. -15, |y| < 170 km (Cartesian) and
# lat 28.4 .. 31.5, lon -3.1 .. -0.1 from (30, 0)
GRID_3D = dict(origin=(-312.0, -180.0), step=(13.0, 9.0), n=(24, 40), edge_max=120.0)
GRID_GLOBAL = dict(origin=(28.2, -3.3), step=(0.15, 0.085), n=(24, 40), edge_max=1.2)
GRID_3DRD = dict(origin=(-312.0, -180.0), step=(13.0, 9.0), n=(24, 40), edge_max=160.0)
GRID_GLOBALRD = dict(origin=(29.2, -3.3), step=(0.15, 0.085), n=(24, 40), edge_max=1.6)
GRID_2SRC = dict(origin=(28.0, -5.4), step=(0.16, 0.12), n=(32, 48), edge_max=1.2)                        # the two sources of TC.TUBE_SOURCES
# lon -180 .. -168: the fan from lon 179 passes the levels at 175.9 .. 182.1 (the state's longitude is continuous), its part beyond 180 is on the
# grid modulo 360
GRID_CIRCLE = dict(origin=(27.0, -180.0), step=(0.1875, 0.0625), n=(32, 48), edge_max=1.2, wrap_lon=True, phi_periodic=True)
GRID_SLOT_MIX = dict(origin=(31.0, -4.4), step=(0.075, 0.05), n=(24, 40), edge_max=1.6)                    # around the leg-1 passages of rays 18, 19, 25
GRID_FINE = dict(origin=(29.0, -3.2), step=(0.0625, 0.0625), n=(32, 48), edge_max=1.2)                   # cells several times smaller than the triangles
GRID_COARSE = dict(origin=(27.6, -4.0), step=(0.8, 0.6), n=(6, 7), edge_max=1.2)                         # cells larger than most triangles
GRID_HALF_OFF = dict(origin=(30.0, -2.0), step=(0.0625, 0.0625), n=(24, 40), edge_max=1.2)               # the crossings end inside the grid

ALL = dict(level_mask=0b111, ord_max=2)
CASES = {
    "3d": dict(launch="3d", spec=dict(GRID_3D, **ALL)),
    "global": dict(launch="global", spec=dict(GRID_GLOBAL, **ALL)),
    "3drd": dict(launch="3drd", spec=dict(GRID_3DRD, **ALL)),
    "globalrd": dict(launch="globalrd", spec=dict(GRID_GLOBALRD, **ALL)),
    "ensemble3": dict(launch="ensemble3", spec=dict(GRID_GLOBAL, **ALL)),
    "sources2x2": dict(launch="sources2x2", spec=dict(GRID_2SRC, **ALL)),
    "gridens2": dict(launch="gridens2", spec=dict(GRID_3DRD, **ALL)),
    "freqs2": dict(launch="freqs2", spec=dict(GRID_GLOBAL, **ALL)),
    "circle-wrap": dict(launch="circle", spec=dict(GRID_CIRCLE, level_mask=0b101, ord_max=1)),
    # neighbours whose leg-0 passages differ: the leg-1 passage sits in record slot 0 of one corner and in slot 2 of the others (mixed_slot_hits)
    "slot-mix": dict(launch="globalrd46", spec=dict(GRID_SLOT_MIX, level_mask=0b1, ord_max=1)),
    "fine": dict(launch="global", spec=dict(GRID_FINE, **ALL), cooperative=True),
    "coarse": dict(launch="global", spec=dict(GRID_COARSE, **ALL)),
    "half-off": dict(launch="global", spec=dict(GRID_HALF_OFF, **ALL)),
    "dir-up": dict(launch="global", spec=dict(GRID_GLOBAL, dir_mask=1, **ALL)),
    "dir-down": dict(launch="global", spec=dict(GRID_GLOBAL, dir_mask=2, **ALL)),
    "level-1": dict(launch="global", spec=dict(GRID_GLOBAL, level_mask=0b010, ord_max=2)),
    "levels-0-2": dict(launch="global", spec=dict(GRID_GLOBAL, level_mask=0b101, ord_max=2)),
    "leg-min-1": dict(launch="global", spec=dict(GRID_GLOBAL, leg_min=1, level_mask=0b011, ord_max=2)),      # (leg 1 ends below 110 km within the range limit)
    "ord-1": dict(launch="global", spec=dict(GRID_GLOBAL, level_mask=0b111, ord_max=1)),
    "edge-max": dict(launch="global", spec=dict(GRID_GLOBAL, **dict(ALL, edge_max=0.45))),               # removes the stretched triangles
}
# the selected levels (by position in the layers) on which a case claims cells with COUNT >= 2: every case not named here claims it on all
MULTIPATH = {"3drd": (0, 1), "globalrd": (0, 1), "gridens2": (0, 1), "coarse": (0,), "half-off": (0, 1), "dir-up": (0, 1)}


def lattice_of(launch):
    return SC.lattice(**launch["lattice"])


def spec_of(case, nt, nph, **overrides):
    return LT.spec(n_theta=nt, n_phi=nph, **dict(case["spec"], **overrides))


def oracle_crossings(launch, tmpdir):
    """member 0 of the launch on the CPU oracle: its paths through the restatement of k_levels (tests/levels_reference.py); crossing counts
    [1][n_rays][L], records [1][n_rays][L][8][12], angles, lattice shape, legs.  A grid ensemble's member 0 is the "3drd" grid itself, an
    ensemble's or a source set's the first profile at the first source, a frequency set's its first frequency."""
    import levels_reference as LV
    eq, kind, prm = launch["eq"], launch["kind"], launch["params"]
    th, ph, nt, nph = lattice_of(launch)
    cfg = dict(bounces=prm["bounces"], calc_amp=False, range_limit=prm["range_limit"])
    if "src" in prm:
        cfg["src"] = prm["src"]
    if kind == "sources":
        cfg["src"] = tuple(launch["sources"][0])
    if kind == "freqs":
        cfg["freq"] = launch["freqs"][0]
    if kind in ("3drd", "globalrd", "gridens"):
        O = H.Oracle(eq, met=None)
        O.load_grid(*MC.write_grid("3drd" if kind == "gridens" else kind, str(tmpdir)))
    else:
        raw = TC.profiles_of(dict(launch, n_prof=launch.get("n_prof", 1)))[0]
        O = H.Oracle(eq, H.TOYATMO if raw is None else None)
        if raw is not None:
            O.load_arrays(*raw)
    c = H.make_cfg(eq, **cfg)
    count, lrec = LV.restate_fan(eq, [O.trace_path(c, t, p) for t, p in zip(th, ph)], launch.get("levels", LEVELS), 8)
    return count[None], lrec[None], th, ph, nt, nph, prm["bounces"] + 1


def mixed_slot_hits(eq, count, lrec, th, ph, legs, sp):
    """the hits of member 0 (rows of the level-station restatement at the centres) whose crossing triangle holds the row's branch in different record
    slots at its three corners: a walk that matched corners by slot, or read a corner's record through another corner's slot, gets these wrong"""
    import lstation_reference as LS
    import station_reference as SR
    sta, lv = LT.stations_of(sp)
    lsp = LT.lstation_spec_of(sp)
    hits, rows = LS.reference_level_stations(eq, count[:1], lrec[:1], th, ph, legs, lsp, sta, lv)
    c0, c1, slot, present = LS.branch_table(eq, count[:1], lrec[:1], lsp, legs)
    tri = SR.triangles(lsp)
    n = 0
    for k in np.flatnonzero(hits[0]):
        for row in rows[0, k, :int(hits[0, k])]:
            b = ((int(row[LS.LSTA["LEG"]]) - sp["leg_min"]) * 2 + (0 if row[LS.LSTA["DIR"]] > 0 else 1)) * sp["ord_max"] + int(row[LS.LSTA["ORD"]])
            s3 = slot[0, lv[k], b][tri[int(row[LS.LSTA["TRI"]])]]
            n += int(len(set(s3.tolist())) > 1)
    return n


def check_non_vacuity(layers, name, m=0):
    """the conditions every case asserts of member m of its reference map (conditions, not measurements): on every selected level cells with COUNT 0
    and 1 occur, cells with COUNT >= 2 on the levels where the case claims multipath, and no centre has more hits than a level-station list holds.
    The conditions are per selected level, not per branch: COUNT has no branch axis.  The branch planes are told apart by the cases "dir-up" and
    "dir-down" (each direction's planes alone, non-empty on every level: tests/test_ltubemap_host.py), "leg-min-1" (leg 1 alone) and by FIRST, which
    names the branch of every reached cell and is compared bit for bit."""
    per = LT.counts_per_level(layers, m)
    claim = MULTIPATH.get(name, range(len(per)))
    for ls, (n0, n1, n2) in enumerate(per):
        assert n0 > 0 and n1 > 0 and (n2 > 0 or ls not in claim), f"{name}, selected level {ls}: cells with COUNT 0 / 1 / >= 2: {n0} / {n1} / {n2}"
    assert int(layers["count"].max()) <= LT.CAP, f"{name}: a centre has {int(layers['count'].max())} hits"
    return per


# ---- the closed form: the raised-ground medium of tests/raised_ground.py (imports only) on the Cartesian sets ----
RG_CELLS = (32, 48)
RG_SPAN = 150.0                                        # [km] the grid's width: the outer ring at 8 km lies 68 km from the source


def rg_spec(eq):
    """32 x 48 cells about the source, the origin moved by an irrational part of a cell so that no centre lies on a lattice edge (RGD.FRAC); levels 8
    and 15 km, leg 0, downward.  edge_max removes no triangle: the longest side is the outer ring's chord to the next ring, below 40 km"""
    import raised_ground as RGD
    step = (RG_SPAN / RG_CELLS[0], RG_SPAN / RG_CELLS[1])
    origin = tuple(RGD.SRC[eq][k] - RG_SPAN / 2 + RGD.FRAC[k] * step[k] for k in (0, 1))
    return LT.spec(origin=origin, step=step, n=RG_CELLS, n_theta=RGD.N_THETA, n_phi=RGD.N_PHI, edge_max=60.0, level_mask=0b11, phi_periodic=True, leg_max=0, dir_mask=2)


def check_raised_ground(eq, layers, count, lrec):
    """layers of rg_spec(eq) and the crossing tables count [360][2], lrec [360][2][cap][12] of the 15 x 24 downward lattice launched with
    RGD.LEVEL_PARAMS.  The rays are straight: the lattice's quadrilaterals tile the region between the ring polygons of theta = -10 and theta = -80
    at each level, so COUNT is the difference of the two winding numbers (RGD.winding_number: plain numpy, not the triangle rule) at every centre
    farther than MARGIN_CELLS from both polygons.  The travel time to a point X of the level is |X - s| / c, a convex function of the horizontal
    position whose Hessian is at most 1 / (c h), h the source's height above the level: a linear interpolant over a triangle of longest side e
    overestimates it by at most e^2 / (2 c h) and - the corners being exact to 1e-9 - does not underestimate it beyond that.  Returns per level
    (largest share of the bound used, lowest (TTIME_MIN - |X - s| / c) / TTIME_MIN)."""
    import raised_ground as RGD
    import station_reference as SR
    from levels_reference import LVL
    P0 = LVL["P0"]
    sp = rg_spec(eq)
    nt, nph = RGD.N_THETA, RGD.N_PHI
    assert (count == 2).all() and (lrec[:, :, 0, LVL["LEG"]] == 0).all() and (lrec[:, :, 0, LVL["DIR"]] == -1.0).all()          # slot 0: leg 0, downward
    cen = RGD.cell_centres(sp)
    tri = SR.triangles(sp)
    n_tri = len(tri)
    src = np.array(RGD.SRC[eq])
    worst = {}
    for ls, z in enumerate(RGD.LEVELS):
        px, py = lrec[:, ls, 0, P0].reshape(nph, nt), lrec[:, ls, 0, P0 + 1].reshape(nph, nt)
        w_out, d_out = RGD.winding_number(cen[:, 0], cen[:, 1], px[:, -1], py[:, -1])          # theta = -10: the outer ring
        w_in, d_in = RGD.winding_number(cen[:, 0], cen[:, 1], px[:, 0], py[:, 0])              # theta = -80
        want = np.abs(w_out) - np.abs(w_in)
        keep = (d_out > RGD.MARGIN_CELLS * max(sp["step"])) & (d_in > RGD.MARGIN_CELLS * max(sp["step"]))
        c = layers["count"][0, ls].reshape(-1).astype(np.int64)
        assert keep.mean() >= 0.99 and (want[keep] == 1).sum() >= 40 and (want[keep] == 0).sum() >= 40, (z, keep.mean(), (want == 1).sum(), (want == 0).sum())
        bad = keep & (c != want)
        assert not bad.any(), f"level {z}: {int(bad.sum())} centres: COUNT {c[bad][:8].tolist()} where the ring polygons say {want[bad][:8].tolist()}, first at {int(np.flatnonzero(bad)[0])}"
        assert np.array_equal(layers["reach"][ls].reshape(-1), (c > 0).astype(np.uint32))
        some = np.flatnonzero(c > 0)
        first = layers["first"][0, ls].reshape(-1)[some]
        assert (first // n_tri == 1).all()                                          # b = ((0 - 0) * 2 + 1) * 1 + 0: leg 0, downward, ordinal 0
        corners = tri[first % n_tri]                                                # [n][3] rays
        X, Y = lrec[:, ls, 0, P0][corners], lrec[:, ls, 0, P0 + 1][corners]
        e = np.max([np.hypot(X[:, a] - X[:, b], Y[:, a] - Y[:, b]) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0)
        h = src[2] - z
        exact = np.sqrt((cen[some, 0] - src[0]) ** 2 + (cen[some, 1] - src[1]) ** 2 + h * h) / RGD.C
        tmin = layers["ttime_min"][0, ls].reshape(-1)[some]
        over = tmin - exact
        bound = e * e / (2.0 * RGD.C * h)
        worst[z] = (float((over / bound).max()), float((over / tmin).min()))
        assert (over >= -1e-9 * tmin).all() and (over <= bound).all(), (z, worst[z], int(np.argmax(over / bound)))
    return worst


def rg_figures(worst):
    return ", ".join(f"level {z} km: largest share of e^2 / (2 c h) used {w[0]:.4f}, lowest (TTIME_MIN - |X - s| / c) / TTIME_MIN {w[1]:.3e}" for z, w in worst.items())
