"""Level stations on the device (include/geoac_lstations.h, FanContext.level_stations): hits and rows against the numpy restatement
(tests/lstation_reference.py) of the same launch's fetched crossing records, bit for bit - on three equation sets, over two chunks and the periodic
seam, under both overflows - and the estimates themselves against a closed form, against a re-launch, against the ground lists of
geoac_fan_stations; members against plain contexts; repeated calls, isolation from the launch, and the refusals.
Fans are small lattices through ToyAtmo (one bounce, range limit 300 km) unless a test says otherwise.  Every test runs under a time limit of its own
(a watchdog ends the process: a hung GPU step is not waited for and nothing is retried)."""
import faulthandler

import numpy as np
import pytest

import harness as H
import jet_data as JD
import known_answers as K
import lstation_reference as LS
import rngdep_data as RD
import station_cases as SC
import station_reference as SR
from levels_reference import LVL
from parity import compare_records

pytestmark = pytest.mark.gpu
S = LS.LSTA
P0 = LVL["P0"]
STEP_LIMIT_S = 120
LEVELS = [20.0, 35.0, 110.0]
TOY = dict(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
SPHERICAL = (H.EQ_GLOBAL, H.EQ_GLOBAL_RNGDEP)
# theta 10 .. 43 in 12 steps of 3, 8 azimuths around the westward direction ToyAtmo's stratospheric duct looks in
LATTICE_12x8 = dict(theta_min=10.0, theta_max=43.0, theta_step=3.0, phi_min=-125.0, phi_max=-55.0, phi_step=10.0)
LATTICE_6x5 = dict(theta_min=10.0, theta_max=35.0, theta_step=5.0, phi_min=-118.0, phi_max=-62.0, phi_step=14.0)
# the physics fans: theta 10 .. 40 step 1, 9 azimuths
LATTICE_31x9 = dict(theta_min=10.0, theta_max=40.0, theta_step=1.0, phi_min=-110.0, phi_max=-70.0, phi_step=5.0)
EDGE_FEW_CELLS = {H.EQ_3D: 60.0, H.EQ_GLOBAL: 0.55}          # [km] / [deg]: a few cells of the 1 x 5 degree lattice at these levels


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


def _run(ctx, th, ph):
    """launch and fetch: records [M][n_rays][legs][32], counts [M][n_rays][L], crossing records [M][n_rays][L][cap][12]"""
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    return _members(rec, 3), _members(count, 2), _members(lrec, 4)


def _toy_ctx(G, eq, levels=LEVELS, cap=8, **params):
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(**dict(TOY, **params))
    if levels is not None:
        ctx.set_levels(levels, cap=cap)
    return ctx


def _source_xy(ctx):
    s = list(ctx.params.src)
    return (s[1], s[2]) if ctx.eqset in SPHERICAL else (s[0], s[1])


def _offset(eq, src_xy, r, az_deg):
    """the point at distance r (axis units) and azimuth az from src_xy, in the map's axes"""
    a = np.radians(az_deg)
    if eq in SPHERICAL:
        return np.stack([src_xy[0] + r * np.cos(a), src_xy[1] + r * np.sin(a) / np.cos(np.radians(src_xy[0]))], axis=-1)
    return np.stack([src_xy[0] + r * np.sin(a), src_xy[1] + r * np.cos(a)], axis=-1)


def _ring(eq, src_xy, count, lrec, ph, level, n=20):
    """n stations around the source on one level: azimuths spread over the fan's sector, radii the quantiles of the distances at which member 0's rays
    pass the level (from the fetched crossing records, not from the lists under test)"""
    c0, c1 = LS.crossing_points(eq, lrec[0, :, level])
    kept = np.arange(lrec.shape[3])[None, :] < np.minimum(count[0, :, level], lrec.shape[3])[:, None]
    dx, dy = c0[kept] - src_xy[0], c1[kept] - src_xy[1]
    if eq in SPHERICAL:
        dy = dy * np.cos(np.radians(src_xy[0]))
    d = np.hypot(dx, dy)
    assert d.size >= n
    r = np.quantile(d, (np.arange(n) + 0.5) / n)
    az = np.linspace(ph.min() + 2.0, ph.max() - 2.0, n)[np.random.default_rng(3 + level).permutation(n)]
    return _offset(eq, src_xy, r, az)


def _served_triangles(eq, count, lrec, sp, legs, level):
    """member 0, the first branch of `level` that has any: the crossing points [n][3][2] of the even triangles (a, b, c) whose three corners all hold it, in
    key order - from the fetched crossing records, not from the lists under test"""
    c0, c1, slot, present = LS.branch_table(eq, count[:1], lrec[:1], sp, legs)
    tri = SR.triangles(sp)[0::2]
    for b in range(present.shape[2]):
        ok = np.flatnonzero(present[0, level, b][tri].all(axis=1))
        if len(ok):
            return np.stack([c0[0, level, b][tri[ok]], c1[0, level, b][tri[ok]]], axis=2)
    raise AssertionError(f"no ray triple passes level {level}")


def _stations_24(eq, src_xy, count, lrec, ph, sp, legs, level):
    """24 stations of one level: the ring, two stations bit for bit on a crossing point (corner a of one served triangle, corner c of another, both from
    the middle of the lattice), one midway between two neighbouring crossing points of one azimuth (corners a, b), one 5 000 km away"""
    ring = _ring(eq, src_xy, count, lrec, ph, level)
    p = _served_triangles(eq, count, lrec, sp, legs, level)
    n = len(p)
    mid = 0.5 * (p[(2 * n) // 3, 0] + p[(2 * n) // 3, 1])
    far = np.array([src_xy[0], src_xy[1] + 52.0]) if eq in SPHERICAL else np.array([src_xy[0] + 5000.0, src_xy[1]])
    return np.concatenate([ring, p[n // 2, 0][None], p[n // 3, 2][None], mid[None], far[None]])


def _check(ctx, eq, count, lrec, th, ph, legs, sta, level_of, **spec_kw):
    got = ctx.level_stations(sta=sta, level_of=level_of, **spec_kw)
    want = LS.reference_level_stations(eq, count, lrec, th, ph, legs, LS.spec(**spec_kw), sta, level_of)
    LS.assert_lists_equal(got, want)
    return got


# ---------------------------------------------------------------- 1. bit for bit against the restatement
def _parity_ctx(G, eq, tmp):
    if eq == H.EQ_3D_RNGDEP:
        ctx = G.FanContext(eq, device=0)
        ctx.load_grid(*RD.write_grid(str(tmp), short_paths=False))
        ctx.set_params(**dict(TOY, src=(0.0, 0.0, 0.0)))
        ctx.set_levels(LEVELS)
        return ctx, SC.lattice(**LATTICE_6x5)
    return _toy_ctx(G, eq), SC.lattice(**LATTICE_12x8)


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP])
def test_lists_equal_reference(G, eq, tmp_path):
    ctx, (th, ph, nt, nph) = _parity_ctx(G, eq, tmp_path)
    rec, count, lrec = _run(ctx, th, ph)
    legs = rec.shape[2]
    sp = LS.spec(nt, nph, ord_max=2, cap=12)
    src = _source_xy(ctx)
    sta = np.concatenate([_stations_24(eq, src, count, lrec, ph, sp, legs, l) for l in range(3)])
    level_of = np.repeat([0, 1, 2], 24)
    hits, rows = _check(ctx, eq, count, lrec, th, ph, legs, sta, level_of, n_theta=nt, n_phi=nph, ord_max=2, cap=12)
    assert hits.shape == (1, 72) and rows.shape == (1, 72, 12, 16)
    print(f"{H.EQ_NAMES[eq]}: hits per level {[int(hits[0, 24 * l:24 * l + 24].sum()) for l in range(3)]}, stations with hits {int((hits[0] > 0).sum())} of 72, "
          f"most {int(hits.max())}, branches seen {sorted(set(map(tuple, rows[0][rows[0][..., S['W0']] != 0][:, :3].astype(int).tolist())))}")
    for l in range(3):
        h = hits[0, 24 * l:24 * l + 24]
        assert h[20] >= 1 and h[21] >= 1, (l, h)                                  # a station on a crossing point lies in every served triangle around it
        assert h[23] == 0 and h[:20].sum() > 0, (l, h)                              # the far station sees nothing, the ring something
    assert (rows[..., S["LEG"]] == 1).any() and (rows[..., S["DIR"]] == -1.0).any()
    # one leg, one ordinal, a finite edge: bit-identical too, and it only ever removes hits
    edge = 0.6 if eq in SPHERICAL else 65.0
    tight, trows = _check(ctx, eq, count, lrec, th, ph, legs, sta, level_of, n_theta=nt, n_phi=nph, leg_min=1, leg_max=1, ord_max=1, edge_max=edge, cap=12)
    assert (tight <= hits).all() and int(tight.sum()) < int(hits.sum())
    assert (trows[..., S["LEG"]][trows[..., S["W0"]] != 0] == 1).all()
    ctx.close()


# ---------------------------------------------------------------- 2. two chunks and the seam
def test_two_chunks_and_the_periodic_seam(G):
    """30 inclinations x 72 azimuths over the whole circle: 29 x 72 = 2 088 cells, one full chunk of 2 048 and a tail of 40 (a partial trip).  Every station is
    a convex blend of the four crossing points of one lattice cell (leg 0, upward, from the fetched records), so it lies inside the cell's image; four cells are
    in the seam column 71 -> 0, which is also the second chunk"""
    eq = H.EQ_GLOBAL
    th, ph, nt, nph = SC.lattice(theta_min=10.0, theta_max=39.0, theta_step=1.0, phi_min=-180.0, phi_max=175.0, phi_step=5.0)
    assert (nt, nph) == (30, 72)
    ctx = _toy_ctx(G, eq, levels=[20.0])
    rec, count, lrec = _run(ctx, th, ph)
    sp = LS.spec(nt, nph, phi_periodic=True, ord_max=1, cap=6)
    c0, c1, slot, present = LS.branch_table(eq, count, lrec, sp, rec.shape[2])
    assert present[0, 0, 0].all()                                                   # branch 0 = (leg 0, up, 0): every ray climbs through 20 km
    tri = SR.triangles(sp)
    cells = [(i, 71) for i in (2, 9, 17, 26)] + [(i, j) for i, j in zip((0, 5, 11, 14, 19, 23, 28, 7, 13, 21, 4, 16), (0, 6, 13, 21, 29, 36, 44, 52, 59, 66, 70, 33))]
    sta = []
    for i, j in cells:
        a, b, c = tri[2 * (j * (nt - 1) + i)]
        d = tri[2 * (j * (nt - 1) + i) + 1][2]
        w = np.array([0.35, 0.3, 0.25, 0.1])                                       # (off the diagonal a - c: inside triangle (a, b, c) of a near-parallelogram)
        lon = c1[0, 0, 0][[a, b, c, d]]
        lon = lon[0] + SR._wrap180(lon - lon[0])
        sta.append([float(w @ c0[0, 0, 0][[a, b, c, d]]), float(w @ lon)])
    sta = np.array(sta)
    hits, rows = _check(ctx, eq, count, lrec, th, ph, rec.shape[2], sta, np.zeros(16, dtype=int), n_theta=nt, n_phi=nph, phi_periodic=True, ord_max=1, cap=6)
    kept = rows[0][rows[0][..., S["W0"]] != 0]
    print(f"2 088 cells: hits {hits[0].tolist()}, triangles {sorted(set(kept[:, S['TRI']].astype(int)))}")
    assert (hits[0] >= 1).all()
    own = [any(int(t) // 2 == j * (nt - 1) + i for t in rows[0, k, :min(int(hits[0, k]), 6), S["TRI"]]) for k, (i, j) in enumerate(cells)]
    assert all(own), own
    assert (kept[:, S["TRI"]] >= 2 * 71 * (nt - 1)).any() and (kept[:, S["TRI"]] >= 2 * 2048).any()          # the seam column; the second chunk
    seam = rows[0, :4, 0]
    assert ((seam[:, S["PHI"]] > 175.0) & (seam[:, S["PHI"]] < 180.0)).all()            # continuous with corner 0 (175), not an average of 175 and -180
    ctx.close()


# ---------------------------------------------------------------- 3. both overflows
def test_overflows_keep_the_first_rows_and_the_first_crossings(G):
    """the 20 km level lies in ToyAtmo's stratospheric duct: a ray that returns passes it four times in two legs.  With two crossings kept per (ray, level) the
    counts run past the cap, and the branches among the first two still hit"""
    eq = H.EQ_GLOBAL
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    ctx = _toy_ctx(G, eq, levels=[20.0], cap=2, range_limit=600.0)
    rec, count, lrec = _run(ctx, th, ph)
    legs = rec.shape[2]
    assert lrec.shape[3] == 2 and (count > 2).sum() >= 6, count[0, :, 0]
    sp = LS.spec(nt, nph, ord_max=2, cap=12)
    src = _source_xy(ctx)
    past = np.flatnonzero(count[0, :, 0] > 2)
    c0, c1 = LS.crossing_points(eq, lrec[0, past, 0, 0])                              # the first kept crossing of rays whose count ran past the cap
    sta = np.concatenate([_stations_24(eq, src, count, lrec, ph, sp, legs, 0), np.stack([c0, c1], axis=1)])
    lv = np.zeros(len(sta), dtype=int)
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2)
    full = _check(ctx, eq, count, lrec, th, ph, legs, sta, lv, cap=12, **kw)
    assert 3 <= int(full[0].max()) <= 12, full[0]
    assert (full[0][0, 24:] >= 1).all()                                               # the kept branches of a ray past the crossing cap still hit
    for cap in (1, 2):
        h, r = _check(ctx, eq, count, lrec, th, ph, legs, sta, lv, cap=cap, **kw)
        assert np.array_equal(h, full[0]) and (h > cap).any()
        assert np.array_equal(SR.bits(r), SR.bits(full[1][:, :, :cap]))
    ctx.close()


# ---------------------------------------------------------------- 4. closed form
THETA_STAR = np.array([13.7, 21.3, 28.9, 33.1, 41.8, 47.2, 52.6, 58.3, 63.9, 68.4, 73.6, 77.7])
PHI_STAR = np.array([21.3, 52.7, 97.9, 131.2, 163.4, 201.6, 229.3, 258.8, 291.1, 318.7, 333.9, 351.2])


def _closed_form(G, fan):
    z, T, u, v, rho = K.isothermal_profile()
    th, ph, nt, nph = SC.lattice(**fan)
    levels = [10.0, 30.0]
    ctx = G.FanContext(G.EQ_3D, device=0)
    ctx.upload_atmo_1d(z, T, u, v, rho)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0, src=(0.0, 0.0, 0.0))
    ctx.set_levels(levels)
    ctx.run(th, ph)
    t, a = np.radians(np.tile(THETA_STAR, 2)), np.radians(np.tile(PHI_STAR, 2))
    zl = np.repeat(levels, 12)
    sta = (zl / np.tan(t))[:, None] * np.stack([np.sin(a), np.cos(a)], axis=1)
    hits, rows = ctx.level_stations(sta=sta, level_of=np.repeat([0, 1], 12), n_theta=nt, n_phi=nph, phi_periodic=True, ord_max=2, cap=4)
    ctx.close()
    c = np.sqrt(K.GAM_R * 250.0)
    want_t = np.sqrt((sta * sta).sum(axis=1) + zl * zl) / c                            # |station - source| / c
    return hits[0], rows[0], want_t


def test_closed_form_and_convergence(G):
    """isothermal windless medium, ground source, straight rays: the station at z_l / tan(theta*) (sin phi*, cos phi*) on level z_l is reached by the ray
    (theta*, phi*) alone, upward, at t = |station - source| / c.  With both lattice steps halved the median errors of THETA, PHI and TTIME must each fall by
    more than 2x (a first-order scheme gives 2, a second-order interpolant predicts 4).  Measured on an MI355X: see DESIGN 8m."""
    coarse = dict(theta_min=10.0, theta_max=80.0, theta_step=5.0, phi_min=0.0, phi_max=345.0, phi_step=15.0)
    fine = dict(theta_min=10.0, theta_max=80.0, theta_step=2.5, phi_min=0.0, phi_max=352.5, phi_step=7.5)
    err = {}
    for name, fan, dth, dph in (("coarse", coarse, 5.0, 15.0), ("fine", fine, 2.5, 7.5)):
        hits, rows, want_t = _closed_form(G, fan)
        assert (hits == 1).all(), (name, hits)
        r = rows[:, 0]
        assert (r[:, S["LEG"]] == 0).all() and (r[:, S["DIR"]] == 1.0).all() and (r[:, S["ORD"]] == 0).all()
        e_th = np.abs(r[:, S["THETA"]] - np.tile(THETA_STAR, 2))
        e_ph = np.abs(SR._wrap180(r[:, S["PHI"]] - np.tile(PHI_STAR, 2)))
        e_t = np.abs(r[:, S["TTIME"]] - want_t)
        assert (e_th <= dth).all() and (e_ph <= dph).all(), (name, e_th.max(), e_ph.max())
        err[name] = [float(np.median(e)) for e in (e_th, e_ph, e_t)]
    ratios = [c / f for c, f in zip(err["coarse"], err["fine"])]
    print("closed form, median errors (THETA [deg], PHI [deg], TTIME [s]): 5 x 15 deg lattice " + ", ".join(f"{e:.4e}" for e in err["coarse"]) +
          "; 2.5 x 7.5 deg lattice " + ", ".join(f"{e:.4e}" for e in err["fine"]) + "; ratios " + ", ".join(f"{q:.3f}" for q in ratios))
    assert all(q > 2.0 for q in ratios), ratios


# ---------------------------------------------------------------- 5. re-launch
def _steep(eq, count, lrec, legs, sp, hits, rows, sta, level_of):
    """(station, row index, longest side) of every kept row whose three corners pass the level with |P3| >= 0.3, and the number of kept rows"""
    out, n = [], 0
    for k in range(len(sta)):
        for j in range(min(int(hits[0, k]), sp["cap"])):
            n += 1
            _, side, recs = LS.crossing_triangle(eq, count, lrec, legs, sp, 0, rows[0, k, j], sta[k], int(level_of[k]))
            if (np.abs(recs[:, P0 + 3]) >= 0.3).all():
                out.append((k, j, side))
    return out, n


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_relaunched_estimates_pass_the_level_inside_their_triangle(G, eq):
    """every estimate whose corners pass the level steeply (vertical slowness |P3| >= 0.3: no corner turns at the level) is integrated again: the ray must
    hold the estimate's (LEG, DIR, ORD) branch and pass the level no farther from the station than the longest side of the estimate's own crossing triangle
    (the bound of the ground stations).  Worst miss / side measured on an MI355X: see DESIGN 8m."""
    th, ph, nt, nph = SC.lattice(**LATTICE_31x9)
    levels = [20.0, 35.0]
    ctx = _toy_ctx(G, eq, levels=levels)
    rec, count, lrec = _run(ctx, th, ph)
    legs = rec.shape[2]
    src = _source_xy(ctx)
    sta = np.concatenate([_ring(eq, src, count, lrec, ph, l) for l in range(2)])
    level_of = np.repeat([0, 1], 20)
    sp = LS.spec(nt, nph, ord_max=2, edge_max=EDGE_FEW_CELLS[eq], cap=16)
    hits, rows = ctx.level_stations(sta=sta, level_of=level_of, **sp)
    sel, n_rows = _steep(eq, count, lrec, legs, sp, hits, rows, sta, level_of)
    print(f"{H.EQ_NAMES[eq]}: {int(hits.sum())} hits, {n_rows} rows kept, {len(sel)} with steep corners")
    assert n_rows >= 10 and 2 * len(sel) >= n_rows
    est = np.array([rows[0, k, j] for k, j, _ in sel])
    _, count2, lrec2 = _run(ctx, est[:, S["THETA"]].copy(), est[:, S["PHI"]].copy())
    worst = 0.0
    for n, (k, j, side) in enumerate(sel):
        l = int(level_of[k])
        slot = LS.branch_of_ray(count2[0, n, l], lrec2[0, n, l], int(est[n, S["LEG"]]), est[n, S["DIR"]], int(est[n, S["ORD"]]))
        assert slot >= 0, (n, est[n, :3], "the re-launched ray does not hold the estimate's branch")
        c0, c1 = LS.crossing_points(eq, lrec2[0, n, l, slot])
        dx, dy = c0 - sta[k, 0], c1 - sta[k, 1]
        if eq in SPHERICAL:
            dy = SR._wrap180(dy)
        miss = float(np.hypot(dx, dy))
        worst = max(worst, miss / side)
        assert miss <= side, (n, est[n, :3], miss, side)
    print(f"{H.EQ_NAMES[eq]}: re-launch of {len(sel)} estimates, worst miss / longest side {worst:.4f}")
    ctx.close()


# ---------------------------------------------------------------- 6. against the ground lists
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_a_level_just_above_the_ground_agrees_with_the_ground_lists(G, eq):
    """the same fan with a level 0.05 km above z_grnd: where geoac_fan_stations and the downward branch of the same leg each have exactly one hit, the two
    estimates' THETA and PHI agree within one lattice step"""
    th, ph, nt, nph = SC.lattice(**LATTICE_31x9)
    ctx = _toy_ctx(G, eq, levels=[0.05, 20.0, 35.0])
    rec, count, lrec = _run(ctx, th, ph)
    sta = SC.draw_stations(eq, rec, n_near=60, n_far=2)
    g_hits, g_rows, _ = ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=8)
    l_hits, l_rows = ctx.level_stations(sta=sta, level_of=np.zeros(len(sta), dtype=int), n_theta=nt, n_phi=nph, ord_max=1, cap=16)
    n, worst = 0, [0.0, 0.0]
    for k in range(len(sta)):
        if g_hits[0, k] != 1 or l_hits[0, k] > 16:
            continue
        g = g_rows[0, k, 0]
        mine = l_rows[0, k, :int(l_hits[0, k])]
        mine = mine[(mine[:, S["DIR"]] == -1.0) & (mine[:, S["LEG"]] == g[SR.STA["LEG"]])]
        if len(mine) != 1:
            continue
        n += 1
        d_th, d_ph = abs(mine[0, S["THETA"]] - g[SR.STA["THETA"]]), abs(mine[0, S["PHI"]] - g[SR.STA["PHI"]])
        worst = [max(worst[0], d_th), max(worst[1], d_ph)]
        assert d_th <= 1.0 and d_ph <= 5.0, (k, d_th, d_ph)
    print(f"{H.EQ_NAMES[eq]}: {n} stations with one ground hit and one downward hit 0.05 km above it; largest difference THETA {worst[0]:.3e} deg, PHI {worst[1]:.3e} deg")
    assert n >= 3
    ctx.close()


# ---------------------------------------------------------------- 7. members
def _member_stations(eq, ctx, count, lrec, ph):
    src = _source_xy(ctx)
    return np.concatenate([_ring(eq, src, count, lrec, ph, l, n=12) for l in range(3)]), np.repeat([0, 1, 2], 12)


def _assert_member(got, m, one):
    assert np.array_equal(got[0][m], one[0][0]), m
    assert np.array_equal(SR.bits(got[1][m]), SR.bits(one[1][0])), m
    assert one[0].sum() > 0


def test_ensemble_members_equal_plain_contexts(G, tmp_path):
    """1-D ensemble of ToyAtmo's winds on the jet profile's nodes and JetAtmo itself"""
    eq = H.EQ_GLOBAL
    paths = [JD.write_toy_on_jet_nodes(str(tmp_path / "toy_on_jet.met")), JD.JET]
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=8)
    ctx = G.FanContext(eq, device=0)
    ctx.load_met_ensemble(paths, fmt=JD.FMT)
    ctx.set_params(**TOY); ctx.set_levels(LEVELS)
    rec, count, lrec = _run(ctx, th, ph)
    sta, lv = _member_stations(eq, ctx, count, lrec, ph)
    got = _check(ctx, eq, count, lrec, th, ph, rec.shape[2], sta, lv, **kw)
    ctx.close()
    assert got[0].shape == (2, 36)
    for m, path in enumerate(paths):
        one = G.FanContext(eq, device=0)
        one.load_met(path, fmt=JD.FMT)
        one.set_params(**TOY); one.set_levels(LEVELS)
        one.run(th, ph)
        _assert_member(got, m, one.level_stations(sta=sta, level_of=lv, **kw))
        one.close()
    assert not np.array_equal(got[1][0], got[1][1])


def test_source_set_members_equal_plain_contexts(G):
    eq = H.EQ_3D
    srcs = np.array([[0.0, 0.0, 0.0], [12.0, -30.0, 1.5]])
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=8)
    ctx = _toy_ctx(G, eq)
    ctx.set_sources(srcs)
    rec, count, lrec = _run(ctx, th, ph)
    sta, lv = _member_stations(eq, ctx, count, lrec, ph)
    got = _check(ctx, eq, count, lrec, th, ph, rec.shape[2], sta, lv, **kw)
    ctx.close()
    assert got[0].shape == (2, 36)
    for s in range(2):
        one = _toy_ctx(G, eq, src=tuple(srcs[s]))
        one.run(th, ph)
        _assert_member(got, s, one.level_stations(sta=sta, level_of=lv, **kw))
        one.close()
    assert not np.array_equal(got[1][0], got[1][1])


def test_grid_ensemble_members_equal_plain_contexts(G, tmp_path):
    """K = 2 grid ensemble, GEOAC_EQ_3D_RNGDEP; the plain contexts with one lane per ray (GRID_LANES=1), as tests/test_gpu_grid_ensemble.py compares"""
    eq = H.EQ_3D_RNGDEP
    th, ph, nt, nph = SC.lattice(**LATTICE_6x5)
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=8)
    p = dict(TOY, src=(0.0, 0.0, 0.0))
    base = G.FanContext(eq, device=0)
    g = base.load_grid(*RD.write_grid(str(tmp_path), short_paths=False))
    base.close()
    members = [dict(T=g["T"], u=g["u"], v=g["v"], rho=g["rho"]), dict(T=g["T"] + 3.0, u=g["u"] * 0.85, v=g["v"] * 0.85, rho=g["rho"])]
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([m[k] for m in members]) for k in ("T", "u", "v", "rho")])
    ctx.set_params(**p); ctx.set_levels(LEVELS)
    rec, count, lrec = _run(ctx, th, ph)
    sta, lv = _member_stations(eq, ctx, count, lrec, ph)
    got = _check(ctx, eq, count, lrec, th, ph, rec.shape[2], sta, lv, **kw)
    ctx.close()
    assert got[0].shape == (2, 36)
    for m in range(2):
        with G.options(GRID_LANES="1"):
            one = G.FanContext(eq, device=0)
            one.upload_atmo_3d(g["x"], g["y"], g["z"], *[members[m][k] for k in ("T", "u", "v", "rho")])
            one.set_params(**p); one.set_levels(LEVELS)
            one.run(th, ph)
            _assert_member(got, m, one.level_stations(sta=sta, level_of=lv, **kw))
            one.close()


def test_frequency_set_gives_the_lists_of_frequency_0(G):
    eq = H.EQ_GLOBAL
    freqs = (0.5, 2.0)
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=8)
    ctx = _toy_ctx(G, eq)
    ctx.set_frequencies(freqs)
    rec, count, lrec = _run(ctx, th, ph)
    sta, lv = _member_stations(eq, ctx, count, lrec, ph)
    got = _check(ctx, eq, count, lrec, th, ph, rec.shape[2], sta, lv, **kw)
    ctx.close()
    plain = _toy_ctx(G, eq, freq=freqs[0])
    plain.run(th, ph)
    _assert_member(got, 0, plain.level_stations(sta=sta, level_of=lv, **kw))
    plain.close()
    other = _toy_ctx(G, eq)                                                         # (ATTEN is the attenuation at that frequency, not at the default 0.1 Hz)
    other.run(th, ph)
    assert not np.array_equal(other.level_stations(sta=sta, level_of=lv, **kw)[1][..., S["ATTEN"]], got[1][..., S["ATTEN"]])
    other.close()


# ---------------------------------------------------------------- 8. calls and state
def test_repeated_calls_leave_the_launch_alone(G):
    eq = H.EQ_GLOBAL
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    ctx = _toy_ctx(G, eq)
    rec, count, lrec = _run(ctx, th, ph)
    legs = rec.shape[2]
    steps, epochs = ctx.total_steps(), ctx.timing()["epochs"]
    sta, lv = _member_stations(eq, ctx, count, lrec, ph)
    first = _check(ctx, eq, count, lrec, th, ph, legs, sta, lv, n_theta=nt, n_phi=nph, ord_max=2, cap=8)
    # other stations and another spec (another branch table: one leg, one ordinal), then the first again
    _check(ctx, eq, count, lrec, th, ph, legs, sta[::3], lv[::3], n_theta=nt, n_phi=nph, leg_min=1, leg_max=1, ord_max=1, edge_max=0.6, cap=3)
    LS.assert_lists_equal(_check(ctx, eq, count, lrec, th, ph, legs, sta, lv, n_theta=nt, n_phi=nph, ord_max=2, cap=8), first)
    ctx.stations(sta=sta, n_theta=nt, n_phi=nph, cap=4)                              # the ground lists live beside them
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=2, cap=8), first)
    assert ctx.level_stations_timing() > 0.0
    after, count2, lrec2 = _members(ctx.fetch()[0], 3), *(_members(a, t) for a, t in zip(ctx.fetch_levels(), (2, 4)))
    assert ctx.total_steps() == steps and ctx.timing()["epochs"] == epochs
    assert np.array_equal(SR.bits(after), SR.bits(rec)) and np.array_equal(count2, count) and np.array_equal(SR.bits(lrec2), SR.bits(lrec))
    ctx.close()


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_a_plain_context_does_not_change(G, golden, eq):
    """run() on a context that never calls the header and sets no levels: the golden parity records of tests/test_gpu_parity.py, under its comparison"""
    g = golden(eq)
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1, mode=0)
    rec, steps = ctx.run(g["theta"], g["phi"])
    assert steps == int(g["steps_amp1_mode0"])
    compare_records(rec, g["rec_amp1_mode0"], E=18 if eq == H.EQ_GLOBAL else 12, hidx=None if eq == H.EQ_GLOBAL else 2)
    ctx.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals(G):
    eq = H.EQ_GLOBAL
    th, ph, nt, nph = SC.lattice(**LATTICE_12x8)
    sta = np.array([[30.0, -1.0], [30.2, -2.0]])
    lv = [0, 2]
    kw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=4)
    ctx = _toy_ctx(G, eq, levels=None)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations: no completed launch"):
        ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations.*no levels set"):
        ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.set_levels(LEVELS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations.*no levels set"):          # (set, but not launched with)
        ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.launch()
    want = ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.set_levels([20.0, 35.0])
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations.*level list has changed"):
        ctx.level_stations(sta=sta, level_of=[0, 1], **kw)
    ctx.set_levels(LEVELS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations.*level list has changed"):          # (the same values again are still a change)
        ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.launch()
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, **kw), want)          # after a new launch the call works again
    # a bad spec or level index names its fault and leaves the current lists alone
    hits = np.zeros((1, 2), dtype=np.uint32)
    import ctypes
    for bad, bad_lv, word in ((dict(kw, cap=0), lv, "cap"), (dict(kw, cap=257), lv, "cap"), (dict(kw, ord_max=0), lv, "ord_max"), (dict(kw, edge_max=float("nan")), lv, "edge_max"),
                              (kw, [0, 3], "level_of"), (kw, [-1, 0], "level_of"), (dict(kw, n_theta=nt + 1), lv, "n_theta \\* n_phi")):
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations: .*" + word):
            ctx.level_stations(sta=sta, level_of=bad_lv, **bad)
        assert ctx.lib.geoac_fan_level_stations_fetch(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), None) == 0 and np.array_equal(hits, want[0])
    # the same number of rays, not a lattice: one inclination off by an ulp; then n_theta and n_phi swapped
    th2 = th.copy()
    th2[nt + 2] = np.nextafter(th2[nt + 2], 90.0)
    ctx.run(th2, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations: .*not an n_theta x n_phi lattice"):
        ctx.level_stations(sta=sta, level_of=lv, **kw)
    ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations: .*not an n_theta x n_phi lattice"):
        ctx.level_stations(sta=sta, level_of=lv, **dict(kw, n_theta=nph, n_phi=nt))
    LS.assert_lists_equal(ctx.level_stations(sta=sta, level_of=lv, **kw), want)
    ctx.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    c2.load_met(H.TOYATMO)
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_stations: .*2-D set"):
        c2.level_stations(sta=sta, level_of=lv, **kw)
    c2.close()
