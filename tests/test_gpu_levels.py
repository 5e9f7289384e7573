"""Level crossings on the GPU (include/geoac_levels.h, k_levels): against the compiled reference's own rows (tests/golden/levels_small.npz), against the
reference's crossings, times and attenuations on every leg of all four sets (tests/golden/levels_legs.npz), against the path of the same launch as sample
capture at stride 1 returns it (every instantiation, rows exactly on a level, elevated sources, chunk seams), against a closed form, against the records
of the same launch on every equation set, bit for bit across launch plans and members, and the refusals.

Fans are small: the fixture's six inclinations at azimuth -90 (plus azimuth 37 where noted), one bounce, range limit 300 km.  Every context of a given
(set, fan, plan) is run once and shared, read-only."""
import faulthandler

import numpy as np
import pytest

import harness as H
import known_answers as K
import levels_reference as LR
import rngdep_data as RD

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120
VALID, TTIME, TURN = H.REC["VALID"], H.REC["TTIME"], H.REC["TURN"]
LEG, DIR, FRAC, LT, LA, P0 = (LR.LVL[k] for k in ("LEG", "DIR", "FRAC", "TTIME", "ATTEN", "P0"))
LEVELS = [20.0, 35.0, 110.0]
ALL_SETS = [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP]


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
def fixture():
    return np.load(LR.FIXTURE)


def _two_azimuths():
    return np.tile(LR.THETAS, 2), np.repeat([LR.PHI, 37.0], len(LR.THETAS))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _toy(G, eq, th, ph, levels=LEVELS, cap=8, opts=None, freqs=None, relaunch=False, **params):
    """ToyAtmo, one bounce, range limit 300 km: (records, steps, count, crossing records, epochs)"""
    with G.options(**(opts or {})):
        ctx = G.FanContext(eq, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(**dict(dict(bounces=1, calc_amp=1, mode=0, range_limit=300.0), **params))
        if freqs is not None:
            ctx.set_frequencies(freqs)
        if levels is not None:
            ctx.set_levels(levels, cap=cap)
        rec, steps = ctx.run(th, ph)
        if relaunch:
            rec, steps = ctx.run(th, ph)
        count, lrec = ctx.fetch_levels() if levels is not None else (None, None)
        epochs = ctx.timing()["epochs"]
        ctx.close()
    return rec, steps, count, lrec, epochs


_runs = {}


def _base(G, eq):
    """the two-azimuth fan under the default plan, shared"""
    if eq not in _runs:
        r = _toy(G, eq, *_two_azimuths())
        _freeze(r[0], r[2], r[3])
        _runs[eq] = r
    return _runs[eq]


def _same_bits(a, b, what):
    assert a[1] == b[1], what
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), (what, "records")
    assert np.array_equal(a[2], b[2]), (what, "counts")
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), (what, "crossing records")


# ---------------------------------------------------------------- against the reference fixture
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_leg0_crossings_match_the_reference_rows(G, fixture, eq):
    """counts and directions exact, FRAC-interpolated positions within 1e-6 relative (LR.position_errors), TTIME inside the bracket of the reference's
    sample-row times.  Largest position error measured on an MI355X: 2.7e-15 (3-D set), 4.4e-16 (Global set); DESIGN 8l."""
    name = H.EQ_NAMES[eq]
    lev = fixture[f"{name}_levels"]
    th = fixture["theta"]
    rec, steps, count, lrec, _ = _toy(G, eq, th, np.full(len(th), float(fixture["phi"])), levels=lev, range_limit=float(fixture["range_limit"]))
    assert count.shape == (len(th), len(lev)) and lrec.shape == (len(th), len(lev), 8, LR.LVL_STRIDE) and count.max() <= 8
    by = LR.fixture_rays(fixture, name)
    pw = LR.PATHW[eq]
    worst, n = 0.0, 0
    for r in range(len(th)):
        for l in range(len(lev)):
            mine = lrec[r, l, :count[r, l]]
            mine = mine[mine[:, LEG] == 0.0]
            idx = by.get((r, l), [])
            assert len(mine) == fixture[f"{name}_count"][r, l] == len(idx), (r, l, len(mine))
            if not idx:
                continue
            assert np.array_equal(mine[:, DIR], fixture[f"{name}_dir"][idx].astype(np.float64)), (r, l)
            err = LR.position_errors(eq, mine[:, P0:P0 + pw], fixture[f"{name}_row"][idx])
            worst = max(worst, float(err.max())); n += len(idx)
            assert (mine[:, FRAC] >= 0.0).all() and (mine[:, FRAC] <= 1.0).all()
            lo, hi = fixture[f"{name}_t_lo"][idx], fixture[f"{name}_t_hi"][idx]
            assert (mine[:, LT] >= lo).all() and (mine[:, LT] <= hi).all(), (r, l, mine[:, LT], lo, hi)
    print(f"{name}: {n} leg-0 crossings, largest position error against the reference's rows {worst:.3e}")
    assert n == fixture[f"{name}_count"].sum() and worst <= 1e-6


# ---------------------------------------------------------------- every leg, four sets, times and attenuation (tests/golden/levels_legs.npz)
@pytest.fixture(scope="module")
def legs_fixture():
    return np.load(LR.LEGS_FIXTURE)


def _open(G, eq, tmp_path):
    """a context with the set's atmosphere: ToyAtmo, or the ragged 7 x 4 grid"""
    ctx = G.FanContext(eq, device=0)
    if eq in (H.EQ_3D, H.EQ_GLOBAL):
        ctx.load_met(H.TOYATMO)
    else:
        glob = eq == H.EQ_GLOBAL_RNGDEP
        ctx.load_grid(*RD.write_grid_ragged(str(tmp_path), glob, short_paths=False), z_grnd=RD.ragged_load_z_grnd(glob))
    return ctx


def _legs_fan(eq, g):
    """rays and parameters of a set of the legs fixture: two bounces"""
    name = H.EQ_NAMES[eq]
    if eq in (H.EQ_3D, H.EQ_GLOBAL):
        params = dict(bounces=2, calc_amp=1, range_limit=float(g[f"{name}_range_limit"]))
    else:
        params = dict(bounces=2, calc_amp=1, src=tuple(g[f"{name}_src"]), z_grnd=float(g[f"{name}_z_grnd"]))
    return g[f"{name}_theta"], g[f"{name}_phi"], params


@pytest.mark.parametrize("eq", ALL_SETS)
def test_all_legs_match_the_reference(G, legs_fixture, eq, tmp_path):
    """LR.compare_with_fixture: counts per (ray, level, leg), LEG and DIR exact; FRAC, the interpolated row in all its components, TTIME and ATTEN within 1e-6
    relative of what the compiled reference's rows and running sums give (tests/test_levels_host.py: the same call refuses five wrong kernels).  Worst
    errors measured on an MI355X: DESIGN 8l."""
    name = H.EQ_NAMES[eq]
    th, ph, params = _legs_fan(eq, legs_fixture)
    ctx = _open(G, eq, tmp_path)
    ctx.set_params(mode=0, **params)
    ctx.set_levels(legs_fixture[f"{name}_levels"], cap=int(legs_fixture[f"{name}_cap_needed"]))
    ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    ctx.close()
    LR.compare_with_fixture(eq, count, lrec, legs_fixture)


# ---------------------------------------------------------------- against the same launch's path (sample capture at stride 1)
U = 2.0 ** -53


def _pair(G, eq, tmp_path, th, ph, levels, cap=8, opts=None, **params):
    """the fan twice under the same options: with levels, and with sample capture at stride 1 in their place (k_rk4<SMP> and k_accum's sample-capture branch:
    code k_levels shares nothing with).  GEOAC_ABS_TABLE=0 in both: the exact post-pass writes every segment's contribution, so that both contexts sum the
    same numbers whatever a table build decides.  Preconditions asserted here: the same step counts, every record column but TTIME / ATTEN the same bits;
    a launch whose sample or event list overflowed raises; LR.rows_from_samples asserts rows 1 .. k - 1 of every leg, once each.
    -> (records, count, crossing records, paths, rows per ray)"""
    with G.options(**dict(opts or {}, GEOAC_ABS_TABLE="0")):
        a = _open(G, eq, tmp_path)
        a.set_params(mode=0, **params)
        a.set_levels(levels, cap=cap)
        rec, steps = a.run(th, ph)
        count, lrec = a.fetch_levels()
        src, geo = tuple(a.params.src), dict(z_grnd=a.params.z_grnd, r_earth=a.params.r_earth)
        a.close()
        b = _open(G, eq, tmp_path)
        b.set_params(mode=G.api.MODE_WRITE_RAYS, sample_stride=1, **params)
        rec_s, steps_s = b.run(th, ph)
        smp = b.fetch_samples()
        b.close()
    assert steps == steps_s and (eq not in LR.SPHERICAL or geo["r_earth"] == LR.R_EARTH)
    other = [c for c in range(H.REC_STRIDE) if c not in (TTIME, H.REC["ATTEN"])]
    assert np.array_equal(np.ascontiguousarray(rec[..., other]).view(np.uint64), np.ascontiguousarray(rec_s[..., other]).view(np.uint64))
    paths, n_rows = LR.rows_from_samples(eq, smp, rec_s, src, geo, rec)
    assert n_rows.sum() == steps + int((rec[..., H.REC["STEPS"]] > 0).sum())
    return rec, count, lrec, paths, n_rows


def _check_against_path(eq, rec, count, lrec, paths, n_rows, levels, what):
    """count, LEG, DIR and FRAC: the same bits as LR.restate_k_levels on the sampled path.  Cartesian sets: P0 .. P2 too (the sample rows hold x, y and
    max(z, 0) unconverted, and no interior row lies below z = 0).  Spherical sets: the sample holds r - r_earth, exact for r_earth = 6370 and r < 8192 km
    (both multiples of 2^-40, the difference needs fewer bits), and r_earth + that is r again - so the heights, FRAC and P0 are the same bits here as well,
    with no room needed around a level; latitude and longitude come back from degrees through x 180, / pi, x pi, / 180, four roundings of 2^-53 relative each
    on either row, and the interpolation's three operations round once each on either side: |got - want| <= 10 x 2^-53 (|want| + 1e-3), 1e-3 rad being more
    than a step spans.  TTIME / ATTEN: both sides add the same contributions (_pair), grouped differently: within 4 n 2^-53 of the ray's final sum, n the
    ray's rows."""
    hi, cap = LR.hidx(eq), lrec.shape[2]
    assert count.max() <= cap, (what, "raise cap")
    lowest = LR.level_values(eq, levels)[0]
    for legs in paths:
        for j, (_, rows, _) in enumerate(legs):
            assert j == 0 or rows[1, hi] < lowest, (what, "a crossing in the first segment behind a bounce: LR.rows_from_samples does not re-do that row")
    wc, wl = LR.restate_fan(eq, paths, levels, cap)
    assert np.array_equal(count, wc), (what, "counts", np.argwhere(count != wc)[:4])
    exact = [LEG, DIR, FRAC, P0] if eq in LR.SPHERICAL else [LEG, DIR, FRAC, P0, P0 + 1, P0 + 2]
    for c in exact:
        assert np.array_equal(lrec[..., c].view(np.uint64), wl[..., c].view(np.uint64)), (what, "column", c, np.argwhere(lrec[..., c] != wl[..., c])[:4])
    worst = {}
    if eq in LR.SPHERICAL:
        e = np.abs(lrec[..., P0 + 1:P0 + 3] - wl[..., P0 + 1:P0 + 3]) / (np.abs(wl[..., P0 + 1:P0 + 3]) + 1e-3)
        worst["lat, lon / (10 x 2^-53)"] = float(e.max() / (10.0 * U))
    final = np.array([[rec[r, len(legs) - 1, c] for c in (TTIME, H.REC["ATTEN"])] for r, legs in enumerate(paths)])
    for q, c in enumerate((LT, LA)):
        bound = 4.0 * n_rows * U * final[:, q]
        e = np.abs(lrec[..., c] - wl[..., c]).max(axis=(1, 2))
        worst[("TTIME", "ATTEN")[q] + " / final"] = float((e / final[:, q]).max())
        worst[("TTIME", "ATTEN")[q] + " / bound"] = float((e / bound).max())
    print(f"{what}: {int(count.sum())} crossings ({int((lrec[..., LEG] >= 1).sum())} behind a bounce) equal the restatement of the sampled path; worst "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 1.0 for k, v in worst.items() if not k.endswith("final")), (what, worst)
    return wc, wl


def _toy_fan(bounces=2, range_limit=500.0):
    th, ph = _two_azimuths()
    return th, ph, dict(bounces=bounces, calc_amp=1, range_limit=range_limit)


@pytest.mark.parametrize("eq", ALL_SETS)
def test_crossings_equal_the_restatement_of_the_sampled_path(G, legs_fixture, eq, tmp_path):
    """the fans of the legs fixture (ToyAtmo at two azimuths, the ragged grids), two bounces"""
    th, ph, params = _legs_fan(eq, legs_fixture)
    rec, count, lrec, paths, n_rows = _pair(G, eq, tmp_path, th, ph, LEVELS, **params)
    _check_against_path(eq, rec, count, lrec, paths, n_rows, LEVELS, H.EQ_NAMES[eq])
    assert (lrec[..., LEG] == 2.0).any()


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_chunk_seams_equal_the_sampled_path(G, eq, tmp_path):
    """64-row chunks in both contexts: crossings on carry rows, sample events on every row of every chunk (test_crossings_do_not_depend_on_the_launch_plan
    proves this plan equal to the default one; this proves both equal to the path)"""
    th, ph, params = _toy_fan()
    rec, count, lrec, paths, n_rows = _pair(G, eq, tmp_path, th, ph, LEVELS, opts={"GEOAC_S_ROWS": "64"}, **params)
    _check_against_path(eq, rec, count, lrec, paths, n_rows, LEVELS, f"{H.EQ_NAMES[eq]}, 64-row chunks")


EIGHT = [5.0, 12.0, 20.0, 35.0, 50.0, 70.0, 90.0, 110.0]


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_every_instantiation_gives_the_same_crossings(G, eq, tmp_path):
    """k_levels<8> against the sampled path; k_levels<1> .. <7> with the first L of the eight levels: every level's count and records the same bits as its
    slice of the eight-level run, the launch's records unchanged"""
    th, ph, params = _toy_fan(bounces=1, range_limit=300.0)
    rec, count, lrec, paths, n_rows = _pair(G, eq, tmp_path, th, ph, EIGHT, **params)
    _check_against_path(eq, rec, count, lrec, paths, n_rows, EIGHT, f"{H.EQ_NAMES[eq]}, 8 levels")
    assert (count > 0).any(axis=0).all(), "every level is crossed by some ray"
    with G.options(GEOAC_ABS_TABLE="0"):
        for L in range(1, 8):
            r, _, c, lr, _ = _toy(G, eq, th, ph, levels=EIGHT[:L], **params)
            assert c.shape == (len(th), L) and np.array_equal(c, count[:, :L]), L
            assert np.array_equal(lr.view(np.uint64), lrec[:, :L].view(np.uint64)), L
            assert np.array_equal(r.view(np.uint64), rec.view(np.uint64)), L


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_elevated_source_and_downward_launches(G, eq, tmp_path):
    """source at 25 km, between the levels, in the stratospheric duct of ToyAtmo: rays launched below the horizontal cross 20 km downward first, on leg 0; the
    steep ones reach the ground and come back up through the levels on leg 1, the shallow ones swing about 20 km until the range limit (hence cap = 32)"""
    inc = np.array([-60.0, -40.0, -18.0, -8.0, 3.0, 20.0])
    th, ph = np.tile(inc, 2), np.repeat([LR.PHI, 37.0], len(inc))
    src = (25.0, 30.0, 0.0) if eq == H.EQ_GLOBAL else (0.0, 0.0, 25.0)
    rec, count, lrec, paths, n_rows = _pair(G, eq, tmp_path, th, ph, LEVELS, cap=32, bounces=2, calc_amp=1, range_limit=400.0, src=src)
    _check_against_path(eq, rec, count, lrec, paths, n_rows, LEVELS, f"{H.EQ_NAMES[eq]}, source at 25 km")
    down = th < 0.0
    assert (count[down, 0] >= 1).all() and (lrec[down, 0, 0, DIR] == -1.0).all() and (lrec[down, 0, 0, LEG] == 0.0).all()
    assert (lrec[down, 0, 1, DIR] == 1.0).all() and (lrec[..., LEG] >= 1.0).any() and (count[:, 0] >= 4).any()


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_a_row_exactly_on_a_level_counts_once(G, eq, tmp_path):
    """levels set to the height of an ascending and of a descending interior row of one ray (azimuth 37, leg 0): the upward crossing is counted once, with
    FRAC == 1.0 in the segment that ends on the row, the downward one once, with FRAC == 0.0 in the segment that starts on it, and the interpolated position
    is the row's (a + 1.0 (b - a) is b where b - a is exact: asserted of the row chosen); every other count is that of levels 1 m higher.  Spherical set:
    the level z must give r_earth + z == r bit for bit, which r - r_earth does (_check_against_path); were it not to, the set is left out with that printed."""
    th, ph, params = _toy_fan(bounces=1, range_limit=500.0)
    _, _, _, paths, _ = _pair(G, eq, tmp_path, th, ph, LEVELS, **params)
    ray, hi = next(r for r in range(6, 12) if paths[r][0][0] > 0), LR.hidx(eq)      # the first ray at azimuth 37 whose first leg comes down to the ground
    rows = paths[ray][0][1]
    off = LR.R_EARTH if eq in LR.SPHERICAL else 0.0
    h = rows[:, hi]
    top = int(np.argmax(h))
    i_up = next(i for i in range(2, top) if h[i] - off > 27.0)
    i_dn = next(i for i in range(top + 1, len(h) - 2) if h[i] - off < 13.0)
    z = []
    for i in (i_dn, i_up):
        near = [h[i] - off]
        for _ in range(3):
            near = [np.nextafter(near[0], -np.inf)] + near + [np.nextafter(near[-1], np.inf)]
        hit = [v for v in near if off + v == h[i]]
        if not hit:
            print(f"{H.EQ_NAMES[eq]}: no level z with r_earth + z == r of row {i} within three steps of r - r_earth: left out")
            return
        z.append(float(hit[len(hit) // 2]))
    rec, count, lrec, paths2, n_rows = _pair(G, eq, tmp_path, th, ph, z, **params)
    assert np.array_equal(paths2[ray][0][1].view(np.uint64), rows.view(np.uint64))
    _, wl = _check_against_path(eq, rec, count, lrec, paths2, n_rows, z, f"{H.EQ_NAMES[eq]}, levels on rows {i_dn} and {i_up}")
    up = lrec[ray, 1, :count[ray, 1]]
    dn = lrec[ray, 0, :count[ray, 0]]
    on_up, on_dn = up[up[:, FRAC] == 1.0], dn[dn[:, FRAC] == 0.0]
    assert len(on_up) == 1 and on_up[0, DIR] == 1.0 and on_up[0, LEG] == 0.0 and len(on_dn) == 1 and on_dn[0, DIR] == -1.0 and on_dn[0, LEG] == 0.0
    assert (up[up[:, LEG] == 0.0][:, DIR] == 1.0).sum() == 1 and (dn[dn[:, LEG] == 0.0][:, DIR] == -1.0).sum() == 1, "the row on the level is counted once"
    n_pos = 1 if eq in LR.SPHERICAL else 3                       # (latitude and longitude come back from degrees: _check_against_path)
    a, b = rows[i_up - 1, :n_pos], rows[i_up, :n_pos]
    assert (a + (b - a) == b).all(), "choose another row: b - a is not exact here"
    assert np.array_equal(on_up[0, P0:P0 + n_pos].view(np.uint64), b.view(np.uint64))
    assert np.array_equal(on_dn[0, P0:P0 + n_pos].view(np.uint64), rows[i_dn, :n_pos].view(np.uint64))
    with G.options(GEOAC_ABS_TABLE="0"):
        moved = _toy(G, eq, th, ph, levels=[v + 1e-3 for v in z], **params)
    assert np.array_equal(moved[2], count), (moved[2], count)


# ---------------------------------------------------------------- known answer
def test_straight_rays_cross_at_the_closed_form_time_and_place(G):
    """isothermal windless medium (tests/known_answers.py), Cartesian set, rays launched upward from a ground source: level z_l is crossed once, upward, at
    t = (z_l - z0) / (sin(theta) c), on the launch line - rtol 1e-9, the tolerance check_straight_rays holds the records to"""
    z, T, u, v, rho = K.isothermal_profile()
    c = np.sqrt(K.GAM_R * 250.0)
    inc = np.array([10.0, 17.0, 31.0, 45.0, 62.0, 80.0])
    th, ph = np.tile(inc, 2), np.repeat([37.0, -120.0], len(inc))
    levels = [10.0, 30.0]
    ctx = G.FanContext(G.EQ_3D, device=0)
    ctx.upload_atmo_1d(z, T, u, v, rho)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0, src=(0.0, 0.0, 0.0))
    ctx.set_levels(levels)
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    ctx.close()
    assert (rec[..., VALID] == 0).all()                          # every ray leaves the medium: the crossings lie before the break
    assert (count == 1).all(), count
    one = lrec[:, :, 0]
    assert (one[..., DIR] == 1.0).all() and (one[..., LEG] == 0.0).all()
    t, a = np.radians(th)[:, None], np.radians(ph)[:, None]
    zl = np.array(levels)[None, :]
    want_t = (zl - 0.0) / (np.sin(t) * c)
    et = np.abs(one[..., LT] / want_t - 1.0)
    d = np.stack([np.cos(t) * np.sin(a), np.cos(t) * np.cos(a), np.sin(t)], axis=-1) * np.ones((1, 2, 1))
    p = one[..., P0:P0 + 3]
    L = np.linalg.norm(p, axis=-1)
    off = np.linalg.norm(p - (p * d).sum(axis=-1, keepdims=True) * d, axis=-1) / L
    horiz = np.abs(np.hypot(p[..., 0], p[..., 1]) * np.tan(t) / zl - 1.0)
    print(f"straight rays: crossing time off by {et.max():.2e}, position off the launch line by {off.max():.2e} of the path, horizontal distance off by {horiz.max():.2e}")
    assert et.max() <= 1e-9 and off.max() <= 1e-9 and horiz.max() <= 1e-9
    assert (lrec[:, :, 1:] == 0.0).all()


# ---------------------------------------------------------------- consistency with the records, every set
def _ragged(G, eq, tmp, levels=LEVELS, lanes=None):
    glob = eq == H.EQ_GLOBAL_RNGDEP
    files = RD.write_grid_ragged(str(tmp), glob, short_paths=False)
    th, ph, params, _, _, _ = RD.ragged_table(RD.ragged_fixture(glob), "a_amp1")
    with G.options(**({"GRID_LANES": str(lanes)} if lanes else {})):
        ctx = G.FanContext(eq, device=0)
        g = ctx.load_grid(*files, z_grnd=RD.ragged_load_z_grnd(glob))
        ctx.set_params(**dict(params, mode=0, bounces=1, range_limit=300.0))
        ctx.set_levels(levels)
        rec, steps = ctx.run(th, ph)
        count, lrec = ctx.fetch_levels()
        ctx.close()
    return g, th, ph, params, rec, steps, count, lrec


def _check_consistency(rec, count, lrec, levels, what):
    n_rays, legs = rec.shape[0], rec.shape[1]
    assert count.max() <= lrec.shape[2], (what, "raise cap: a count beyond it leaves crossings unseen")
    seen = 0
    for r in range(n_rays):
        end = rec[r, :, TTIME]
        for l, z in enumerate(levels):
            c = lrec[r, l, :count[r, l]]
            assert (lrec[r, l, count[r, l]:] == 0.0).all()
            if len(c):
                assert (np.diff(c[:, LT]) > 0.0).all(), (what, r, l, "crossing times do not increase in path order")
                assert (np.diff(c[:, LEG]) >= 0.0).all() and np.array_equal(c[:, DIR], np.where(np.arange(len(c)) % 2 == 0, 1.0, -1.0)), (what, r, l)
                assert (c[:, FRAC] >= 0.0).all() and (c[:, FRAC] <= 1.0).all() and (c[:, LA] >= 0.0).all() and (np.diff(c[:, LA]) >= 0.0).all()
            for j in range(legs):
                cj = c[c[:, LEG] == j]
                if len(cj) and j >= 1:
                    assert rec[r, j - 1, VALID] > 0 and (cj[:, LT] >= end[j - 1]).all(), (what, r, l, j)
                if rec[r, j, VALID] > 0:
                    assert (cj[:, LT] <= end[j]).all(), (what, r, l, j)
                    if rec[r, j, TURN] > z + 0.1:
                        assert (cj[:, DIR] == 1.0).any() and (cj[:, DIR] == -1.0).any(), (what, r, l, j, "a leg that turns above the level crosses it both ways")
                    if rec[r, j, TURN] < z - 0.1:
                        assert len(cj) == 0, (what, r, l, j, "a leg that turns below the level does not cross it")
                    seen += 1
            assert ((c[:, LEG] >= 0) & (c[:, LEG] < legs)).all()
    return seen


@pytest.mark.parametrize("eq", ALL_SETS)
def test_crossings_are_consistent_with_the_records(G, eq, tmp_path):
    if eq in (H.EQ_3D, H.EQ_GLOBAL):
        rec, _, count, lrec, _ = _base(G, eq)
    else:
        _, _, _, _, rec, _, count, lrec = _ragged(G, eq, tmp_path)
    seen = _check_consistency(rec, count, lrec, LEVELS, H.EQ_NAMES[eq])
    print(f"{H.EQ_NAMES[eq]}: {int(count.sum())} crossings of {rec.shape[0]} rays, {seen} (arrival, level) pairs checked against TURN")
    # (every set's fan has first legs that arrive inside the range limit and second legs that climb through 20 km again: crossings behind a leg end are covered)
    assert count.sum() >= 2 * rec.shape[0] and seen >= 6 and (rec[:, 0, VALID] > 0).any() and (lrec[..., LEG] == 1.0).any()


# ---------------------------------------------------------------- schedule independence, bit for bit
PLANS = {
    "s_rows_64": {"GEOAC_S_ROWS": "64"},
    "s_rows_64_two_chunks": {"GEOAC_S_ROWS": "64", "GEOAC_TWO_CHUNKS": "1"},
    "no_overlap": {"GEOAC_NO_OVERLAP": "1"},
    "compact_0": {"GEOAC_COMPACT": "0"},
    "accum_batch_1": {"GEOAC_ACCUM_BATCH": "1"},
    "late_post_pass": {"PP_TEST_DELAY_MS": "5", "GEOAC_S_ROWS": "64"},
}


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_crossings_do_not_depend_on_the_launch_plan(G, eq, plan):
    base = _base(G, eq)
    got = _toy(G, eq, *_two_azimuths(), opts=PLANS[plan])
    if "GEOAC_S_ROWS" in PLANS[plan]:
        assert got[4] >= 100 and got[4] > 4 * base[4], (got[4], base[4])      # many epochs: crossings on carry rows, the rotation wraps
    _same_bits(got, base, plan)


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_relaunch_gives_the_same_bits(G, eq):
    _same_bits(_toy(G, eq, *_two_azimuths(), relaunch=True), _base(G, eq), "relaunch")


# ---------------------------------------------------------------- members
def test_ensemble_members_equal_plain_contexts(G):
    """1-D ensemble, K = 3, Global set"""
    from test_gpu_ensemble import _raw_members, _device_arrays
    eq = H.EQ_GLOBAL
    profs = [_device_arrays(eq, *m) for m in _raw_members()]
    th, ph = _two_azimuths()
    params = dict(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d_ensemble(profs[0][0], *[np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)])
    ctx.set_params(**params); ctx.set_levels(LEVELS)
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    ctx.close()
    assert count.shape == (3, len(th), 3) and lrec.shape == (3, len(th), 3, 8, LR.LVL_STRIDE)
    for m, prof in enumerate(profs):
        one = G.FanContext(eq, device=0)
        one.upload_atmo_1d(*prof)
        one.set_params(**params); one.set_levels(LEVELS)
        r1, _ = one.run(th, ph)
        c1, l1 = one.fetch_levels()
        one.close()
        assert c1.sum() > 0
        assert np.array_equal(rec[m].view(np.uint64), r1.view(np.uint64)), m
        assert np.array_equal(count[m], c1) and np.array_equal(lrec[m].view(np.uint64), l1.view(np.uint64)), m
    assert not np.array_equal(lrec[0], lrec[1])


def test_source_set_members_equal_plain_contexts(G):
    """source set, n_src = 2, 3-D set"""
    eq = H.EQ_3D
    th, ph = _two_azimuths()
    srcs = np.array([[0.0, 0.0, 0.0], [12.0, -30.0, 1.5]])
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
    ctx.set_sources(srcs); ctx.set_levels(LEVELS)
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    ctx.close()
    assert count.shape == (2, len(th), 3)
    for s in range(2):
        r1, _, c1, l1, _ = _toy(G, eq, th, ph, src=tuple(srcs[s]))
        assert np.array_equal(rec[s].view(np.uint64), r1.view(np.uint64)), s
        assert np.array_equal(count[s], c1) and np.array_equal(lrec[s].view(np.uint64), l1.view(np.uint64)), s
    assert not np.array_equal(lrec[0], lrec[1])


def test_grid_ensemble_members_equal_plain_contexts(G, tmp_path):
    """grid ensemble, K = 2, GEOAC_EQ_3D_RNGDEP; the plain contexts with one lane per ray (GRID_LANES=1), as tests/test_gpu_grid_ensemble.py compares"""
    eq = H.EQ_3D_RNGDEP
    g, th, ph, params, rec0, _, count0, lrec0 = _ragged(G, eq, tmp_path, lanes=1)
    members = [dict(T=g["T"], u=g["u"], v=g["v"], rho=g["rho"]), dict(T=g["T"] + 3.0, u=g["u"] * 0.85, v=g["v"] * 0.85, rho=g["rho"])]
    p = dict(params, mode=0, bounces=1, range_limit=300.0)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([m[k] for m in members]) for k in ("T", "u", "v", "rho")])
    ctx.set_params(**p); ctx.set_levels(LEVELS)
    rec, _ = ctx.run(th, ph)
    count, lrec = ctx.fetch_levels()
    ctx.close()
    assert count.shape == (2, len(th), 3)
    assert np.array_equal(rec[0].view(np.uint64), rec0.view(np.uint64))
    assert np.array_equal(count[0], count0) and np.array_equal(lrec[0].view(np.uint64), lrec0.view(np.uint64))
    with G.options(GRID_LANES="1"):
        one = G.FanContext(eq, device=0)
        one.upload_atmo_3d(g["x"], g["y"], g["z"], *[members[1][k] for k in ("T", "u", "v", "rho")])
        one.set_params(**p); one.set_levels(LEVELS)
        r1, _ = one.run(th, ph)
        c1, l1 = one.fetch_levels()
        one.close()
    assert np.array_equal(rec[1].view(np.uint64), r1.view(np.uint64))
    assert np.array_equal(count[1], c1) and np.array_equal(lrec[1].view(np.uint64), l1.view(np.uint64)) and c1.sum() > 0


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_frequency_set_crossings_are_those_of_frequency_0(G, eq):
    th, ph = _two_azimuths()
    freqs = (0.5, 2.0)
    got = _toy(G, eq, th, ph, freqs=freqs)
    plain = _toy(G, eq, th, ph, freq=freqs[0])
    _same_bits(got, plain, "frequency set")
    assert not np.array_equal(plain[3][..., LA], _base(G, eq)[3][..., LA])          # (ATTEN is the attenuation at that frequency, not at the default 0.1 Hz)


# ---------------------------------------------------------------- cap
def test_count_runs_past_cap_and_the_first_crossings_are_kept(G):
    eq = H.EQ_GLOBAL
    base = _base(G, eq)
    got = _toy(G, eq, *_two_azimuths(), cap=1)
    assert got[3].shape[2] == 1 and (base[2][:, 1] >= 2).any()                      # a ray crosses 35 km at least twice
    assert np.array_equal(got[2], base[2])
    assert np.array_equal(got[0].view(np.uint64), base[0].view(np.uint64))
    assert np.array_equal(got[3][:, :, 0].view(np.uint64), base[3][:, :, 0].view(np.uint64))
    for r, l in zip(*np.nonzero(base[2] < 8)):
        assert (base[3][r, l, base[2][r, l]:] == 0.0).all()
    assert (got[3][got[2] == 0] == 0.0).all()


# ---------------------------------------------------------------- off means off, and the refusals
def test_zero_levels_leave_the_mode(G):
    eq = H.EQ_GLOBAL
    th, ph = _two_azimuths()
    never = _toy(G, eq, th, ph, levels=None)
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
    ctx.set_levels(LEVELS, cap=4)
    z, cap = ctx.levels
    assert list(z) == LEVELS and cap == 4
    ctx.run(th, ph)
    assert ctx.fetch_levels()[0].sum() > 0
    (rp, rb), (cp, cb) = ctx.levels_dev()
    assert rp and cp and rb == len(th) * 3 * 4 * LR.LVL_STRIDE * 8 and cb == len(th) * 3 * 4
    ctx.set_levels([])
    assert len(ctx.levels[0]) == 0
    with pytest.raises(G.GeoAcError, match="invalid argument.*no levels set"):
        ctx.fetch_levels()
    rec, steps = ctx.run(th, ph)
    with pytest.raises(G.GeoAcError, match="invalid argument.*no levels set"):
        ctx.fetch_levels()
    with pytest.raises(G.GeoAcError, match="invalid argument.*no levels set"):
        ctx.levels_dev()
    ctx.close()
    assert steps == never[1] and np.array_equal(rec.view(np.uint64), never[0].view(np.uint64))
    assert np.array_equal(never[0].view(np.uint64), _base(G, eq)[0].view(np.uint64))   # (and levels change no bit of the records)


def test_refusals(G):
    eq = H.EQ_GLOBAL
    th, ph = _two_azimuths()
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0)
    ctx.set_levels(LEVELS)
    ctx.set_angles(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*clone: not available while levels are set"):
        ctx.clone()
    with pytest.raises(G.GeoAcError, match="not implemented.*eig_search: not available while levels are set"):
        ctx.eig_search([[30.5, -1.0]])
    for mode in (G.api.MODE_WRITE_RAYS, G.api.MODE_WRITE_CAUSTICS):
        ctx.set_params(mode=mode)
        with pytest.raises(G.GeoAcError, match="not implemented.*sample capture .* is not available while levels are set"):
            ctx.launch()
    ctx.set_params(mode=0, z_grnd=20.0)
    with pytest.raises(G.GeoAcError, match="invalid argument.*fan_launch: levels .*strictly above z_grnd"):
        ctx.launch()
    ctx.set_params(z_grnd=0.0)
    with pytest.raises(G.GeoAcError, match="invalid argument.*set_levels: levels must be strictly ascending"):
        ctx.set_levels([35.0, 20.0])
    with pytest.raises(G.GeoAcError, match="invalid argument.*vertical limit"):
        ctx.set_levels([20.0, 150.0])
    assert list(ctx.levels[0]) == LEVELS                        # (a refused list leaves the current one in place)
    ctx.launch()
    assert ctx.fetch_levels()[0].sum() > 0
    ctx.set_levels([20.0])
    with pytest.raises(G.GeoAcError, match="invalid argument.*level list has changed"):
        ctx.fetch_levels()
    ctx.close()
    two = G.FanContext(G.EQ_2D, device=0)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D"):
        two.set_levels([20.0])
    two.close()
