"""Level refinement on the device (include/geoac_level_refine.h, FanContext.level_refine): rows and counters against the numpy restatement
(tests/level_refine_reference.py) driven by a second context's launches, bit for bit, on the four 3-D-capable sets; a closed form; the eigenray
condition from a fresh launch; members of an ensemble, a source set, a grid ensemble and a frequency set against plain contexts; launch-plan
independence; the call's lifecycle and refusals; a plain context against the golden records.
Fans are small lattices through ToyAtmo (one bounce, range limit 300 km) unless a test says otherwise: the lattices, stations and helpers of
tests/test_gpu_lstations.py.  Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and
nothing is retried)."""
import ctypes
import faulthandler

import numpy as np
import pytest

import harness as H
import known_answers as K
import level_refine_reference as LR
import lstation_reference as LS
import rngdep_data as RD
import station_cases as SC
import station_reference as SR
import test_gpu_lstations as TL
from levels_reference import LVL
from parity import compare_records
from test_gpu_ensemble import _device_arrays, _raw_members
from test_gpu_sources import _toy, _upload

pytestmark = pytest.mark.gpu
R, S, P0 = LR.LRF, LS.LSTA, LVL["P0"]
STEP_LIMIT_S = 120
LEVELS2, LEVELS3 = [20.0, 35.0], [20.0, 35.0, 110.0]
TOY = TL.TOY
SPHERICAL = TL.SPHERICAL
STATUS_NAMES = {1: "CONVERGED", 2: "ITER_LIMIT", 3: "STALLED", 4: "LOST", 5: "SINGULAR"}
COARSE = dict(max_iter=6, max_shrink=2, tol=0.5, step_max_deg=1.0)                 # test 1: the rule's branches, not convergence (probe_deg: the default 0.02)
EIGEN = dict(tol=0.1, step_max_deg=0.2, probe_deg=0.02, max_iter=10, max_shrink=4)   # test 3
# theta 10 .. 35 in steps of 2.5, 9 azimuths: the grid sets' lattice of the member test (the 6 x 5 lattice at half its steps)
LATTICE_11x9 = dict(theta_min=10.0, theta_max=35.0, theta_step=2.5, phi_min=-118.0, phi_max=-62.0, phi_step=7.0)


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


def _integrator(ctx):
    """launches of a context as the restatement takes them: (theta, phi) -> (count [M][n][L], lrec [M][n][L][cap][12])"""
    def integrate(th, ph):
        ctx.run(th, ph)
        count, lrec = ctx.fetch_levels()
        return TL._members(count, 2), TL._members(lrec, 4)
    return integrate


def _sources(ctx, srcs=None, K_prof=1):
    """[M][2] source points of the launch's members (m = source * K + profile) in the stations' axes"""
    s = np.array([list(ctx.params.src)]) if srcs is None else np.asarray(srcs)
    return LR.sources(ctx.eqset, np.repeat(s, K_prof if srcs is not None else ctx.n_members, axis=0))


def _rings(eq, ctx, count, lrec, ph, levels, n):
    """n ring stations (tests/test_gpu_lstations.py) on each of the levels: sta [len(levels) * n][2], level_of"""
    src = TL._source_xy(ctx)
    return np.concatenate([TL._ring(eq, src, count, lrec, ph, l, n=n) for l in levels]), np.repeat(levels, n)


def _far(eq, ctx, n=3):
    src = TL._source_xy(ctx)
    one = np.array([src[0], src[1] + 52.0]) if eq in SPHERICAL else np.array([src[0] + 5000.0, src[1]])          # 5 000 km away
    return np.tile(one, (n, 1)) + np.arange(n)[:, None] * 0.25


def _status_counts(rows):
    return np.bincount(rows[:, R["STATUS"]].astype(int), minlength=6)[1:].tolist()


def _check_rows(rows, stats, M, tol):
    n = len(rows)
    status = rows[:, R["STATUS"]].astype(int)
    assert rows.shape == (n, 16) and stats["seeds"] == n and set(status) <= {1, 2, 3, 4, 5} and np.isfinite(rows).all()
    assert stats["ray_members"] == stats["launches"] * 3 * n * M
    assert stats["converged"] + stats["stalled_or_limit"] + stats["lost_or_singular"] == n
    done = status != LR.CONVERGED
    assert (rows[done, R["TTIME"]:] == 0).all() and (rows[~done, R["MISS"]] <= tol).all() and (rows[~done, R["TTIME"]] > 0).all()
    assert (rows[status == LR.LOST, R["MISS"]] == -1.0).all() and (rows[status != LR.LOST, R["MISS"]] >= 0.0).all()


# ---------------------------------------------------------------- 1. bit for bit against the restatement
def _parity_ctx(G, eq, tmp, levels=LEVELS3, options=None, **params):
    """a context of the equation set with levels set, nothing launched, and its coarse lattice"""
    if eq in (H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP):
        ctx = G.FanContext(eq, device=0, options=options)
        if eq == H.EQ_3D_RNGDEP:
            ctx.load_grid(*RD.write_grid(str(tmp), short_paths=False))
            ctx.set_params(**dict(TOY, src=(0.0, 0.0, 0.0), **params))
        else:
            ctx.load_grid(*RD.write_grid_global(str(tmp), short_paths=False))
            ctx.set_params(**dict(TOY, src=(0.0, 31.0, 0.0), **params))
        ctx.set_levels(levels)
        return ctx, SC.lattice(**TL.LATTICE_6x5)
    ctx = G.FanContext(eq, device=0, options=options)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(**dict(TOY, **params))
    ctx.set_levels(levels)
    return ctx, SC.lattice(**TL.LATTICE_12x8)


def _refine_both(G, eq, tmp, sta_of, lsta_kw, spec_kw, levels=LEVELS3, **params):
    """refine on one context; restate with a second context of the same set-up as the integrator; compare.  Returns the context, the device's result
    and the lists"""
    ctx, (th, ph, nt, nph) = _parity_ctx(G, eq, tmp, levels, **params)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = sta_of(ctx, count, lrec, ph)
    hits, lrows = ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, **lsta_kw)
    got = ctx.level_refine(**spec_kw)
    other, _ = _parity_ctx(G, eq, tmp, levels, **params)
    want = LR.reference_level_refine(eq, hits, lrows, sta, lv, levels, LR.spec(**spec_kw), _integrator(other), _sources(ctx), r_earth=ctx.params.r_earth)
    other.close()
    LR.assert_equal_bits(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])
    return ctx, got, (hits, lrows, sta, lv, th)


RESTATED = [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP]
CAP1 = 12


@pytest.fixture(scope="module")
def restated(G, tmp_path_factory):
    """the four cases of test 1, each refined and compared once on first use and kept: case(eq) -> dict"""
    done = {}

    def case(eq):
        if eq not in done:
            def stations(ctx, count, lrec, ph):
                # the 3 x 24 stations of test_lists_equal_reference: per level the ring, two stations bit for bit on a crossing point, one midway
                # between two, one 5 000 km away - with both ordinals and twelve rows kept, so that the later branches (leg 1, a second passage
                # through the duct) are seeds too: branches that end between two lattice rays are where a seed is lost or its step fails
                nt, nph = SC.lattice(**(TL.LATTICE_6x5 if eq in (H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP) else TL.LATTICE_12x8))[2:]
                sp = LS.spec(nt, nph, ord_max=2, cap=CAP1)
                src = TL._source_xy(ctx)
                return np.concatenate([TL._stations_24(eq, src, count, lrec, ph, sp, 2, l) for l in range(3)]), np.repeat([0, 1, 2], 24)

            ctx, (rows, stats), (hits, lrows, sta, lv, th) = _refine_both(G, eq, tmp_path_factory.mktemp("lrf"), stations, dict(ord_max=2, cap=CAP1), COARSE)
            done[eq] = dict(rows=rows, stats=stats, hits=hits, sta=sta, rec_shape=ctx.fetch()[0].shape, count_shape=ctx.fetch_levels()[0].shape)
            ctx.close()
        return done[eq]
    return case


@pytest.mark.parametrize("eq", RESTATED)
def test_rows_equal_restatement(restated, eq):
    """the coarse lattices of the level-station tests (3 x 10 degrees; 5 x 14 on the grids): the estimates are far from their eigenrays, so the rounds are
    cut steps, rejected trials and every final status - the step rule's branches, not its convergence"""
    c = restated(eq)
    rows, stats, hits, sta = c["rows"], c["stats"], c["hits"], c["sta"]
    n = int(np.minimum(hits, CAP1).sum())
    print(f"{H.EQ_NAMES[eq]}: seeds {n} launches {stats['launches']} status counts {_status_counts(rows)} (converged, limit, stalled, lost, singular); "
          f"branches {sorted(set(map(tuple, rows[:, R['LEG']:R['ORD'] + 1].astype(int).tolist())))}")
    _check_rows(rows, stats, 1, COARSE["tol"])
    assert len(rows) == n and n >= 8 and 1 <= stats["launches"] <= 6
    assert n % 64 != 0                                                              # a part-filled last wave
    assert (rows[:, R["MEMBER"]] == 0).all() and np.array_equal(rows[:, R["STATION"]], np.repeat(np.arange(len(sta)), np.minimum(hits[0], CAP1)))
    # the launch's own tables are those of the last round: 3 n rays
    assert c["rec_shape"][0] == 3 * n and c["count_shape"] == (3 * n, 3)


def test_at_least_three_statuses_over_the_four_cases(restated):
    every = set()
    for eq in RESTATED:
        every |= set(restated(eq)["rows"][:, R["STATUS"]].astype(int))
    print("statuses over the four cases:", sorted(STATUS_NAMES[s] for s in every))
    assert len(every) >= 3


def test_single_seed(G):
    eq, picked = H.EQ_GLOBAL, {}

    def one(ctx, count, lrec, ph):
        sta, lv = _rings(eq, ctx, count, lrec, ph, [0], 12)
        th, _, nt, nph = SC.lattice(**TL.LATTICE_12x8)
        hits, _ = ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=1, cap=1)
        k = int(np.flatnonzero(hits[0] >= 1)[0])
        picked["k"] = k
        return sta[k:k + 1], lv[k:k + 1]

    ctx, (rows, stats), (hits, _, _, _, _) = _refine_both(G, eq, None, one, dict(ord_max=1, cap=1), dict(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=1.0))
    print(f"single seed: station {picked['k']} of the ring, {stats}, status {STATUS_NAMES[int(rows[0, R['STATUS']])]}, miss {rows[0, R['MISS']]:.4g}")
    assert hits[0, 0] >= 1 and rows.shape == (1, 16) and stats["seeds"] == 1 and stats["ray_members"] == 3 * stats["launches"]
    ctx.close()


def test_zero_seeds_launch_nothing_and_keep_the_lists(G):
    eq = H.EQ_GLOBAL
    ctx, (th, ph, nt, nph) = _parity_ctx(G, eq, None)
    TL._run(ctx, th, ph)
    steps, epochs = ctx.total_steps(), ctx.timing()["epochs"]
    far = _far(eq, ctx)
    hits, _ = ctx.level_stations(sta=far, level_of=[0, 1, 2], n_theta=nt, n_phi=nph, ord_max=2, cap=4)
    assert hits.sum() == 0
    rows, stats = ctx.level_refine(**COARSE)
    assert rows.shape == (0, 16) and stats == dict(launches=0, ray_members=0, seeds=0, converged=0, stalled_or_limit=0, lost_or_singular=0)
    assert ctx.n_rays == len(th) and ctx.total_steps() == steps and ctx.timing()["epochs"] == epochs          # nothing was launched
    h2 = np.ones((1, 3), dtype=np.uint32)
    assert ctx.lib.geoac_fan_level_stations_fetch(ctx._h, h2.ctypes.data_as(ctypes.c_void_p), None) == 0 and (h2 == 0).all()          # the lists are still current
    ptr, nbytes = ctypes.c_void_p(1), ctypes.c_size_t(1)
    assert ctx.lib.geoac_fan_level_refine_dev(ctx._h, ctypes.byref(ptr), ctypes.byref(nbytes)) == 0 and not ptr.value and nbytes.value == 0
    ctx.close()


# ---------------------------------------------------------------- 2. closed form
def test_closed_form(G):
    """isothermal windless medium, ground source, straight rays (tests/test_gpu_lstations.py, test_closed_form_and_convergence, its 5 x 15 degree lattice): the
    station at z_l / tan(theta*) (sin phi*, cos phi*) on level z_l is reached by the ray (theta*, phi*) alone, at t = |station - source| / c.  A ray that
    passes within tol of the station horizontally has, by the straight-line geometry r = z / tan(theta): |d theta| <= tol sin^2(theta*) / z,
    |d phi| <= tol tan(theta*) / z [rad], and a path at most tol longer or shorter (1e-6 TTIME for the integration's own error)."""
    z, T, u, v, rho = K.isothermal_profile()
    th, ph, nt, nph = SC.lattice(theta_min=10.0, theta_max=80.0, theta_step=5.0, phi_min=0.0, phi_max=345.0, phi_step=15.0)
    levels, tol = [10.0, 30.0], 0.01
    ctx = G.FanContext(G.EQ_3D, device=0)
    ctx.upload_atmo_1d(z, T, u, v, rho)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=300.0, src=(0.0, 0.0, 0.0))
    ctx.set_levels(levels)
    ctx.run(th, ph)
    th_s, ph_s = np.tile(TL.THETA_STAR, 2), np.tile(TL.PHI_STAR, 2)
    t, a = np.radians(th_s), np.radians(ph_s)
    zl = np.repeat(levels, 12)
    sta = (zl / np.tan(t))[:, None] * np.stack([np.sin(a), np.cos(a)], axis=1)
    hits, _ = ctx.level_stations(sta=sta, level_of=np.repeat([0, 1], 12), n_theta=nt, n_phi=nph, phi_periodic=True, ord_max=2, cap=4)
    assert (hits == 1).all(), hits
    rows, stats = ctx.level_refine(tol=tol, step_max_deg=1.0, probe_deg=0.02, max_iter=12)
    ctx.close()
    c = np.sqrt(K.GAM_R * 250.0)
    want_t = np.sqrt((sta * sta).sum(axis=1) + zl * zl) / c
    e_th = np.abs(rows[:, R["THETA"]] - th_s)
    e_ph = np.abs(SR._wrap180(rows[:, R["PHI"]] - ph_s))
    e_t = np.abs(rows[:, R["TTIME"]] - want_t)
    b_th, b_ph, b_t = np.degrees(tol * np.sin(t) ** 2 / zl), np.degrees(tol * np.tan(t) / zl), tol / c + 1e-6 * rows[:, R["TTIME"]]
    print(f"closed form: {stats}, rounds {rows[:, R['ITER']].astype(int).tolist()}; worst |THETA - theta*| {e_th.max():.3e} deg ({(e_th / b_th).max():.3f} of its bound), "
          f"|PHI - phi*| {e_ph.max():.3e} deg ({(e_ph / b_ph).max():.3f}), |TTIME - t| {e_t.max():.3e} s ({(e_t / b_t).max():.3f}), miss {rows[:, R['MISS']].max():.3e} km")
    assert len(rows) == 24 and (rows[:, R["STATUS"]] == LR.CONVERGED).all(), _status_counts(rows)
    assert (rows[:, R["LEG"]] == 0).all() and (rows[:, R["DIR"]] == 1.0).all() and (rows[:, R["ORD"]] == 0).all()
    assert (e_th <= b_th).all() and (e_ph <= b_ph).all() and (e_t <= b_t).all()
    cel = np.sqrt((sta * sta).sum(axis=1)) / rows[:, R["TTIME"]]                     # the source is the origin here
    assert np.array_equal(SR.bits(rows[:, R["CELERITY"]]), SR.bits(cel))


# ---------------------------------------------------------------- 3. the eigenray condition from a fresh launch
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_converged_rows_pass_through_their_station(G, eq):
    """the 31 x 9 lattice, ring stations and spec of test_relaunched_estimates_pass_the_level_inside_their_triangle (tests/test_gpu_lstations.py).  Every
    CONVERGED row's (THETA, PHI) is integrated again on a second context, the rays of all rows as one fan without probes: the ray holds the row's branch,
    its miss by the restatement is the row's MISS bit for bit and <= tol, and TTIME, ATTEN, N0 .. N2 are that crossing record's.  Against a vacuous pass: at
    least 10 seeds have steep corners (|P3| >= 0.3 at all three) and at least three quarters of those end CONVERGED.  Measured on an MI355X: see DESIGN 8n."""
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_31x9)
    ctx = TL._toy_ctx(G, eq, levels=LEVELS2)
    rec, count, lrec = TL._run(ctx, th, ph)
    legs = rec.shape[2]
    sta, level_of = _rings(eq, ctx, count, lrec, ph, [0, 1], 20)
    sp = LS.spec(nt, nph, ord_max=2, edge_max=TL.EDGE_FEW_CELLS[eq], cap=16)
    hits, lrows = ctx.level_stations(sta=sta, level_of=level_of, **sp)
    steep, n_rows = TL._steep(eq, count, lrec, legs, sp, hits, lrows, sta, level_of)
    rows, stats = ctx.level_refine(**EIGEN)
    ms = ctx.level_refine_timing()
    r_earth = ctx.params.r_earth
    ctx.close()
    assert len(rows) == n_rows
    _check_rows(rows, stats, 1, EIGEN["tol"])
    first = np.concatenate([[0], np.cumsum(np.minimum(hits[0], sp["cap"]))])          # seeds before a station's list
    steep_idx = np.array([first[k] + j for k, j, _ in steep], dtype=int)
    for i, (k, j, _) in zip(steep_idx, steep):                                     # (the seed of a row is the row: station and branch)
        assert rows[i, R["STATION"]] == k and np.array_equal(rows[i, R["LEG"]:R["ORD"] + 1], lrows[0, k, j, S["LEG"]:S["ORD"] + 1])
    status = rows[:, R["STATUS"]].astype(int)
    conv_steep = int((status[steep_idx] == LR.CONVERGED).sum())
    share = conv_steep / max(1, len(steep_idx))
    print(f"{H.EQ_NAMES[eq]}: {n_rows} seeds, status counts {_status_counts(rows)} (converged, limit, stalled, lost, singular), launches {stats['launches']}, "
          f"rounds of the converged {np.bincount(rows[status == 1, R['ITER']].astype(int)).tolist()}; {len(steep_idx)} seeds with steep corners, {conv_steep} of them CONVERGED "
          f"(share {share:.3f}); launches {ms['launch_ms']:.1f} ms, own kernels {ms['kernel_ms']:.3f} ms")
    for i in steep_idx[status[steep_idx] != LR.CONVERGED]:
        print(f"  steep seed {i} not converged: station {int(rows[i, R['STATION']])} branch {rows[i, R['LEG']:R['ORD'] + 1].astype(int).tolist()} {STATUS_NAMES[status[i]]} "
              f"after {int(rows[i, R['ITER']])} rounds, best miss {rows[i, R['MISS']]:.4g} km at theta {rows[i, R['THETA']]:.4f} phi {rows[i, R['PHI']]:.4f}")
    conv = rows[status == LR.CONVERGED]
    fresh = TL._toy_ctx(G, eq, levels=LEVELS2)
    _, count2, lrec2 = TL._run(fresh, conv[:, R["THETA"]].copy(), conv[:, R["PHI"]].copy())
    fresh.close()
    for n, row in enumerate(conv):
        k = int(row[R["STATION"]])
        l = int(level_of[k])
        slot = LS.branch_of_ray(count2[0, n, l], lrec2[0, n, l], int(row[R["LEG"]]), row[R["DIR"]], int(row[R["ORD"]]))
        assert slot >= 0, (n, row[:5], "the re-launched ray does not hold the row's branch")
        X = lrec2[0, n, l, slot]
        c0, c1 = LS.crossing_points(eq, X[None])
        miss = LR.miss_of(eq, c0, c1, np.array([True]), sta[k:k + 1, 0], sta[k:k + 1, 1], np.array([r_earth + LEVELS2[l]]))[0]
        assert SR.bits(np.array([miss]))[0] == SR.bits(row[R["MISS"]:R["MISS"] + 1])[0] and miss <= EIGEN["tol"], (n, miss, row[R["MISS"]])
        want = np.array([X[LVL["TTIME"]], X[LVL["ATTEN"]], X[P0 + 3], X[P0 + 4], X[P0 + 5]])
        assert np.array_equal(SR.bits(row[[R["TTIME"], R["ATTEN"], R["N0"], R["N0"] + 1, R["N0"] + 2]]), SR.bits(want)), (n, row, want)
    assert len(steep_idx) >= 10 and 4 * conv_steep >= 3 * len(steep_idx), (len(steep_idx), conv_steep)


# ---------------------------------------------------------------- 4. members equal plain contexts
MEMBER_SPEC = dict(tol=0.1, step_max_deg=1.0, probe_deg=0.02, max_iter=10, max_shrink=4)


def _lists_and_refine(ctx, th, ph, nt, nph, sta, lv, **spec_kw):
    ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=2, cap=4)
    return ctx.level_refine(**dict(MEMBER_SPEC, **spec_kw))


def _member_rows(rows, m):
    r = rows[rows[:, R["MEMBER"]] == m].copy()
    r[:, R["MEMBER"]] = 0.0
    return r


def _converged_per_member(rows, M):
    return [int(((rows[:, R["MEMBER"]] == m) & (rows[:, R["STATUS"]] == LR.CONVERGED)).sum()) for m in range(M)]


def test_ensemble_members_equal_plain_contexts(G):
    """a 1-D ensemble of 3: ToyAtmo and two perturbations (winds scaled, T shifted)"""
    eq = H.EQ_GLOBAL
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_31x9)
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(**TOY); ctx.set_levels(LEVELS2)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1], 6)
    rows, stats = _lists_and_refine(ctx, th, ph, nt, nph, sta, lv)
    ctx.close()
    per_member = _converged_per_member(rows, 3)
    print(f"ensemble of 3: {stats}, converged per member {per_member}")
    _check_rows(rows, stats, 3, MEMBER_SPEC["tol"])
    assert sum(c > 0 for c in per_member) >= 2
    for m, prof in enumerate(profs):
        one = G.FanContext(eq, device=0)
        one.upload_atmo_1d(*prof)
        one.set_params(**TOY); one.set_levels(LEVELS2)
        one.run(th, ph)
        LR.assert_equal_bits(_member_rows(rows, m), _lists_and_refine(one, th, ph, nt, nph, sta, lv)[0], f"member {m}")
        one.close()


def test_source_set_members_equal_plain_contexts(G):
    """2 sources x 2 profiles; CELERITY is taken from each member's own source point"""
    eq = H.EQ_GLOBAL
    profs = [_device_arrays(eq, *r) for r in _raw_members()[:2]]
    srcs = np.array([[0.0, 30.0, 0.0], [0.0, 30.5, 0.4]])                            # half a degree apart: the same stations serve both
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_31x9)
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(**TOY); ctx.set_levels(LEVELS2)
    ctx.set_sources(srcs)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1], 6)
    rows, stats = _lists_and_refine(ctx, th, ph, nt, nph, sta, lv)
    ctx.close()
    per_member = _converged_per_member(rows, 4)
    print(f"sources 2 x 2: {stats}, converged per member {per_member}")
    _check_rows(rows, stats, 4, MEMBER_SPEC["tol"])
    assert sum(c > 0 for c in per_member) >= 2
    for s, src in enumerate(srcs):
        for k, prof in enumerate(profs):
            one = G.FanContext(eq, device=0)
            one.upload_atmo_1d(*prof)
            one.set_params(**dict(TOY, src=tuple(src))); one.set_levels(LEVELS2)
            one.run(th, ph)
            LR.assert_equal_bits(_member_rows(rows, s * 2 + k), _lists_and_refine(one, th, ph, nt, nph, sta, lv)[0], f"source {s} profile {k}")
            one.close()
    # the range of a converged row is its own source's: the two sources see one station at different ranges
    c = rows[rows[:, R["STATUS"]] == LR.CONVERGED]
    rng = c[:, R["CELERITY"]] * c[:, R["TTIME"]]
    src_of = srcs[(c[:, R["MEMBER"]] // 2).astype(int)]
    want = LR.DIST(src_of[:, 1], src_of[:, 2], sta[c[:, R["STATION"]].astype(int), 0], sta[c[:, R["STATION"]].astype(int), 1], 6370.0)
    assert np.allclose(rng, want, rtol=1e-12, atol=0.0)


def test_grid_ensemble_members_equal_plain_contexts(G, tmp_path):
    """K = 2 grid ensemble, GEOAC_EQ_3D_RNGDEP (geoac_fan_refine refuses these: this call needs no medium at the source); the plain contexts with one lane
    per ray (GRID_LANES=1), as tests/test_gpu_grid_ensemble.py compares"""
    eq = H.EQ_3D_RNGDEP
    th, ph, nt, nph = SC.lattice(**LATTICE_11x9)
    p = dict(TOY, src=(0.0, 0.0, 0.0))
    base = G.FanContext(eq, device=0)
    g = base.load_grid(*RD.write_grid(str(tmp_path), short_paths=False))
    base.close()
    members = [dict(T=g["T"], u=g["u"], v=g["v"], rho=g["rho"]), dict(T=g["T"] + 3.0, u=g["u"] * 0.85, v=g["v"] * 0.85, rho=g["rho"])]
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([m[k] for m in members]) for k in ("T", "u", "v", "rho")])
    ctx.set_params(**p); ctx.set_levels(LEVELS2)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1], 4)
    rows, stats = _lists_and_refine(ctx, th, ph, nt, nph, sta, lv, max_iter=3)          # (a launch through a grid costs the most: three rounds)
    ctx.close()
    per_member = _converged_per_member(rows, 2)
    print(f"grid ensemble of 2: {stats}, status counts {_status_counts(rows)}, converged per member {per_member}")
    _check_rows(rows, stats, 2, MEMBER_SPEC["tol"])
    assert sum(c > 0 for c in per_member) >= 2
    for m in range(2):
        with G.options(GRID_LANES="1"):
            one = G.FanContext(eq, device=0)
            one.upload_atmo_3d(g["x"], g["y"], g["z"], *[members[m][k] for k in ("T", "u", "v", "rho")])
            one.set_params(**p); one.set_levels(LEVELS2)
            one.run(th, ph)
            LR.assert_equal_bits(_member_rows(rows, m), _lists_and_refine(one, th, ph, nt, nph, sta, lv, max_iter=3)[0], f"member {m}")
            one.close()


def test_frequency_set_equals_the_plain_context_at_frequency_0(G):
    eq, freqs = H.EQ_GLOBAL, (0.5, 2.0)
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_31x9)
    ctx = TL._toy_ctx(G, eq, levels=LEVELS2)
    ctx.set_frequencies(freqs)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1], 6)
    rows, stats = _lists_and_refine(ctx, th, ph, nt, nph, sta, lv)
    ctx.close()
    print(f"frequency set: {stats}")
    assert stats["converged"] >= 1
    plain = TL._toy_ctx(G, eq, levels=LEVELS2, freq=freqs[0])
    plain.run(th, ph)
    LR.assert_equal_bits(rows, _lists_and_refine(plain, th, ph, nt, nph, sta, lv)[0])
    plain.close()
    other = TL._toy_ctx(G, eq, levels=LEVELS2)                                        # (ATTEN is the attenuation at that frequency, not at the default 0.1 Hz)
    other.run(th, ph)
    o = _lists_and_refine(other, th, ph, nt, nph, sta, lv)[0]
    other.close()
    conv = rows[:, R["STATUS"]] == LR.CONVERGED
    assert np.array_equal(o[:, :R["ATTEN"]], rows[:, :R["ATTEN"]]) and (o[conv, R["ATTEN"]] != rows[conv, R["ATTEN"]]).all()


# ---------------------------------------------------------------- 5. launch-plan independence
def test_rows_do_not_depend_on_the_launch_plan(G):
    eq = H.EQ_GLOBAL
    out = {}
    for name, opts in (("default", None), ("no_overlap", {"NO_OVERLAP": "1"}), ("compact_0", {"COMPACT": "0"})):
        ctx, (th, ph, nt, nph) = _parity_ctx(G, eq, None, LEVELS2, options=opts)
        rec, count, lrec = TL._run(ctx, th, ph)
        if not out:
            sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1], 8)
        ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=2, cap=4)
        out[name] = ctx.level_refine(max_iter=8, max_shrink=3, tol=0.2, step_max_deg=1.0)
        ctx.close()
    print(f"launch plans: {out['default'][1]}, status counts {_status_counts(out['default'][0])}")
    assert out["default"][1]["seeds"] >= 8 and out["default"][1]["launches"] >= 2
    for name in ("no_overlap", "compact_0"):
        LR.assert_equal_bits(out[name][0], out["default"][0], name)
        assert out[name][1] == out["default"][1]


# ---------------------------------------------------------------- 6. lifecycle and refusals
def test_lifecycle_and_refusals(G):
    eq = H.EQ_GLOBAL
    spec = dict(max_iter=6, max_shrink=3, tol=0.2, step_max_deg=1.0)
    prof = _toy(eq)
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_12x8)

    def make(**params):
        c = G.FanContext(eq, device=0)
        c.upload_atmo_1d(*prof)
        c.set_params(**dict(TOY, **params))
        c.set_levels(LEVELS3)
        return c

    ctx = make(calc_amp=0)                                                          # (nothing reads a Jacobian: calc_amp = 0 serves)
    lib = ctx.lib
    buf = np.zeros((256, 16))
    lkw = dict(n_theta=nt, n_phi=nph, ord_max=2, cap=4)

    def fetch_rc():
        return lib.geoac_fan_level_refine_fetch(ctx._h, buf.ctypes.data_as(ctypes.c_void_p))

    def lists_rc():
        h = np.zeros((1, len(sta)), dtype=np.uint32)
        return lib.geoac_fan_level_stations_fetch(ctx._h, h.ctypes.data_as(ctypes.c_void_p), None)

    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: no level-station lists"):
        ctx.level_refine(**spec)
    rec, count, lrec = TL._run(ctx, th, ph)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: no level-station lists"):          # a launch alone makes no lists
        ctx.level_refine(**spec)
    assert fetch_rc() == -1 and "fan_level_refine_fetch" in lib.geoac_last_error(ctx._h).decode()
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0, 1, 2], 6)
    ctx.level_stations(sta=sta, level_of=lv, **lkw)
    first = ctx.level_refine(**spec)
    n = first[1]["seeds"]
    assert 3 <= n <= 256 and fetch_rc() == 0 and ctx.level_refine_timing()["launch_ms"] > 0.0 and ctx.level_refine_timing()["kernel_ms"] > 0.0
    _check_rows(first[0], first[1], 1, spec["tol"])
    # the context's launch is the last round's: 3 n rays in the records and in the crossing tables; the lattice's lists went with the launches
    assert ctx.n_rays == 3 * n and ctx.fetch()[0].shape == (3 * n, 2, 32) and ctx.fetch_levels()[0].shape == (3 * n, 3)
    assert lists_rc() == -1
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_stations_fetch"):
        ctx._chk(lists_rc())
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: no level-station lists"):          # lists invalidated by a launch (the call's own)
        ctx.level_refine(**spec)
    assert fetch_rc() == 0                                                          # a refused call leaves the result alone
    # lattice launch, lists, refine: works again, and gives the same bits
    ctx.run(th, ph)
    assert fetch_rc() == -1                                                         # a later launch invalidates the result
    ctx.level_stations(sta=sta, level_of=lv, **lkw)
    second = ctx.level_refine(**spec)
    LR.assert_equal_bits(second[0], first[0])
    assert second[1] == first[1]
    # a bad spec names its fault, leaves the lists alone and the earlier result readable
    ctx.run(th, ph)
    ctx.level_stations(sta=sta, level_of=lv, **lkw)
    for bad, word in ((dict(spec, max_iter=0), "max_iter"), (dict(spec, max_shrink=17), "max_shrink"), (dict(spec, tol=0.0), "tol"),
                      (dict(spec, step_max_deg=float("nan")), "step_max_deg"), (dict(spec, probe_deg=0.0), "probe_deg"), (dict(spec, probe_deg=1.5), "probe_deg")):
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: " + word):
            ctx.level_refine(**bad)
    assert lists_rc() == 0
    third = ctx.level_refine(**spec)
    for bad in (dict(spec, tol=-1.0), dict(spec, probe_deg=float("inf"))):
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: "):
            ctx.level_refine(**bad)
        assert fetch_rc() == 0 and np.array_equal(SR.bits(buf[:n]), SR.bits(third[0]))
    # what invalidates the result
    prof_src = list(ctx.params.src)
    for what, act in (("set_angles", lambda: ctx.set_angles(th, ph)), ("set_frequencies", lambda: ctx.set_frequencies([0.1])),
                      ("set_sources", lambda: ctx.set_sources(np.array([prof_src]))), ("upload", lambda: ctx.upload_atmo_1d(*prof)),
                      ("set_levels", lambda: ctx.set_levels(LEVELS3))):
        assert fetch_rc() == 0, what
        act()
        assert fetch_rc() == -1 and "fan_level_refine_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        ctx.run(th, ph)
        ctx.level_stations(sta=sta, level_of=lv, **lkw)
        LR.assert_equal_bits(ctx.level_refine(**spec)[0], first[0], what)
    # the level list changed since the launch
    ctx.run(th, ph)
    ctx.level_stations(sta=sta, level_of=lv, **lkw)
    ctx.set_levels(LEVELS3)                                                         # (the same values again are still a change)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: .*level list has changed"):
        ctx.level_refine(**spec)
    # sample capture
    ctx.run(th, ph)
    ctx.level_stations(sta=sta, level_of=lv, **lkw)
    ctx.set_params(mode=H.MODE_WRITE_RAYS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_refine: .*sample capture"):
        ctx.level_refine(**spec)
    assert lists_rc() == 0
    ctx.set_params(mode=0)
    LR.assert_equal_bits(ctx.level_refine(**spec)[0], first[0])
    ctx.close()
    # calc_amp = 1 gives the same rows: the crossing records do not depend on it
    amp = make()
    amp.run(th, ph)
    amp.level_stations(sta=sta, level_of=lv, **lkw)
    LR.assert_equal_bits(amp.level_refine(**spec)[0], first[0], "calc_amp = 1")
    amp.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    c2.run(th, ph)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_refine: .*2-D set"):
        c2.level_refine(**spec)
    c2.close()


def test_ray_member_cap(G):
    """more than GEOAC_RFN_MAX_RAY_MEMBERS = 2^20 rays x members in a round (3 per seed): one station with an estimate, repeated; refused before anything
    is launched, the lists stay"""
    eq = H.EQ_GLOBAL
    ctx, (th, ph, nt, nph) = _parity_ctx(G, eq, None, LEVELS2)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = _rings(eq, ctx, count, lrec, ph, [0], 12)
    hits, _ = ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=1, cap=1)
    k = int(np.flatnonzero(hits[0] >= 1)[0])
    n_many = G.RFN_MAX_RAY_MEMBERS // 3 + 1
    many = np.ascontiguousarray(np.repeat(sta[k:k + 1], n_many, axis=0))
    hm, _ = ctx.level_stations(sta=many, level_of=np.zeros(n_many, dtype=np.int32), n_theta=nt, n_phi=nph, ord_max=1, cap=1)
    assert (hm >= 1).all()
    with pytest.raises(G.GeoAcError, match="capacity.*fan_level_refine: .*ray-members"):
        ctx.level_refine(**COARSE)
    h2 = np.zeros((1, n_many), dtype=np.uint32)
    assert ctx.lib.geoac_fan_level_stations_fetch(ctx._h, h2.ctypes.data_as(ctypes.c_void_p), None) == 0 and np.array_equal(h2, hm) and ctx.n_rays == len(th)
    ctx.level_stations(sta=sta[k:k + 1], level_of=[0], n_theta=nt, n_phi=nph, ord_max=1, cap=1)
    assert ctx.level_refine(**COARSE)[1]["seeds"] == 1
    ctx.close()


# ---------------------------------------------------------------- 7. a plain context does not change
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
