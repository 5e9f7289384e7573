"""Level amplitudes on the device (include/geoac_level_amp.h, FanContext.level_amp_at / level_amp): rows against the numpy restatement
(tests/level_amp_reference.py) driven by the same context's fetch_levels() and public probe calls, bit for bit, on the three sets served (the spherical grid set is refused); the closed
form of tests/level_amp_cases.py; level_amp() after a refinement against level_amp_at() on a second context; members of a source set and a frequency
set against plain contexts, ensembles refused; the ABSENT status; launch-plan independence; the calls' lifecycle and refusals.
Fans are at most 195 rays.  Every test runs under a time limit of its own (a watchdog ends the process: a hung GPU step is not waited for and nothing
is retried)."""
import ctypes
import faulthandler

import numpy as np
import pytest

import harness as H
import level_amp_cases as LC
import level_amp_reference as LA
import level_refine_reference as LR
import lstation_reference as LS
import raised_ground as RG
import rngdep_data as RD
import station_cases as SC
import test_gpu_level_refine as TR
import test_gpu_lstations as TL
from test_gpu_ensemble import _device_arrays, _raw_members
from test_gpu_sources import _toy, _upload

pytestmark = pytest.mark.gpu
A = LA.LAMP
STEP_LIMIT_S = 120
LEVELS2 = [20.0, 35.0]
TOY = TL.TOY
H_DEG = 0.02
ALL_SETS = [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP]          # (GEOAC_EQ_GLOBAL_RNGDEP is refused: test_the_spherical_grid_set_is_refused)
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


def _src3(ctx, srcs=None):
    return np.array([list(ctx.params.src)]) if srcs is None else np.asarray(srcs, dtype=np.float64)


def _restate(ctx, th, ph, level_of, leg, direction, ordinal, h, levels, srcs=None):
    """the restatement of the rows that ctx.level_amp_at(...) has just made, from the same context's crossing tables and probes"""
    count, lrec = ctx.fetch_levels()
    p = ctx.params
    return LA.rows_at(ctx.eqset, TL._members(count, 2), TL._members(lrec, 4), th, ph, level_of, leg, direction, ordinal, h, levels, LA.medium_of_context(ctx), _src3(ctx, srcs),
                      z_grnd=p.z_grnd, r_earth=p.r_earth)


def _status_counts(rows):
    return np.bincount(rows[..., A["STATUS"]].astype(int).ravel(), minlength=6)[1:].tolist()


def _rays(eq, n):
    """n rays of the set's parity medium: inclinations 12 .. 40 and azimuths of its sector, both levels, the three branches a one-bounce ray can hold
    (leg 0 upward, leg 0 downward, leg 1 upward) - the steep rays leave through the top and never come down, the shallow ones turn below 35 km"""
    i = np.arange(n)
    n_th = 6 if eq in GRID_SETS else 8
    th = 12.0 + 4.0 * (i % n_th) + 0.37 * (i // n_th % 3)
    ph = -110.0 + 7.0 * (i * 5 % 7) + 0.11 * (i // 7)
    level_of = (i // 2) % 2
    branch = (i // 3) % 3
    leg, direction = np.where(branch == 2, 1, 0), np.where(branch == 1, -1, 1)
    return th, ph, level_of.astype(np.int32), leg.astype(np.int32), direction.astype(np.int32), np.zeros(n, dtype=np.int32)


# ---------------------------------------------------------------- 1. against the reference's tube
FIXTURE = {"3d": H.EQ_3D, "global": H.EQ_GLOBAL, "3drd": H.EQ_3D_RNGDEP}


@pytest.fixture(scope="module")
def fixture():
    return np.load(LA.FIXTURE)


@pytest.mark.parametrize("name", list(FIXTURE))
def test_rows_against_the_reference_tube(G, fixture, name, tmp_path):
    """tests/golden/level_amp.npz (tests/golden/make_level_amp.py: the compiled reference's own rays): level_amp_at on the fixture's rays, one row per fixture
    crossing.  Statuses, LEG, DIR, ORD exact; DET, TZ, D, AMP within max(1e-6, 4 fd_sens) of the reference's tube at the same h (the project's amplitude rule,
    the margin 4 is tests/parity.py's); the gap to the Jacobian amplitude (the cos form on the spherical set) within the fixture's cap of 2e-2 on every
    crossing.  Measured on an MI355X: DESIGN 8p."""
    g, eq = fixture, FIXTURE[name]
    ctx = G.FanContext(eq, device=0)
    if eq in GRID_SETS:
        ctx.load_grid(*RD.write_grid_ragged(str(tmp_path), False, short_paths=False), z_grnd=RD.ragged_load_z_grnd(False))
    else:
        ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1, mode=0, src=tuple(g[f"{name}_src"]), z_grnd=float(g[f"{name}_z_grnd"]))
    ctx.set_levels(g[f"{name}_levels"], cap=16)
    ray = g[f"{name}_ray"]
    th, ph = g[f"{name}_theta"][ray], g[f"{name}_phi"][ray]
    tol = np.maximum(1e-6, 4.0 * g[f"{name}_fd_sens"])[:, None]
    worst = {}
    for h, key in zip(g["steps"], ("tube02", "tube04")):
        rows = ctx.level_amp_at(th, ph, g[f"{name}_level"], g[f"{name}_leg"], g[f"{name}_dir"], g[f"{name}_ord"], probe_deg=float(h))[0]
        assert (rows[:, A["STATUS"]] == LA.OK).all(), _status_counts(rows)
        assert np.array_equal(rows[:, A["LEG"]], g[f"{name}_leg"]) and np.array_equal(rows[:, A["DIR"]], g[f"{name}_dir"]) and np.array_equal(rows[:, A["ORD"]], g[f"{name}_ord"])
        want = g[f"{name}_{key}"]
        err = np.abs(rows[:, A["DET"]:A["AMP"] + 1] / want - 1.0)
        worst[key] = err.max(axis=0)
        print(f"{name} h = {h:g}: worst |got / reference tube - 1| DET {worst[key][0]:.3e} TZ {worst[key][1]:.3e} D {worst[key][2]:.3e} AMP {worst[key][3]:.3e} "
              f"(worst of its tolerance {(err / tol).max():.3f}; fd_sens up to {g[f'{name}_fd_sens'].max():.3e})")
        if key == "tube02":
            first, e02 = rows, err
    jac = g[f"{name}_amp_jac_cos"] if f"{name}_amp_jac_cos" in g.files else g[f"{name}_amp_jac"]
    gap = np.abs(first[:, A["AMP"]] / jac - 1.0)
    t_err = max(np.abs(first[:, A["TTIME"]] / g[f"{name}_ttime"] - 1.0).max(), np.abs(first[:, A["ATTEN"]] / g[f"{name}_atten"] - 1.0).max())
    print(f"{name}: {len(ray)} crossings; gap of AMP to the Jacobian amplitude: worst {gap.max():.3e}; TTIME / ATTEN against the reference's {t_err:.3e}")
    ctx.close()
    assert (e02 <= tol).all(), (name, "h = 0.02", worst["tube02"])
    assert (np.abs(rows[:, A["DET"]:A["AMP"] + 1] / g[f"{name}_tube04"] - 1.0) <= tol).all(), (name, "h = 0.04", worst["tube04"])
    assert (gap <= float(g["cap"])).all(), (name, gap.max())
    assert t_err <= 1e-6


# ---------------------------------------------------------------- 2. bit for bit against the restatement
@pytest.mark.parametrize("eq", ALL_SETS)
def test_rows_equal_restatement(G, eq, tmp_path):
    """n = 65 (more than one block of 64, not a multiple of it) and n = 1 on the parity media of the level refinement: ToyAtmo, the 5 x 5 grid"""
    ctx, _ = TR._parity_ctx(G, eq, tmp_path, LEVELS2)
    every = []
    for n in (65, 1):
        th, ph, lv, leg, dr, od = _rays(eq, n)
        rows = ctx.level_amp_at(th, ph, lv, leg, dr, od, probe_deg=H_DEG)
        assert rows.shape == (1, n, 16) and ctx.n_rays == 3 * n and ctx.fetch_levels()[0].shape == (3 * n, 2)
        LA.assert_equal_bits(rows, _restate(ctx, th, ph, lv, leg, dr, od, H_DEG, LEVELS2), f"n = {n}")
        ms = ctx.level_amp_timing()
        assert ms["launch_ms"] > 0.0 and ms["kernel_ms"] > 0.0
        every.append(rows[0])
    rows = every[0]
    ok = rows[:, A["STATUS"]] == LA.OK
    print(f"{H.EQ_NAMES[eq]}: n = 65 status counts {_status_counts(rows)} (ok, absent, no probe, singular, skipped); branches of the OK rows "
          f"{sorted(set(map(tuple, rows[ok][:, A['LEG']:A['ORD'] + 1].astype(int).tolist())))}; AMP {rows[ok, A['AMP']].min():.3e} .. {rows[ok, A['AMP']].max():.3e}")
    assert set(rows[:, A["STATUS"]].astype(int)) <= {LA.OK, LA.ABSENT, LA.NO_PROBE} and ok.sum() >= 12
    assert len(set(map(tuple, rows[ok][:, A["LEG"]:A["ORD"] + 1].astype(int).tolist()))) >= 2
    assert np.isfinite(rows).all() and (rows[~ok, A["DET"]:] == 0).all() and (rows[ok, A["AMP"]] > 0).all() and (rows[ok, A["D"]] > 0).all()
    assert (np.sign(rows[ok, A["TZ"]]) == rows[ok, A["DIR"]]).all()                  # the group velocity points the way the passage goes
    assert every[1][0, A["STATUS"]] == LA.OK
    ctx.close()


# ---------------------------------------------------------------- 3. closed form
@pytest.fixture(scope="module")
def uniform_grid(tmp_path_factory):
    return RG.write_uniform_grid(H.EQ_3D_RNGDEP, str(tmp_path_factory.mktemp("lamp_grid")))


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form(G, uniform_grid, eq):
    """straight rays in the isothermal windless medium of tests/raised_ground.py: DET, TZ and AMP against forms that owe nothing to the code
    (tests/level_amp_cases.py, where the bounds are derived)"""
    ctx = G.FanContext(eq, device=0)
    if eq in GRID_SETS:
        ctx.load_grid(*uniform_grid, z_grnd=RG.Z_GRND)
    else:
        ctx.upload_atmo_1d(*RG.profile())
    ctx.set_params(**dict(RG.params(eq), **LC.PARAMS))
    ctx.set_levels(LC.LEVELS)
    th, ph, lv = LC.rays()
    rows = ctx.level_amp_at(th, ph, lv, LC.BRANCH["leg"], LC.BRANCH["dir"], LC.BRANCH["ord"], probe_deg=LC.H_DEG)[0]
    ctx.close()
    out = LC.check_closed_form(rows)
    print(f"{H.EQ_NAMES[eq]} closed form: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()))


# ---------------------------------------------------------------- 4. after a refinement
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_level_amp_after_refinement_equals_level_amp_at(G, eq):
    """the 12 x 8 lattice case of tests/test_gpu_level_refine.py (test_rows_equal_restatement: 3 x 24 stations, both ordinals, twelve rows kept, the coarse
    spec): level_amp() reads the refinement's final launch and launches nothing; every CONVERGED seed's row is the row level_amp_at() makes on a second
    context at that seed's angles, level and branch, bit for bit; every other seed is SKIPPED"""
    levels = TR.LEVELS3
    ctx, (th, ph, nt, nph) = TR._parity_ctx(G, eq, None, levels)
    rec, count, lrec = TL._run(ctx, th, ph)
    sp = LS.spec(nt, nph, ord_max=2, cap=TR.CAP1)
    src = TL._source_xy(ctx)
    sta, lv = np.concatenate([TL._stations_24(eq, src, count, lrec, ph, sp, 2, l) for l in range(3)]), np.repeat([0, 1, 2], 24)
    ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=2, cap=TR.CAP1)
    rrows, stats = ctx.level_refine(**TR.COARSE)
    steps, epochs, n_rays = ctx.total_steps(), ctx.timing()["epochs"], ctx.n_rays
    rows = ctx.level_amp()
    ms = ctx.level_amp_timing()
    assert ms["launch_ms"] == 0.0 and ms["kernel_ms"] > 0.0                          # the timing word shows no launch ...
    assert ctx.total_steps() == steps and ctx.timing()["epochs"] == epochs and ctx.n_rays == n_rays          # ... and the context has made none
    n = stats["seeds"]
    R = LR.LRF
    conv = rrows[:, R["STATUS"]] == LR.CONVERGED
    print(f"{H.EQ_NAMES[eq]}: {n} seeds, {int(conv.sum())} CONVERGED; level_amp status counts {_status_counts(rows)}; own kernels {ms['kernel_ms']:.3f} ms")
    assert rows.shape == (n, 16) and conv.sum() >= 3 and n % 64 != 0
    assert (rows[~conv, A["STATUS"]] == LA.SKIPPED).all() and (rows[~conv, A["DET"]:] == 0).all() and (rows[conv, A["STATUS"]] != LA.SKIPPED).all()
    assert np.array_equal(rows[:, A["INDEX"]], np.arange(float(n))) and np.array_equal(rows[:, A["MEMBER"]], rrows[:, R["MEMBER"]])
    for a, r in (("LEG", "LEG"), ("DIR", "DIR"), ("ORD", "ORD"), ("THETA", "THETA"), ("PHI", "PHI")):
        assert np.array_equal(LA.bits(rows[:, A[a]]), LA.bits(rrows[:, R[r]])), a
    okc = rows[:, A["STATUS"]] == LA.OK
    for a, r in (("TTIME", "TTIME"), ("ATTEN", "ATTEN")):                            # the same crossing record
        assert np.array_equal(LA.bits(rows[okc, A[a]]), LA.bits(rrows[okc, R[r]])), a
    # again: the same bits, still no launch
    LA.assert_equal_bits(ctx.level_amp(), rows, "second call")
    # one round under a tolerance of a metre: most seeds end as ITER_LIMIT and are SKIPPED; the whole result against the restatement on the final tables
    ctx.run(th, ph)
    ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=2, cap=TR.CAP1)
    r1, s1 = ctx.level_refine(max_iter=1, max_shrink=2, tol=1e-3, step_max_deg=1.0)
    one = ctx.level_amp()
    count1, lrec1 = ctx.fetch_levels()
    p = ctx.params
    want = LA.reference_rows(eq, count1[None], lrec1[None], r1[:, R["THETA"]], r1[:, R["PHI"]], LR.spec()["probe_deg"], r1[:, R["MEMBER"]], np.arange(len(r1)),
                             lv[r1[:, R["STATION"]].astype(int)], r1[:, R["LEG"]], r1[:, R["DIR"]], r1[:, R["ORD"]], levels, LA.medium_of_context(ctx), _src3(ctx),
                             z_grnd=p.z_grnd, r_earth=p.r_earth, refine_status=r1[:, R["STATUS"]])
    LA.assert_equal_bits(one, want, "one round")
    print(f"  one round: refinement {TR._status_counts(r1)} (converged, limit, stalled, lost, singular), level_amp {_status_counts(one)}")
    assert (one[:, A["STATUS"]] == LA.SKIPPED).sum() >= 3 and s1["launches"] == 1
    ctx.close()
    other, _ = TR._parity_ctx(G, eq, None, levels)
    c = rrows[conv]
    at = other.level_amp_at(c[:, R["THETA"]].copy(), c[:, R["PHI"]].copy(), lv[c[:, R["STATION"]].astype(int)], c[:, R["LEG"]].astype(int), c[:, R["DIR"]].astype(int),
                            c[:, R["ORD"]].astype(int), probe_deg=LR.spec(**TR.COARSE)["probe_deg"])[0]
    other.close()
    cols = [k for k in range(16) if k != A["INDEX"]]                                  # (INDEX is the seed's index there, the ray's here)
    LA.assert_equal_bits(rows[conv][:, cols], at[:, cols], "CONVERGED rows against level_amp_at")
    assert (at[:, A["STATUS"]] == LA.OK).sum() >= 3


# ---------------------------------------------------------------- 5. members
def _at(ctx, n=12, eq=H.EQ_GLOBAL):
    th, ph, lv, leg, dr, od = _rays(eq, n)
    return ctx.level_amp_at(th, ph, lv, leg, dr, od, probe_deg=H_DEG), (th, ph, lv, leg, dr, od)


def test_source_set_members_equal_plain_contexts(G):
    """two sources x one profile; the sources differ in height as well, so each member's own medium at the source shows"""
    eq = H.EQ_GLOBAL
    prof = _toy(eq)
    srcs = np.array([[0.0, 30.0, 0.0], [1.5, 30.5, 0.4]])
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(**TOY); ctx.set_levels(LEVELS2)
    ctx.set_sources(srcs)
    rows, args = _at(ctx)
    LA.assert_equal_bits(rows, _restate(ctx, *args, H_DEG, LEVELS2, srcs=srcs), "source set against the restatement")
    ctx.close()
    assert rows.shape == (2, 12, 16) and (rows[0, :, A["MEMBER"]] == 0).all() and (rows[1, :, A["MEMBER"]] == 1).all()
    print(f"sources: status counts {_status_counts(rows)}")
    assert (rows[..., A["STATUS"]] == LA.OK).sum() >= 8
    for s, src in enumerate(srcs):
        one = G.FanContext(eq, device=0)
        one.upload_atmo_1d(*prof)
        one.set_params(**dict(TOY, src=tuple(src))); one.set_levels(LEVELS2)
        want = _at(one)[0][0]
        one.close()
        got = rows[s].copy()
        got[:, A["MEMBER"]] = 0.0
        LA.assert_equal_bits(got, want, f"source {s}")
    both = (rows[0, :, A["STATUS"]] == LA.OK) & (rows[1, :, A["STATUS"]] == LA.OK)
    assert (rows[0, both, A["AMP"]] != rows[1, both, A["AMP"]]).all()


def test_frequency_set_equals_the_plain_context(G):
    eq, freqs = H.EQ_GLOBAL, (0.5, 2.0)
    ctx = TL._toy_ctx(G, eq, levels=LEVELS2)
    ctx.set_frequencies(freqs)
    rows, _ = _at(ctx)
    ctx.close()
    plain = TL._toy_ctx(G, eq, levels=LEVELS2, freq=freqs[0])
    want, _ = _at(plain)
    plain.close()
    LA.assert_equal_bits(rows, want)
    other = TL._toy_ctx(G, eq, levels=LEVELS2)                                        # (another frequency: only ATTEN moves - AMP does not depend on it)
    o, _ = _at(other)
    other.close()
    ok = rows[0, :, A["STATUS"]] == LA.OK
    assert ok.sum() >= 4 and np.array_equal(LA.bits(o[..., :A["ATTEN"]]), LA.bits(rows[..., :A["ATTEN"]])) and (o[0, ok, A["ATTEN"]] != rows[0, ok, A["ATTEN"]]).all()


def test_ensembles_are_refused(G, tmp_path):
    eq = H.EQ_GLOBAL
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, [_device_arrays(eq, *r) for r in _raw_members()[:2]])
    ctx.set_params(**TOY); ctx.set_levels(LEVELS2)
    with pytest.raises(G.GeoAcError, match=r"not implemented.*fan_level_amp_at: not available for an ensemble or a grid ensemble \(K > 1\): the medium probes evaluate member 0"):
        _at(ctx)
    th, ph, nt, nph = SC.lattice(**TL.LATTICE_12x8)
    rec, count, lrec = TL._run(ctx, th, ph)
    sta, lv = TR._rings(eq, ctx, count, lrec, ph, [0], 6)
    ctx.level_stations(sta=sta, level_of=lv, n_theta=nt, n_phi=nph, ord_max=1, cap=2)
    ctx.level_refine(**TR.COARSE)
    with pytest.raises(G.GeoAcError, match=r"not implemented.*fan_level_amp: not available for an ensemble or a grid ensemble \(K > 1\)"):
        ctx.level_amp()
    ctx.close()
    eq = H.EQ_3D_RNGDEP
    base = G.FanContext(eq, device=0)
    g = base.load_grid(*RD.write_grid(str(tmp_path), short_paths=False))
    base.close()
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_3d_ensemble(g["x"], g["y"], g["z"], *[np.stack([g[k], g[k] * (1.0 if k == "rho" else 0.9)]) for k in ("T", "u", "v", "rho")])
    ctx.set_params(**dict(TOY, src=(0.0, 0.0, 0.0))); ctx.set_levels(LEVELS2)
    with pytest.raises(G.GeoAcError, match=r"not implemented.*fan_level_amp_at: not available for an ensemble or a grid ensemble \(K > 1\)"):
        _at(ctx, eq=eq)
    assert ctx.lib.geoac_fan_level_amp_fetch(ctx._h, None) == -1                      # a refused call has made nothing
    ctx.close()


def test_the_spherical_grid_set_is_refused(G, tmp_path):
    """GEOAC_EQ_GLOBAL_RNGDEP: on the ragged spherical grid the forward tube is not converged in probe_deg behind a turning point (profiles/level_amp_scan_globalrd.txt)
    and a row could not say so: both calls return GEOAC_E_UNSUPPORTED with the message, make nothing and launch nothing"""
    eq = H.EQ_GLOBAL_RNGDEP
    ctx, (th, ph, nt, nph) = TR._parity_ctx(G, eq, tmp_path, LEVELS2)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_amp_at: not available for GEOAC_EQ_GLOBAL_RNGDEP: .*not converged in probe_deg"):
        _at(ctx, eq=eq)
    rec, count, lrec = TL._run(ctx, th, ph)
    steps = ctx.total_steps()
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_amp_at: not available for GEOAC_EQ_GLOBAL_RNGDEP"):
        _at(ctx, eq=eq)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_amp: not available for GEOAC_EQ_GLOBAL_RNGDEP"):
        ctx.level_amp()
    assert ctx.total_steps() == steps and ctx.n_rays == len(th) and ctx.lib.geoac_fan_level_amp_fetch(ctx._h, None) == -1
    ctx.close()


# ---------------------------------------------------------------- 6. ABSENT
def test_a_ray_that_turns_below_the_level_is_absent(G):
    eq = H.EQ_3D
    ctx = TL._toy_ctx(G, eq, levels=[20.0, 110.0])
    th, ph = np.array([14.0, 14.0, 30.0]), np.array([-90.0, -90.0, -90.0])
    rows = ctx.level_amp_at(th, ph, [0, 1, 1], 0, 1, 0, probe_deg=H_DEG)[0]
    count, _ = ctx.fetch_levels()
    ctx.close()
    print(f"turning ray: crossings of (20 km, 110 km) by the three base rays {count[:3].tolist()}, statuses {[LA.STATUS_NAMES[int(s)] for s in rows[:, A['STATUS']]]}")
    assert count[1, 1] == 0 and count[0, 0] >= 1                                     # the 14 degree ray passes 20 km and never reaches 110 km
    assert rows[:, A["STATUS"]].astype(int).tolist()[:2] == [LA.OK, LA.ABSENT] and (rows[1, A["DET"]:] == 0).all()
    assert np.array_equal(rows[1, :A["DET"]], [0.0, 1.0, 0.0, 1.0, 0.0, float(LA.ABSENT), 14.0, -90.0])


# ---------------------------------------------------------------- 7. launch plans
def test_rows_do_not_depend_on_the_launch_plan(G):
    eq, out = H.EQ_GLOBAL, {}
    for name, opts in (("default", None), ("no_overlap", {"NO_OVERLAP": "1"}), ("compact_0", {"COMPACT": "0"})):
        ctx, _ = TR._parity_ctx(G, eq, None, LEVELS2, options=opts)
        out[name] = _at(ctx, n=40)[0]
        ctx.close()
    assert (out["default"][..., A["STATUS"]] == LA.OK).sum() >= 12
    for name in ("no_overlap", "compact_0"):
        LA.assert_equal_bits(out[name], out["default"], name)


# ---------------------------------------------------------------- 8. lifecycle and refusals
def test_lifecycle_and_refusals(G):
    eq = H.EQ_GLOBAL
    prof = _toy(eq)
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(**dict(TOY, calc_amp=0))                                          # (nothing reads a Jacobian: calc_amp = 0 serves)
    lib = ctx.lib
    buf = np.zeros((64, 16))
    th, ph, lv, leg, dr, od = _rays(eq, 12)

    def fetch_rc():
        return lib.geoac_fan_level_amp_fetch(ctx._h, buf.ctypes.data_as(ctypes.c_void_p))

    assert fetch_rc() == -1 and "fan_level_amp_fetch: no level amplitude rows" in lib.geoac_last_error(ctx._h).decode()
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_amp_at: the context has no level list"):
        ctx.level_amp_at(th, ph, lv, leg, dr, od)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_amp: no level refinement result"):
        ctx.level_amp()
    ctx.set_levels(LEVELS2)
    first = ctx.level_amp_at(th, ph, lv, leg, dr, od, probe_deg=H_DEG)
    assert fetch_rc() == 0 and np.array_equal(LA.bits(buf[:12]), LA.bits(first[0])) and (first[0, :, A["STATUS"]] == LA.OK).sum() >= 6
    ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
    assert lib.geoac_fan_level_amp_dev(ctx._h, ctypes.byref(ptr), ctypes.byref(nbytes)) == 0 and ptr.value and nbytes.value == 12 * 16 * 8
    # bad arguments name their fault and leave the earlier rows readable
    one = np.array([20.0])
    for kw, word in ((dict(level_of=2), "level_of outside"), (dict(level_of=-1), "level_of outside"), (dict(dir=0), "dir must be"), (dict(dir=2), "dir must be"),
                     (dict(leg=-1), "leg and ord"), (dict(ord=-1), "leg and ord"), (dict(probe_deg=0.0), "probe_deg"), (dict(probe_deg=1.5), "probe_deg"),
                     (dict(probe_deg=float("nan")), "probe_deg")):
        a = dict(dict(level_of=0, leg=0, dir=1, ord=0, probe_deg=H_DEG), **kw)
        with pytest.raises(G.GeoAcError, match="invalid.*fan_level_amp_at: .*" + word):
            ctx.level_amp_at(one, one - 110.0, a["level_of"], a["leg"], a["dir"], a["ord"], probe_deg=a["probe_deg"])
        assert fetch_rc() == 0
    assert lib.geoac_fan_level_amp_at(ctx._h, 0, None, None, None, None, None, None, ctypes.c_double(H_DEG)) == -1 and "n must be > 0" in lib.geoac_last_error(ctx._h).decode()
    n_many = G.RFN_MAX_RAY_MEMBERS // 3 + 1
    big, zi = np.full(n_many, 20.0), np.zeros(n_many, dtype=np.int32)
    with pytest.raises(G.GeoAcError, match="capacity.*fan_level_amp_at: .*ray-members"):
        ctx.level_amp_at(big, big - 110.0, zi, zi, zi + 1, zi)
    assert fetch_rc() == 0 and ctx.n_rays == 36 and ctx.fetch_levels()[0].shape == (36, 2)          # (the refused call launched nothing)
    # what ends the result
    src = list(ctx.params.src)
    for what, act in (("launch", lambda: ctx.launch()), ("set_angles", lambda: ctx.set_angles(th, ph)), ("upload", lambda: ctx.upload_atmo_1d(*prof)),
                      ("set_levels", lambda: ctx.set_levels(LEVELS2)), ("set_sources", lambda: ctx.set_sources(np.array([src]))),
                      ("set_frequencies", lambda: ctx.set_frequencies([0.1]))):
        assert fetch_rc() == 0, what
        act()
        assert fetch_rc() == -1 and "fan_level_amp_fetch" in lib.geoac_last_error(ctx._h).decode(), what
        LA.assert_equal_bits(ctx.level_amp_at(th, ph, lv, leg, dr, od, probe_deg=H_DEG), first, what)
    # sample capture
    ctx.set_params(mode=H.MODE_WRITE_RAYS)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_amp_at: not available with sample capture"):
        ctx.level_amp_at(th, ph, lv, leg, dr, od)
    ctx.set_params(mode=0)
    ctx.close()
    # calc_amp = 1 gives the same rows: the crossing records do not depend on it
    amp = G.FanContext(eq, device=0)
    amp.upload_atmo_1d(*prof)
    amp.set_params(**TOY); amp.set_levels(LEVELS2)
    LA.assert_equal_bits(amp.level_amp_at(th, ph, lv, leg, dr, od, probe_deg=H_DEG), first, "calc_amp = 1")
    # level_amp() after a refinement whose result a launch has ended
    lt, lp, nt, nph = SC.lattice(**TL.LATTICE_12x8)
    rec, count, lrec = TL._run(amp, lt, lp)
    sta, lvl = TR._rings(eq, amp, count, lrec, lp, [0, 1], 6)
    amp.level_stations(sta=sta, level_of=lvl, n_theta=nt, n_phi=nph, ord_max=2, cap=4)
    amp.level_refine(max_iter=6, max_shrink=3, tol=0.2, step_max_deg=1.0)
    got = amp.level_amp()
    assert len(got) >= 3 and (got[:, A["STATUS"]] == LA.OK).sum() >= 3
    # the source point and the ground are the launch's: new parameters (which end no result) do not move them
    amp.set_params(src=(3.0, 31.0, 0.5), z_grnd=0.2, r_earth=6371.0)
    LA.assert_equal_bits(amp.level_amp(), got, "after set_params")
    amp.set_params(**TOY, src=(0.0, 30.0, 0.0), z_grnd=0.0, r_earth=6370.0)
    amp.set_levels(LEVELS2)                                                         # (the same values again are still a change)
    with pytest.raises(G.GeoAcError, match="invalid.*fan_level_amp: no level refinement result"):
        amp.level_amp()
    amp.close()
    c2 = G.FanContext(H.EQ_2D, device=0)
    _upload(c2, [_toy(H.EQ_2D)])
    c2.set_params(bounces=0, calc_amp=0)
    with pytest.raises(G.GeoAcError, match="not implemented.*fan_level_amp_at: .*2-D set"):
        c2.level_amp_at(one, one, 0, 0, 1, 0)
    c2.close()
