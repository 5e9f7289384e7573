"""Frequency sets (geoac_set_frequencies): one launch gives the Sutherland-Bass attenuation of every arrival at F frequencies.  atten[f] must be the
very bits of the ATTEN column a plain context with freq = freqs[f] returns - on every launch plan, on the table path, the fix-up path and the exact
path - the records must be those of the plain freq = freqs[0] run, and every frequency must match the plain-C oracle run at that frequency."""
import ctypes
import os

import numpy as np
import pytest

import harness as H
from parity import RTOL, compare_compact, compare_records
from test_gpu_ensemble import ESIZE, HIDX, SETS, _angles, _device_arrays, _raw_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS = [0.1, 0.01, 0.5, 2.0, 10.0]
ATTEN = H.REC["ATTEN"]


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _toy(eq):
    raw = np.loadtxt(H.TOYATMO)
    return _device_arrays(eq, raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4])


def _single(G, eq, prof, freq, th, ph, options=None, **params):
    """a fresh plain context at one frequency: records, steps, abs_table_info, fan_status"""
    ctx = G.FanContext(eq, device=0, options=options)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(freq=freq, **params)
    rec, steps = ctx.run(th, ph)
    info, status = ctx.abs_table_info(), ctx.fan_status()
    ctx.close()
    return rec, steps, info, status


def _freq_set(G, eq, prof, freqs, th, ph, options=None, **params):
    ctx = G.FanContext(eq, device=0, options=options)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(**params)
    ctx.set_frequencies(freqs)
    rec, steps = ctx.run(th, ph)
    att = ctx.fetch_atten()
    legs = params.get("bounces", 2) + 1
    assert ctx.n_frequencies == len(freqs) and rec.shape == (len(th), legs, 32) and att.shape == (len(freqs), len(th), legs)
    return ctx, rec, steps, att


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_freqs(G, eq, prof, freqs, th, ph, options=None, single_options="same", want_fallback=False, need_idle=False, **params):
    """the set against one fresh plain context per frequency (single_options: the singles' launch-plan options, default the set's)"""
    ctx, rec, steps, att = _freq_set(G, eq, prof, freqs, th, ph, options=options, **params)
    info, status = ctx.abs_table_info(), ctx.fan_status()
    ctx.close()
    assert bool(status & G.FAN_ABS_FALLBACK) == want_fallback
    sopt = options if single_options == "same" else single_options
    for f, fr in enumerate(freqs):
        want, s, _, st1 = _single(G, eq, prof, fr, th, ph, options=sopt, **params)
        assert not (st1 & G.FAN_ABS_FALLBACK)
        assert s == steps
        ndiff = int((_bits(att[f]) != _bits(want[:, :, ATTEN])).sum())
        assert ndiff == 0, f"frequency {f} ({fr} Hz): {ndiff} of {att[f].size} (ray, leg) differ from the single run, max abs {np.abs(att[f] - want[:, :, ATTEN]).max():.3e}"
        if f == 0:
            assert np.array_equal(_bits(rec), _bits(want)), "the set's records differ from the plain freq = freqs[0] run"
            assert np.array_equal(_bits(att[0]), _bits(rec[:, :, ATTEN]))
            ran = want[:, :, H.REC["STEPS"]] > 0
            broke = want[:, :, H.REC["BROKE"]] > 0
            assert ran.any() and broke.any(), "the comparison must cover legs that ran and legs that broke"
            if need_idle:
                assert (~ran).any(), "the comparison must cover legs that did not run"
            assert (want[:, :, ATTEN][ran] > 0).any()
    if len(set(freqs)) > 1:
        assert len({_bits(att[f]).tobytes() for f in range(len(freqs))}) == len(set(freqs))      # (the frequencies do differ)
    return rec, steps, att, info


@pytest.mark.parametrize("eq", SETS)
@pytest.mark.parametrize("amp", [0, 1])
@pytest.mark.parametrize("bounces", [0, 2])
def test_frequency_equals_single_context(G, eq, amp, bounces):
    th, ph = _angles()
    if bounces == 0:
        ctx, rec, steps, att = _freq_set(G, eq, _toy(eq), FREQS, th, ph, bounces=0, calc_amp=amp)
        ctx.close()
        for f, fr in enumerate(FREQS):
            want, s, _, _ = _single(G, eq, _toy(eq), fr, th, ph, bounces=0, calc_amp=amp)
            assert s == steps
            assert np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN])), f"frequency {f}"
            if f == 0:
                assert np.array_equal(_bits(rec), _bits(want))
                # (a single leg: every leg runs, and on some sets none breaks - the bounces = 2 cases cover legs that broke and legs that did not run)
                assert (want[:, :, H.REC["STEPS"]] > 0).all() and (want[:, :, H.REC["VALID"]] > 0).any() and (want[:, :, ATTEN] > 0).any()
        return
    _check_freqs(G, eq, _toy(eq), FREQS, th, ph, bounces=bounces, calc_amp=amp)


def test_legs_that_did_not_run_hold_zero_at_every_frequency(G):
    """a short range limit ends most rays of the spherical set on their first or second leg: the legs behind a break never run"""
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    rec, steps, att, _ = _check_freqs(G, eq, _toy(eq), FREQS, th, ph, need_idle=True, bounces=2, calc_amp=1, range_limit=250.0)
    idle = rec[:, :, H.REC["STEPS"]] == 0
    assert idle.any() and not att[:, idle].any()


@pytest.mark.parametrize("eq", SETS)
def test_frequencies_vs_oracle(G, eq):
    """each frequency against the plain-C oracle at that frequency: ATTEN on the legs that ran, parity.RTOL relative with the floor 1e-12 (the rule of
    compare_records); the records against the oracle at freqs[0] on every field"""
    th, ph = _angles()
    ctx, rec, steps, att = _freq_set(G, eq, _toy(eq), FREQS, th, ph, bounces=2, calc_amp=1)
    ctx.close()
    O = H.Oracle(eq, H.TOYATMO)
    worst = {}
    for f, fr in enumerate(FREQS):
        so, ro, _, _ = O.fan(H.make_cfg(eq, bounces=2, calc_amp=True, freq=fr), th, ph)
        ro = np.asarray(ro).reshape(len(th), 3, -1)
        assert so == steps
        ran = ro[:, :, H.REC["STEPS"]] > 0
        assert ran.any() and (ro[:, :, ATTEN][ran] > 0).any()
        e = np.abs(att[f][ran] - ro[:, :, ATTEN][ran]) / np.maximum(np.abs(ro[:, :, ATTEN][ran]), 1e-12)
        worst[fr] = float(e.max())
        print(f"eq {eq} freq {fr} Hz: legs that ran {int(ran.sum())}, ATTEN max rel err {worst[fr]:.3e}, largest ATTEN {ro[:, :, ATTEN][ran].max():.4e} dB")
        if f == 0:
            compare_records(rec, ro, E=ESIZE[eq][1], hidx=HIDX[eq])
    bad = {fr: e for fr, e in worst.items() if not e <= RTOL}
    assert not bad, f"ATTEN beyond {RTOL:g} of the oracle: {bad}"


def test_metric_fan_vs_golden(G):
    """the metric fan with two frequencies against the reference's records, as the plain run is checked"""
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_frequencies([0.1, 1.0])
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    rec, steps = ctx.run(th, ph)
    att = ctx.fetch_atten()
    ctx.close()
    assert rec.shape == (32400, 3, 32) and att.shape == (2, 32400, 3)
    assert steps == 874273730 == int(rec[:, :, 1].sum())
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_metric.npz"))
    compare_compact(rec, g, idx=np.arange(32400))
    assert np.array_equal(_bits(att[0]), _bits(rec[:, :, ATTEN]))
    ran = rec[:, :, H.REC["STEPS"]] > 0
    assert (att[1][ran] > att[0][ran]).all() and not att[1][~ran].any()      # (absorption grows with frequency; legs that did not run hold 0)


SCHEDULES = [{"S_ROWS": "64"}, {"S_ROWS": "777"}, {"COMPACT": "0"}, {"COMPACT": "1", "S_ROWS": "256"},      # (the option sets of the ensemble and source tests)
             {"S_ROWS": "40", "TWO_CHUNKS": "1"},                                                            # rays over hundreds of epochs, two chunks in rotation
             {"NO_OVERLAP": "1", "S_ROWS": "512"}, {"CU_SPLIT": "64", "S_ROWS": "1024"}, {"ACCUM_BATCH": "1", "S_ROWS": "300"}, {"ACCUM_BATCH": "0"},
             {"ABS_TABLE": "0"}, {"ABS_TABLE": "0", "S_ROWS": "200"}]


@pytest.mark.parametrize("opts", SCHEDULES)
def test_schedule_independence(G, opts):
    """under the options on the set's side, against singles on the DEFAULT plan (ABS_TABLE=0: on both sides)"""
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    exact = opts.get("ABS_TABLE") == "0"
    _, _, _, info = _check_freqs(G, eq, _toy(eq), FREQS, th, ph, options=opts, single_options={"ABS_TABLE": "0"} if exact else None, bounces=2, calc_amp=1)
    assert info["entries"] == 0 if exact else info["entries"] > 0


def test_default_plan_serves_the_set_from_the_tables(G):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    ctx, rec, steps, att = _freq_set(G, eq, _toy(eq), FREQS, th, ph, bounces=2, calc_amp=1)
    info = ctx.abs_table_info()
    ctx.close()
    one = _single(G, eq, _toy(eq), FREQS[0], th, ph, bounces=2, calc_amp=1)[2]
    assert one["entries"] > 0 and info["entries"] == len(FREQS) * one["entries"]      # (summed over the frequencies' tables)
    assert 4 * info["flagged"] <= info["entries"]


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_large_profile_not_in_lds(G, eq):
    """about 1 800 nodes: the table is read from memory, 64-lane workgroups"""
    n = 1800
    raw = np.loadtxt(H.TOYATMO)
    z = np.linspace(0.0, 150.0, n)
    zz = np.minimum(z, raw[-1, 0])
    prof = _device_arrays(eq, z, *[np.interp(zz, raw[:, 0], raw[:, c]) for c in (1, 2, 3, 4)])
    th = np.array([3.0, 12.0, 24.0, 33.0, 41.0]); ph = np.array([-90.0, -30.0, 10.0, 77.0, 140.0])
    ctx, rec, steps, att = _freq_set(G, eq, prof, [0.2, 0.05, 3.0], th, ph, bounces=1, calc_amp=1)
    ctx.close()
    for f, fr in enumerate([0.2, 0.05, 3.0]):
        want, s, _, _ = _single(G, eq, prof, fr, th, ph, bounces=1, calc_amp=1)
        assert s == steps and np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN])), f"frequency {f}"
        if f == 0:
            assert np.array_equal(_bits(rec), _bits(want))


def test_limits_and_transitions(G):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    prof = _toy(eq)
    # sixteen frequencies, duplicates allowed
    f16 = [0.05 * 1.4 ** i for i in range(15)] + [0.05]
    ctx, rec, steps, att = _freq_set(G, eq, prof, f16, th, ph, bounces=2, calc_amp=1)
    assert np.array_equal(_bits(att[15]), _bits(att[0]))
    for f in (0, 7, 14):
        want, s, _, _ = _single(G, eq, prof, f16[f], th, ph, bounces=2, calc_amp=1)
        assert s == steps and np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN])), f"frequency {f} of 16"
    # bad arguments: GEOAC_E_INVALID, the set stays
    buf = np.full(17, 0.3)
    setf = ctx.lib.geoac_set_frequencies
    setf.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for bad in (17, 0, -1):
        assert setf(ctx._h, bad, ctypes.c_void_p(buf.ctypes.data)) == -1
    for badv in (-0.5, 0.0, float("nan"), float("inf")):
        b = np.array([0.1, badv, 0.2])
        assert setf(ctx._h, 3, ctypes.c_void_p(b.ctypes.data)) == -1
    assert setf(ctx._h, 2, None) == -1
    assert ctx.n_frequencies == 16
    # set_params(freq=...) while a set is active: the set stays, frequency 0 is reported
    ctx.set_params(freq=7.0)
    p = G.Params()
    ctx._chk(ctx.lib.geoac_get_params(ctx._h, ctypes.byref(p)))
    assert p.freq == f16[0] and ctx.n_frequencies == 16
    ctx.launch()
    again, s_again = ctx.fetch()
    assert s_again == steps and np.array_equal(_bits(again), _bits(rec)) and np.array_equal(_bits(ctx.fetch_atten()), _bits(att))
    # changing the list between launches rebuilds the tables
    f3 = [2.0, 0.1, 0.7]
    ctx.set_frequencies(f3)
    ctx.launch()
    att3 = ctx.fetch_atten()
    rec3, _ = ctx.fetch()
    assert att3.shape == (3, len(th), 3)
    for f, fr in enumerate(f3):
        want, s, _, _ = _single(G, eq, prof, fr, th, ph, bounces=2, calc_amp=1)
        assert np.array_equal(_bits(att3[f]), _bits(want[:, :, ATTEN])), f"frequency {f} after the list changed"
        if f == 0:
            assert np.array_equal(_bits(rec3), _bits(want))
    # a second upload keeps the set and still matches single runs on the new profile
    prof2 = _device_arrays(eq, *_raw_members()[1])
    ctx.upload_atmo_1d(*prof2)
    assert ctx.n_frequencies == 3
    ctx.launch()
    att2 = ctx.fetch_atten()
    for f, fr in enumerate(f3):
        want, s, _, _ = _single(G, eq, prof2, fr, th, ph, bounces=2, calc_amp=1)
        assert np.array_equal(_bits(att2[f]), _bits(want[:, :, ATTEN])), f"frequency {f} on the second profile"
    # one frequency leaves the mode: a plain context at that frequency, fetch_atten = the ATTEN column
    ctx.set_frequencies([0.7])
    assert ctx.n_frequencies == 1
    ctx._chk(ctx.lib.geoac_get_params(ctx._h, ctypes.byref(p)))
    assert p.freq == 0.7
    ctx.launch()
    rec1, s1 = ctx.fetch()
    att1 = ctx.fetch_atten()
    want, s, _, _ = _single(G, eq, prof2, 0.7, th, ph, bounces=2, calc_amp=1)
    assert s1 == s and np.array_equal(_bits(rec1), _bits(want))
    assert att1.shape == (1, len(th), 3) and np.array_equal(_bits(att1[0]), _bits(want[:, :, ATTEN]))
    assert np.array_equal(_bits(att1[0]), _bits(att2[2]))
    # the device table of a single frequency
    ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
    ctx._chk(ctx.lib.geoac_fan_atten_dev(ctx._h, ctypes.byref(ptr), ctypes.byref(nbytes)))
    assert ptr.value and nbytes.value == 8 * len(th) * 3
    # set_params(freq=...) acts again
    ctx.set_params(freq=0.1)
    ctx.launch()
    want, s, _, _ = _single(G, eq, prof2, 0.1, th, ph, bounces=2, calc_amp=1)
    assert np.array_equal(_bits(ctx.fetch()[0]), _bits(want))
    # fetch_atten(out=)
    with pytest.raises(G.GeoAcError, match="shape"):
        ctx.fetch_atten(out=np.zeros((2, len(th), 3)))
    good = np.zeros((1, len(th), 3))
    assert ctx.fetch_atten(out=good) is good
    ctx.close()


def test_refused_combinations(G):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    prof = _toy(eq)
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    stack = [np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)]
    srcs = np.array([[0.0, 30.0, 0.0], [20.0, 45.0, -100.0]])
    # a range-dependent set
    for rd in (G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        c = G.FanContext(rd, device=0)
        with pytest.raises(G.GeoAcError, match="not implemented"):
            c.set_frequencies([0.1, 0.2])
        assert c.n_frequencies == 1
        c.close()
    # an ensemble / a source set made active BEFORE the set is given
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d_ensemble(profs[0][0], *stack)
    with pytest.raises(G.GeoAcError, match="not implemented.*ensemble"):
        ctx.set_frequencies([0.1, 0.2])
    ctx.set_frequencies([0.3])                                       # (one frequency is no set)
    ctx.upload_atmo_1d(*prof)
    ctx.set_sources(srcs)
    with pytest.raises(G.GeoAcError, match="not implemented.*source set"):
        ctx.set_frequencies([0.1, 0.2])
    ctx.set_sources(srcs[:1])
    # ... and AFTER it: refused at the launch, usable again once either side is single
    ctx.set_params(bounces=1, calc_amp=1, freq=0.1)
    ctx.set_frequencies([0.1, 0.2])
    ctx.set_angles(th, ph)
    ctx.upload_atmo_1d_ensemble(profs[0][0], *stack)
    with pytest.raises(G.GeoAcError, match="not implemented.*frequency set"):
        ctx.launch()
    ctx.upload_atmo_1d(*prof)
    ctx.set_sources(srcs)
    with pytest.raises(G.GeoAcError, match="not implemented.*frequency set"):
        ctx.launch()
    ctx.set_sources(srcs[:1])
    # WriteRays / WriteCaustics
    for mode in (1, 2):                                             # GEOAC_MODE_WRITE_RAYS, GEOAC_MODE_WRITE_CAUSTICS
        ctx.set_params(bounces=1, calc_amp=1, mode=mode)
        with pytest.raises(G.GeoAcError, match="not implemented.*sample capture"):
            ctx.launch()
    ctx.set_params(bounces=1, calc_amp=1, mode=0)
    # clone, eigenray search
    with pytest.raises(G.GeoAcError, match="not implemented.*frequency set"):
        ctx.clone()
    with pytest.raises(G.GeoAcError, match="not implemented.*frequency set"):
        ctx.eig_search(np.array([[31.0, 0.5]]))
    # the context is still usable, and right
    rec, steps = ctx.run(th, ph)
    att = ctx.fetch_atten()
    ctx.close()
    for f, fr in enumerate([0.1, 0.2]):
        want, s, _, _ = _single(G, eq, prof, fr, th, ph, bounces=1, calc_amp=1)
        assert s == steps and np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN]))
    # the pool
    pool = G.FanPool(eq, [0])
    pool.load_met(H.TOYATMO)
    pool.set_params(bounces=1, calc_amp=1)
    h = ctypes.c_void_p(pool.lib.geoac_pool_ctx(pool._h, 0))
    fr = np.array([0.1, 0.2])
    pool.lib.geoac_set_frequencies.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert pool.lib.geoac_set_frequencies(h, 2, ctypes.c_void_p(fr.ctypes.data)) == 0
    with pytest.raises(G.GeoAcError, match="not implemented.*frequency set"):
        pool.run(th, ph)
    assert pool.lib.geoac_set_frequencies(h, 1, ctypes.c_void_p(fr.ctypes.data)) == 0
    rec, _ = pool.run(th, ph)
    pool.close()
    ctx = G.FanContext(eq, device=0)                                 # (the pool reads the profile as load_met does)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=1, calc_amp=1)
    want, _ = ctx.run(th, ph)
    ctx.close()
    assert np.array_equal(_bits(rec), _bits(want))


def test_fix_up_path_and_fallback(G):
    """A tolerance tighter than the interpolants reach (ABS_TABLE_TOL) flags part of every frequency's table: the (segment, frequency) pairs that fall
    into flagged entries go through the per-frequency fix-up and the set still equals the single runs under the same option.  With a fix-up list of one
    entry (PPFIX_CAP=1) the list overflows: the fan is repeated with the exact post-pass for all frequencies, the context says so, and atten[f] equals the
    ABS_TABLE=0 single runs."""
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    prof = _toy(eq)
    freqs = [0.1, 0.5, 2.0]
    found = None
    for tol in ("2e-11", "1e-11", "5e-12", "2e-12", "1e-12"):
        ctx, rec, steps, att = _freq_set(G, eq, prof, freqs, th, ph, options={"ABS_TABLE_TOL": tol}, bounces=2, calc_amp=1)
        info, status = ctx.abs_table_info(), ctx.fan_status()
        ctx.close()
        print("tolerance", tol, info, "status", hex(status))
        if info["entries"] > 0 and info["flagged"] > 0 and info["fixup_segments"] > 0 and not (status & G.FAN_ABS_FALLBACK):
            found = tol
            break
    assert found is not None, "no tolerance flagged a part, and less than a quarter, of every frequency's table"
    assert 4 * info["flagged"] <= info["entries"]
    for f, fr in enumerate(freqs):
        want, s, i1, st1 = _single(G, eq, prof, fr, th, ph, options={"ABS_TABLE_TOL": found}, bounces=2, calc_amp=1)
        assert i1["entries"] > 0 and not (st1 & G.FAN_ABS_FALLBACK)
        assert s == steps and np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN])), f"frequency {f} on the fix-up path"
        if f == 0:
            assert np.array_equal(_bits(rec), _bits(want))
    # the list overflows
    ctx, rec, steps, att = _freq_set(G, eq, prof, freqs, th, ph, options={"ABS_TABLE_TOL": found, "PPFIX_CAP": "1"}, bounces=2, calc_amp=1)
    info, status = ctx.abs_table_info(), ctx.fan_status()
    ctx.close()
    assert status & G.FAN_ABS_FALLBACK and info["entries"] == 0
    for f, fr in enumerate(freqs):
        want, s, _, _ = _single(G, eq, prof, fr, th, ph, options={"ABS_TABLE": "0"}, bounces=2, calc_amp=1)
        assert s == steps and np.array_equal(_bits(att[f]), _bits(want[:, :, ATTEN])), f"frequency {f} after the fallback"
        if f == 0:
            assert np.array_equal(_bits(rec), _bits(want))
