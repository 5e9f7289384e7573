"""Ensemble fans (geoac_upload_atmo_1d_ensemble): one launch integrates one set of launch angles through K stratified profiles that share
their nodes.  Member m's records must be the very bits a context loaded with profile m alone returns, on every launch plan, and must match
the plain-C oracle loaded with that profile."""
import ctypes
import os

import numpy as np
import pytest

import harness as H
from parity import compare_compact, compare_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESIZE = {H.EQ_GLOBAL: (6, 18), H.EQ_3D: (4, 12), H.EQ_2D: (3, 6)}
HIDX = {H.EQ_GLOBAL: None, H.EQ_3D: 2, H.EQ_2D: 1}
SETS = [H.EQ_2D, H.EQ_3D, H.EQ_GLOBAL]


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _angles():
    """the phi = -90 slice plus a few odd azimuths: 97 rays, not a multiple of 64 or 256"""
    th, ph = H.fan_angles()
    th = np.concatenate([th, [4.5, 11.0, 17.5, 23.0, 29.5, 36.0, 42.5]])
    ph = np.concatenate([ph, [-31.0, 7.0, 45.0, 83.0, 121.0, 159.0, -157.0]])
    return th, ph


def _raw_members(wind=(1.0, 0.6, 1.4), dT=(0.0, 5.0, -5.0), z=None, base=None):
    """raw .met-like columns (z, T, u, v, rho) of ToyAtmo and its perturbations: winds scaled, T shifted"""
    if base is None:
        raw = np.loadtxt(H.TOYATMO)
        base = (raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4])
    z0, T0, u0, v0, r0 = base
    return [(z0, T0 + t, u0 * w, v0 * w, r0) for w, t in zip(wind, dT)]


def _device_arrays(eq, z, T, u, v, rho):
    """what the library is given for raw columns (the oracle's own conversion: radius for the spherical set, tapered winds in km/s)"""
    x = z + (6370.0 if eq == H.EQ_GLOBAL else 0.0)
    taper = (2.0 / (1.0 + np.exp(-(z - 0.0) / 0.2)) - 1.0) / 1000.0
    return x, T, u * taper, v * taper, rho


def _single(G, eq, prof, th, ph, options=None, **params):
    ctx = G.FanContext(eq, device=0, options=options)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(**params)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    return rec, steps


def _ensemble(G, eq, profs, th, ph, options=None, **params):
    ctx = G.FanContext(eq, device=0, options=options)
    x = profs[0][0]
    ctx.upload_atmo_1d_ensemble(x, *[np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)])
    ctx.set_params(**params)
    rec, steps = ctx.run(th, ph)
    assert ctx.n_members == len(profs) and rec.shape == (len(profs), len(th), params.get("bounces", 2) + 1, 32)
    return ctx, rec, steps


def _check_members(G, eq, profs, th, ph, options=None, **params):
    ctx, rec, steps = _ensemble(G, eq, profs, th, ph, options=options, **params)
    ctx.close()
    total = 0
    for m, prof in enumerate(profs):
        want, s = _single(G, eq, prof, th, ph, **params)
        assert np.array_equal(rec[m].view(np.uint64), want.view(np.uint64)), f"member {m} differs from its single-profile run"
        total += s
    assert steps == total
    return rec, steps


@pytest.mark.parametrize("eq", SETS)
@pytest.mark.parametrize("amp", [0, 1])
@pytest.mark.parametrize("bounces", [0, 2])
def test_member_equals_single_context(G, eq, amp, bounces):
    th, ph = _angles()
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    _check_members(G, eq, profs, th, ph, bounces=bounces, calc_amp=amp)


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_members_vs_oracle(G, eq):
    th, ph = _angles()
    raws = _raw_members()
    ctx, rec, steps = _ensemble(G, eq, [_device_arrays(eq, *r) for r in raws], th, ph, bounces=2, calc_amp=1)
    ctx.close()
    total = 0
    for m, r in enumerate(raws):
        O = H.Oracle(eq, met=None)
        O.load_arrays(*r)
        so, ro, _, _ = O.fan(H.make_cfg(eq, bounces=2, calc_amp=True), th, ph)
        assert int(rec[m][:, :, 1].sum()) == so
        compare_records(rec[m], ro, E=ESIZE[eq][1], hidx=HIDX[eq])
        total += so
    assert steps == total


def test_member0_metric_fan_vs_golden(G):
    """member 0 (ToyAtmo as load_met reads it) of a Global ensemble on the metric fan against the reference's records"""
    a = G.met_load(H.TOYATMO, G.EQ_GLOBAL)
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.upload_atmo_1d_ensemble(a["x"], np.stack([a["T"], a["T"] + 4.0]), np.stack([a["u"], 1.3 * a["u"]]), np.stack([a["v"], 1.3 * a["v"]]),
                                np.stack([a["rho"], a["rho"]]))
    ctx.set_params(bounces=2, calc_amp=1)
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (2, 32400, 3, 32)
    assert int(rec[0][:, :, 1].sum()) == 874273730
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_metric.npz"))
    compare_compact(rec[0], g, idx=np.arange(32400))


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_mixed_lengths(G, eq):
    """one member with four times the winds: its rays end far from the others' - late epochs hold many live rays of one member and few of another"""
    th, ph = _angles()
    profs = [_device_arrays(eq, *r) for r in _raw_members(wind=(1.0, 4.0, 0.2), dT=(0.0, 0.0, 3.0))]
    _check_members(G, eq, profs, th, ph, bounces=2, calc_amp=1)


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_large_profile_not_in_lds(G, eq):
    """about 1 800 nodes: the table is read from memory, 64-lane workgroups - against the single runs and the oracle"""
    n = 1800
    raw = np.loadtxt(H.TOYATMO)
    z = np.linspace(0.0, 150.0, n)
    zz = np.minimum(z, raw[-1, 0])
    base = [z] + [np.interp(zz, raw[:, 0], raw[:, c]) for c in (1, 2, 3, 4)]
    raws = _raw_members(base=base)
    th = np.array([3.0, 12.0, 24.0, 33.0, 41.0]); ph = np.array([-90.0, -30.0, 10.0, 77.0, 140.0])
    rec, _ = _check_members(G, eq, [_device_arrays(eq, *r) for r in raws], th, ph, bounces=1, calc_amp=1)
    for m, r in enumerate(raws):
        O = H.Oracle(eq, met=None)
        O.load_arrays(*r)
        so, ro, _, _ = O.fan(H.make_cfg(eq, bounces=1, calc_amp=True), th, ph)
        assert int(rec[m][:, :, 1].sum()) == so
        compare_records(rec[m], ro, E=ESIZE[eq][1], hidx=HIDX[eq])


@pytest.mark.parametrize("opts", [{"S_ROWS": "64"}, {"S_ROWS": "777"}, {"COMPACT": "0"}, {"COMPACT": "1", "S_ROWS": "256"}])
def test_schedule_independence(G, opts):
    th, ph = _angles()
    profs = [_device_arrays(H.EQ_GLOBAL, *r) for r in _raw_members(wind=(1.0, 3.0, 0.5), dT=(0.0, 5.0, -5.0))]
    ctx, ref, s_ref = _ensemble(G, H.EQ_GLOBAL, profs, th, ph, bounces=2, calc_amp=1)
    ctx.close()
    ctx, rec, steps = _ensemble(G, H.EQ_GLOBAL, profs, th, ph, options=opts, bounces=2, calc_amp=1)
    ctx.close()
    assert steps == s_ref
    assert np.array_equal(rec.view(np.uint64), ref.view(np.uint64))


def test_k1_ensemble_equals_plain_upload(G):
    th, ph = _angles()
    prof = _device_arrays(H.EQ_GLOBAL, *_raw_members()[1])
    want, s = _single(G, H.EQ_GLOBAL, prof, th, ph, bounces=2, calc_amp=1)
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.upload_atmo_1d_ensemble(prof[0], *[a[None, :] for a in prof[1:]])
    ctx.set_params(bounces=2, calc_amp=1)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == want.shape and steps == s
    assert np.array_equal(rec.view(np.uint64), want.view(np.uint64))


def test_plain_upload_after_ensemble_restores_shapes(G):
    th, ph = _angles()
    profs = [_device_arrays(H.EQ_3D, *r) for r in _raw_members()]
    want, s = _single(G, H.EQ_3D, profs[2], th, ph, bounces=1, calc_amp=0)
    ctx, rec, _ = _ensemble(G, H.EQ_3D, profs, th, ph, bounces=1, calc_amp=0)
    ctx.upload_atmo_1d(*profs[2])
    assert ctx.n_members == 1
    k = ctypes.c_int(0)
    ctx._chk(ctx.lib.geoac_get_members(ctx._h, ctypes.byref(k)))
    assert k.value == 1
    ctx.launch()                                   # (angles kept from the ensemble run: the slot layout follows K)
    rec1, s1 = ctx.fetch()
    ctx.close()
    assert rec1.shape == want.shape and s1 == s
    assert np.array_equal(rec1.view(np.uint64), want.view(np.uint64))


def test_refused_combinations(G, tmp_path):
    th, ph = _angles()
    profs = [_device_arrays(H.EQ_GLOBAL, *r) for r in _raw_members()]
    x = profs[0][0]
    stack = [np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)]
    # a range-dependent set
    c = G.FanContext(G.EQ_3D_RNGDEP, device=0)
    with pytest.raises(G.GeoAcError, match="not implemented"):
        c.upload_atmo_1d_ensemble(x, *stack)
    c.close()
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    # n_members = 0
    s4 = np.zeros(4 * len(x))
    rc = ctx.lib.geoac_upload_atmo_1d_ensemble(ctx._h, 0, len(x), *[ctypes.c_void_p(a.ctypes.data) for a in (x, profs[0][1], profs[0][2], profs[0][3], profs[0][4], s4)])
    assert rc == -1 and b"n_members" in ctx.lib.geoac_last_error(ctx._h)
    ctx.upload_atmo_1d_ensemble(x, *stack)
    # WriteRays
    ctx.set_params(bounces=1, calc_amp=1, mode=1)
    ctx.set_angles(th, ph)
    with pytest.raises(G.GeoAcError, match="sample capture"):
        ctx.launch()
    ctx.set_params(bounces=1, calc_amp=1, mode=0)
    # clone
    with pytest.raises(G.GeoAcError, match="ensemble"):
        ctx.clone()
    # eigenray search
    with pytest.raises(G.GeoAcError, match="ensemble"):
        ctx.eig_search(np.array([[31.0, 0.5]]))
    # fetch(out=) with a wrongly shaped array
    ctx.launch()
    with pytest.raises(G.GeoAcError, match="shape"):
        ctx.fetch(out=np.zeros((len(th), 2, 32)))
    good = np.zeros((3, len(th), 2, 32))
    rec, _ = ctx.fetch(out=good)
    assert rec is good
    ctx.close()
    # load_met_ensemble with differing altitude columns
    raw = np.loadtxt(H.TOYATMO)
    other = raw.copy(); other[:, 0] *= 1.01
    p0 = tmp_path / "a.met"; p1 = tmp_path / "b.met"
    np.savetxt(p0, raw); np.savetxt(p1, other)
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    with pytest.raises(G.GeoAcError, match="altitude"):
        ctx.load_met_ensemble([str(p0), str(p1)])
    ctx.load_met_ensemble([str(p0), str(p0)])
    assert ctx.n_members == 2
    ctx.close()
