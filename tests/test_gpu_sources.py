"""Source sets (geoac_set_sources): one launch integrates one set of launch angles from n_src source points, and through K profiles when an
ensemble is loaded.  The records of (source s, profile k) must be the very bits a context loaded with profile k alone and src = src[s]
returns, on every launch plan, and must match the plain-C oracle run from that source."""
import ctypes
import os

import numpy as np
import pytest

import harness as H
from parity import compare_compact, compare_records
from test_gpu_ensemble import _angles, _device_arrays, _raw_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESIZE = {H.EQ_GLOBAL: (6, 18), H.EQ_3D: (4, 12), H.EQ_2D: (3, 6)}
HIDX = {H.EQ_GLOBAL: None, H.EQ_3D: 2, H.EQ_2D: 1}
SETS = [H.EQ_2D, H.EQ_3D, H.EQ_GLOBAL]
# rows in the layout of geoac_params.src: Global (z, lat, lon), 3D (x, y, z), 2D (z, -, -)
SOURCES = {
    H.EQ_GLOBAL: np.array([[0.0, 30.0, 0.0], [20.0, 45.0, -100.0], [0.5, -60.0, 170.0], [45.0, 10.0, 179.5]]),
    H.EQ_3D: np.array([[0.0, 0.0, 0.0], [100.0, -50.0, 20.0], [-30.0, 40.0, 0.5], [5.0, 5.0, 45.0]]),
    H.EQ_2D: np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0], [0.5, 0.0, 0.0], [45.0, 0.0, 0.0]]),
}


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def _toy(eq):
    """ToyAtmo as the library is given it (the oracle's own conversion of the raw columns)"""
    raw = np.loadtxt(H.TOYATMO)
    return _device_arrays(eq, raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4])


def _upload(ctx, profs):
    if len(profs) == 1:
        ctx.upload_atmo_1d(*profs[0])
    else:
        ctx.upload_atmo_1d_ensemble(profs[0][0], *[np.stack([p[k] for p in profs]) for k in (1, 2, 3, 4)])


def _single(G, eq, prof, src, th, ph, **params):
    """a plain context: one profile, the source in the parameters"""
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*prof)
    ctx.set_params(src=tuple(src), **params)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (len(th), params.get("bounces", 2) + 1, 32)
    return rec, steps


def _source_set(G, eq, profs, srcs, th, ph, options=None, **params):
    ctx = G.FanContext(eq, device=0, options=options)
    _upload(ctx, profs)
    ctx.set_params(**params)
    ctx.set_sources(srcs)
    rec, steps = ctx.run(th, ph)
    legs = params.get("bounces", 2) + 1
    want = (len(srcs),) + ((len(profs),) if len(profs) > 1 else ()) + (len(th), legs, 32)
    assert ctx.n_sources == len(srcs) and rec.shape == want
    return ctx, rec, steps


def _check_sources(G, eq, profs, srcs, th, ph, options=None, **params):
    ctx, rec, steps = _source_set(G, eq, profs, srcs, th, ph, options=options, **params)
    ctx.close()
    total = 0
    for s, src in enumerate(srcs):
        for k, prof in enumerate(profs):
            want, st = _single(G, eq, prof, src, th, ph, **params)
            got = rec[s] if len(profs) == 1 else rec[s, k]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"source {s}, profile {k} differs from its single-context run"
            total += st
    assert steps == total
    return rec, steps


@pytest.mark.parametrize("eq", SETS)
@pytest.mark.parametrize("amp", [0, 1])
@pytest.mark.parametrize("bounces", [0, 2])
def test_source_equals_single_context(G, eq, amp, bounces):
    th, ph = _angles()
    _check_sources(G, eq, [_toy(eq)], SOURCES[eq], th, ph, bounces=bounces, calc_amp=amp)


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_sources_vs_oracle(G, eq):
    th, ph = _angles()
    srcs = SOURCES[eq]
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_sources(srcs)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (len(srcs), len(th), 3, 32)
    O = H.Oracle(eq, H.TOYATMO)
    total = 0
    for s, src in enumerate(srcs):
        so, ro, _, _ = O.fan(H.make_cfg(eq, bounces=2, calc_amp=True, src=tuple(src)), th, ph)
        print(f"eq {eq} source {s}: steps {int(rec[s][:, :, 1].sum())} (oracle {so}), result rows {int((rec[s][:, :, 0] != 0).sum())}")
        assert int(rec[s][:, :, 1].sum()) == so
        ro3 = np.asarray(ro).reshape(len(th), 3, -1)
        assert (ro3[:, :, 0] != 0).sum() > 0 and (ro3[:, :, 2] != 0).sum() > 0      # (result rows and broken legs from every source: no empty comparison)
        compare_records(rec[s], ro, E=ESIZE[eq][1], hidx=HIDX[eq])
        total += so
    assert steps == total


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_sources_times_profiles(G, eq):
    th, ph = _angles()
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    rec, _ = _check_sources(G, eq, profs, SOURCES[eq][:3], th, ph, bounces=2, calc_amp=1)
    assert rec.shape == (3, 3, 97, 3, 32)
    # one source on an ensemble: today's ensemble run
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(bounces=2, calc_amp=1, src=tuple(SOURCES[eq][1]))
    want, s_want = ctx.run(th, ph)
    ctx.close()
    ctx = G.FanContext(eq, device=0)
    _upload(ctx, profs)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_sources(SOURCES[eq][1:2])
    got, s_got = ctx.run(th, ph)
    ctx.close()
    assert got.shape == want.shape == (3, 97, 3, 32) and s_got == s_want
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), rec[1].view(np.uint64))


@pytest.mark.parametrize("opts", [{"S_ROWS": "64"}, {"S_ROWS": "777"}, {"COMPACT": "0"}, {"COMPACT": "1", "S_ROWS": "256"}])
def test_schedule_independence(G, opts):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    ctx, ref, s_ref = _source_set(G, eq, [_toy(eq)], SOURCES[eq], th, ph, bounces=2, calc_amp=1)
    ctx.close()
    ctx, rec, steps = _source_set(G, eq, [_toy(eq)], SOURCES[eq], th, ph, options=opts, bounces=2, calc_amp=1)
    ctx.close()
    assert steps == s_ref
    assert np.array_equal(rec.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_large_profile_not_in_lds(G, eq):
    """about 1 800 nodes: the table is read from memory, 64-lane workgroups"""
    n = 1800
    raw = np.loadtxt(H.TOYATMO)
    z = np.linspace(0.0, 150.0, n)
    zz = np.minimum(z, raw[-1, 0])
    prof = _device_arrays(eq, z, *[np.interp(zz, raw[:, 0], raw[:, c]) for c in (1, 2, 3, 4)])
    th = np.array([3.0, 12.0, 24.0, 33.0, 41.0]); ph = np.array([-90.0, -30.0, 10.0, 77.0, 140.0])
    _check_sources(G, eq, [prof], SOURCES[eq][:2], th, ph, bounces=1, calc_amp=1)


def test_source0_metric_fan_vs_golden(G):
    """the default source first in a set of two, on the metric fan, against the reference's records"""
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1)
    ctx.set_sources(np.array([[0.0, 30.0, 0.0], [0.0, 35.0, 0.0]]))
    th, ph = H.fan_angles(phi_min=-180.0, phi_max=179.0, phi_step=1.0)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (2, 32400, 3, 32)
    assert int(rec[0][:, :, 1].sum()) == 874273730
    assert steps == int(rec[:, :, :, 1].sum())
    g = np.load(os.path.join(ROOT, "tests", "golden", "full_metric.npz"))
    compare_compact(rec[0], g, idx=np.arange(32400))


def test_mode_transitions(G):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    srcs = SOURCES[eq]
    prof = _toy(eq)
    plain, s_plain = _single(G, eq, prof, srcs[2], th, ph, bounces=2, calc_amp=1)
    ctx, rec4, s4 = _source_set(G, eq, [prof], srcs, th, ph, bounces=2, calc_amp=1)
    # set_params(src=...) while a set is active: the set stays, source 0 is reported
    ctx.set_params(src=(3.0, -20.0, 50.0))
    p = G.Params()
    ctx._chk(ctx.lib.geoac_get_params(ctx._h, ctypes.byref(p)))
    assert tuple(p.src) == tuple(srcs[0])
    n = ctypes.c_int(0)
    ctx._chk(ctx.lib.geoac_get_sources(ctx._h, ctypes.byref(n)))
    assert n.value == 4
    ctx.launch()
    again, s_again = ctx.fetch()
    assert again.shape == rec4.shape and s_again == s4
    assert np.array_equal(again.view(np.uint64), rec4.view(np.uint64))
    # one row: a plain context again (angles kept: the slot layout follows the number of members)
    ctx.set_sources(srcs[2:3])
    assert ctx.n_sources == 1
    ctx._chk(ctx.lib.geoac_get_sources(ctx._h, ctypes.byref(n)))
    assert n.value == 1
    ctx.launch()
    rec1, s1 = ctx.fetch()
    assert rec1.shape == plain.shape and s1 == s_plain
    assert np.array_equal(rec1.view(np.uint64), plain.view(np.uint64))
    assert np.array_equal(rec1.view(np.uint64), rec4[2].view(np.uint64))
    # ... and back to four
    ctx.set_sources(srcs)
    ctx.launch()
    back, s_back = ctx.fetch()
    ctx.close()
    assert back.shape == rec4.shape and s_back == s4
    assert np.array_equal(back.view(np.uint64), rec4.view(np.uint64))


def test_refused_combinations(G):
    th, ph = _angles()
    eq = H.EQ_GLOBAL
    srcs = SOURCES[eq]
    # a range-dependent set
    c = G.FanContext(G.EQ_3D_RNGDEP, device=0)
    with pytest.raises(G.GeoAcError, match="not implemented"):
        c.set_sources(SOURCES[H.EQ_3D])
    c.close()
    ctx = G.FanContext(eq, device=0)
    ctx.upload_atmo_1d(*_toy(eq))
    # n_src = 0 and more than GEOAC_MAX_MEMBERS
    buf = np.zeros((65, 3))
    for bad in (0, 65):
        assert ctx.lib.geoac_set_sources(ctx._h, bad, ctypes.c_void_p(buf.ctypes.data)) == -1
    assert b"65" in ctx.lib.geoac_last_error(ctx._h) and b"1 profiles" in ctx.lib.geoac_last_error(ctx._h)
    with pytest.raises(G.GeoAcError, match="shape"):
        ctx.set_sources(np.zeros((4, 2)))
    ctx.set_sources(srcs)
    # WriteRays
    ctx.set_params(bounces=1, calc_amp=1, mode=1)
    ctx.set_angles(th, ph)
    with pytest.raises(G.GeoAcError, match="source set"):
        ctx.launch()
    ctx.set_params(bounces=1, calc_amp=1, mode=0)
    # clone
    with pytest.raises(G.GeoAcError, match="source set"):
        ctx.clone()
    # eigenray search
    with pytest.raises(G.GeoAcError, match="source set"):
        ctx.eig_search(np.array([[31.0, 0.5]]))
    # fetch(out=) with a wrongly shaped array
    ctx.launch()
    with pytest.raises(G.GeoAcError, match="shape"):
        ctx.fetch(out=np.zeros((len(th), 2, 32)))
    good = np.zeros((4, len(th), 2, 32))
    rec, _ = ctx.fetch(out=good)
    assert rec is good
    # n_src * K > 64: at set_sources ...
    profs = [_device_arrays(eq, *r) for r in _raw_members()]
    _upload(ctx, profs)
    with pytest.raises(G.GeoAcError, match="22 sources x 3 profiles"):
        ctx.set_sources(np.tile(srcs[0], (22, 1)))
    assert ctx.n_sources == 4
    # ... and at the launch, when an ensemble upload changed K behind a set that fitted
    ctx.upload_atmo_1d(*profs[0])
    ctx.set_sources(np.tile(srcs[0], (22, 1)))
    _upload(ctx, profs)
    with pytest.raises(G.GeoAcError, match="22 sources x 3 profiles"):
        ctx.launch()
    ctx.set_sources(srcs[:2])
    rec, _ = ctx.run(th, ph)
    assert rec.shape == (2, 3, len(th), 2, 32)
    ctx.close()
