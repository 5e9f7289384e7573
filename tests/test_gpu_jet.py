"""The stratified sets (2D, 3D, Global) on a jet profile with meridional wind against the compiled reference (tests/golden/jet_small.npz, make_golden.py
`jet`; the profile: tests/golden/JetAtmo.met, tests/jet_data.py).  Every other atmosphere of the suite is ToyAtmo or a rescaling of it, whose v is 1e-15 m/s:
here v is 40 / -22 / 15 m/s and u -50 .. 38 m/s, the elevated source sits inside the wind, rays are launched below the horizontal, ducted rays run to the
range limit, and every context reads the file through the second profile format, `zuvwTdp`.  The fixture holds the reference's own answer to a 1e-12 relative
change of theta for every compared field of every arrival (4 x that <= 1e-6, asserted when it was made): the project's 1e-6 rule applies to every arrival, no
exemption list.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

import harness as H
import jet_data as JD
import known_answers as K
from parity import compare_records, field_errors
from test_gpu_probes import _colwise

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 120
SETS = [H.EQ_GLOBAL, H.EQ_3D, H.EQ_2D]
RTOL = 1e-6


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
def gold():
    return np.load(JD.FIXTURE)


def _params(gold, eq, tag, **over):
    p = dict(src=JD.src(eq, JD.fan(gold, tag)[2]), range_limit=float(gold["range_limit"]), mode=0, **JD.TABLES[tag][1])
    p.update(over)
    return p


def _ctx(G, eq, **params):
    ctx = G.FanContext(eq, device=0)
    ctx.load_met(JD.JET, fmt=JD.FMT)                     # (the host parser's second format is on every tested path)
    ctx.set_params(**params)
    return ctx


def _run(G, gold, eq, tag, env=None, **over):
    th, ph, _ = JD.fan(gold, tag)
    with G.options(**(env or {})):
        ctx = _ctx(G, eq, **_params(gold, eq, tag, **over))
        rec, steps = ctx.run(th, ph)
        info = ctx.abs_table_info()
        ctx.close()
    return rec, steps, info


@pytest.mark.parametrize("tag", list(JD.TABLES))
@pytest.mark.parametrize("eq", SETS)
def test_jet_fan_vs_reference(G, gold, eq, tag):
    """three sets x (fan a: ground source; fan b: source at 12 km, inside the wind, launches below the horizontal) x CalcAmp on / off, and fan b with a raised
    ground, 10 Hz and another absorption factor, and at 0.01 Hz: step total exact, every field to 1e-6 (parity.compare_records)"""
    th, ph, _ = JD.fan(gold, tag)
    want, want_steps, sens = JD.table(gold, eq, tag)
    E = JD.ESIZE[eq][1 if JD.TABLES[tag][1]["calc_amp"] else 0]
    assert 4.0 * np.nanmax(sens) <= 1e-6                  # the reference's own conditioning covers every compared field of every arrival
    valid, broke = want[..., H.REC["VALID"]] > 0, want[..., H.REC["BROKE"]] > 0
    # no empty comparison: arrivals, arrivals off the east-west line (where v sin(phi) and ny v vanish); fan b: of rays launched downwards, and broken legs
    assert valid.sum() >= 60 and valid[np.abs(np.abs(ph) - 90.0) > 1.0].sum() >= 40
    if JD.TABLES[tag][0] == "b":
        assert valid[th < 0.0].sum() >= 9 and broke.sum() >= 50
    rec, steps, _ = _run(G, gold, eq, tag)
    fe = field_errors(rec, want, E, JD.HIDX[eq])
    print(f"jet {H.EQ_NAMES[eq]} {tag}: worst error per field: " + ", ".join(f"{f} {np.nanmax(fe[f]):.2e}" for f in sorted(fe))
          + f"; worst reference sensitivity {np.nanmax(sens):.1e}")
    assert steps == want_steps
    compare_records(rec, want, E=E, hidx=JD.HIDX[eq])


@pytest.mark.parametrize("eq", SETS)
def test_jet_spline_accessors_and_absorption_vs_reference(G, gold, eq):
    """c, c', c'', u, u', u'', v, v', v'', rho at 1000 abscissae of the irregular profile - nodes, both ends, beyond both ends, on and beside the 3 .. 10 m
    segments - and SuthBass_Alpha at 200 (altitude, frequency) pairs.  The v columns are of a wind of tens of m/s, not of ToyAtmo's rounding noise."""
    ctx = _ctx(G, eq, bounces=0, calc_amp=1, mode=0)
    ctx.run(np.array([20.0]), np.array([-90.0]))          # the probes use the parameter block of a completed launch
    want9, want_rho = JD.atmo(gold, eq, "probe_out9"), JD.atmo(gold, eq, "probe_rho")
    assert (np.abs(want9[:, 6:9]).max(axis=0)[0] > 1e-3) and np.abs(want9[:, 3]).max() > 1e-3          # km/s
    o9, rho = ctx.probe_atmo_1d(JD.atmo(gold, eq, "probe_x"))
    e = _colwise(o9, want9)
    er = _colwise(rho[:, None], want_rho[:, None])
    print("jet", H.EQ_NAMES[eq], "out9 max rel err per column", [f"{v:.1e}" for v in e], "rho", f"{er[0]:.1e}")
    assert e.max() <= RTOL and er.max() <= RTOL
    a = ctx.probe_absorption(JD.atmo(gold, eq, "abs_x"), JD.atmo(gold, eq, "abs_f"))
    want = JD.atmo(gold, eq, "abs_alpha")
    rel = np.abs(a - want) / np.abs(want)
    print("jet", H.EQ_NAMES[eq], "alpha: max rel err", rel.max())
    ctx.close()
    assert (want > 0).all() and rel.max() <= RTOL


@pytest.mark.parametrize("eq", SETS)
def test_jet_absorption_table_vs_exact_routine_and_reference(G, gold, eq):
    """test_gpu_probes.py::test_absorption_table_vs_exact_routine_and_reference on the irregular grid (segments of 3 m .. 0.3 km): the table against the exact
    device routine to 1e-9 wherever it serves a point, against the reference's values to 1e-6.  Entries the build flags (interpolant beyond its tolerance on
    a long segment) are reported, not assumed absent: a point inside the profile is unserved only if there are flagged entries.

    What this test found: before k_atab_build held the nu^2 piece to a bound of its own, 2.05e-9 at 98.915 km inside a served 0.28 km segment - one step
    of the staircase the exact routine has in sqrt(1 + nu^2) - 1, where the interpolant of nu^2 rounded the other way.  Since: 41 of 901 entries flagged, worst 6.0e-10."""
    ctx = _ctx(G, eq, bounces=0, calc_amp=1, mode=0)
    ctx.run(np.array([20.0]), np.array([-90.0]))
    info = ctx.abs_table_info()
    nodes = G.met_load(JD.JET, eq, fmt=JD.FMT)["x"]
    x0, x1 = nodes[0], nodes[-1]
    assert info["entries"] == len(nodes) + 1, info                   # nseg + 2
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.uniform(x0 - 0.04, x1 + 0.04, 36000), nodes, nodes[1:] - 1e-9, nodes[:-1] + 1e-9,
                         np.array([x0 - 0.049, x0 - 1e-12, x1 + 1e-12, x1 + 0.049, x0 - 0.2, x1 + 0.2])])
    tab = ctx.probe_absorption_table(xs)
    ex = ctx.probe_absorption(xs, np.full(len(xs), 0.1))
    served = tab >= 0.0
    beyond = (xs < x0 - 0.05) | (xs > x1 + 0.05)
    assert not served[beyond].any()                                   # beyond the strips: left to the exact pass
    inside = ~beyond
    print("jet", H.EQ_NAMES[eq], "table entries", info["entries"], "flagged", info["flagged"], "served", served[inside].mean())
    assert served[inside].all() or info["flagged"] > 0
    at_node = np.isin(xs, nodes)
    rel = np.abs(tab - ex) / ex
    print("jet", H.EQ_NAMES[eq], "table vs exact routine: max rel err off the nodes", rel[served & ~at_node].max(), "at the nodes", rel[served & at_node].max())
    iw = np.flatnonzero(served & ~at_node)[np.argmax(rel[served & ~at_node])]
    print("jet", H.EQ_NAMES[eq], f"   the worst point off the nodes: height {xs[iw] - (6370.0 if eq == H.EQ_GLOBAL else 0.0):.6f} km")
    assert rel[served & ~at_node].max() <= 1e-9
    assert rel[served & at_node].max() <= 1e-2 and np.median(rel[served & at_node]) <= 1e-12
    abs_x, abs_f, abs_alpha = (JD.atmo(gold, eq, k) for k in ("abs_x", "abs_f", "abs_alpha"))
    idx = np.argsort(abs_f)[np.linspace(0, len(abs_f) - 1, 12).astype(int)]
    worst, n = 0.0, 0
    for i in idx:
        ctx.set_params(freq=float(abs_f[i]))
        ctx.run(np.array([20.0]), np.array([-90.0]))
        t = ctx.probe_absorption_table(abs_x[i:i + 1])
        if t[0] >= 0.0:
            worst = max(worst, float(np.abs(t[0] - abs_alpha[i]) / abs_alpha[i])); n += 1
    ctx.close()
    print("jet", H.EQ_NAMES[eq], "table vs reference SuthBass_Alpha at", n, "of", len(idx), "frequencies: max rel err", worst)
    assert (n == len(idx) or info["flagged"] > 0) and n >= 6 and worst <= RTOL


def _plans(G):
    """the launch plans of test_gpu_polar.py::test_polar_fan_is_schedule_independent"""
    plans = [{"GEOAC_PAIR_FRAC": "0.03"}, {"GEOAC_NO_PAIR": "1"}, {"GEOAC_NO_PAIR": "1", "GEOAC_COMPACT": "0"},
             {"GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "4096"}, {"GEOAC_PAIR_FRAC": "1.0"}, {"GEOAC_PAIR_FRAC": "0"}]
    plans += [{"GEOAC_ACCUM_BATCH": "1"}, {"GEOAC_ACCUM_BATCH": "0"}, {"GEOAC_CHUNK_GIB": "1", "GEOAC_ACCUM_BATCH": "1"}]
    plans += [{"GEOAC_NO_PAIR": "1", "GEOAC_CU_SPLIT": "64"}]
    if G.has_ab_kernels():
        plans += [{"GEOAC_DUO": "1"}, {"GEOAC_DUO": "1", "GEOAC_COMPACT": "0"}, {"GEOAC_DUO": "1", "GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "3000"}]
        plans += [{"GEOAC_TRIO": "1"}, {"GEOAC_TRIO": "1", "GEOAC_PAIR_FRAC": "1.0"}, {"GEOAC_TRIO": "1", "GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "3000"}]
    return plans


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_jet_fan_is_schedule_independent(G, gold, eq):
    """fan b under every launch plan: the records of the default plan, bit for bit.  The one-lane and the two-lane kernels (cart3_rhs<true, 1>, EqGlobalPair)
    - and the wave-specialised ones of A/B builds - each hold their own copy of the v terms' operands; with v = 1e-15 m/s a wrong one could not show."""
    ref, steps, _ = _run(G, gold, eq, "b_amp1")
    assert steps == JD.table(gold, eq, "b_amp1")[1]
    for env in _plans(G):
        rec, st, _ = _run(G, gold, eq, "b_amp1", env)
        assert st == steps, env
        assert np.array_equal(rec.view(np.uint64), ref.view(np.uint64)), env


LONG_TH = [-20.0, 6.0, 25.0, 41.0]          # (6: ducted in the tropospheric jet, runs to the range limit)
LONG_RANGE = 800.0


@pytest.mark.parametrize("eq", [H.EQ_GLOBAL, H.EQ_3D])
def test_jet_profile_read_through_l2(G, gold, eq):
    """the kernels that read the spline table from memory (a profile beyond 1463 segments does not fit the 160 KiB of LDS): the jet resampled on 1800 nodes, a
    4 x 8 fan from 12 km, against the oracle on the same columns (steps exact, fields to 1e-6: the oracle's own answer to theta (1 + 1e-12) is measured here and
    held to the fixture's rule, 4 x sens <= 1e-6) and bit for bit between one lane and two lanes per ray, compaction on and off"""
    z, T, u, v, rho = JD.resampled(1800)
    az = np.unique(JD.fan(gold, "b_amp1")[1])
    th = np.array([t for a in az for t in LONG_TH]); ph = np.array([a for a in az for t in LONG_TH])
    src = JD.src(eq, float(gold["src_z"]))
    O = H.Oracle(eq, met=None)
    O.load_arrays(z, T, u, v, rho)
    cfg = H.make_cfg(eq, bounces=2, calc_amp=True, src=src, range_limit=LONG_RANGE)
    so, ro, _, _ = O.fan(cfg, th, ph)
    _, rp, _, _ = O.fan(cfg, th * (1.0 + 1e-12), ph)
    assert np.array_equal(rp[..., :3], ro[..., :3])
    E = JD.ESIZE[eq][1]
    fe = field_errors(rp, ro, E, JD.HIDX[eq])
    sens = max(float(np.nanmax(fe[f])) for f in fe)
    assert 4.0 * sens <= 1e-6, sens
    assert (ro[..., H.REC["VALID"]] > 0).sum() >= 10 and (ro[..., H.REC["BROKE"]] > 0).sum() > 0
    x = z + (6370.0 if eq == H.EQ_GLOBAL else 0.0)
    taper = (2.0 / (1.0 + np.exp(-(z - 0.0) / 0.2)) - 1.0) / 1000.0
    out = []
    for env in ({}, {"GEOAC_NO_PAIR": "1"}, {"GEOAC_NO_PAIR": "1", "GEOAC_COMPACT": "0"}, {"GEOAC_PAIR_FRAC": "1.0"}):
        with G.options(**env):
            ctx = G.FanContext(eq, device=0)
            ctx.upload_atmo_1d(x, T, u * taper, v * taper, rho)
            ctx.set_params(bounces=2, calc_amp=1, mode=0, src=src, range_limit=LONG_RANGE)
            out.append(ctx.run(th, ph))
            ctx.close()
    rec, steps = out[0]
    fe = field_errors(rec, ro, E, JD.HIDX[eq])
    print(f"jet on 1800 nodes, {H.EQ_NAMES[eq]}: worst error per field: " + ", ".join(f"{f} {np.nanmax(fe[f]):.2e}" for f in sorted(fe)) + f"; oracle sensitivity {sens:.1e}")
    assert steps == so
    compare_records(rec, ro, E=E, hidx=JD.HIDX[eq])
    for r, s in out[1:]:
        assert s == steps and np.array_equal(r.view(np.uint64), rec.view(np.uint64))


@pytest.mark.parametrize("eq", SETS)
def test_jet_table_and_exact_post_pass_agree(G, gold, eq):
    """fan b through the table post-pass and through the exact one (ABS_TABLE=0), as test_gpu_probes.py::test_table_and_exact_post_pass_agree: travel times to
    1e-14, attenuations to 1e-10 relative, every other field identical"""
    r1, s1, i1 = _run(G, gold, eq, "b_amp1", {"ABS_TABLE": "1"})
    r0, s0, i0 = _run(G, gold, eq, "b_amp1", {"ABS_TABLE": "0"})
    assert s1 == s0 and i1["entries"] > 0 and i0["entries"] == 0
    valid = r0[:, :, G.REC["VALID"]] == 1.0
    tt1, tt0 = r1[:, :, G.REC["TTIME"]][valid], r0[:, :, G.REC["TTIME"]][valid]
    at1, at0 = r1[:, :, G.REC["ATTEN"]][valid], r0[:, :, G.REC["ATTEN"]][valid]
    print("jet", H.EQ_NAMES[eq], "arrivals", valid.sum(), "flagged", i1["flagged"], "fix-up segments", i1["fixup_segments"], "TTIME max rel", np.abs(tt1 / tt0 - 1).max(),
          "ATTEN max rel", np.abs(at1 / at0 - 1).max())
    assert valid.sum() >= 60
    assert np.abs(tt1 / tt0 - 1).max() <= 1e-14
    assert np.abs(at1 / at0 - 1).max() <= 1e-10
    for k in [k for k in G.REC if k not in ("TTIME", "ATTEN")]:
        np.testing.assert_array_equal(r1[:, :, G.REC[k]], r0[:, :, G.REC[k]])


@pytest.mark.parametrize("eq", SETS)
def test_jet_beside_toyatmo_in_an_ensemble(G, gold, eq, tmp_path):
    """K = 2: ToyAtmo's winds and the jet's on the jet's nodes (an ensemble's members share their nodes), both files in `zuvwTdp` order through
    load_met_ensemble; each member's records are the bits of a context loaded with that file alone - fan b, source inside the jet's wind"""
    th, ph, _ = JD.fan(gold, "b_amp1")
    paths = [JD.write_toy_on_jet_nodes(str(tmp_path / "toy.met")), JD.JET]
    p = _params(gold, eq, "b_amp1")
    ctx = G.FanContext(eq, device=0)
    ctx.load_met_ensemble(paths, fmt=JD.FMT)
    ctx.set_params(**p)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (2, len(th), 3, 32)
    total = 0
    for m, path in enumerate(paths):
        c1 = G.FanContext(eq, device=0)
        c1.load_met(path, fmt=JD.FMT)
        c1.set_params(**p)
        want, st = c1.run(th, ph)
        c1.close()
        assert np.array_equal(rec[m].view(np.uint64), want.view(np.uint64)), f"member {m} differs from its single-profile run"
        total += st
    assert steps == total
    assert int(rec[1][:, :, H.REC["STEPS"]].sum()) == JD.table(gold, eq, "b_amp1")[1]
    assert not np.array_equal(rec[0], rec[1])


@pytest.mark.parametrize("eq", SETS)
def test_jet_ground_and_elevated_source_in_one_launch(G, gold, eq):
    """set_sources {ground, 12 km}, the angles of fan b: each source's records are the bits of its single-source run (one windless, one inside the wind)"""
    th, ph, z = JD.fan(gold, "b_amp1")
    srcs = np.array([JD.src(eq, 0.0), JD.src(eq, z)])
    p = _params(gold, eq, "b_amp1")
    ctx = _ctx(G, eq, **p)
    ctx.set_sources(srcs)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (2, len(th), 3, 32)
    total = 0
    for s, src in enumerate(srcs):
        c1 = _ctx(G, eq, **dict(p, src=tuple(src)))
        want, st = c1.run(th, ph)
        c1.close()
        assert np.array_equal(rec[s].view(np.uint64), want.view(np.uint64)), f"source {s} differs from its single-source run"
        total += st
    assert steps == total
    assert int(rec[1][:, :, H.REC["STEPS"]].sum()) == JD.table(gold, eq, "b_amp1")[1]


@pytest.mark.parametrize("tag", ["a_amp1", "b_amp1"])
def test_hamiltonian_residuals_of_the_jet_fans(G, gold, tag):
    """GeoAc_EvalHamiltonian / GeoAc_EvalHamiltonian_Deriv at every arrival of the device's records, Global set; the bounds the oracle meets on these fans in
    the CPU suite (test_oracle_known_answers.py::test_hamiltonian_residuals_at_arrivals_jet: 3.9e-6 / 5.3e-6 and 1.7e-2 / 1.0e-2)"""
    th, ph, z = JD.fan(gold, tag)
    ctx = _ctx(G, H.EQ_GLOBAL, **_params(gold, H.EQ_GLOBAL, tag))
    rec, _ = ctx.run(th, ph)
    c_src = ctx.probe_atmo_1d(np.array([K.R_EARTH + z]))[0][0, 0]
    n, h, hd = K.hamiltonian_residuals(H.EQ_GLOBAL, rec, lambda x: ctx.probe_atmo_1d(x)[0], c_src)
    n0, h0, hd0 = K.hamiltonian_residuals(H.EQ_GLOBAL, rec[:, :1], lambda x: ctx.probe_atmo_1d(x)[0], c_src)
    ctx.close()
    print(f"jet {tag}: {n} arrivals: |H| <= {h:.2e}; first legs ({n0}): |H_deriv| / |mu| <= {hd0:.2e}; all legs: {hd:.2e}")
    assert n >= 60 and n0 >= 20 and h < 1e-4 and hd0 < 2e-2
