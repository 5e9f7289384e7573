"""Level loudness maps without a GPU (include/geoac_lampmap.h): geoac_lampmap_check on the host - every refusal with its code and a named fault -,
the symbols of the header in the built library, the EXP series against numpy.exp, the numpy restatement (tests/lampmap_reference.py) on synthetic
straight-ray crossing tables against the closed form and its derived bound (tests/lampmap_cases.py), and the restatement on the CPU oracle's crossing
tables against the compiled reference's Jacobian amplitude (tests/golden/level_amp.npz): the measurement behind the caps of tests/test_gpu_lampmap.py."""
import ctypes

import numpy as np
import pytest

import geoac_amd as G
import harness as H
import lampmap_cases as LC
import lampmap_reference as LM
import level_amp_reference as LA
import levels_reference as LV
import raised_ground as RG
import test_level_amp_host as TLA
import test_ltubemap_host as TLT

INF, NAN = float("inf"), float("nan")
E_INVALID, E_UNSUPPORTED = -1, -4
GOOD, N_RAYS, N_LEVELS = TLT.GOOD, TLT.N_RAYS, TLT.N_LEVELS


@pytest.fixture(scope="module")
def lib():
    lib = G.load_library()
    lib.geoac_lampmap_fault.restype = ctypes.c_char_p
    return lib


def _check(lib, eq, n_rays=N_RAYS, n_levels=N_LEVELS, **kw):
    cells, n_sel = ctypes.c_int64(-7), ctypes.c_int(-7)
    spec = G.lampmap_spec(**kw)
    rc = lib.geoac_lampmap_check(eq, ctypes.byref(spec), n_rays, n_levels, ctypes.byref(cells), ctypes.byref(n_sel))
    return rc, cells.value, n_sel.value, lib.geoac_lampmap_fault(eq, ctypes.byref(spec), n_rays, n_levels)


# ---------------------------------------------------------------- the host-only check
def test_header_symbols_and_python_mirror(lib):
    for name in ("geoac_lampmap_check", "geoac_lampmap_fault", "geoac_fan_level_ampmap", "geoac_fan_level_ampmap_shape", "geoac_fan_level_ampmap_fetch",
                 "geoac_fan_level_ampmap_dev", "geoac_fan_level_ampmap_fetch_detect", "geoac_fan_level_ampmap_timing", "geoac_fan_level_ampmap_stats"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    for name in ("level_ampmap", "level_ampmap_timing", "level_ampmap_stats"):
        assert hasattr(G.FanContext, name)
    assert ctypes.sizeof(G.LAmpMapSpec) == ctypes.sizeof(G.LTubeSpec) + 16 == 104          # the fields of geoac_ltube_spec, then two doubles
    assert [f[0] for f in G.LAmpMapSpec._fields_][:-2] == [f[0] for f in G.LTubeSpec._fields_]
    assert G.LAMPMAP == dict(COUNT=0, WEAK=1, AMP_MAX=2, RAMP_MAX=3, LOUDEST=4)
    kw = dict(origin=(1.0, 2.0), step=(0.5, 0.25), n=(3, 4), n_theta=9, n_phi=7, edge_max=40.0, level_mask=0b110, wrap_lon=True, phi_periodic=True, leg_min=1,
              leg_max=3, ord_max=2, dir_mask=2, det_floor=0.25, detect_amp=1e-4)
    sp, ref = G.lampmap_spec(**kw), LM.spec(**kw)
    got = {k: (tuple(getattr(sp, k)) if k in ("origin", "step", "n") else bool(getattr(sp, k)) if k in ("wrap_lon", "phi_periodic") else getattr(sp, k)) for k in kw}
    assert got == ref
    d = G.lampmap_spec(**GOOD)
    assert d.det_floor == 0.0 and np.isnan(d.detect_amp) and np.isnan(LM.spec(**GOOD)["detect_amp"])


def test_lampmap_check_accepts_good_specs(lib):
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP):
        assert _check(lib, eq, **GOOD) == (0, 3200, 2, None)
        assert _check(lib, eq, det_floor=0.0, detect_amp=NAN, **GOOD) == (0, 3200, 2, None)
        assert _check(lib, eq, det_floor=1e300, detect_amp=5e-324, phi_periodic=True, ord_max=64, dir_mask=1, **dict(GOOD, level_mask=0b111)) == (0, 3200, 3, None)
    assert G.lampmap_check(G.EQ_GLOBAL, G.lampmap_spec(**GOOD), N_RAYS, N_LEVELS) == (3200, 2)
    assert lib.geoac_lampmap_check(G.EQ_GLOBAL, ctypes.byref(G.lampmap_spec(**GOOD)), N_RAYS, N_LEVELS, None, None) == 0          # either pointer may be NULL


# every refusal of geoac_ltube_check, on a set this header serves (the spherical grid set has a refusal of its own, below)
SHARED_BAD = [(what, G.EQ_GLOBAL if eq == G.EQ_GLOBAL_RNGDEP else eq, kw, nr, nl, word) for what, eq, kw, nr, nl, word in TLT.BAD]
OWN_BAD = [
    ("det_floor negative", G.EQ_GLOBAL, dict(GOOD, det_floor=-1e-300), N_RAYS, N_LEVELS, "det_floor must be finite and >= 0"),
    ("det_floor nan", G.EQ_3D, dict(GOOD, det_floor=NAN), N_RAYS, N_LEVELS, "det_floor must be finite and >= 0"),
    ("det_floor inf", G.EQ_3D_RNGDEP, dict(GOOD, det_floor=INF), N_RAYS, N_LEVELS, "det_floor must be finite and >= 0"),
    ("detect_amp zero", G.EQ_GLOBAL, dict(GOOD, detect_amp=0.0), N_RAYS, N_LEVELS, "detect_amp must be NaN .* or finite and > 0"),
    ("detect_amp negative", G.EQ_GLOBAL, dict(GOOD, detect_amp=-1.0), N_RAYS, N_LEVELS, "detect_amp must be NaN .* or finite and > 0"),
    ("detect_amp inf", G.EQ_3D, dict(GOOD, detect_amp=INF), N_RAYS, N_LEVELS, "detect_amp must be NaN .* or finite and > 0"),
]
BAD = SHARED_BAD + OWN_BAD


@pytest.mark.parametrize("what,eq,kw,n_rays,n_levels,word", BAD, ids=[b[0] for b in BAD])
def test_lampmap_check_refuses_each_bad_field_and_names_it(lib, what, eq, kw, n_rays, n_levels, word):
    rc, cells, n_sel, fault = _check(lib, eq, n_rays, n_levels, **kw)
    assert rc == E_INVALID and cells == -7 and n_sel == -7 and fault is not None, what
    with pytest.raises(G.GeoAcError, match="invalid.*" + word):
        G.lampmap_check(eq, G.lampmap_spec(**kw), n_rays, n_levels)
    if (what, eq, kw, n_rays, n_levels, word) in SHARED_BAD and eq != 9:
        # the shared fields earn the verdict of geoac_ltube_check, word for word
        lib.geoac_ltube_fault.restype = ctypes.c_char_p
        assert fault == lib.geoac_ltube_fault(eq, ctypes.byref(G.ltube_spec(**kw)), n_rays, n_levels)


def test_lampmap_check_unsupported_sets_and_null(lib):
    rc, cells, n_sel, fault = _check(lib, G.EQ_2D, **GOOD)
    assert rc == E_UNSUPPORTED and cells == -7 and b"2-D set" in fault
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.lampmap_check(G.EQ_2D, G.lampmap_spec(**GOOD), N_RAYS, N_LEVELS)
    rc, cells, n_sel, fault = _check(lib, G.EQ_GLOBAL_RNGDEP, **GOOD)
    assert rc == E_UNSUPPORTED and cells == -7 and b"GEOAC_EQ_GLOBAL_RNGDEP" in fault and b"no better conditioned" in fault
    with pytest.raises(G.GeoAcError, match="not implemented.*not available for GEOAC_EQ_GLOBAL_RNGDEP"):
        G.lampmap_check(G.EQ_GLOBAL_RNGDEP, G.lampmap_spec(**GOOD), N_RAYS, N_LEVELS)
    assert lib.geoac_lampmap_check(G.EQ_GLOBAL_RNGDEP, ctypes.byref(G.lampmap_spec(**dict(GOOD, det_floor=NAN))), N_RAYS, N_LEVELS, None, None) == E_UNSUPPORTED   # (the set first)
    assert lib.geoac_lampmap_check(G.EQ_GLOBAL, None, N_RAYS, N_LEVELS, None, None) == E_INVALID
    assert lib.geoac_lampmap_fault(G.EQ_GLOBAL, None, N_RAYS, N_LEVELS) == b"spec is NULL"
    word = (ctypes.c_uint64 * 4)()
    spec = G.lampmap_spec(**GOOD)
    assert lib.geoac_fan_level_ampmap(None, ctypes.byref(spec)) < 0                                          # (no context: never a result)
    assert lib.geoac_fan_level_ampmap_fetch(None, 0, word) < 0 and lib.geoac_fan_level_ampmap_fetch_detect(None, word) < 0
    assert lib.geoac_fan_level_ampmap_shape(None, None, None, None, None, None) < 0 and lib.geoac_fan_level_ampmap_dev(None, 0, None, None) < 0
    assert lib.geoac_fan_level_ampmap_timing(None, None) < 0 and lib.geoac_fan_level_ampmap_stats(None, word) < 0


# ---------------------------------------------------------------- EXP
EXP_ULP = 2.0          # measured here against numpy.exp: 1 ulp at most over the 4.5 million arguments below; numpy's own exp is faithful, not correctly
#                        rounded, and differs by an ulp between its vector paths, so the pin is the measured ulp plus that one


def test_exp_series_against_numpy_exp():
    rng = np.random.default_rng(1)
    x = np.concatenate([np.linspace(-700.0, 0.0, 2000001), -rng.uniform(0.0, 700.0, 2000000), -np.exp(rng.uniform(-40.0, np.log(700.0), 500000))])
    got, want = LM.EXP(x), np.exp(x)
    ulp = np.abs(got - want) / np.spacing(want)
    print(f"EXP against numpy.exp on [-700, 0]: worst {ulp.max():.2f} ulp at {x[ulp.argmax()]!r}, mean {ulp.mean():.3f} ulp")
    assert ulp.max() <= EXP_ULP
    assert (got > 2.2250738585072014e-308).all()                                     # no subnormal result above the cut-off
    assert LM.EXP(-700.0) == got[0] > 0.0 and LM.EXP(np.nextafter(-700.0, -INF)) == 0.0 and LM.EXP(-1e308) == 0.0 and LM.EXP(-INF) == 0.0
    assert LM.EXP(0.0) == 1.0 and LM.EXP(-0.0) == 1.0 and np.isnan(LM.EXP(NAN)) and LM.EXP(700.5) == INF and LM.EXP(INF) == INF
    assert abs(LM.EXP(1.0) / np.e - 1.0) < 4e-16 and LM.EXP(-np.log(2.0)) == 0.5
    assert (np.diff(LM.EXP(np.linspace(-30.0, 0.0, 100001))) >= 0.0).all()           # monotone at the resolution of a map's attenuations


# ---------------------------------------------------------------- the closed form on synthetic straight-ray tables
def _synthetic_map(eq, halvings, atten_per_km=0.0, **kw):
    th, ph, nt, nph = LC.rg_lattice(halvings)
    count, lrec = LC.rg_tables(eq, th, ph, atten_per_km)
    sp = LC.rg_spec(eq, nt, nph, **kw)
    G.lampmap_check(eq, G.lampmap_spec(**sp), th.size, len(RG.LEVELS))
    layers, hits = LM.reference_level_ampmap(eq, count, lrec, th, ph, 1, sp, RG.LEVELS, [LC.rg_medium], [RG.SRC[eq]], hits_too=True, z_grnd=RG.Z_GRND)
    return layers, hits, sp, th, ph, nt


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form_on_straight_ray_tables_and_the_halved_step(eq):
    """DET of a lattice triangle is known without any ray, the exact amplitude at a centre is exp(dz / 2H) / (4 pi L): the restatement stays inside the
    bound derived in tests/lampmap_cases.py, and its error shrinks when the lattice step is halved"""
    worst, median = [], []
    for halvings in (0, 1):
        layers, hits, sp, th, ph, nt = _synthetic_map(eq, halvings)
        out = LC.check_closed_form(eq, layers, sp, th, ph, nt)
        print(f"{H.EQ_NAMES[eq]}, lattice step {5.0 / 2 ** halvings:g} x {15.0 / 2 ** halvings:g} deg, restatement on straight-ray tables: " + LC.cf_figures(out))
        assert int(layers["weak"].sum()) == 0 and np.array_equal(SRbits(layers["amp_max"]), SRbits(layers["ramp_max"]))          # ATTEN = 0: EXP(-0) = 1
        worst.append([v[1] for v in out.values()])
        median.append([v[2] for v in out.values()])
    assert (np.array(worst[1]) < 0.6 * np.array(worst[0])).all() and (np.array(median[1]) < 0.6 * np.array(median[0])).all(), (worst, median)


def SRbits(a):
    return LM.SR.bits(a)


def test_det_of_a_lattice_triangle_and_the_received_amplitude():
    eq = H.EQ_3D
    layers, h, sp, th, ph, nt = _synthetic_map(eq, 0, atten_per_km=0.05, detect_amp=2.5e-3)
    assert h["usable"].all() and len(h["det"]) > 1000
    # DET = |rho_2 - rho_1| rho_k sin(h_phi) / (h_theta h_phi), rho_k the radius the triangle holds twice: corner b for (a, b, c), corner a for (a, c, d)
    n_tri = 2 * (nt - 1) * sp["n_phi"]
    t = h["key"] % n_tri
    i = (t // 2) % (nt - 1)
    dz = RG.Z_SRC - np.asarray(RG.LEVELS)[h["ls"]]
    r1, r2 = dz / np.tan(np.radians(-th[i])), dz / np.tan(np.radians(-th[i + 1]))
    want = np.abs(r2 - r1) * np.where(t % 2 == 0, r2, r1) * np.sin(np.radians(15.0)) / (5.0 * 15.0)
    assert np.abs(np.abs(h["det"]) / want - 1.0).max() < 1e-10
    # RAMP = AMP 10^(-ATTEN / 20), and the layers are the hits' maxima
    assert np.abs(h["ramp"] / (h["amp"] * 10.0 ** (-h["atten"] / 20.0)) - 1.0).max() < 1e-14 and (h["ramp"] < h["amp"]).all()
    word = (h["ls"] * sp["n"][0] * sp["n"][1] + h["cell"])
    for name in ("amp", "ramp"):
        best = np.full(2 * sp["n"][0] * sp["n"][1], -INF)
        np.maximum.at(best, word, h[name])
        assert np.array_equal(best.reshape(layers[name + "_max"].shape[1:]), layers[name + "_max"][0])
    assert layers["detect"].dtype == np.uint32 and np.array_equal(layers["detect"], (layers["ramp_max"][0] >= 2.5e-3).astype(np.uint32))
    assert 0 < int(layers["detect"].sum()) < int((layers["count"] > 0).sum())
    assert ((layers["count"] == 0) == (layers["loudest"] == -1)).all() and (layers["amp_max"][layers["count"] == 0] == -INF).all()


def test_det_floor_moves_hits_to_weak_and_never_back():
    eq = H.EQ_3D_RNGDEP
    base, h, sp, th, ph, nt = _synthetic_map(eq, 0)
    total = base["count"] + base["weak"]
    last = base["count"]
    for floor in (0.0, float(np.median(np.abs(h["det"]))), float(np.abs(h["det"]).max())):
        layers = _synthetic_map(eq, 0, det_floor=floor)[0]
        assert np.array_equal(layers["count"] + layers["weak"], total) and (layers["count"] <= last).all()
        assert int(layers["count"].sum()) == int((np.abs(h["det"]) > floor).sum())
        last = layers["count"]
    assert int(last.sum()) == 0 and (layers["amp_max"] == -INF).all() and (layers["loudest"] == -1).all()
    # with +0.0 only singular hits are WEAK: a triangle folded flat (two rays of a cell made to cross at one point) has DET = 0
    th, ph, nt, nph = LC.rg_lattice(0)
    count, lrec = LC.rg_tables(eq, th, ph)
    lrec[0, nt + 3, :, 0, LM.P0:LM.P0 + 2] = lrec[0, nt + 4, :, 0, LM.P0:LM.P0 + 2]
    _, h2 = LM.reference_level_ampmap(eq, count, lrec, th, ph, 1, sp, RG.LEVELS, [LC.rg_medium], [RG.SRC[eq]], hits_too=True, z_grnd=RG.Z_GRND)
    assert (h2["usable"] | (h2["det"] == 0.0)).all()


# ---------------------------------------------------------------- the reference's Jacobian amplitude: the measurement
@pytest.mark.parametrize("name,eq", LC.FIX_SETS)
def test_gap_to_the_references_jacobian_amplitude(name, eq, tmp_path):
    """the chain without the device code: the oracle's paths (the compiled reference's, bit for bit) through the restated k_levels, then this restatement,
    against the fixture's amp_jac, ttime and atten at two lattice steps.  The figures printed here are LC.GAP_MEASURED; tests/test_gpu_lampmap.py holds the
    device to twice them."""
    g = np.load(LA.FIXTURE)
    O, src, cfg = TLA._fixture_oracle(name, eq, g, tmp_path)
    levels, zg = g[f"{name}_levels"], float(g[f"{name}_z_grnd"])
    media = [LA.medium_of_oracle(O)]

    def tables_of(th, ph):
        count, lrec = LV.restate_fan(eq, [O.trace_path(cfg, t, p) for t, p in zip(th, ph)], levels, 16)
        return count[None], lrec[None], th, ph

    def hit_of(tab, sp):
        count, lrec, th, ph = tab
        G.lampmap_check(eq, G.lampmap_spec(**sp), 4, len(levels))
        layers, h = LM.reference_level_ampmap(eq, count, lrec, th, ph, 2, sp, levels, media, [src], hits_too=True, z_grnd=zg)
        u = np.flatnonzero(h["usable"])
        if len(u) == 0:
            return None
        assert len(u) == 1 and layers["count"][0, 0, 0, 0] == 1 and layers["amp_max"][0, 0, 0, 0] == h["amp"][u[0]]
        return h["amp"][u[0]], h["ttime"][u[0]], h["atten"][u[0]]

    medians = []
    for step in LC.FIX_STEPS:
        gaps = LC.fix_gaps(name, eq, g, step, tables_of, hit_of)
        print("CPU chain, " + LC.fix_summary(name, step, gaps))
        left = np.flatnonzero(np.isnan(gaps[:, 0]))
        assert left.tolist() == LC.GAP_LEFT_OUT[(name, step)] and len(left) * 8 <= len(gaps)
        kept = gaps[~np.isnan(gaps[:, 0])]
        assert (kept.max(axis=0) <= np.array(LC.GAP_MEASURED[(name, step)])).all(), kept.max(axis=0)
        assert (kept.max(axis=0) >= 0.98 * np.array(LC.GAP_MEASURED[(name, step)])).all(), kept.max(axis=0)          # (the table states the measurement, not a roomier figure)
        medians.append(float(np.median(kept[:, 0])))
    assert medians[1] < medians[0], medians
