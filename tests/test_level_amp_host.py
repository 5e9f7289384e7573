"""Level amplitudes without a GPU (include/geoac_level_amp.h): geoac_level_amp_check on the host, the Python names against the restatement
(tests/level_amp_reference.py), the restatement's own pieces on synthetic crossing tables whose crossing point is an affine function of the launch
angles, and the restatement on the plain-C oracle's paths in the closed-form medium of tests/level_amp_cases.py."""
import ctypes
import sys

import numpy as np
import pytest

import harness as H
import level_amp_cases as LC
import level_amp_reference as LA
import levels_reference as LV
import raised_ground as RG
from levels_reference import LVL, LVL_STRIDE

A_ = LA.LAMP
EQ_3D, EQ_GLOBAL = LA.EQ_3D, LA.EQ_GLOBAL


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def test_level_amp_check_accepts_and_refuses(G):
    lib = G.load_library()
    lib.geoac_level_amp_check.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_char_p)]
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP):
        for h in (0.02, 1e-9, 1.0):
            G.level_amp_check(eq, h)
            fault = ctypes.c_char_p(b"x")
            assert lib.geoac_level_amp_check(eq, h, ctypes.byref(fault)) == 0 and fault.value is None
    for h in (0.0, -0.02, float(np.nextafter(1.0, 2.0)), float("nan"), float("inf"), -float("inf")):
        with pytest.raises(G.GeoAcError, match="invalid.*probe_deg must be finite, > 0 and <= 1"):
            G.level_amp_check(G.EQ_GLOBAL, h)
        assert lib.geoac_level_amp_check(G.EQ_3D_RNGDEP, h, None) == -1                # (a NULL fault pointer is allowed)
    with pytest.raises(G.GeoAcError, match="not implemented.*not available for GEOAC_EQ_GLOBAL_RNGDEP: .*not converged in probe_deg behind a turning point"):
        G.level_amp_check(G.EQ_GLOBAL_RNGDEP, 0.02)
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set: it has no level crossings"):
        G.level_amp_check(G.EQ_2D, 0.02)
    fault = ctypes.c_char_p()
    assert lib.geoac_level_amp_check(G.EQ_2D, float("nan"), ctypes.byref(fault)) == -4          # (the set is refused before the step is looked at)
    for eq in (7, -1):
        assert lib.geoac_level_amp_check(eq, 0.02, ctypes.byref(fault)) == -1 and fault.value == b"unknown equation set"


def test_python_names_mirror_the_restatement(G):
    assert G.LAMP == LA.LAMP and G.LAMP_STRIDE == LA.LAMP_STRIDE
    assert G.LAMP_STATUS == dict(OK=LA.OK, ABSENT=LA.ABSENT, NO_PROBE=LA.NO_PROBE, SINGULAR=LA.SINGULAR, SKIPPED=LA.SKIPPED)


def test_header_symbols_exist_in_the_built_library(G):
    lib = G.load_library()
    for name in ("geoac_level_amp_check", "geoac_fan_level_amp_at", "geoac_fan_level_amp", "geoac_fan_level_amp_shape", "geoac_fan_level_amp_fetch",
                 "geoac_fan_level_amp_dev", "geoac_fan_level_amp_timing"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    for name in ("level_amp_at", "level_amp", "level_amp_timing"):
        assert hasattr(G.FanContext, name)


# ---- the restatement on synthetic crossing tables ----
CAP = 4


def _affine_tables(eq, A, c_at0, th, ph, h, n_up=2, absent=(), lost_probe=(), flat=()):
    """crossing tables [1][3 n][2][CAP][12] of a made-up medium, level 1 only: every ray passes the level n_up times upward on leg 0 (the passages 0.5 apart
    along axis 0) and once downward, at c = c_at0 + A (theta, phi); count runs to n_up + 1 even past CAP.  Rays `absent` pass nothing, rays `lost_probe` lose
    their theta probe, rays `flat` cross at a point that does not depend on the angles."""
    n = len(th)
    T, Pp = LA.fan_angles(th, ph, h)
    count, lrec = np.zeros((1, 3 * n, 2), dtype=np.int32), np.zeros((1, 3 * n, 2, CAP, LVL_STRIDE))
    for ray in range(3 * n):
        i, j = ray % n, ray // n
        if i in absent or (i in lost_probe and j == 1):
            continue
        t, p = (th[i], ph[i]) if i in flat else (T[ray], Pp[ray])
        c0 = c_at0[0] + A[0][0] * t + A[0][1] * p
        c1 = c_at0[1] + A[1][0] * t + A[1][1] * p
        count[0, ray, 1] = n_up + 1
        for k in range(min(n_up + 1, CAP)):
            rec = lrec[0, ray, 1, k]
            up = k < n_up
            rec[LVL["DIR"]] = 1.0 if up else -1.0
            rec[LVL["TTIME"]], rec[LVL["ATTEN"]] = 100.0 + t + k, 0.5 * p + k
            shift = 0.5 * k
            if LA.spherical(eq):
                rec[LVL["P0"]], rec[LVL["P0"] + 1], rec[LVL["P0"] + 2] = 6400.0, np.radians(c0 + shift), np.radians(c1)
            else:
                rec[LVL["P0"]], rec[LVL["P0"] + 1], rec[LVL["P0"] + 2] = c0 + shift, c1, 30.0
            rec[LVL["P0"] + 3], rec[LVL["P0"] + 4], rec[LVL["P0"] + 5] = (0.7, -0.1, 0.2) if up else (-0.7, -0.1, -0.2)
    return count, lrec


def _still_medium(hc, a, b):
    """sound speed falling with the height coordinate, a light wind, an exponential density"""
    z = np.where(hc > 1000.0, hc - 6370.0, hc)
    return 0.34 - 0.001 * z, 0.001 + 0.0 * z, -0.0005 + 0.0 * z, 1.2e-3 * np.exp(-z / 8.0)


@pytest.mark.parametrize("eq", [EQ_3D, LA.EQ_3D_RNGDEP, EQ_GLOBAL, LA.EQ_GLOBAL_RNGDEP])
def test_det_is_the_affine_maps_determinant(eq):
    sph = LA.spherical(eq)
    A = [[0.05, -0.01], [0.004, 0.1]] if sph else [[3.0, -0.5], [0.4, 2.0]]
    c00 = [20.0, 178.0] if sph else [10.0, -20.0]                                    # spherical: longitudes 178 + 0.1 phi pass +180 for phi > 20: WRAP
    th, ph, h = np.array([20.3, 31.7, 12.2]), np.array([25.1, 19.95, 30.0]), 0.02
    count, lrec = _affine_tables(eq, A, c00, th, ph, h)
    src3 = [[0.0, 20.0, 170.0]] if sph else [[1.0, 2.0, 0.0]]
    kw = dict(z_km=[20.0, 30.0], medium=_still_medium, src3=src3)
    rows = LA.rows_at(eq, count, lrec, th, ph, 1, 0, 1, 0, h, **kw)[0]
    want = A[0][0] * A[1][1] - A[0][1] * A[1][0]
    assert (rows[:, A_["STATUS"]] == LA.OK).all() and np.abs(rows[:, A_["DET"]] / want - 1.0).max() < 1e-9, rows[:, A_["DET"]]
    assert np.array_equal(rows[:, A_["THETA"]], th) and np.array_equal(rows[:, A_["PHI"]], ph) and np.array_equal(rows[:, A_["INDEX"]], np.arange(3.0))
    assert np.array_equal(rows[:, A_["TTIME"]], 100.0 + th) and np.array_equal(rows[:, A_["ATTEN"]], 0.5 * ph)          # the base record's, bit for bit
    assert (np.abs(rows[:, A_["TZ"]]) < 1.0).all() and (rows[:, A_["TZ"]] > 0.2).all() and (rows[:, A_["D"]] > 0).all() and (rows[:, A_["AMP"]] > 0).all()
    # D is |TZ DET| times the set's metric factor, AMP falls as its root
    if sph:
        lat = c00[0] + A[0][0] * th + A[0][1] * ph
        assert np.allclose(rows[:, A_["D"]], 6400.0 ** 2 * np.cos(np.radians(lat)) * np.abs(rows[:, A_["TZ"]] * rows[:, A_["DET"]]), rtol=1e-13)
    else:
        assert np.allclose(rows[:, A_["D"]], np.abs(rows[:, A_["TZ"]] * rows[:, A_["DET"]]) * (180.0 / np.pi) ** 2, rtol=1e-14)
    # a second ordinal: the passage 0.5 farther along axis 0, one second later, the same determinant
    second = LA.rows_at(eq, count, lrec, th, ph, 1, 0, 1, 1, h, **kw)[0]
    assert (second[:, A_["STATUS"]] == LA.OK).all() and (second[:, A_["ORD"]] == 1).all() and np.array_equal(second[:, A_["TTIME"]], 101.0 + th)
    assert np.abs(second[:, A_["DET"]] / want - 1.0).max() < 1e-9
    down = LA.rows_at(eq, count, lrec, th, ph, 1, 0, -1, 0, h, **kw)[0]
    assert (down[:, A_["STATUS"]] == LA.OK).all() and (down[:, A_["DIR"]] == -1.0).all() and (down[:, A_["TZ"]] < -0.2).all() and np.array_equal(down[:, A_["TTIME"]], 102.0 + th)
    # the other level holds nothing
    none = LA.rows_at(eq, count, lrec, th, ph, 0, 0, 1, 0, h, **kw)[0]
    assert (none[:, A_["STATUS"]] == LA.ABSENT).all() and (none[:, A_["DET"]:] == 0).all()


def test_a_count_past_the_crossing_cap():
    """five upward passages and a downward one under a cap of four: the count says six, four records exist - ordinal 3 is served, ordinal 4 and the downward
    passage are absent"""
    A, c00 = [[3.0, -0.5], [0.4, 2.0]], [10.0, -20.0]
    th, ph, h = np.array([20.3]), np.array([-80.4]), 0.05
    count, lrec = _affine_tables(EQ_3D, A, c00, th, ph, h, n_up=5)
    assert count[0, 0, 1] == 6 and lrec.shape[3] == CAP
    kw = dict(z_km=[20.0, 30.0], medium=_still_medium, src3=[[0.0, 0.0, 0.0]])
    assert LA.rows_at(EQ_3D, count, lrec, th, ph, 1, 0, 1, 3, h, **kw)[0, 0, A_["STATUS"]] == LA.OK
    assert LA.rows_at(EQ_3D, count, lrec, th, ph, 1, 0, 1, 4, h, **kw)[0, 0, A_["STATUS"]] == LA.ABSENT
    assert LA.rows_at(EQ_3D, count, lrec, th, ph, 1, 0, -1, 0, h, **kw)[0, 0, A_["STATUS"]] == LA.ABSENT


def test_every_status_has_its_row():
    A, c00 = [[3.0, -0.5], [0.4, 2.0]], [10.0, -20.0]
    th, ph, h = np.array([20.0, 21.0, 22.0, 23.0, 24.0]), np.array([-80.0, -81.0, -82.0, -83.0, -84.0]), 0.02
    count, lrec = _affine_tables(EQ_3D, A, c00, th, ph, h, absent=(1,), lost_probe=(2,), flat=(3,))
    n = len(th)
    rows = LA.reference_rows(EQ_3D, count, lrec, th, ph, h, np.zeros(n, dtype=int), np.arange(n), np.ones(n, dtype=int), np.zeros(n, dtype=int), np.ones(n), np.zeros(n, dtype=int),
                             [20.0, 30.0], _still_medium, [[0.0, 0.0, 0.0]], refine_status=[LA.CONVERGED] * 4 + [LA.CONVERGED + 1])
    assert rows[:, A_["STATUS"]].astype(int).tolist() == [LA.OK, LA.ABSENT, LA.NO_PROBE, LA.SINGULAR, LA.SKIPPED]
    assert (rows[1:, A_["DET"]:] == 0).all() and (rows[0, A_["DET"]:] != 0).all() and np.isfinite(rows).all()
    assert np.array_equal(rows[:, A_["THETA"]], th) and np.array_equal(rows[:, A_["PHI"]], ph)          # every row keeps its head


# ---- the restatement on the oracle's paths: the closed form ----
@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_closed_form_on_the_oracle(eq, tmp_path):
    O = RG.oracle(eq, tmp_path)
    cfg = H.make_cfg(eq, bounces=LC.PARAMS["bounces"], calc_amp=True, src=RG.SRC[eq], z_grnd=RG.Z_GRND, vert_limit=LC.PARAMS["vert_limit"])
    th, ph, lv = LC.rays()
    T, P = LA.fan_angles(th, ph, LC.H_DEG)
    count, lrec = LV.restate_fan(eq, [O.trace_path(cfg, t, p) for t, p in zip(T, P)], LC.LEVELS, 8)
    rows = LA.rows_at(eq, count[None], lrec[None], th, ph, lv, LC.BRANCH["leg"], LC.BRANCH["dir"], LC.BRANCH["ord"], LC.H_DEG, LC.LEVELS, LA.medium_of_oracle(O), [RG.SRC[eq]],
                      z_grnd=RG.Z_GRND)[0]
    out = LC.check_closed_form(rows)
    print(f"{H.EQ_NAMES[eq]} closed form on the oracle: {out}")


# ---- the restatement on the oracle's paths: the fixture's tube ----
def _fixture_oracle(name, eq, g, tmp_path):
    if eq == H.EQ_3D_RNGDEP:
        import rngdep_data as RD
        O = H.Oracle(eq, met=None)
        O.load_grid(*RD.write_grid_ragged(str(tmp_path), False, short_paths=False), z_grnd=RD.ragged_load_z_grnd(False))
    else:
        O = H.Oracle(eq)
    src = tuple(g[f"{name}_src"])
    return O, src, H.make_cfg(eq, bounces=1, calc_amp=True, src=src, z_grnd=float(g[f"{name}_z_grnd"]))


@pytest.mark.parametrize("name,eq", [("3d", H.EQ_3D), ("global", H.EQ_GLOBAL), ("3drd", H.EQ_3D_RNGDEP)])
def test_restatement_on_the_oracle_equals_the_fixture(name, eq, tmp_path):
    """tests/golden/level_amp.npz holds the tube of the compiled reference's rays, made with this restatement: the plain-C oracle's paths are the reference's
    bit for bit, so the same rows come out again - to 1e-12, the fixture's medium being the reference's probes and this one the oracle's"""
    g = np.load(LA.FIXTURE)
    O, src, cfg = _fixture_oracle(name, eq, g, tmp_path)
    th, ph, levels = g[f"{name}_theta"], g[f"{name}_phi"], g[f"{name}_levels"]
    ray = g[f"{name}_ray"]
    for h, key in zip(g["steps"], ("tube02", "tube04")):
        T, P = LA.fan_angles(th, ph, float(h))
        count, lrec = LV.restate_fan(eq, [O.trace_path(cfg, t, p) for t, p in zip(T, P)], levels, 16)
        rows = LA.reference_rows(eq, count[None], lrec[None], th, ph, float(h), np.zeros(len(ray), dtype=int), ray, g[f"{name}_level"], g[f"{name}_leg"], g[f"{name}_dir"],
                                 g[f"{name}_ord"], levels, LA.medium_of_oracle(O), [src], z_grnd=float(g[f"{name}_z_grnd"]))
        assert (rows[:, A_["STATUS"]] == LA.OK).all()
        err = np.abs(rows[:, A_["DET"]:A_["AMP"] + 1] / g[f"{name}_{key}"] - 1.0).max()
        print(f"{name} h = {h:g}: restatement on the oracle against the fixture's tube: {err:.3e}")
        assert err <= 1e-12
    # the fixture's own conditions
    jac = g[f"{name}_amp_jac_cos"] if f"{name}_amp_jac_cos" in g.files else g[f"{name}_amp_jac"]
    assert (np.abs(g[f"{name}_tube02"][:, 3] / jac - 1.0) <= float(g["cap"])).all() and float(g[f"{name}_arrival_amp_err"]) <= 1e-9
    assert len(set(zip(g[f"{name}_leg"].tolist(), g[f"{name}_dir"].tolist()))) == 4          # (leg 0 | 1) x (up | down)


@pytest.mark.parametrize("name,eq", [("3d", H.EQ_3D), ("global", H.EQ_GLOBAL), ("3drd", H.EQ_3D_RNGDEP)])
def test_the_amplitude_factor_equals_the_oracles_own_at_ground_arrivals(name, eq, tmp_path):
    """what the gap to the Jacobian amplitude does not check - the factor rho nu c^3 Q cos(theta) / (rho_s nu_s c_s^3 G) with its winds and quirk Q4, which the
    fixture's amp_jac, the restatement and the kernel share: the restatement's num / den with GeoAc_Jacobian's own D at the last row of every landed leg is
    GEOAC_REC_AMP of the oracle's fan (the reference's GeoAc_Amplitude, bit-equal) to 1e-9"""
    sys.path.insert(0, H.GOLDEN_DIR)
    import make_level_amp as MK
    g = np.load(LA.FIXTURE)
    O, src, cfg = _fixture_oracle(name, eq, g, tmp_path)
    th, ph = g[f"{name}_theta"], g[f"{name}_phi"]
    paths = [O.trace_path(cfg, t, p) for t, p in zip(th, ph)]
    err, n = MK.arrival_amp_check(eq, O, cfg, th, ph, paths, LA.medium_of_oracle(O), src, float(g[f"{name}_z_grnd"]))
    print(f"{name}: numpy amplitude against the oracle's AMP at {n} ground arrivals: {err:.2e}")
    assert n >= 2 and err <= 1e-9
