"""Level refinement without a GPU (include/geoac_level_refine.h): geoac_level_refine_check / _fault on the host, the Python names against the
restatement (tests/level_refine_reference.py), and the restatement's own pieces - the round's fan, the finite-difference Newton step, the step
rule on a synthetic integrator whose crossing point is a known function of the launch angles."""
import ctypes

import numpy as np
import pytest

import level_refine_reference as LR
from levels_reference import LVL, LVL_STRIDE

R = LR.LRF
EQ_3D, EQ_GLOBAL = LR.LS.SR.EQ_3D, LR.LS.SR.EQ_GLOBAL


@pytest.fixture(scope="module")
def G():
    import geoac_amd
    geoac_amd.load_library()
    return geoac_amd


def test_level_refine_check_accepts_and_refuses(G):
    for eq in (G.EQ_3D, G.EQ_GLOBAL, G.EQ_3D_RNGDEP, G.EQ_GLOBAL_RNGDEP):
        G.level_refine_check(eq, G.level_refine_spec())
        G.level_refine_check(eq, G.level_refine_spec(max_iter=1, max_shrink=0, tol=1e-9, step_max_deg=1e-6, probe_deg=1e-9))
        G.level_refine_check(eq, G.level_refine_spec(max_iter=32, max_shrink=16, tol=50.0, step_max_deg=5.0, probe_deg=1.0))
    bad = [(dict(max_iter=0), "max_iter"), (dict(max_iter=33), "max_iter"), (dict(max_shrink=-1), "max_shrink"), (dict(max_shrink=17), "max_shrink"),
           (dict(tol=0.0), "tol"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
           (dict(step_max_deg=0.0), "step_max_deg"), (dict(step_max_deg=-0.2), "step_max_deg"), (dict(step_max_deg=float("nan")), "step_max_deg"),
           (dict(step_max_deg=float("inf")), "step_max_deg"),
           (dict(probe_deg=0.0), "probe_deg"), (dict(probe_deg=-0.02), "probe_deg"), (dict(probe_deg=np.nextafter(1.0, 2.0)), "probe_deg"),
           (dict(probe_deg=float("nan")), "probe_deg"), (dict(probe_deg=float("inf")), "probe_deg")]
    lib = G.load_library()
    lib.geoac_level_refine_fault.restype = ctypes.c_char_p
    for kw, word in bad:
        sp = G.level_refine_spec(**kw)
        with pytest.raises(G.GeoAcError, match="invalid.*" + word):
            G.level_refine_check(G.EQ_GLOBAL, sp)
        assert lib.geoac_level_refine_check(G.EQ_3D_RNGDEP, ctypes.byref(sp)) == -1
        assert word in lib.geoac_level_refine_fault(G.EQ_3D_RNGDEP, ctypes.byref(sp)).decode()
    with pytest.raises(G.GeoAcError, match="not implemented.*2-D set"):
        G.level_refine_check(G.EQ_2D, G.level_refine_spec())
    good = G.level_refine_spec()
    assert lib.geoac_level_refine_check(G.EQ_2D, ctypes.byref(good)) == -4
    assert lib.geoac_level_refine_check(G.EQ_2D, None) == -4                          # (the set is refused before the spec is looked at)
    assert lib.geoac_level_refine_check(G.EQ_GLOBAL, None) == -1 and b"NULL" in lib.geoac_level_refine_fault(G.EQ_GLOBAL, None)
    assert lib.geoac_level_refine_check(7, ctypes.byref(good)) == -1 and lib.geoac_level_refine_check(-1, ctypes.byref(good)) == -1
    assert lib.geoac_level_refine_fault(G.EQ_GLOBAL, ctypes.byref(good)) is None


def test_python_names_mirror_the_restatement(G):
    assert G.LRF == LR.LRF and G.LRF_STRIDE == LR.LRF_STRIDE
    assert G.LRF_STATUS == dict(CONVERGED=LR.CONVERGED, ITER_LIMIT=LR.ITER_LIMIT, STALLED=LR.STALLED, LOST=LR.LOST, SINGULAR=LR.SINGULAR)
    sp = G.level_refine_spec(max_iter=5, max_shrink=3, tol=0.25, step_max_deg=0.1, probe_deg=0.05)
    assert {k: getattr(sp, k) for k in ("max_iter", "max_shrink", "tol", "step_max_deg", "probe_deg")} == LR.spec(5, 3, 0.25, 0.1, 0.05)
    assert ctypes.sizeof(sp) == 32                                                   # two ints and three doubles, as the C struct lays them out
    d = G.level_refine_spec()
    assert {k: getattr(d, k) for k in ("max_iter", "max_shrink", "tol", "step_max_deg", "probe_deg")} == LR.spec()


def test_header_symbols_exist_in_the_built_library(G):
    lib = G.load_library()
    for name in ("geoac_level_refine_check", "geoac_level_refine_fault", "geoac_fan_level_refine", "geoac_fan_level_refine_shape", "geoac_fan_level_refine_fetch",
                 "geoac_fan_level_refine_dev", "geoac_fan_level_refine_timing", "geoac_fan_level_refine_stats"):
        assert hasattr(lib, name), f"{name} is missing from {G.library_path()}"
    assert hasattr(G.FanContext, "level_refine") and hasattr(G.FanContext, "level_refine_timing")


# ---- the restatement on a synthetic integrator ----
def _linear_integrator(eq, A, c_at0, level=1, absent_below=None):
    """crossing tables of a made-up medium: every ray passes level `level` once on leg 0 upward and once downward at c = c_at0 + A (theta, phi) (the
    downward passage 1 km farther along axis 0); rays with theta < absent_below pass nothing"""
    def integrate(th, ph):
        n = len(th)
        count, lrec = np.zeros((1, n, 2), dtype=np.int32), np.zeros((1, n, 2, 4, LVL_STRIDE))
        c0 = c_at0[0] + A[0][0] * th + A[0][1] * ph
        c1 = c_at0[1] + A[1][0] * th + A[1][1] * ph
        ok = np.ones(n, dtype=bool) if absent_below is None else th >= absent_below
        count[0, ok, level] = 2
        for k, (d, shift) in enumerate(((1.0, 0.0), (-1.0, 1.0))):
            rec = lrec[0, :, level, k]
            rec[ok, LVL["DIR"]] = d
            rec[ok, LVL["TTIME"]] = 100.0 + th[ok] + k
            rec[ok, LVL["ATTEN"]] = 0.5 * ph[ok]
            if eq == EQ_GLOBAL:
                rec[ok, LVL["P0"]] = 6400.0
                rec[ok, LVL["P0"] + 1] = np.radians(c0[ok] + shift)
                rec[ok, LVL["P0"] + 2] = np.radians(c1[ok])
            else:
                rec[ok, LVL["P0"]], rec[ok, LVL["P0"] + 1], rec[ok, LVL["P0"] + 2] = c0[ok] + shift, c1[ok], 30.0
            rec[ok, LVL["P0"] + 3], rec[ok, LVL["P0"] + 4], rec[ok, LVL["P0"] + 5] = 0.7, -0.1, 0.2
        return count, lrec
    return integrate


def _lists(theta, phi, direction):
    """level-station lists of one member with one kept row per station: the seed angles, leg 0, the given direction, ordinal 0"""
    n = len(theta)
    rows = np.zeros((1, n, 2, 16))
    rows[0, :, 0, LR.S["THETA"]], rows[0, :, 0, LR.S["PHI"]], rows[0, :, 0, LR.S["DIR"]] = theta, phi, direction
    return np.ones((1, n), dtype=np.uint32), rows


def test_a_linear_crossing_map_converges_in_two_launches():
    """c = c(0) + A (theta, phi): the finite-difference Jacobian is A up to rounding, so one uncut Newton step lands within rounding of the station"""
    A, c00 = [[3.0, -0.5], [0.4, 2.0]], [10.0, -20.0]
    th_star, ph_star = np.array([20.3, 31.7, 12.2]), np.array([-80.4, -95.1, -70.9])
    sta = np.stack([c00[0] + A[0][0] * th_star + A[0][1] * ph_star, c00[1] + A[1][0] * th_star + A[1][1] * ph_star], axis=1)
    hits, rows = _lists(th_star + np.array([0.3, -0.4, 0.2]), ph_star + np.array([-0.2, 0.1, 0.45]), 1.0)
    sp = LR.spec(max_iter=4, tol=1e-6, step_max_deg=1.0, probe_deg=0.02)
    out, stats, _ = LR.reference_level_refine(EQ_3D, hits, rows, sta, [1, 1, 1], [20.0, 35.0], sp, _linear_integrator(EQ_3D, A, c00), LR.sources(EQ_3D, [[1.0, 2.0, 0.0]]))
    assert stats == dict(launches=2, ray_members=18, seeds=3, converged=3, stalled_or_limit=0, lost_or_singular=0)
    assert (out[:, R["STATUS"]] == LR.CONVERGED).all() and (out[:, R["ITER"]] == 2).all() and (out[:, R["MISS"]] <= 1e-6).all()
    assert np.abs(out[:, R["THETA"]] - th_star).max() < 1e-7 and np.abs(out[:, R["PHI"]] - ph_star).max() < 1e-7
    assert np.array_equal(out[:, R["TTIME"]], 100.0 + out[:, R["THETA"]]) and np.array_equal(out[:, R["ATTEN"]], 0.5 * out[:, R["PHI"]])
    assert np.array_equal(out[:, R["N0"]:], np.tile([0.7, -0.1, 0.2], (3, 1))) and (out[:, R["DIR"]] == 1.0).all() and (out[:, R["LEG"]] == 0).all()
    rng = np.sqrt((sta[:, 0] - 1.0) * (sta[:, 0] - 1.0) + (sta[:, 1] - 2.0) * (sta[:, 1] - 2.0))          # from the source point, not from the origin
    assert np.array_equal(out[:, R["CELERITY"]], rng / out[:, R["TTIME"]])
    # the downward branch is 1 km farther along axis 0: the same stations are reached at other angles, and that record's time is one second later
    hits, rows = _lists(th_star, ph_star, -1.0)
    down, stats, _ = LR.reference_level_refine(EQ_3D, hits, rows, sta, [1, 1, 1], [20.0, 35.0], sp, _linear_integrator(EQ_3D, A, c00), LR.sources(EQ_3D, [[1.0, 2.0, 0.0]]))
    assert stats["converged"] == 3 and (down[:, R["DIR"]] == -1.0).all()
    assert np.abs(down[:, R["THETA"]] - th_star).min() > 0.1 and np.array_equal(down[:, R["TTIME"]], 101.0 + down[:, R["THETA"]])


def test_cut_steps_and_the_spherical_wrap():
    """a seed 2.5 degrees of inclination from its eigenray under step_max_deg = 1: three cut steps, then the rest; stations and crossing points either side of the
    antimeridian: every longitude difference goes through WRAP"""
    A, c00 = [[0.05, 0.0], [0.0, 0.1]], [20.0, 178.0]                                # latitude 21 .. 22, longitude 178 + 0.1 phi: phi > 20 lies past +180
    th_star, ph_star = np.array([25.0]), np.array([23.0])
    sta = np.array([[c00[0] + 0.05 * 25.0, c00[1] + 0.1 * 23.0 - 360.0]])           # the station's longitude given as -179.7
    hits, rows = _lists(th_star - 2.5, ph_star - 4.2, 1.0)                            # the seed's ray crosses at +179.88: the other side
    sp = LR.spec(max_iter=8, tol=1e-6, step_max_deg=1.0, probe_deg=0.02)
    out, stats, _ = LR.reference_level_refine(EQ_GLOBAL, hits, rows, sta, [1], [20.0, 35.0], sp, _linear_integrator(EQ_GLOBAL, A, c00), LR.sources(EQ_GLOBAL, [[0.0, 20.0, 170.0]]))
    assert stats["converged"] == 1 and stats["launches"] == 6 and out[0, R["ITER"]] == 6          # 4.2 degrees of azimuth at 1 degree a step: four cut steps, one free, one to see it
    assert abs(out[0, R["THETA"]] - 25.0) < 1e-6 and abs(out[0, R["PHI"]] - 23.0) < 1e-6
    want = LR.DIST(np.array([20.0]), np.array([170.0]), sta[:1, 0], sta[:1, 1], 6370.0)[0] / out[0, R["TTIME"]]
    assert out[0, R["CELERITY"]] == want and 900.0 < want * out[0, R["TTIME"]] < 1100.0          # about 9.7 degrees of longitude at latitude 20, not 350


def test_every_status_has_its_row():
    """LOST: the seed's own ray passes nothing; SINGULAR: a probe passes nothing, or the crossing point does not depend on the angles; STALLED: the
    crossing point never moves towards the station; ITER_LIMIT: one launch is not enough"""
    A, c00 = [[3.0, -0.5], [0.4, 2.0]], [10.0, -20.0]
    src = LR.sources(EQ_3D, [[0.0, 0.0, 0.0]])
    sta = np.array([[100.0, 50.0]])
    hits, rows = _lists(np.array([20.0]), np.array([-80.0]), 1.0)
    sp = LR.spec(max_iter=8, max_shrink=2, tol=1e-6, step_max_deg=1.0, probe_deg=0.02)
    run = lambda integrate, s=sp: LR.reference_level_refine(EQ_3D, hits, rows, sta, [1], [20.0, 35.0], s, integrate, src)          # noqa: E731
    out, stats, _ = run(_linear_integrator(EQ_3D, A, c00, absent_below=30.0))
    assert out[0, R["STATUS"]] == LR.LOST and out[0, R["MISS"]] == -1.0 and stats["launches"] == 1 and (out[0, R["TTIME"]:] == 0).all()
    out, stats, _ = run(_linear_integrator(EQ_3D, A, c00, level=0))                    # (the crossings lie on another level: absent on the seed's)
    assert out[0, R["STATUS"]] == LR.LOST
    flat = _linear_integrator(EQ_3D, [[0.0, 0.0], [0.0, 0.0]], c00)
    out, stats, _ = run(flat)
    assert out[0, R["STATUS"]] == LR.SINGULAR and stats["launches"] == 1 and np.isfinite(out).all() and out[0, R["MISS"]] > 0 and stats["lost_or_singular"] == 1

    def probe_lost(th, ph):                                                           # rays above the seed's inclination pass nothing: the theta probe is absent
        count, lrec = _linear_integrator(EQ_3D, A, c00)(th, ph)
        count[0, th > 20.0, :] = 0
        return count, lrec
    out, stats, _ = run(probe_lost)
    assert out[0, R["STATUS"]] == LR.SINGULAR and out[0, R["ITER"]] == 1
    first = {}

    def frozen(th, ph):                                                               # the first launch's tables for ever: no trial improves on the first
        if not first:
            first["t"] = _linear_integrator(EQ_3D, A, c00)(th, ph)
        return first["t"]
    out, stats, _ = run(frozen)
    assert out[0, R["STATUS"]] == LR.STALLED and stats["launches"] == 4 and out[0, R["ITER"]] == 4 and stats["stalled_or_limit"] == 1
    assert out[0, R["THETA"]] == 20.0 and out[0, R["PHI"]] == -80.0 and (out[0, R["TTIME"]:] == 0).all()
    out, stats, _ = run(_linear_integrator(EQ_3D, A, c00), LR.spec(max_iter=1, tol=1e-6))
    assert out[0, R["STATUS"]] == LR.ITER_LIMIT and stats["launches"] == 1 and out[0, R["THETA"]] == 20.0 and out[0, R["MISS"]] > 1.0


def test_zero_seeds_launch_nothing():
    hits, rows = np.zeros((2, 3), dtype=np.uint32), np.zeros((2, 3, 4, 16))

    def never(th, ph):
        raise AssertionError("no launch is made without seeds")
    out, stats, tables = LR.reference_level_refine(EQ_GLOBAL, hits, rows, np.zeros((3, 2)), [0, 0, 1], [20.0, 35.0], LR.spec(), never, np.zeros((2, 2)))
    assert out.shape == (0, 16) and tables is None and stats == dict(launches=0, ray_members=0, seeds=0, converged=0, stalled_or_limit=0, lost_or_singular=0)
