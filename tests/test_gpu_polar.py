"""The stratified Global set near and over the poles against the compiled reference (tests/golden/global_polar.npz, make_golden.py `polar`): sources at
89 N, 85.5 N and 89 S, fans whose rays pass the pole at 0.004 .. 0.05 degrees on either side, and away from it; rays OVER it in the checks that need no
reference.  There cos(lat) changes by up to 6 % of itself within one RK4 step (and changes sign over the pole), which the stage reciprocals of global_base (GEOAC_RCPC) must survive.  The fixture holds the
reference's own answer to a 1e-12 relative change of theta for every compared field of every arrival (4 x that <= 1e-6, asserted when it was made), so the
project's 1e-6 rule applies to every arrival: no exemption list.  Every test runs under a time limit of its own."""
import faulthandler
import os

import numpy as np
import pytest

import harness as H
import known_answers as K
from parity import compare_records, field_errors

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 120
NAMES = ["n89", "n855", "s89"]


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
    return np.load(os.path.join(H.GOLDEN_DIR, "global_polar.npz"))


def _run(G, src, th, ph, amp, env=None):
    with G.options(**(env or {})):
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=2, calc_amp=amp, mode=0, src=tuple(src))
        rec, steps = ctx.run(th, ph)
        ctx.close()
    return rec, steps


def _report(tag, gold, name, rec, want, E):
    """the worst error per field, and per azimuth (relative to the poleward direction) the worst over all fields: how the error grows towards the pole.
    GEOAC_POLAR_LOG names a file that gets the same lines (profiles/polar_parity.txt is made that way)."""
    fe = field_errors(rec, want, E)
    az = np.asarray(gold["az_rel"]); nth = len(want) // len(az)
    worst = np.nanmax(np.stack([fe[f] for f in sorted(fe)], axis=-1), axis=(1, 2)).reshape(len(az), nth)      # [azimuth][inclination]
    valid = want[..., H.REC["VALID"]] > 0
    dlat = np.abs(rec[..., H.REC["STATE"] + 1] - want[..., H.REC["STATE"] + 1])[valid].max()
    lines = [f"{tag}: worst error per field: " + ", ".join(f"{f} {np.nanmax(fe[f]):.2e}" for f in sorted(fe)) + f"; arrival latitude off by <= {dlat:.2e} rad",
             f"{tag}: worst error per azimuth off the pole: " + ", ".join(f"{a:g}: {w:.2e}" for a, w in zip(az, np.nanmax(worst, axis=1)))]
    for line in lines:
        print(line)
    if os.environ.get("GEOAC_POLAR_LOG"):
        with open(os.environ["GEOAC_POLAR_LOG"], "a") as fh:
            fh.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_polar_fan_vs_reference(G, gold, name, amp):
    th, ph, src = gold[f"{name}_theta"], gold[f"{name}_phi"], gold[f"{name}_src"]
    want = gold[f"{name}_amp{amp}_rec"]
    E = 18 if amp else 6
    assert 4.0 * np.nanmax(gold[f"{name}_amp{amp}_sens"]) <= 1e-6          # the reference's own conditioning covers every compared field of every arrival
    rec, steps = _run(G, src, th, ph, amp)
    _report(f"{name} amp{amp}", gold, name, rec, want, E)
    assert (want[..., H.REC["VALID"]] > 0).sum() >= 100 and (want[..., H.REC["BROKE"]] > 0).sum() > 0      # (arrivals and broken legs: no empty comparison)
    assert steps == int(gold[f"{name}_amp{amp}_steps"])
    compare_records(rec, want, E=E)


def test_polar_lane_beside_mid_latitude_lane(G, gold):
    """one set_sources launch of the 89 N source and the (0, 30, 0) source: each source's records are the bits of its single-source run (the fixture's fan
    and the rays aimed at the pole, which cross it)"""
    src89, th, ph, nfix = K.polar_fan_with_crossing("n89")
    srcs = np.array([src89, [0.0, 30.0, 0.0]])
    ctx = G.FanContext(G.EQ_GLOBAL, device=0)
    ctx.load_met(H.TOYATMO)
    ctx.set_params(bounces=2, calc_amp=1, mode=0)
    ctx.set_sources(srcs)
    rec, steps = ctx.run(th, ph)
    ctx.close()
    assert rec.shape == (2, len(th), 3, 32)
    total = 0
    for s, src in enumerate(srcs):
        want, st = _run(G, src, th, ph, 1)
        assert np.array_equal(rec[s].view(np.uint64), want.view(np.uint64)), f"source {s} differs from its single-source run"
        total += st
    assert steps == total
    assert np.degrees(rec[0][nfix:, :, H.REC["STATE"] + 1]).max() > 90.0          # (the added rays did cross the pole: lat beyond pi/2, as in the reference)
    compare_records(rec[0][:nfix], gold["n89_amp1_rec"], E=18)


def test_polar_fan_is_schedule_independent(G, gold):
    """the 89 N fan under the launch plans of test_gpu_fullsize.py::test_full_fan_is_schedule_independent: bit-identical records - the one-lane, the
    two-lane and (A/B builds) the wave-specialised kernels all take the stage reciprocals from the same global_base.  With the rays that cross the pole.
    Which plans differ at this size: the fan has 65 rays, far below the 16 384 at which a fan is split between the two kernels (hybrid), so the PAIR_FRAC values
    and CU_SPLIT select the default's single two-lane launch again and are kept only so that the list stays the full-size test's.  What the fan does tell apart:
    two lanes per ray against one (NO_PAIR), live-ray compaction on and off, one chunk against two of 4096 rows, the accumulation batches, and DUO / TRIO on
    A/B builds - every kernel that holds global_base."""
    src, th, ph, nfix = K.polar_fan_with_crossing("n89")
    ref, steps = _run(G, src, th, ph, 1)
    assert int(ref[:nfix, :, H.REC["STEPS"]].sum()) == int(gold["n89_amp1_steps"])
    plans = [{"GEOAC_PAIR_FRAC": "0.03"}, {"GEOAC_NO_PAIR": "1"}, {"GEOAC_NO_PAIR": "1", "GEOAC_COMPACT": "0"},
             {"GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "4096"}, {"GEOAC_PAIR_FRAC": "1.0"}, {"GEOAC_PAIR_FRAC": "0"}]
    plans += [{"GEOAC_ACCUM_BATCH": "1"}, {"GEOAC_ACCUM_BATCH": "0"}, {"GEOAC_CHUNK_GIB": "1", "GEOAC_ACCUM_BATCH": "1"}]
    plans += [{"GEOAC_NO_PAIR": "1", "GEOAC_CU_SPLIT": "64"}]
    if G.has_ab_kernels():
        plans += [{"GEOAC_DUO": "1"}, {"GEOAC_DUO": "1", "GEOAC_COMPACT": "0"}, {"GEOAC_DUO": "1", "GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "3000"}]
        plans += [{"GEOAC_TRIO": "1"}, {"GEOAC_TRIO": "1", "GEOAC_PAIR_FRAC": "1.0"}, {"GEOAC_TRIO": "1", "GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "3000"}]
    for env in plans:
        rec, st = _run(G, src, th, ph, 1, env)
        assert st == steps, env
        assert np.array_equal(rec.view(np.uint64), ref.view(np.uint64)), env


def test_hamiltonian_residuals_of_the_polar_fan(G, gold):
    """GeoAc_EvalHamiltonian / GeoAc_EvalHamiltonian_Deriv at every arrival of the 89 N fan and of the rays that cross the pole; the bounds of the mid-latitude
    test, which the oracle meets on this fan in the CPU suite (5.3e-6 and 2.4e-3: test_oracle_known_answers.py::test_hamiltonian_residuals_at_arrivals_polar)"""
    src, th, ph, _ = K.polar_fan_with_crossing("n89")
    ctx = G.FanContext(G.EQ_GLOBAL, device=0); ctx.load_met(H.TOYATMO); ctx.set_params(bounces=2, calc_amp=1, mode=0, src=tuple(src))
    rec, _ = ctx.run(th, ph)
    c_src = ctx.probe_atmo_1d(np.array([K.R_EARTH]))[0][0, 0]
    n, h, hd = K.hamiltonian_residuals(H.EQ_GLOBAL, rec, lambda x: ctx.probe_atmo_1d(x)[0], c_src)
    n0, h0, hd0 = K.hamiltonian_residuals(H.EQ_GLOBAL, rec[:, :1], lambda x: ctx.probe_atmo_1d(x)[0], c_src)
    ctx.close()
    print(f"{n} arrivals of the 89 N fan: |H| <= {h:.2e}; first legs ({n0}): |H_deriv| / |mu| <= {hd0:.2e}; all legs: {hd:.2e}")
    assert n >= 100 and h < 1e-4 and hd0 < 2e-2
