"""The step-count horizon of the spherical stratified set's step loop (k_rk4, EqGlobal::checks_hz / horizon): range limit, pole_k latitude and step limit are
tested on the rows where a ray's horizon expires and nowhere else (the vertical limit on every row).  The horizon may decide nothing: with a range horizon of one step (RANGE_SKIP=0) and
with every step guarded (POLE_FAST=0) the records are the same bits, under every launch plan - chunks of 8 rows, where the chunk bound, the horizon and leg ends
fall on the same rows - and they are the plain-C oracle's answers, step count for step count.  (The bounds behind the horizon: tests/test_step_horizon.py, no GPU.)

Fans: 8 azimuths x inclinations 0.5, 3, 15 and 60 degrees, two bounces.  The 60-degree rays leave through the top of the profile after ~3 300 steps (the vertical
limit); the others run to the range limit - 600 km: every ray breaks, most of them after an arrival or two; 1500 km from 30 N: legs of up to 42 909 steps, 59
arrivals; 48 N aimed north: the rays cross the pole_k latitude (51.87 N) in flight and end at 53.3 N.  Every GPU test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

import harness as H
import known_answers as K
from parity import compare_records
from test_step_horizon import TOP, vote_consts

STEP_LIMIT_S = 120
AZ = np.arange(-180.0, 136.0, 45.0)
INC = np.array([0.5, 3.0, 15.0, 60.0])
TH, PH = np.tile(INC, len(AZ)), np.repeat(AZ, len(INC))
PH48 = np.repeat(np.linspace(-14.0, 14.0, len(AZ)), len(INC))
SRC89 = tuple(float(v) for v in K.polar_fan_with_crossing("n89")[0])
# (source, azimuths, range limit, arrivals required)
CASES = {
    "n30_600": ((0.0, 30.0, 0.0), PH, 600.0, True),
    "n30_1500": ((0.0, 30.0, 0.0), PH, 1500.0, True),
    "n48north_600": ((0.0, 48.0, 0.0), PH48, 600.0, True),
    "n60_300": ((0.0, 60.0, 0.0), PH, 300.0, False),
    "n89_300": (SRC89, PH, 300.0, False),
}

gpu = pytest.mark.gpu


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


def _run(G, case, amp, env=None):
    src, ph, rng, _ = CASES[case]
    with G.options(**(env or {})):
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=2, calc_amp=amp, mode=0, src=src, range_limit=rng)
        rec, steps = ctx.run(TH, ph)
        ctx.close()
    return rec, steps


_default = {}


def _ref(G, case, amp):
    """the default plan's records of a case: computed once, shared, never written to"""
    if (case, amp) not in _default:
        rec, steps = _run(G, case, amp)
        rec.setflags(write=False)
        broke = rec[..., H.REC["BROKE"]] > 0
        top = broke & (rec[..., H.REC["STATE"]] > TOP)                # the leg's last row is above the profile: the vertical limit ended it
        # (and it cannot have been the range limit: all the ray's steps, each at most 0.05 km long, do not add up to it)
        short = broke.any(axis=1) & (rec[..., H.REC["STEPS"]].sum(axis=1) * 0.05 < CASES[case][2])
        assert np.array_equal(top.any(axis=1), short), (top.any(axis=1), short)
        on_range = (broke & ~top).any(axis=1).sum()
        valid = int((rec[..., H.REC["VALID"]] > 0).sum())
        print(f"{case} amp{amp}: {steps} steps, longest leg {int(rec[..., H.REC['STEPS']].max())}, {on_range} of {len(TH)} rays broke on the range limit "
              f"({CASES[case][2]:g} km), {int(top.any(axis=1).sum())} on the vertical limit, {valid} arrivals")
        assert 4 * on_range >= len(TH)                                # no empty comparison: range breaks happen ...
        assert top.any()                                              # ... a ray leaves through the top ...
        assert valid >= 15 or not CASES[case][3]                      # ... and rays arrive (60 N / 89 N at 300 km: only the breaks)
        _default[(case, amp)] = (rec, steps)
    return _default[(case, amp)]


def _same(rec, steps, ref, what):
    assert steps == ref[1], what
    assert np.array_equal(rec.view(np.uint64), ref[0].view(np.uint64)), what


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_options_change_nothing(G, case, amp):
    ref = _ref(G, case, amp)
    if case == "n48north_600":                                        # the rays start below the pole_k latitude and end beyond it
        lat_k = np.degrees(np.arctan(1.0 / vote_consts(CASES[case][2])["pole_k"]))
        lat_end = np.degrees(ref[0][..., H.REC["STATE"] + 1])
        assert CASES[case][0][1] < lat_k < lat_end.max(), (lat_k, lat_end.max())
    for env in ({"GEOAC_RANGE_SKIP": "0"}, {"GEOAC_POLE_FAST": "0"}, {"GEOAC_RANGE_SKIP": "0", "GEOAC_POLE_FAST": "0"}):
        rec, steps = _run(G, case, amp, env)
        _same(rec, steps, ref, (case, amp, env))


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_launch_plan_changes_nothing(G, case, amp):
    """chunks of 8 and 64 rows (the chunk bound, the horizon and leg ends on the same rows), one lane per ray against two, two chunks of 4096: the horizon is the
    ray's, carried from launch to launch, and the chunk bound is kept apart from it"""
    ref = _ref(G, case, amp)
    for env in ({"GEOAC_S_ROWS": "8"}, {"GEOAC_S_ROWS": "64"}, {"GEOAC_NO_PAIR": "1"}, {"GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "4096"}):
        rec, steps = _run(G, case, amp, env)
        _same(rec, steps, ref, (case, amp, env))


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", ["n30_600", "n30_1500", "n48north_600"])
def test_against_the_oracle(G, case, amp):
    rec, steps = _ref(G, case, amp)
    src, ph, rng, _ = CASES[case]
    O = H.Oracle(H.EQ_GLOBAL, H.TOYATMO)
    so, ro, _, _ = O.fan(H.make_cfg(H.EQ_GLOBAL, bounces=2, calc_amp=bool(amp), src=src, range_limit=rng), TH, ph)
    assert steps == so
    assert np.array_equal(rec[..., H.REC["STEPS"]], ro[..., H.REC["STEPS"]])
    compare_records(rec, ro, E=18 if amp else 6)
