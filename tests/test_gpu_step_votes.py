"""The rare per-row tests of the spherical stratified set ride in the step loop's wave vote (EqGlobal::checks_fast, k_rk4): the range test near the limit, and the
rows from which a step needs the pole guard of global_base.  Neither may decide anything: with the range skip off (RANGE_SKIP=0: every row takes the range
test) and the unguarded step off (POLE_FAST=0: every step is the guarded one) the records are the same bits, under every launch plan, and they are the plain-C
oracle's answers.  The two constants behind the cheap tests are checked on the host against what they promise (no GPU).

Fans: 8 azimuths x 3 inclinations, range limit 200 km, so that the legs end ON the range limit after a few thousand steps - the range test and the slow rows in
front of it happen in every wave.  No ray of ToyAtmo from a source on the ground comes back down within 200 km, whatever its inclination (the first returns land
at 230 - 250 km: the oracle, on the CPU), so at 200 km every ray breaks and none arrives; each fan therefore runs at 300 km as well, where every ray still ends on
the range limit and 2 - 8 of the 24 have arrived before: ground reflections, leg ends and range breaks in the same waves.  Every GPU test runs under a time
limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

import harness as H
import known_answers as K
from parity import compare_records

STEP_LIMIT_S = 120
R_EARTH = K.R_EARTH
AZ = np.arange(-180.0, 136.0, 45.0)
INC = np.array([0.5, 3.0, 15.0])
TH, PH = np.tile(INC, len(AZ)), np.repeat(AZ, len(INC))
RNGS = (200.0, 300.0)
SRC89 = tuple(float(v) for v in K.polar_fan_with_crossing("n89")[0])
# (source, azimuths, range limit).  30 N: the fast loop throughout; 60 N, 89 N: the guarded step is the main path and lanes at different latitudes change over in
# mid-ray (89 N: the azimuth-0 rays pass over the pole); 50 N aimed north with 400 km: the rays cross the pole_k latitude (51.87 N, 208 km away) in flight
CASES = {f"{name}_{int(rng)}": (src, PH, rng) for name, src in (("n30", (0.0, 30.0, 0.0)), ("n60", (0.0, 60.0, 0.0)), ("n89", SRC89)) for rng in RNGS}
CASES["n50north_400"] = ((0.0, 50.0, 0.0), np.repeat(np.linspace(-14.0, 14.0, len(AZ)), len(INC)), 400.0)

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
    src, ph, rng = CASES[case]
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
        broke = (rec[..., H.REC["BROKE"]] > 0).any(axis=1).sum()
        valid = int((rec[..., H.REC["VALID"]] > 0).sum())
        print(f"{case} amp{amp}: {steps} steps, {broke} of {len(TH)} rays broke (range limit {CASES[case][2]:g} km), {valid} arrivals")
        assert 3 * broke >= len(TH)                               # no empty comparison: range breaks happen ...
        assert valid > 0 or CASES[case][2] == 200.0               # ... and arrivals, except at 200 km where ToyAtmo has none (see above)
        _default[(case, amp)] = (rec, steps)
    return _default[(case, amp)]


def _same(rec, steps, ref, what):
    assert steps == ref[1], what
    assert np.array_equal(rec.view(np.uint64), ref[0].view(np.uint64)), what


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_skip_and_guard_decide_nothing(G, case, amp):
    ref = _ref(G, case, amp)
    if case == "n50north_400":                                        # the rays start below the pole_k latitude and end beyond it
        c = _consts(CASES[case][2])
        lat_k = np.degrees(np.arctan(1.0 / c["pole_k"]))
        lat_end = np.degrees(ref[0][..., H.REC["STATE"] + 1])
        assert CASES[case][0][1] < lat_k < lat_end.max(), (lat_k, lat_end.max())
    for env in ({"GEOAC_RANGE_SKIP": "0"}, {"GEOAC_POLE_FAST": "0"}, {"GEOAC_RANGE_SKIP": "0", "GEOAC_POLE_FAST": "0"}):
        rec, steps = _run(G, case, amp, env)
        _same(rec, steps, ref, (case, amp, env))


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_votes_that_coincide(G, case, amp):
    """chunks of 8 and 64 rows: a chunk fills every few steps, on the same step as slow rows and pole votes; one lane per ray against two; two chunks of 4096"""
    ref = _ref(G, case, amp)
    for env in ({"GEOAC_S_ROWS": "8"}, {"GEOAC_S_ROWS": "64"}, {"GEOAC_NO_PAIR": "1"}, {"GEOAC_TWO_CHUNKS": "1", "GEOAC_S_ROWS": "4096"}):
        rec, steps = _run(G, case, amp, env)
        _same(rec, steps, ref, (case, amp, env))


@gpu
@pytest.mark.parametrize("amp", [1, 0])
@pytest.mark.parametrize("case", ["n30_200", "n30_300", "n60_200", "n60_300"])
def test_against_the_oracle(G, case, amp):
    rec, steps = _ref(G, case, amp)
    src, ph, rng = CASES[case]
    O = H.Oracle(H.EQ_GLOBAL, H.TOYATMO)
    so, ro, _, _ = O.fan(H.make_cfg(H.EQ_GLOBAL, bounces=2, calc_amp=bool(amp), src=src, range_limit=rng), TH, ph)
    assert steps == so
    assert np.array_equal(rec[..., H.REC["STEPS"]], ro[..., H.REC["STEPS"]])
    compare_records(rec, ro, E=18 if amp else 6)


# ---------------- the two bounds, on the host ----------------
def _consts(limit, ds_min=0.001, ds_max=0.5, z_grnd=0.0):          # (geoac_default_params)
    import geoac_amd
    lib = geoac_amd.load_library()
    out = (ctypes.c_double * 5)()
    lib.geoac_probe_step_vote_consts.restype = None
    lib.geoac_probe_step_vote_consts.argtypes = [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_double)]
    lib.geoac_probe_step_vote_consts(limit, R_EARTH, R_EARTH + z_grnd, ds_min, ds_max, out)
    return dict(zip(("range_thresh", "range_skip2", "pole_k", "emax", "delta"), out))


def test_range_skip_bound_never_hides_a_range_break():
    """q < range_skip2  =>  hav <= range_thresh, hav as EqGlobal::checks forms it; 10^6 points (source latitude, azimuth, distance, limit), a third of them
    within 1 % of the limit on either side, where the bound is decided"""
    rng = np.random.default_rng(20240607)
    n = 1_000_000
    limits = np.exp(rng.uniform(np.log(50.0), np.log(5000.0), 64))
    per = n // len(limits)
    skipped = tested = 0
    for limit in limits:
        c = _consts(limit)
        lat0 = np.radians(rng.uniform(-89.9, 89.9, per))
        az = rng.uniform(-np.pi, np.pi, per)
        d = rng.uniform(0.0, 1.0, per)
        near = rng.uniform(0.0, 1.0, per) < 1.0 / 3.0
        d = np.where(near, rng.uniform(0.99, 1.01, per), d) * limit / R_EARTH
        # the point at angular distance d in direction az (spherical direct problem)
        slat = np.sin(lat0) * np.cos(d) + np.cos(lat0) * np.sin(d) * np.cos(az)
        lat = np.arcsin(np.clip(slat, -1.0, 1.0))
        dlon = np.arctan2(np.sin(az) * np.sin(d) * np.cos(lat0), np.cos(d) - np.sin(lat0) * slat)
        sl0, cl0, st, ct = np.sin(lat0), np.cos(lat0), np.sin(lat), np.cos(lat)
        hav = (cl0 * ct) * (0.5 * (1.0 - np.cos(dlon))) + 0.5 * (1.0 - (ct * cl0 + st * sl0))        # EqGlobal::checks
        A = lat - lat0
        q = np.abs(cl0 * ct) * (dlon * dlon) + A * A                                                # EqGlobal::checks_fast
        skip = q < c["range_skip2"]
        assert abs(c["range_thresh"] / np.sin(limit / (2 * R_EARTH)) ** 2 - 1.0) < 1e-14
        assert not (skip & ~(hav <= c["range_thresh"])).any(), limit
        inside = d * R_EARTH < 0.98 * limit
        skipped += int((skip & inside).sum()); tested += int(inside.sum())
    # (and the bound is worth having: at 5000 km it still holds for 97 % of the path, at 1500 km for 99.8 %)
    print(f"{skipped} of {tested} points closer than 98 % of the limit are skipped")
    assert skipped > 0.9 * tested


def test_range_skip_degenerate_limits():
    assert _consts(0.0)["range_skip2"] == -1.0 and _consts(-5.0)["range_skip2"] == -1.0             # (always tested, as range_skip has it)
    c = _consts(np.pi * R_EARTH * 1.01)
    assert c["range_thresh"] == 2.0 and c["range_skip2"] == 1e300                                    # (the test can never fire)
    assert _consts(1e-4)["range_skip2"] == -1.0                                                      # (10 cm: nothing left of the bound - every row is tested)


@pytest.mark.parametrize("ds_max,z_grnd", [(0.5, 0.0), (0.5, 4.0), (0.05, 0.0), (0.01, 0.0)])
def test_pole_k_keeps_the_guard_idle(ds_max, z_grnd):
    """|sin(lat)| pole_k <= |cos(lat)| and |dlat| <= delta  =>  |1 - cos(lat + dlat) / cos(lat)| <= GEOAC_RCPC_EMAX, and delta is what a stage can move:
    the step size is 0.05 - 0.049 exp(..) <= 0.05 km clamped to [ds_min, ds_max] (set_ds), over the smallest radius a stage can have"""
    c = _consts(1500.0, ds_max=ds_max, z_grnd=z_grnd)
    assert c["emax"] == 1e-5
    ds_b = max(min(0.05, ds_max), 0.001)
    assert c["delta"] >= ds_b / (R_EARTH + z_grnd - 3 * ds_b) and c["delta"] < 1.001 * ds_b / (R_EARTH + z_grnd - 3 * ds_b)
    rng = np.random.default_rng(7)
    n = 1_000_000
    lat_k = np.arctan(1.0 / c["pole_k"])
    # latitudes everywhere (beyond the poles too: a ray over a pole carries lat > pi / 2), half of them within 1e-3 rad of the four latitudes where the test changes
    lat = rng.uniform(-np.pi, np.pi, n)
    edge = rng.choice([lat_k, -lat_k, np.pi - lat_k, lat_k - np.pi], n) + rng.uniform(-1e-3, 1e-3, n)
    lat = np.where(rng.uniform(0, 1, n) < 0.5, edge, lat)
    dlat = rng.uniform(-1.0, 1.0, n) * c["delta"]
    dlat[: n // 4] = np.sign(dlat[: n // 4]) * c["delta"]                      # the largest move, both ways
    ok = np.abs(np.sin(lat)) * c["pole_k"] <= np.abs(np.cos(lat))
    e2 = np.abs(1.0 - np.cos(lat + dlat) / np.cos(lat))
    assert ok.sum() > n // 10 and (~ok).sum() > n // 10
    assert (e2[ok] <= c["emax"]).all(), e2[ok].max()
    if ds_max >= 0.05 and z_grnd == 0.0:
        assert 51.8 < np.degrees(lat_k) < 51.95
    assert _consts(1500.0, ds_max=-1.0, ds_min=-1.0)["pole_k"] == np.inf      # (no bound on the step: every step guarded)
