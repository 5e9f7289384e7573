"""The step-count horizon of the spherical stratified set's step loop (geoac_horizon_steps in geoac_device.h - the function EqGlobal::horizon calls in k_rk4 -
with the constants of geoac_probe_step_horizon_consts), on the host: a row with horizon n promises that on the next n rows of its ray neither the range test nor
the test for the pole_k latitude can fire (the vertical limit stays a compare in the loop: as a horizon it was measured slower).  Each promise is checked on 10^6 seeded points against the test it stands for, formed as the
kernel forms it; then the whole rule on rays the plain-C oracle traced.  No GPU."""
import ctypes

import numpy as np
import pytest

import harness as H
import known_answers as K

R_EARTH = K.R_EARTH
TOP = R_EARTH + 139.9                                              # ToyAtmo's top node, as a radius (tests/test_gpu_step_horizon.py)
NAMES = ("rng_s", "rng_per", "pole_s", "pole_c", "pole_eps", "pole_per", "ds_bound")
_ip = ctypes.POINTER(ctypes.c_int)
_dp = ctypes.POINTER(ctypes.c_double)


def _lib():
    import geoac_amd
    lib = geoac_amd.load_library()
    lib.geoac_probe_step_horizon_consts.restype = None
    lib.geoac_probe_step_horizon_consts.argtypes = [ctypes.c_double] * 5 + [_dp]
    lib.geoac_probe_step_horizon.restype = None
    lib.geoac_probe_step_horizon.argtypes = [_dp, ctypes.c_int, _dp, _dp, _dp, _ip]
    lib.geoac_probe_step_vote_consts.restype = None
    lib.geoac_probe_step_vote_consts.argtypes = [ctypes.c_double] * 5 + [_dp]
    return lib


def consts(limit, ds_min=0.001, ds_max=0.5, z_grnd=0.0):              # (geoac_default_params)
    out = (ctypes.c_double * 7)()
    _lib().geoac_probe_step_horizon_consts(limit, R_EARTH, R_EARTH + z_grnd, ds_min, ds_max, out)
    return dict(zip(NAMES, out))


def vote_consts(limit, ds_min=0.001, ds_max=0.5, z_grnd=0.0):
    out = (ctypes.c_double * 5)()
    _lib().geoac_probe_step_vote_consts(limit, R_EARTH, R_EARTH + z_grnd, ds_min, ds_max, out)
    return dict(zip(("range_thresh", "range_skip2", "pole_k", "emax", "delta"), out))


def horizon(hz, hav, slat, clat):
    hav, slat, clat = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(hav))) for a in (hav, slat, clat))
    out = np.zeros(hav.shape, dtype=np.int32)
    c = np.array([hz[k] for k in NAMES[:6]])
    _lib().geoac_probe_step_horizon(c.ctypes.data_as(_dp), hav.size, *(a.ctypes.data_as(_dp) for a in (hav, slat, clat)), out.ctypes.data_as(_ip))
    return out


def hav_of(lat0, lat, dlon):
    """the haversine as EqGlobal::checks / range_far form it"""
    sl0, cl0, st, ct = np.sin(lat0), np.cos(lat0), np.sin(lat), np.cos(lat)
    return (cl0 * ct) * (0.5 * (1.0 - np.cos(dlon))) + 0.5 * (1.0 - (ct * cl0 + st * sl0))


def _direct(lat0, az, d):
    """the point at angular distance d in direction az from (lat0, 0): latitude, longitude"""
    slat = np.sin(lat0) * np.cos(d) + np.cos(lat0) * np.sin(d) * np.cos(az)
    lat = np.arcsin(np.clip(slat, -1.0, 1.0))
    return lat, np.arctan2(np.sin(az) * np.sin(d) * np.cos(lat0), np.cos(d) - np.sin(lat0) * slat)


GRID = [(0.5, 0.0), (0.5, 4.0), (0.05, 0.0), (0.01, 0.0)]            # ds_max, z_grnd
EQUATOR = (0.0, 1.0)                                                # sin / cos of a latitude far from the pole_k latitudes: the range term alone
LAT30 = (np.sin(np.radians(30.0)), np.cos(np.radians(30.0)))


@pytest.mark.parametrize("ds_max,z_grnd", GRID)
def test_range_horizon_never_hides_a_range_break(ds_max, z_grnd):
    """a row at range r0 with horizon >= n, and a second point no further from it than n rows can move (n x the angle `adv` the period stands for, in any
    direction): the second point's haversine is <= range_thresh.  A third of the rows within 1 % of the limit, where the horizon is short and the bound tight;
    the second point as far as the horizon allows for half of them"""
    rng = np.random.default_rng(20240911)
    n_pts = 1_000_000
    limits = np.exp(rng.uniform(np.log(50.0), np.log(5000.0), 50))
    per = n_pts // len(limits)
    long_ones = short_ones = 0
    for limit in limits:
        hz = consts(limit, ds_max=ds_max, z_grnd=z_grnd)
        vc = vote_consts(limit, ds_max=ds_max, z_grnd=z_grnd)
        adv = 2.0 / hz["rng_per"]
        assert adv >= vc["delta"] and adv < 1.001 * vc["delta"]                 # a row's angle: a stage's latitude increment, with its margin
        lat0 = np.radians(rng.uniform(-89.9, 89.9, per))
        near = rng.uniform(0.0, 1.0, per) < 1.0 / 3.0
        d0 = np.where(near, rng.uniform(0.99, 1.0, per), rng.uniform(0.0, 1.0, per)) * limit / R_EARTH
        lat1, lon1 = _direct(lat0, rng.uniform(-np.pi, np.pi, per), d0)
        h = horizon(hz, hav_of(lat0, lat1, lon1), *EQUATOR)
        n = np.where(rng.uniform(0.0, 1.0, per) < 0.5, h, np.floor(rng.uniform(0.0, 1.0, per) * (h + 1))).astype(np.int64)
        n = np.minimum(n, h)
        # second point: n adv from the first, in any direction
        lat2, dl = _direct(lat1, rng.uniform(-np.pi, np.pi, per), n * adv)
        ok = hav_of(lat0, lat2, lon1 + dl) <= vc["range_thresh"]
        assert ok.all(), (limit, int((~ok).sum()))
        # and straight on: the point n adv further along the great circle from the source
        lat3, lon3 = _direct(lat0, 0.3, d0 + n * adv)
        assert (hav_of(lat0, lat3, lon3) <= vc["range_thresh"]).all(), limit
        long_ones += int((h[~near] > 100).sum()); short_ones += int((h[near] < 100).sum())
    assert long_ones > n_pts // 4 and short_ones > 0
    # the bound is worth having: from the source the first horizon at 1500 km is nearly the whole way (30 000 steps of 0.05 km)
    first = horizon(consts(1500.0), np.zeros(1), *LAT30)[0]
    print("first horizon at 1500 km:", first)
    assert 29_000 <= first <= 30_000


@pytest.mark.parametrize("ds_max,z_grnd", GRID)
def test_pole_horizon_keeps_the_rows_below_the_pole_k_latitude(ds_max, z_grnd):
    """a latitude move of n delta, either way, from a row with horizon >= n stays where |sin| pole_k <= |cos|; latitudes everywhere, beyond pi / 2 too (a ray over
    a pole), a third within 1 % of the pole_k latitudes"""
    rng = np.random.default_rng(11)
    n_pts = 1_000_000
    hz = consts(np.pi * R_EARTH * 1.01, ds_max=ds_max, z_grnd=z_grnd)     # (a range limit that can never fire: the pole term alone)
    vc = vote_consts(1500.0, ds_max=ds_max, z_grnd=z_grnd)
    lat_k = np.arctan(1.0 / vc["pole_k"])
    assert abs(hz["pole_s"] - np.sin(lat_k)) < 1e-15 and abs(hz["pole_c"] - np.cos(lat_k)) < 1e-15 and abs(hz["pole_per"] * vc["delta"] - 1.0) < 1e-12
    lat = rng.uniform(-1.5 * np.pi, 1.5 * np.pi, n_pts)
    edge = rng.choice([lat_k, -lat_k, np.pi - lat_k, lat_k - np.pi, np.pi + lat_k], n_pts) * rng.uniform(0.99, 1.01, n_pts)
    lat = np.where(rng.uniform(0, 1, n_pts) < 1.0 / 3.0, edge, lat)
    h = horizon(hz, np.zeros(n_pts), np.sin(lat), np.cos(lat))
    inside = np.abs(np.sin(lat)) * vc["pole_k"] <= np.abs(np.cos(lat))
    assert not (h[~inside] > 0).any()                                    # a row beyond the latitude: the next row is tested
    assert (h[inside] > 0).sum() > n_pts // 4 and (h[inside] < 50).sum() > 100
    n = np.where(rng.uniform(0, 1, n_pts) < 0.5, h, np.floor(rng.uniform(0, 1, n_pts) * (h + 1))).astype(np.int64)
    n = np.minimum(n, h)
    for sign in (1.0, -1.0):
        lat2 = lat + sign * n * vc["delta"]
        ok = np.abs(np.sin(lat2)) * vc["pole_k"] <= np.abs(np.cos(lat2))
        assert ok[h > 0].all(), int((~ok[h > 0]).sum())
    # and the horizon is worth having: from 30 N the pole_k latitude (51.87 N at ds_bound = 0.05) is 21.87 degrees away: 48 600 rows of delta, 47 455 by the sine
    # the rule takes for the angle
    if ds_max >= 0.05 and z_grnd == 0.0:
        assert 47_000 < horizon(hz, np.zeros(1), *LAT30)[0] < 48_700


def test_vertical_limit_is_not_part_of_the_horizon():
    """the vertical limit is a compare on every row of the loop (EqGlobal::checks_hz): the rule takes no radius and its constants know no top"""
    hz = consts(1500.0)
    assert set(hz) == set(NAMES) and hz["ds_bound"] == 0.05
    assert consts(1500.0, ds_max=0.01)["ds_bound"] == 0.01 and consts(1500.0, ds_max=0.0001)["ds_bound"] == 0.001      # max(min(0.05, ds_max), ds_min)


def test_degenerate_inputs_test_every_row_or_none():
    eq = (np.zeros(1),) + EQUATOR
    for limit in (0.0, -5.0, float("nan"), 1e-4):                              # always fires / a NaN / 10 cm: the next row is tested
        assert horizon(consts(limit), *eq)[0] == 0, limit
    never = consts(np.pi * R_EARTH * 1.01)                                     # the range test can never fire: only the pole term counts
    assert horizon(never, np.full(1, 0.999), *EQUATOR)[0] > 100_000
    hz = consts(1500.0, ds_min=-1.0, ds_max=-1.0)                              # no bound on the step: every row is tested (and every step guarded: pole_k = inf)
    assert all(hz[k] == 0.0 for k in NAMES[:6]) and horizon(hz, *eq)[0] == 0
    assert vote_consts(1500.0, ds_min=-1.0, ds_max=-1.0)["pole_k"] == np.inf
    for bad in (float("nan"), float("inf")):                                    # a NaN in the row: tested
        assert horizon(consts(1500.0), np.full(1, bad), *EQUATOR)[0] == 0
    assert horizon(consts(1500.0), np.zeros(1), float("nan"), 1.0)[0] == 0 and horizon(consts(1500.0), np.zeros(1), 0.0, float("nan"))[0] == 0
    assert horizon(consts(1500.0), np.zeros(1), 1.0, 0.0)[0] == 0              # on the pole
    assert horizon(consts(1500.0), np.full(1, 1.0), *EQUATOR)[0] == 0           # beyond the limit


# ---------------- the rule on traced rays ----------------
AZ8 = np.arange(-180.0, 136.0, 45.0)


@pytest.fixture(scope="module")
def traces():
    """leg 0 of 24 rays of the oracle at 200 and 300 km: rows (r, lat, lon) up to and including the row that broke on the range limit; traced once, never written to"""
    O = H.Oracle(H.EQ_GLOBAL, H.TOYATMO)
    out = {}
    for limit in (200.0, 300.0):
        cfg = H.make_cfg(H.EQ_GLOBAL, bounces=0, calc_amp=False, range_limit=limit)
        for inc in (0.5, 3.0, 15.0):
            for az in AZ8:
                k, rows = O.trace_leg0(cfg, inc, az)
                rows = rows[:, :3].copy(); rows.setflags(write=False)
                out[(limit, inc, float(az))] = rows
    return out


def test_rule_on_oracle_traces(traces):
    """the rule as the step loop applies it (row 0's horizon gives the first row to test; a tested row within the limit gives the next one: n rows are skipped), on
    the rows of each traced ray: the first row beyond the limit is a tested row, no row before it that is beyond the limit was skipped (there is none: the first
    one ends the leg), and a ray takes at most 12 tests"""
    lat0 = np.radians(30.0)
    worst = checked = 0
    for (limit, inc, az), rows in traces.items():
        hz = consts(limit)
        thresh = vote_consts(limit)["range_thresh"]
        r, lat, lon = rows[:, 0], rows[:, 1], rows[:, 2]
        hav = hav_of(lat0, lat, lon)
        beyond = hav > thresh
        if not beyond.any():                                          # (300 km: a ray that came down before the limit ends its leg 0 on the ground)
            continue
        first = int(np.argmax(beyond))
        assert first == len(rows) - 1, (limit, inc, az)               # (the oracle stopped on it)
        step = np.stack([np.diff(r), r[:-1] * np.diff(lat), r[:-1] * np.cos(lat[:-1]) * np.diff(lon)], 1)
        assert np.sqrt((step ** 2).sum(1)).max() <= hz["ds_bound"] * (1 + 1e-4)      # no row moves further than the longest step
        h = horizon(hz, hav, np.sin(lat), np.cos(lat))
        k, tests = 1 + int(h[0]), 0
        while True:
            tests += 1
            assert k <= first, (limit, inc, az, k, first)             # a row beyond the limit was skipped
            if k == first:
                break
            k += 1 + int(h[k])
        worst = max(worst, tests); checked += 1
        assert tests <= 12, (limit, inc, az, tests)
    print("most tests on a traced ray:", worst, "rays:", checked)
    assert checked >= 40 and worst > 1                                  # (24 rays at 200 km, and those at 300 km that have not come down before)
