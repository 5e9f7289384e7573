"""Chunk reuse follows the data (epoch pipeline): on the stratified sets, arrivals only, one frequency, k_rk4 of epoch e waits for the post-pass of
epoch e - n alone, the post-pass of epoch e waits for k_accum of epoch e - n itself, and the small per-epoch arrays rotate over 2 n sets.  None of that may change
a bit: the oracle of every case is the same fan in the same build with NO_OVERLAP=1 - every kernel on one stream, no edge to miss.  PP_TEST_DELAY_MS holds the
post-pass stream back in every epoch (k_gate, a bounded wait on the wall clock): a graph with its edges in place waits and gives the same bits, a graph with one
missing overwrites a buffer that is still being read.

Hybrid case - the plan the bench runs, more than 16 384 rays: 47 inclinations x 360 azimuths on ToyAtmo, spherical set with amplitudes, one bounce, range limit
300 km (ToyAtmo has no ground arrival nearer, tests/test_gpu_step_votes.py) and epochs of 64 rows, so that the rotation wraps hundreds of times.  Compacted case
(one launch per epoch over the list of live rays: colmap, ncols): 256 rays, epochs of 8 rows.  No ray of ToyAtmo needs fewer than 7 000 steps to 300 km (the
oracle, on the CPU) - 900 epochs of 8 rows and more, 5 s with the post-pass 5 ms late in each: the late post-pass therefore gets the fan with a range limit of 60 km
(the rays end on it after 1 600 - 2 700 steps, in different epochs, so the list shrinks from launch to launch; no leg end), and the fan to 300 km, with its leg
ends, runs with the post-pass on time.  Kept-edge case: a frequency set, whose buffers keep the wait for k_accum.  Every GPU test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

import harness as H

STEP_LIMIT_S = 120
gpu = pytest.mark.gpu

# (inclinations, azimuths, S_ROWS, range limit [km]): angles in fan order, azimuth outer
FANS = {
    "hybrid": (np.linspace(0.5, 23.5, 47), np.arange(-180.0, 180.0, 1.0), 64, 300.0),
    "compacted": (np.linspace(1.0, 32.0, 32), np.arange(-180.0, 180.0, 45.0), 8, 60.0),
    "compacted_far": (np.linspace(1.0, 32.0, 32), np.arange(-180.0, 180.0, 45.0), 8, 300.0),
    "freqset": (np.linspace(1.0, 32.0, 32), np.arange(-180.0, 180.0, 45.0), 64, 300.0),
}
FREQS = (0.1, 0.5, 2.0)
VARIANTS = [(two, delay) for two in (0, 1) for delay in (0, 5)]


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


def _run(G, fan, env):
    inc, az, s_rows, rng = FANS[fan]
    th, ph = np.tile(inc, len(az)), np.repeat(az, len(inc))
    with G.options(GEOAC_S_ROWS=str(s_rows), **env):
        ctx = G.FanContext(G.EQ_GLOBAL, device=0)
        ctx.load_met(H.TOYATMO)
        ctx.set_params(bounces=1, calc_amp=1, mode=0, range_limit=rng)
        if fan == "freqset":
            ctx.set_frequencies(FREQS)
        rec, steps = ctx.run(th, ph)
        att = ctx.fetch_atten() if fan == "freqset" else None
        tm = ctx.timing()
        ctx.close()
    return rec, steps, att, tm


_oracle = {}


def _ref(G, fan):
    """the fan with every kernel on one stream: computed once, shared, never written to"""
    if fan not in _oracle:
        rec, steps, att, tm = _run(G, fan, {"GEOAC_NO_OVERLAP": "1"})
        rec.setflags(write=False)
        valid = int((rec[..., H.REC["VALID"]] > 0).sum())
        last_epoch = np.unique(rec[..., H.REC["STEPS"]].sum(axis=1).astype(np.int64) // FANS[fan][2])
        print(f"{fan}: {len(rec)} rays, {steps} steps, {tm['epochs']} epochs, {valid} arrivals, rays end in {len(last_epoch)} different epochs")
        assert tm["epochs"] >= 100, tm                              # the rotation wraps many times ...
        if fan == "compacted":
            assert len(last_epoch) >= 10                            # ... the list of live rays changes from launch to launch ...
        else:
            assert valid > 0                                        # ... and leg ends (legend, nlegend) are among what rotates
        _oracle[fan] = (rec, steps, att)
    return _oracle[fan]


def _same(got, ref, what):
    assert got[1] == ref[1], what
    assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), what
    if ref[2] is not None:
        assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64)), what


@gpu
@pytest.mark.parametrize("two,delay", VARIANTS)
def test_hybrid_fan_same_bits_as_one_stream(G, two, delay):
    ref = _ref(G, "hybrid")
    assert len(ref[0]) > 16384
    env = {"GEOAC_TWO_CHUNKS": str(two), "PP_TEST_DELAY_MS": str(delay)}
    _same(_run(G, "hybrid", env), ref, env)


@gpu
@pytest.mark.parametrize("two,delay", VARIANTS)
def test_compacted_fan_same_bits_as_one_stream(G, two, delay):
    ref = _ref(G, "compacted")
    env = {"GEOAC_TWO_CHUNKS": str(two), "PP_TEST_DELAY_MS": str(delay)}
    _same(_run(G, "compacted", env), ref, env)
    if delay == 0:                                                   # the fan to 300 km, with leg ends; and over all slots in every epoch
        _same(_run(G, "compacted_far", env), _ref(G, "compacted_far"), env)
        env["GEOAC_COMPACT"] = "0"
        _same(_run(G, "compacted_far", env), _ref(G, "compacted_far"), env)


@gpu
@pytest.mark.parametrize("two,delay", VARIANTS)
def test_frequency_set_keeps_the_wait_for_the_sums(G, two, delay):
    """fcontrib and the per-frequency sums rotate with the chunk and keep the edge behind k_accum: records and the attenuation table [F][rays][legs], with the
    post-pass late, and with the data-following edges switched off altogether (REUSE_EDGES=0), where nothing may differ for a frequency set"""
    ref = _ref(G, "freqset")
    env = {"GEOAC_TWO_CHUNKS": str(two), "PP_TEST_DELAY_MS": str(delay)}
    _same(_run(G, "freqset", env), ref, env)
    if delay == 0:
        env["REUSE_EDGES"] = "0"
        _same(_run(G, "freqset", env), ref, env)


@gpu
def test_reuse_edges_off_same_bits(G):
    """REUSE_EDGES=0 (A/B runs): every fan waits for k_accum before a chunk is reused"""
    for fan in ("hybrid", "compacted", "compacted_far"):
        env = {"REUSE_EDGES": "0", "PP_TEST_DELAY_MS": "0"}
        _same(_run(G, fan, env), _ref(G, fan), (fan, env))


@gpu
def test_ms_wait_is_reported(G):
    """the time between the RK4 epochs: present, non-negative, at most the launch (no assertion on its size: a time is not a test)"""
    for env in ({}, {"GEOAC_NO_OVERLAP": "1"}):
        tm = _run(G, "compacted", env)[3]
        print(env, tm)
        assert "ms_wait" in tm
        assert 0.0 <= tm["ms_wait"] <= tm["ms_total"], tm


def test_new_options_are_listed(G):
    assert {"PP_TEST_DELAY_MS", "REUSE_EDGES", "ACCUM_BATCH_LIVE"} <= set(G.option_names())


@gpu
def test_test_delay_is_bounded(G):
    """PP_TEST_DELAY_MS takes 0 .. 50 ms and nothing else"""
    for bad in ("51", "-1", "1.5", "x"):
        with pytest.raises(G.GeoAcError):
            G.FanContext(G.EQ_GLOBAL, device=0, options={"PP_TEST_DELAY_MS": bad})
    G.FanContext(G.EQ_GLOBAL, device=0, options={"PP_TEST_DELAY_MS": "50"}).close()
