"""GPU parity of the range-dependent spherical set (GeoAcGlobal.RngDep) against golden vectors from the compiled reference:
synthetic 5x5 lat/lon grid of perturbed profiles, 3 x 4 degree cells (tests/rngdep_data.py)."""
import faulthandler

import numpy as np
import pytest

import harness as H
from geoac_amd.api import DEFAULT_OPTIONS as OPT      # launch-plan options of the contexts the tests create (geoac_set_option)
import rngdep_data as RD
from parity import compare_records, field_errors, max_rel_errors

pytestmark = pytest.mark.gpu
EQ = H.EQ_GLOBAL_RNGDEP


@pytest.fixture(scope="module")
def gold():
    return np.load(f"{H.GOLDEN_DIR}/globalrd_small.npz")


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return RD.write_grid_global(str(tmp_path_factory.mktemp("gg")), short_paths=False)


def _ctx(grid, **params):
    import geoac_amd as G
    ctx = G.FanContext(G.EQ_GLOBAL_RNGDEP, device=0)
    ctx.load_grid(*grid, z_grnd=0.0)          # -prop loads before any z_grnd= is seen (GeoAcGlobal.RngDep_main.cpp:133)
    ctx.set_params(**params)
    return ctx


@pytest.mark.parametrize("amp", [1, 0])
def test_globalrd_fan_vs_golden(gold, grid, amp):
    ctx = _ctx(grid, bounces=1, calc_amp=amp, mode=0, src=(0.0, 31.0, 0.0))
    rec, steps = ctx.run(gold["theta"], gold["phi"])
    want = gold[f"rec_amp{amp}_mode0"]
    E = 18 if amp else 6
    print("globalrd", amp, max_rel_errors(rec, want, E, 0))
    assert steps == int(gold[f"steps_amp{amp}_mode0"])
    compare_records(rec, want, E=E, hidx=0)


def test_globalrd_alt_config_vs_golden(gold, grid):
    ctx = _ctx(grid, bounces=2, calc_amp=1, mode=0, src=(1.5, 29.0, 1.0), z_grnd=0.3, freq=0.4, tweak_abs=0.6,
               xy_limits=tuple(np.radians([26.0, 36.5, -7.0, 6.0])))
    rec, steps = ctx.run(gold["theta"], gold["phi"])
    print("globalrd alt", max_rel_errors(rec, gold["rec_alt"], 18, 0))
    assert steps == int(gold["steps_alt"])
    compare_records(rec, gold["rec_alt"], E=18, hidx=0)


def test_globalrd_write_rays_caustics_vs_golden(gold, grid):
    ctx = _ctx(grid, bounces=1, calc_amp=1, mode=3, src=(0.0, 31.0, 0.0))
    rec, steps = ctx.run(gold["theta"], gold["phi"])
    compare_records(rec, gold["rec_amp1_mode3"], E=18, hidx=0)
    smp = ctx.fetch_samples()
    assert len(smp) == int(gold["nsmp_amp1_mode3"])
    gs = smp[gold["smp_idx_amp1_mode3"]]; ws = gold["smp_amp1_mode3"]
    assert np.array_equal(gs[:, :4], ws[:, :4])
    for col in range(4, 10):
        d = np.abs(gs[:, col] - ws[:, col])
        scale = np.maximum(np.abs(ws[:, col]), 1e-3 * max(np.abs(ws[:, col]).max(), 1e-30))
        if col == 7:
            ray_rows = ws[:, 3] == 0        # amplitude in dB on raypath rows: absolute 20 log10(1 + 1e-6); travel time on caustic rows
            assert (d[ray_rows] <= 8.7e-6 + 1e-6 * np.abs(ws[ray_rows, col])).all()
            assert (d[~ray_rows] / scale[~ray_rows] <= 1e-6).all()
        else:
            assert (d / scale).max() <= 1e-6, (col, (d / scale).max())


@pytest.mark.parametrize("lanes", [1, 2, 4, "coop", "dense", "coop+sub"])
def test_every_lanes_per_ray_variant_vs_golden(gold, grid, lanes, monkeypatch):
    if lanes == "coop+sub":
        # the launch plan of saturated fans forced on the small one: cooperative LDS-DMA gather, 512-row epochs in four sub-epochs handed from
        # workgroup to workgroup (sample and caustic events carried across the hand-off)
        monkeypatch.setitem(OPT, "SUB_MIN_WAVES", "0")
        monkeypatch.setitem(OPT, "SUB_EPOCHS", "4")
        monkeypatch.setitem(OPT, "S_ROWS", "512")
        lanes = "coop"
    if lanes == 2:
        import geoac_amd
        if not geoac_amd.has_ab_kernels():
            pytest.skip("the two-lane grid kernels are part of A/B builds only (make AB=1; GEOAC_LIB=<that build> runs this case)")
    if lanes in ("coop", "dense"):
        # one lane per ray without lane thinning, as a large fan runs: "coop" = wave-cooperative table gather through LDS (58 of the
        # wave's 64 lanes are helpers without a ray here), "dense" = the same launch with per-lane gathers
        monkeypatch.setitem(OPT, "GRID_LANES", "1")
        monkeypatch.setitem(OPT, "SPREAD", "1")
        monkeypatch.setitem(OPT, "GRID_COOP", "1" if lanes == "coop" else "0")
    else:
        monkeypatch.setitem(OPT, "GRID_LANES", str(lanes))
    ctx = _ctx(grid, bounces=1, calc_amp=1, mode=3, src=(0.0, 31.0, 0.0))
    rec, steps = ctx.run(gold["theta"], gold["phi"])
    assert steps == int(gold["steps_amp1_mode3"])
    compare_records(rec, gold["rec_amp1_mode3"], E=18, hidx=0)
    assert len(ctx.fetch_samples()) == int(gold["nsmp_amp1_mode3"])


def test_eight_lane_kernel_gives_the_four_lane_kernels_bits(gold, grid, monkeypatch):
    """small arrivals-only fans with amplitudes run eight lanes per ray (four cell corners x the two launch-angle systems, EqGlobalRngDepOct);
    GEOAC_OCT=0 keeps them on the four-lane kernel: same records bit for bit, and both within tolerance of the golden ones"""
    out = {}
    monkeypatch.setitem(OPT, "HEX", "0")
    for oct_on in ("1", "0"):
        monkeypatch.setitem(OPT, "OCT", oct_on)
        ctx = _ctx(grid, bounces=2, calc_amp=1, mode=0, src=(0.0, 31.0, 0.0))
        out[oct_on] = ctx.run(gold["theta"], gold["phi"])
    assert out["1"][1] == out["0"][1]
    assert np.array_equal(out["1"][0], out["0"][0])
    # ... and the sixteen-lane kernel (one field of one corner per lane, EqGlobalRngDepHex: the default for fans this small) the same bits again
    monkeypatch.setitem(OPT, "OCT", "1"); monkeypatch.setitem(OPT, "HEX", "1")
    ctx = _ctx(grid, bounces=2, calc_amp=1, mode=0, src=(0.0, 31.0, 0.0))
    rec16, steps16 = ctx.run(gold["theta"], gold["phi"])
    assert steps16 == out["1"][1]
    assert np.array_equal(rec16, out["1"][0])
    # a fan that is not a multiple of four rays (part-filled wave), and one ray alone
    for n in (5, 1):
        got = {}
        for hx in ("1", "0"):
            monkeypatch.setitem(OPT, "HEX", hx)
            ctx = _ctx(grid, bounces=2, calc_amp=1, mode=0, src=(0.0, 31.0, 0.0))
            got[hx] = ctx.run(gold["theta"][:n], gold["phi"][:n])
        assert got["1"][1] == got["0"][1] and np.array_equal(got["1"][0], got["0"][0])


def test_sixteen_lane_scan_kernel_gives_the_four_lane_kernels_bits(gold, grid, monkeypatch):
    """amplitude-less arrivals-only fans of a few hundred rays (the inclination scans of an eigenray search) split the table evaluation over sixteen lanes
    (EqGlobalRngDepScan16); HEX=0 keeps them on the four-lane kernel: the same records bit for bit, also for a part-filled wave and a single ray"""
    for n in (len(gold["theta"]), 5, 1):
        got = {}
        for hx in ("1", "0"):
            monkeypatch.setitem(OPT, "HEX", hx)
            ctx = _ctx(grid, bounces=2, calc_amp=0, mode=0, src=(0.0, 31.0, 0.0))
            got[hx] = ctx.run(gold["theta"][:n], gold["phi"][:n])
        assert got["1"][1] == got["0"][1] and np.array_equal(got["1"][0], got["0"][0])



@pytest.mark.parametrize("amp", [0, 1])
def test_leg_records_do_not_depend_on_the_number_of_bounces(grid, amp):
    """A ray launched with b bounces goes through the states of the same ray launched with fewer: its records of legs 0 .. a are, bit for bit, the
    records of the fan with a bounces (a broken ray's later legs are empty either way).  The eigenray scheduler relies on it: inclination scans
    of one round that differ only in the bounce count are integrated once, with the largest (geoac_eigenray.cpp, serve)."""
    th = np.linspace(1.0, 40.0, 79); ph = np.full_like(th, -77.0)
    recs = {}
    for b in (0, 1, 2):
        ctx = _ctx(grid, bounces=b, calc_amp=amp, mode=0, src=(0.0, 31.0, 0.0))
        recs[b] = ctx.run(th, ph)[0].copy(); ctx.close()
    for a in (0, 1):
        for b in range(a + 1, 3):
            assert np.array_equal(recs[b][:, :a + 1].view(np.uint64), recs[a].view(np.uint64)), (a, b)


# ---- the same set at high latitude: rows at 82 .. 89.5 N, 15 degrees of longitude apart (116 km at the source, 14.6 km on the last row); fixture
#      tests/golden/globalrd_polar.npz from the compiled reference (make_golden.py globalrd_polar) ----
STEP_LIMIT_S = 120


@pytest.fixture
def time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gold_polar():
    return np.load(f"{H.GOLDEN_DIR}/globalrd_polar.npz")


@pytest.fixture(scope="module")
def grid_polar(tmp_path_factory):
    return RD.write_grid_global(str(tmp_path_factory.mktemp("ggp")), short_paths=False, **RD.POLAR_GRID)


def test_globalrd_polar_fan_vs_golden(gold_polar, grid_polar, time_limit):
    """5 x 7 fan from 86 N, towards the pole and beside it, sideways and away, one bounce, amplitudes on: VALID / STEPS / BROKE of every leg and the
    step total exact, every field compare_records judges within 1e-6.  The reference's own conditioning (theta (1 + 1e-12), in the fixture) covers every
    field of every arrival: no exemptions."""
    g = gold_polar
    assert 4.0 * np.nanmax(g["sens"]) <= 1e-6
    want = g["rec_amp1"]
    valid = want[..., H.REC["VALID"]] > 0
    assert valid.sum() >= 10 and np.degrees(want[..., H.REC["STATE"] + 1][valid]).max() > 89.0 and (want[..., H.REC["BROKE"]] > 0).sum() > 0
    ctx = _ctx(grid_polar, bounces=1, calc_amp=1, mode=0, src=tuple(g["src"]))
    rec, steps = ctx.run(g["theta"], g["phi"])
    fe = field_errors(rec, want, 18, 0)
    print("globalrd polar: worst error per field: " + ", ".join(f"{f} {np.nanmax(fe[f]):.2e}" for f in sorted(fe)))
    assert steps == int(g["steps_amp1"])
    compare_records(rec, want, E=18, hidx=0)


@pytest.mark.parametrize("lanes", [1, 4, "coop", "dense"])
def test_globalrd_polar_lanes_per_ray_variants_vs_golden(gold_polar, grid_polar, lanes, monkeypatch, time_limit):
    """the launches of test_every_lanes_per_ray_variant_vs_golden that every build holds, on the polar grid: the wave-cooperative gather ("coop") and its
    per-lane twin ("dense") as a large fan runs them, one and four lanes per ray"""
    g = gold_polar
    if lanes in ("coop", "dense"):
        monkeypatch.setitem(OPT, "GRID_LANES", "1")
        monkeypatch.setitem(OPT, "SPREAD", "1")
        monkeypatch.setitem(OPT, "GRID_COOP", "1" if lanes == "coop" else "0")
    else:
        monkeypatch.setitem(OPT, "GRID_LANES", str(lanes))
    ctx = _ctx(grid_polar, bounces=1, calc_amp=1, mode=0, src=tuple(g["src"]))
    rec, steps = ctx.run(g["theta"], g["phi"])
    assert steps == int(g["steps_amp1"])
    compare_records(rec, g["rec_amp1"], E=18, hidx=0)


# ---- the ragged 7 x 4 jet grid (rngdep_data.write_grid_ragged): nx != ny, unequal node spacing on all three axes, 3.3 m height segments, winds of +-50 m/s with a
#      meridional part, raised ground, sources on the ground and inside the jet at 12 km, rays launched below the horizontal, 10 Hz and 0.01 Hz; fixture
#      tests/golden/rngdep_ragged_globalrd.npz from the compiled reference (make_golden.py raggedglobal) ----

# launch-plan options -> every kernel the shipped library can select for the amplitudes-on table of fan b (25 rays)
RAGGED_VARIANTS = {
    "default": {},                                                              # sixteen lanes per ray (EqGlobalRngDepHex)
    "hex0": {"HEX": "0"},                                                       # eight lanes per ray (EqGlobalRngDepOct)
    "oct0": {"HEX": "0", "OCT": "0"},                                                      # four lanes per ray, as the plan picks them
    "lanes4": {"GRID_LANES": "4"},
    "lanes1": {"GRID_LANES": "1"},
    "coop": {"GRID_LANES": "1", "SPREAD": "1", "GRID_COOP": "1"},               # one lane per ray without lane thinning, wave-cooperative gather: as a large fan runs
    "dense": {"GRID_LANES": "1", "SPREAD": "1", "GRID_COOP": "0"},              # the same launch with per-lane gathers
    "coop+sub": {"GRID_LANES": "1", "SPREAD": "1", "GRID_COOP": "1", "SUB_MIN_WAVES": "0", "SUB_EPOCHS": "4", "S_ROWS": "512"},     # the plan of saturated fans
    "tile0": {"GRID_LANES": "1", "TILE": "0"},                                  # slot order: by inclination ...
    "sort0": {"GRID_LANES": "1", "SORT": "0"},                                  # ... and the caller's
}
# variants that perform the same operations on the same operands (the tests above state it for the 5 x 5 grid): the same records bit for bit
RAGGED_SAME_BITS = [("default", "hex0", "oct0", "lanes4"), ("lanes1", "tile0", "sort0")]
_ragged_runs = {}


@pytest.fixture(scope="module")
def gold_ragged():
    return RD.ragged_fixture(True)


@pytest.fixture(scope="module")
def grid_ragged(tmp_path_factory):
    return RD.write_grid_ragged(str(tmp_path_factory.mktemp("rr")), True, short_paths=False)


def _ragged_run(grid, g, tag, opts):
    from geoac_amd.api import options
    import geoac_amd as G
    th, ph, params, want, steps_want, sens = RD.ragged_table(g, tag)
    with options(**opts):
        ctx = G.FanContext(EQ, device=0)
        ctx.load_grid(*grid, z_grnd=RD.ragged_load_z_grnd(True))          # -prop loads before any z_grnd= is seen
        ctx.set_params(mode=0, **params)
        rec, steps = ctx.run(th, ph)
        rec = rec.copy(); ctx.close()
    return rec, steps, want, steps_want, sens


def _ragged_variant(grid, g, name):
    if name not in _ragged_runs:
        _ragged_runs[name] = _ragged_run(grid, g, "b_amp1", RAGGED_VARIANTS[name])
    return _ragged_runs[name]


def _ragged_check(tag, what, rec, steps, want, steps_want, E):
    fe = field_errors(rec, want, E, 0)
    print(f"globalrd ragged {tag} {what}: worst error per field: " + ", ".join(f"{f} {np.nanmax(fe[f]):.2e}" for f in sorted(fe)), max_rel_errors(rec, want, E, 0))
    assert steps == steps_want
    compare_records(rec, want, E=E, hidx=0)


@pytest.mark.parametrize("tag", list(RD.RAGGED_TABLES))
def test_ragged_fan_vs_golden(gold_ragged, grid_ragged, tag, time_limit):
    """every table of the fixture under the plan's own kernel: the step total and VALID / STEPS / BROKE of every leg exact, every field compare_records judges within
    1e-6.  The reference's own answer to theta (1 + 1e-12) is in the fixture for every field of every arrival: no exemptions (the generator names the rays it left out)."""
    g = gold_ragged
    rec, steps, want, steps_want, sens = _ragged_run(grid_ragged, g, tag, {})
    assert 4.0 * np.nanmax(sens) <= 1e-6
    if tag == "b_amp1":
        both = np.concatenate([want, RD.ragged_table(g, "a_amp1")[3]])
        assert (both[..., H.REC["VALID"]] > 0).sum() >= 15 and (both[..., H.REC["BROKE"]] > 0).sum() >= 10 and both[..., H.REC["STEPS"]].max() > 15000
        assert (want[g["b_theta"] < 0][..., H.REC["VALID"]] > 0).any()
    _ragged_check(tag, "default", rec, steps, want, steps_want, 18 if RD.RAGGED_TABLES[tag][1]["calc_amp"] else 6)


@pytest.mark.parametrize("variant", list(RAGGED_VARIANTS))
def test_ragged_kernel_variants_vs_golden(gold_ragged, grid_ragged, variant, time_limit):
    """fan b with amplitudes (from 12 km inside the jet, 10 Hz, raised ground) under every kernel the shipped library can select: each against the reference's records"""
    rec, steps, want, steps_want, _ = _ragged_variant(grid_ragged, gold_ragged, variant)
    _ragged_check("b_amp1", variant, rec, steps, want, steps_want, 18)


def test_ragged_variants_that_associate_alike_give_the_same_bits(gold_ragged, grid_ragged, time_limit):
    for group in RAGGED_SAME_BITS:
        first = _ragged_variant(grid_ragged, gold_ragged, group[0])
        for name in group[1:]:
            got = _ragged_variant(grid_ragged, gold_ragged, name)
            assert got[1] == first[1] and np.array_equal(got[0].view(np.uint64), first[0].view(np.uint64)), (group[0], name)


def test_ragged_sixteen_lane_scan_kernel_vs_golden_and_the_four_lane_kernels_bits(gold_ragged, grid_ragged, time_limit):
    """the amplitude-less table of fan b runs on EqGlobalRngDepScan16 by default (test_ragged_fan_vs_golden); HEX=0 keeps it on the four-lane kernel: within
    tolerance of the reference's records too, and the same bits"""
    r16 = _ragged_run(grid_ragged, gold_ragged, "b_amp0", {})
    r4 = _ragged_run(grid_ragged, gold_ragged, "b_amp0", {"HEX": "0"})
    _ragged_check("b_amp0", "hex0", r4[0], r4[1], r4[2], r4[3], 6)
    assert r16[1] == r4[1] and np.array_equal(r16[0].view(np.uint64), r4[0].view(np.uint64))
