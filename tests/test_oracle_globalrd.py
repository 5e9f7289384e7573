"""CPU suite: the plain-C oracle of the range-dependent spherical set (GeoAcGlobal.RngDep: lat/lon grid of vertical splines,
quirks Q12 kept) against golden vectors generated from the compiled reference (make_golden.py globalrd)."""
import numpy as np
import pytest

import harness as H
import rngdep_data as RD

EQ = H.EQ_GLOBAL_RNGDEP


@pytest.fixture(scope="module")
def gold():
    return np.load(f"{H.GOLDEN_DIR}/globalrd_small.npz")


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    d = tmp_path_factory.mktemp("gg")
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid_global(str(d), short_paths=False))
    return O


def test_grid_interpolant_bitexact(gold, oracle):
    o30, a8 = oracle.grid_probe(gold["probe_r"], gold["probe_lat"], gold["probe_lon"])
    assert np.array_equal(o30, gold["probe_out30"])          # Eval_Spline_AllOrder2 of T, u, v
    assert np.array_equal(a8, gold["probe_api8"])            # c, rho, u, v, c_diff(r), u_diff(r), v_diff(r), c_diff(lat)


@pytest.mark.parametrize("amp,mode", [(1, 0), (0, 0), (1, 3)])
def test_fan_records_bitexact(gold, oracle, amp, mode):
    cfg = H.make_cfg(EQ, bounces=1, calc_amp=bool(amp), mode=mode, src=(0.0, 31.0, 0.0))
    want_smp = (amp == 1 and mode == 3)
    steps, rec, smp, nsmp = oracle.fan(cfg, gold["theta"], gold["phi"], smp_cap=40000 if want_smp else 0)
    tag = f"amp{amp}_mode{mode}"
    assert steps == int(gold[f"steps_{tag}"])
    assert np.array_equal(rec, gold[f"rec_{tag}"])
    if want_smp:
        assert nsmp == int(gold[f"nsmp_{tag}"])
        assert np.array_equal(smp[gold[f"smp_idx_{tag}"]], gold[f"smp_{tag}"])


def test_alt_config_bitexact(gold):
    """fresh context: the grid is loaded with the z_grnd the fan then uses (what -interactive / -eig_* do)"""
    import tempfile, os
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid_global(os.path.join(tempfile.mkdtemp(), "a"), short_paths=False), z_grnd=0.0)
    cfg = H.make_cfg(EQ, bounces=2, calc_amp=True, mode=0, src=(1.5, 29.0, 1.0), z_grnd=0.3, freq=0.4, tweak_abs=0.6,
                     xy_limits=tuple(np.radians([26.0, 36.5, -7.0, 6.0])))
    steps, rec, _, _ = O.fan(cfg, gold["theta"], gold["phi"])
    assert steps == int(gold["steps_alt"])
    assert np.array_equal(rec, gold["rec_alt"])


def test_polar_grid_bitexact(tmp_path):
    """the grid whose rows lie at 82 .. 89.5 N (rngdep_data.POLAR_GRID; make_golden.py globalrd_polar): interpolant and fan records of the compiled reference"""
    g = np.load(f"{H.GOLDEN_DIR}/globalrd_polar.npz")
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid_global(str(tmp_path), short_paths=False, **RD.POLAR_GRID))
    o30, a8 = O.grid_probe(g["probe_r"], g["probe_lat"], g["probe_lon"])
    assert np.array_equal(o30, g["probe_out30"]) and np.array_equal(a8, g["probe_api8"])
    cfg = H.make_cfg(EQ, bounces=1, calc_amp=True, mode=0, src=tuple(g["src"]))
    rows = np.array([2, 9, 18, 25, 31])          # a ray per direction (the fixture script ran the oracle on all 35): arrivals at 89.3 N and 82.1 N, short tropospheric legs
    steps, rec, _, _ = O.fan(cfg, g["theta"][rows], g["phi"][rows])
    assert steps == int(g["rec_amp1"][rows][..., H.REC["STEPS"]].sum())
    assert np.array_equal(rec, g["rec_amp1"][rows])


def test_default_grid_files_are_unchanged(tmp_path):
    """write_grid_global without a centre latitude writes the node files the mid-latitude fixtures were made from"""
    _, loclat, loclon = RD.write_grid_global(str(tmp_path), short_paths=False)
    assert open(loclat).read() == "25\n28\n31\n34\n37\n" and open(loclon).read() == "-8\n-4\n0\n4\n8\n"


# ---- the ragged 7 x 4 jet grid (rngdep_data.write_grid_ragged; make_golden.py raggedglobal): loaded with z_grnd = 0 as -prop does, the ground raised afterwards ----
@pytest.fixture(scope="module")
def oracle_ragged(tmp_path_factory):
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid_ragged(str(tmp_path_factory.mktemp("rg")), True, short_paths=False), z_grnd=RD.ragged_load_z_grnd(True))
    return O


def test_ragged_grid_interpolant_bitexact(oracle_ragged):
    g = RD.ragged_fixture(True)
    o30, a8 = oracle_ragged.grid_probe(g["probe_r"], g["probe_lat"], g["probe_lon"])
    assert np.array_equal(o30, g["probe_out30"]) and np.array_equal(a8, g["probe_api8"])


@pytest.mark.parametrize("tag,rows", [("b_amp1", [15, 16, 19]), ("a_amp1", [0]), ("b_amp0", [17]), ("b_f001", [4])])
def test_ragged_fan_records_bitexact(oracle_ragged, tag, rows):
    """six rays of the fixture's tables (rays are independent; the fixture script ran the oracle on all of them): a ray launched downwards that arrives three
    times, legs that BREAK at the edge after one and two arrivals (one after 18 017 steps), 10 Hz and 0.01 Hz"""
    th, ph, params, want, _, _ = RD.ragged_table(RD.ragged_fixture(True), tag)
    steps, rec, _, _ = oracle_ragged.fan(H.make_cfg(EQ, **params), th[rows], ph[rows])
    assert steps == int(want[rows][..., H.REC["STEPS"]].sum())
    assert np.array_equal(rec, want[rows])
