"""CPU suite: the plain-C oracle of the range-dependent Cartesian set (bicubic-of-vertical-splines interpolant +
6/18-equation system) against golden vectors generated from the compiled reference (make_golden.py rngdep)."""
import numpy as np
import pytest

import harness as H
import rngdep_data as RD

EQ = H.EQ_3D_RNGDEP


@pytest.fixture(scope="module")
def gold():
    return np.load(f"{H.GOLDEN_DIR}/3drd_small.npz")


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    d = tmp_path_factory.mktemp("gd")
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid(str(d), short_paths=False))          # the oracle takes paths of any length
    return O


def test_grid_interpolant_bitexact(gold, oracle):
    o30, a8 = oracle.grid_probe(gold["probe_x"], gold["probe_y"], gold["probe_z"])
    assert np.array_equal(o30, gold["probe_out30"])          # Eval_Spline_AllOrder2 of T, u, v
    assert np.array_equal(a8, gold["probe_api8"])            # c, rho, u, v, c_diff, u_diff, v_diff (Q11 forms)


@pytest.mark.parametrize("amp,mode", [(1, 0), (0, 0), (1, 3)])
def test_fan_records_bitexact(gold, oracle, amp, mode):
    cfg = H.make_cfg(EQ, bounces=1, calc_amp=bool(amp), mode=mode, src=(0.0, 0.0, 0.0))
    want_smp = (amp == 1 and mode == 3)
    steps, rec, smp, nsmp = oracle.fan(cfg, gold["theta"], gold["phi"], smp_cap=40000 if want_smp else 0)
    tag = f"amp{amp}_mode{mode}"
    assert steps == int(gold[f"steps_{tag}"])
    assert np.array_equal(rec, gold[f"rec_{tag}"])
    if want_smp:
        assert nsmp == int(gold[f"nsmp_{tag}"])
        assert np.array_equal(smp[gold[f"smp_idx_{tag}"]], gold[f"smp_{tag}"])


def test_alt_config_bitexact(gold, oracle):
    """off-centre elevated source, other frequency and absorption scale, tighter box, two bounces (the ground stays at 0: this set tapers the winds around z_grnd
    when it LOADS, and `oracle` loaded with 0)"""
    cfg = H.make_cfg(EQ, bounces=2, calc_amp=True, mode=0, src=(120.0, -60.0, 1.0), freq=0.4, tweak_abs=0.6, xy_limits=(-700.0, 900.0, -600.0, 700.0))
    steps, rec, _, _ = oracle.fan(cfg, gold["theta"], gold["phi"])
    assert steps == int(gold["steps_alt"])
    assert np.array_equal(rec, gold["rec_alt"])


# ---- the ragged 7 x 4 jet grid (rngdep_data.write_grid_ragged; make_golden.py ragged3d): loaded with z_grnd = 0.3 as the set's main does ----
@pytest.fixture(scope="module")
def oracle_ragged(tmp_path_factory):
    O = H.Oracle(EQ, met=None)
    O.load_grid(*RD.write_grid_ragged(str(tmp_path_factory.mktemp("rc")), False, short_paths=False), z_grnd=RD.ragged_load_z_grnd(False))
    return O


def test_ragged_grid_interpolant_bitexact(oracle_ragged):
    g = RD.ragged_fixture(False)
    o30, a8 = oracle_ragged.grid_probe(g["probe_x"], g["probe_y"], g["probe_z"])
    assert np.array_equal(o30, g["probe_out30"]) and np.array_equal(a8, g["probe_api8"])


@pytest.mark.parametrize("tag,rows", [("b_amp1", [15, 17, 19]), ("a_amp1", [1]), ("b_amp0", [9]), ("b_f001", [4])])
def test_ragged_fan_records_bitexact(oracle_ragged, tag, rows):
    """six rays of the fixture's tables (rays are independent; the fixture script ran the oracle on all of them): a ray launched downwards that arrives three
    times, the ducted ray that leaves the grid after 27 080 steps, legs that BREAK at the edge after one and two arrivals, 10 Hz and 0.01 Hz"""
    th, ph, params, want, _, _ = RD.ragged_table(RD.ragged_fixture(False), tag)
    steps, rec, _, _ = oracle_ragged.fan(H.make_cfg(EQ, **params), th[rows], ph[rows])
    assert steps == int(want[rows][..., H.REC["STEPS"]].sum())
    assert np.array_equal(rec, want[rows])
