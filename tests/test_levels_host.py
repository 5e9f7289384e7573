"""CPU suite for level crossings (include/geoac_levels.h): the crossing rule of tests/levels_reference.py on the plain-C oracle's rows against the
fixture made from the compiled reference's rows (tests/golden/levels_small.npz, tests/golden/make_golden_levels.py); the numpy restatement of k_levels
on every leg of the oracle's paths against the reference's crossings, times and attenuations of all four sets (tests/golden/levels_legs.npz), with five
deliberately wrong restatements that the comparison must refuse; and the validation of a level list through the ABI's host-only check - no device is
needed for any of it."""
import ctypes
import os

import numpy as np
import pytest

import harness as H
import levels_reference as LR
import rngdep_data as RD

import geoac_amd as G


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(G.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return G.load_library()


@pytest.fixture(scope="module")
def fixture():
    return np.load(LR.FIXTURE)


def test_fixture_is_conditioned(fixture):
    """what make_golden_levels.py asserts when it writes the fixture, read back: no turning height within 0.1 km of a level, no flat crossing segment"""
    for eq in (H.EQ_3D, H.EQ_GLOBAL):
        name = H.EQ_NAMES[eq]
        lev = fixture[f"{name}_levels"]
        assert len(lev) == 3 and (np.diff(lev) > 0).all() and (lev == np.round(lev)).all()
        assert (np.abs(fixture[f"{name}_turn"][:, None] - lev[None, :]) > 0.1).all()
        hi = LR.hidx(eq)
        assert (np.abs(fixture[f"{name}_b"][:, hi] - fixture[f"{name}_a"][:, hi]) > 1e-6).all()
        assert (fixture[f"{name}_count"] >= 2).any() and len(fixture[f"{name}_ray"]) == fixture[f"{name}_count"].sum()
        assert (fixture[f"{name}_t_lo"] <= fixture[f"{name}_t_hi"]).all()


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL])
def test_restatement_on_oracle_rows_gives_the_fixture(fixture, eq):
    """counts and directions exactly, FRAC-interpolated positions within 1e-6 relative (LR.position_errors)"""
    name = H.EQ_NAMES[eq]
    lev = fixture[f"{name}_levels"]
    O = H.Oracle(eq)
    cfg = H.make_cfg(eq, bounces=0, calc_amp=True, range_limit=float(fixture["range_limit"]))
    by = LR.fixture_rays(fixture, name)
    worst = 0.0
    for r, th in enumerate(fixture["theta"]):
        k, rows = O.trace_leg0(cfg, float(th), float(fixture["phi"]))
        assert k == fixture[f"{name}_k"][r]
        groups = LR.per_level(LR.crossings(eq, rows, lev), len(lev))
        for l, cr in enumerate(groups):
            idx = by.get((r, l), [])
            assert len(cr) == fixture[f"{name}_count"][r, l] == len(idx), (r, l)
            if not cr:
                continue
            assert [c["dir"] for c in cr] == list(fixture[f"{name}_dir"][idx]), (r, l)
            err = LR.position_errors(eq, np.array([c["row"] for c in cr]), fixture[f"{name}_row"][idx])
            worst = max(worst, float(err.max()))
    print(f"{name}: largest position error of the oracle's crossings against the reference's {worst:.3e}")
    assert worst <= 1e-6


# ---------------------------------------------------------------- every leg, four sets (tests/golden/levels_legs.npz)
@pytest.fixture(scope="module")
def legs_fixture():
    return np.load(LR.LEGS_FIXTURE)


_paths = {}


def _oracle_paths(name, g, tmp_path_factory):
    """every leg of the fixture's rays from the plain-C oracle's orc_trace_path, traced once per set and shared (read-only)"""
    eq = LR.LEGS_SETS[name]
    if name not in _paths:
        th, ph = g[f"{name}_theta"], g[f"{name}_phi"]
        if eq in (H.EQ_3D, H.EQ_GLOBAL):
            O = H.Oracle(eq)
            cfg = H.make_cfg(eq, bounces=2, calc_amp=True, range_limit=float(g[f"{name}_range_limit"]))
        else:
            glob = eq == H.EQ_GLOBAL_RNGDEP
            O = H.Oracle(eq, met=None)
            O.load_grid(*RD.write_grid_ragged(str(tmp_path_factory.mktemp("ragged")), glob, short_paths=False), z_grnd=RD.ragged_load_z_grnd(glob))
            cfg = H.make_cfg(eq, bounces=2, calc_amp=True, src=tuple(g[f"{name}_src"]), z_grnd=float(g[f"{name}_z_grnd"]))
        _paths[name] = [O.trace_path(cfg, t, p) for t, p in zip(th, ph)]
        for legs in _paths[name]:
            for _, rows, sums in legs:
                rows.setflags(write=False); sums.setflags(write=False)
    return _paths[name]


def test_legs_fixture_is_conditioned(legs_fixture):
    """what make_golden_levels.py asserts when it writes levels_legs.npz, read back"""
    g = legs_fixture
    for name, eq in list(LR.LEGS_SETS.items()) + [("3d_onrow", H.EQ_3D)]:
        lev, leg = g[f"{name}_levels"], g[f"{name}_leg"]
        assert (np.diff(lev) > 0).all() and int(g[f"{name}_cap_needed"]) == g[f"{name}_count"].max() <= 64
        assert len(leg) == g[f"{name}_count"].sum() and (leg >= 1).sum() >= 6 and (leg == 2).any()
        assert (np.abs(g[f"{name}_dab"][:, LR.hidx(eq)]) > 1e-6).all()
        assert g[f"{name}_row"].shape == (len(leg), LR.PATHW[eq]) and (g[f"{name}_ttime"] > 0).all() and (g[f"{name}_atten"] > 0).all()
        if name != "3d_onrow":
            assert len(lev) == 3 and (lev == np.round(lev)).all()
            assert (np.abs(g[f"{name}_turn"][:, None] - lev[None, :]) > 0.1).all() and float(g[f"{name}_sum_diff"]) <= 1e-12
    on = g["3d_onrow_frac"]
    assert ((on == 0.0) | (on == 1.0)).sum() == 2


@pytest.mark.parametrize("name", list(LR.LEGS_SETS) + ["3d_onrow"])
def test_restatement_on_oracle_paths_gives_the_legs_fixture(legs_fixture, tmp_path_factory, name):
    """restate_k_levels on the oracle's rows and running sums, through the comparison the GPU suite puts k_levels through"""
    eq = LR.LEGS_SETS[name.split("_")[0]]
    paths = _oracle_paths(name.split("_")[0], legs_fixture, tmp_path_factory)
    cap = int(legs_fixture[f"{name}_cap_needed"])
    count, lrec = LR.restate_fan(eq, paths, legs_fixture[f"{name}_levels"], cap)
    LR.compare_with_fixture(eq, count, lrec, legs_fixture, name=name)


@pytest.mark.parametrize("mutation", LR.MUTATIONS)
def test_comparison_refuses_a_wrong_restatement(legs_fixture, tmp_path_factory, mutation):
    """each deliberately wrong k_levels (LR.MUTATIONS) fails compare_with_fixture on every set.  The swapped up rule differs from the right one only where
    a row lies exactly on a level, so it is put to the set that has such rows (3d_onrow: FRAC 1.0 in the segment before becomes 0.0 in the one after)."""
    for name in (["3d_onrow"] if mutation == "up_rule_swapped" else list(LR.LEGS_SETS)):
        eq = LR.LEGS_SETS[name.split("_")[0]]
        paths = _oracle_paths(name.split("_")[0], legs_fixture, tmp_path_factory)
        count, lrec = LR.restate_fan(eq, paths, legs_fixture[f"{name}_levels"], int(legs_fixture[f"{name}_cap_needed"]), mutate=mutation)
        with pytest.raises(AssertionError) as why:
            LR.compare_with_fixture(eq, count, lrec, legs_fixture, name=name)
        print(name, mutation, "refused:", why.value.args[0] if why.value.args else why.value)


def test_restatement_counts_a_row_on_a_level_once():
    """the half-open intervals: a row lying exactly on a level belongs to the segment that arrives at it going up, and to the one that leaves it going down"""
    rows = np.zeros((7, 4))
    rows[:, 2] = [0.0, 1.0, 2.0, 1.0, 1.0, 0.5, 1.0]
    rows[:, 0] = np.arange(7.0)
    cr = LR.crossings(H.EQ_3D, rows, [1.0, 2.0])
    got = [(c["level"], c["seg"], c["dir"], c["frac"]) for c in cr]
    assert got == [(0, 0, 1, 1.0), (1, 1, 1, 1.0), (1, 2, -1, 0.0), (0, 4, -1, 0.0), (0, 5, 1, 1.0)]
    assert np.array_equal(cr[3]["row"], rows[4, :4]) and np.array_equal(cr[0]["row"], rows[1, :4])


def test_k_levels_uses_no_scratch(lib):
    """the compiler's own resource report of the shipped build (csrc/Makefile, -Rpass-analysis=kernel-resource-usage): one instantiation per level count,
    none of them with scratch memory or spilled vector registers"""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "geoac_amd", "csrc", "build", "geoac_levels.hip.resource_usage.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(root, "geoac_amd", "csrc"), "ARCH=gfx950"])
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"remark: .*?(Function Name|VGPRs Spill|ScratchSize \[bytes/lane\]): (\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    rows = [r for r in rows if "k_levels" in r["name"]]
    assert len(rows) == G.MAX_LEVELS
    assert all(r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 for r in rows), rows


def _check(lib, eq, z, cap=8, **kw):
    p = G.default_params(eq)
    for k, v in kw.items():
        setattr(p, k, v)
    z = np.ascontiguousarray(z, dtype=np.float64)
    fault = ctypes.c_char_p()
    rc = lib.geoac_levels_check(int(eq), ctypes.byref(p), len(z), z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(cap), ctypes.byref(fault))
    return rc, (fault.value or b"").decode()


E_INVALID, E_UNSUPPORTED = -1, -4


def test_error_codes_are_the_headers(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "geoac_hip.h")).read()
    import re
    codes = dict(re.findall(r"(GEOAC_E_[A-Z]+)\s*=\s*(-?\d+)", txt))
    assert int(codes["GEOAC_E_INVALID"]) == E_INVALID and int(codes["GEOAC_E_UNSUPPORTED"]) == E_UNSUPPORTED


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_GLOBAL, H.EQ_3D_RNGDEP, H.EQ_GLOBAL_RNGDEP])
def test_level_list_validation(lib, eq):
    sph = eq in (H.EQ_GLOBAL, H.EQ_GLOBAL_RNGDEP)
    top = 6370.0 + 140.0 if sph else 140.0
    assert _check(lib, eq, [20.0, 35.0, 110.0], vert_limit=top) == (0, "")
    assert _check(lib, eq, [], vert_limit=top) == (0, "")                            # 0 levels: leaves the mode
    assert _check(lib, eq, [20.0], cap=0) == (0, "")                                 # cap 0: the default
    assert _check(lib, eq, [20.0], cap=64) == (0, "")
    rc, why = _check(lib, eq, [35.0, 20.0])
    assert rc == E_INVALID and "ascending" in why
    rc, why = _check(lib, eq, [20.0, 20.0])
    assert rc == E_INVALID and "ascending" in why
    rc, why = _check(lib, eq, [0.3, 20.0], z_grnd=0.3)
    assert rc == E_INVALID and "z_grnd" in why
    rc, why = _check(lib, eq, [0.2, 20.0], z_grnd=0.3)
    assert rc == E_INVALID and "z_grnd" in why
    rc, why = _check(lib, eq, np.arange(1.0, 10.0))
    assert rc == E_INVALID and "n_levels" in why
    rc, why = _check(lib, eq, [20.0], cap=65)
    assert rc == E_INVALID and "cap" in why
    rc, why = _check(lib, eq, [20.0], cap=-1)
    assert rc == E_INVALID and "cap" in why
    rc, why = _check(lib, eq, [20.0, np.nan])
    assert rc == E_INVALID and "finite" in why
    rc, why = _check(lib, eq, [20.0, np.inf])
    assert rc == E_INVALID and "finite" in why
    rc, why = _check(lib, eq, [20.0, 140.0], vert_limit=top)
    assert rc == E_INVALID and "vertical limit" in why
    assert _check(lib, eq, [20.0, 139.9], vert_limit=top)[0] == 0
    assert _check(lib, eq, [20.0, 500.0], vert_limit=float("nan"))[0] == 0           # (no atmosphere yet: the launch checks again)


def test_two_d_set_is_refused(lib):
    rc, why = _check(lib, H.EQ_2D, [20.0])
    assert rc == E_UNSUPPORTED and "2-D" in why
    with pytest.raises(G.GeoAcError, match="2-D"):
        G.levels_check(G.EQ_2D, G.default_params(G.EQ_2D), [20.0])


def test_python_check_raises_with_the_fault(lib):
    p = G.default_params(G.EQ_3D)
    G.levels_check(G.EQ_3D, p, [10.0, 30.0], cap=4)
    with pytest.raises(G.GeoAcError, match="strictly ascending"):
        G.levels_check(G.EQ_3D, p, [30.0, 10.0])
