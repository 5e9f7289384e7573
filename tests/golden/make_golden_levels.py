"""Generates tests/golden/levels_small.npz and tests/golden/levels_legs.npz: level crossings of the COMPILED, UNMODIFIED reference's own rows (oracle/_ref/libref_*.so).

    make -C oracle all && python tests/golden/make_golden_levels.py

For the 3-D and the Global set on ToyAtmo: the six rays of tests/levels_reference.py, every row of leg 0 from the reference's ref_trace_leg0, the
crossing rule of tests/levels_reference.py applied to them at 20, 35 and 110 km, and - from a ref_fan run with mode = 1 (WriteRays) - the travel
times of the two reference sample rows (every 25th step) that bracket each crossing.

Conditioning is a condition here, not a measurement: no ray's turning height on the leg may lie within 0.1 km of a level (the level is moved up by
whole kilometres until that holds, and the levels chosen are part of the fixture), and every segment that crosses must have
|h_{i+1} - h_i| > 1e-6 km.  Counts can then be compared exactly, without exemptions.

levels_legs.npz (main_legs) holds every leg of all four 3-D sets, two bounces: the stratified sets on ToyAtmo with the six inclinations at azimuths -90 and 37,
the range-dependent sets on the ragged 7 x 4 grid with the rays of its table a_amp1 (tests/rngdep_data.py).  Rows and running sums come from the reference's
ref_trace_path (oracle/ref_shim.h): per crossing the leg, direction, segment, FRAC, the interpolated row in all its components, the segment's extent (dab = b - a of the position, single precision: a scale only), and travel time and attenuation
interpolated between the running sums of the segment's two rows.  The set 3d_onrow is the 3-D set once more with two levels placed exactly on a row of the path
(one going up, one going down), for the plain-C oracle alone - its rows are the reference's bit for bit, which is asserted here.
"""
import os
import sys
import tempfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import harness as H  # noqa: E402
import levels_reference as LR  # noqa: E402
import rngdep_data as RD  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LEVELS = [20.0, 35.0, 110.0]
RANGE_LIMIT = 300.0


def main():
    out = {"theta": LR.THETAS, "phi": np.float64(LR.PHI), "range_limit": np.float64(RANGE_LIMIT)}
    for eq in (H.EQ_3D, H.EQ_GLOBAL):
        name = H.EQ_NAMES[eq]
        R = H.RefShim(eq)
        cfg = H.make_cfg(eq, bounces=0, calc_amp=True, range_limit=RANGE_LIMIT)
        traces = [R.trace_leg0(cfg, float(t), LR.PHI) for t in LR.THETAS]
        turn = np.array([LR.turning_height(eq, rows) for _, rows in traces])
        levels = []
        for z in LEVELS:
            while (np.abs(turn - z) <= 0.1).any() or z in levels:
                z += 1.0
            levels.append(z)
        assert all(b > a for a, b in zip(levels, levels[1:])), levels
        # sample rows of the reference (every 25th step) and its arrival records
        th, ph = LR.THETAS, np.full(len(LR.THETAS), LR.PHI)
        _, rec, _, _ = R.fan(cfg, th, ph)
        cfg_s = H.make_cfg(eq, bounces=0, calc_amp=True, mode=H.MODE_WRITE_RAYS, range_limit=RANGE_LIMIT)
        _, _, smp, nsmp = R.fan(cfg_s, th, ph, smp_cap=40000)
        assert nsmp == len(smp)
        ray, level, direc, seg, frac, a, b, row, t_lo, t_hi = ([] for _ in range(10))
        count = np.zeros((len(th), len(levels)), dtype=np.int32)
        for r, (k, rows) in enumerate(traces):
            h = rows[:, LR.hidx(eq)]
            mine = smp[(smp[:, 0] == r) & (smp[:, 1] == 0) & (smp[:, 3] == 0)]
            m_s, t_s = mine[:, 2].astype(int), mine[:, 4 + 5]
            for c in LR.crossings(eq, rows, levels):
                i = c["seg"]
                assert abs(h[i + 1] - h[i]) > 1e-6, (name, r, i)
                below, above = m_s <= i, m_s >= i + 1
                t_lo.append(t_s[below].max() if below.any() else 0.0)
                valid = rec[r, 0, H.REC["VALID"]] > 0
                t_hi.append(t_s[above].min() if above.any() else (rec[r, 0, H.REC["TTIME"]] if valid else np.inf))
                ray.append(r); level.append(c["level"]); direc.append(c["dir"]); seg.append(i); frac.append(c["frac"])
                a.append(c["a"]); b.append(c["b"]); row.append(c["row"])
                count[r, c["level"]] += 1
        assert count.sum() > 0 and (count >= 2).any()
        out[f"{name}_levels"] = np.array(levels)
        out[f"{name}_turn"] = turn
        out[f"{name}_k"] = np.array([k for k, _ in traces], dtype=np.int64)
        out[f"{name}_count"] = count
        for key, v, dt in (("ray", ray, np.int32), ("level", level, np.int32), ("dir", direc, np.int32), ("seg", seg, np.int32), ("frac", frac, np.float64),
                           ("a", a, np.float64), ("b", b, np.float64), ("row", row, np.float64), ("t_lo", t_lo, np.float64), ("t_hi", t_hi, np.float64)):
            out[f"{name}_{key}"] = np.array(v, dtype=dt)
        print(name, "levels", levels, "turning heights", np.round(turn, 3), "counts", count.tolist())
    path = os.path.join(OUT, "levels_small.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


# ---------------------------------------------------------------- levels_legs.npz
def _legs_inputs(name):
    """(reference, oracle, theta, phi, cfg keywords, range-dependent?) of a set of levels_legs.npz"""
    eq = LR.LEGS_SETS[name]
    if eq in (H.EQ_3D, H.EQ_GLOBAL):
        th, ph = np.tile(LR.THETAS, 2), np.repeat([LR.PHI, 37.0], len(LR.THETAS))
        return H.RefShim(eq), H.Oracle(eq), th, ph, dict(bounces=2, calc_amp=True), False
    glob = eq == H.EQ_GLOBAL_RNGDEP
    grid = RD.write_grid_ragged(os.path.join(tempfile.gettempdir(), "rg" if glob else "rc"), glob)      # as make_golden.py ragged3d / raggedglobal load it
    zl = RD.ragged_load_z_grnd(glob)
    R = H.RefShim(eq, grid=grid, z_grnd=zl)
    O = H.Oracle(eq, met=None); O.load_grid(*grid, z_grnd=zl)
    th, ph, params, _, _, _ = RD.ragged_table(RD.ragged_fixture(glob), "a_amp1")
    assert params["bounces"] == 2
    return R, O, th, ph, dict(bounces=2, calc_amp=bool(params["calc_amp"]), src=params["src"], z_grnd=params["z_grnd"]), True


def _condition(eq, paths, wanted):
    """the levels moved up by whole kilometres until no leg's turning height lies within 0.1 km of one"""
    turn = np.array([LR.turning_height(eq, rows) for legs in paths for _, rows, _ in legs])
    levels = []
    for z in wanted:
        while (np.abs(turn - z) <= 0.1).any() or (levels and z <= levels[-1]):
            z += 1.0
        levels.append(z)
    assert all(b > a for a, b in zip(levels, levels[1:])), levels
    return levels, turn


def _crossing_arrays(eq, name, paths, levels):
    """the per-crossing content of a set, ray by ray, leg by leg, in path order"""
    pw = LR.PATHW[eq]
    cols = {k: [] for k in ("ray", "level", "leg", "dir", "seg", "frac", "dab", "row", "ttime", "atten")}
    count = np.zeros((len(paths), len(levels)), dtype=np.int32)
    for r, legs in enumerate(paths):
        for j, (k, rows, sums) in enumerate(legs):
            h = rows[:, LR.hidx(eq)]
            for c in LR.crossings(eq, rows, levels):
                i, f = c["seg"], c["frac"]
                assert abs(h[i + 1] - h[i]) > 1e-6, (name, r, j, i)
                cols["ray"].append(r); cols["level"].append(c["level"]); cols["leg"].append(j); cols["dir"].append(c["dir"]); cols["seg"].append(i)
                cols["frac"].append(f); cols["dab"].append((c["b"] - c["a"])[:3]); cols["row"].append(c["row"])
                cols["ttime"].append(sums[i, 0] + f * (sums[i + 1, 0] - sums[i, 0]))
                cols["atten"].append(sums[i, 1] + f * (sums[i + 1, 1] - sums[i, 1]))
                count[r, c["level"]] += 1
    out = {f"{name}_{k}": np.array(v, dtype=np.float64 if k in ("frac", "row", "ttime", "atten") else np.float32 if k == "dab" else np.int32) for k, v in cols.items()}
    assert out[f"{name}_row"].shape == (count.sum(), pw) and (out[f"{name}_ttime"] > 0).all() and (out[f"{name}_atten"] > 0).all()
    out[f"{name}_levels"] = np.array(levels)
    out[f"{name}_count"] = count
    out[f"{name}_cap_needed"] = np.int64(count.max())
    assert count.max() <= 64, (name, count.max())
    return out


def _legs_set(name):
    eq = LR.LEGS_SETS[name]
    R, O, th, ph, kw, rngdep = _legs_inputs(name)
    range_limit = RANGE_LIMIT
    while True:
        cfg = H.make_cfg(eq, **kw) if rngdep else H.make_cfg(eq, range_limit=range_limit, **kw)
        paths = [R.trace_path(cfg, t, p) for t, p in zip(th, ph)]
        levels, turn = _condition(eq, paths, LEVELS)
        out = _crossing_arrays(eq, name, paths, levels)
        leg = out[f"{name}_leg"]
        if (leg >= 1).sum() >= 6 and (leg == 2).any():
            break
        assert not rngdep, (name, "too few crossings behind a bounce, and the grid sets have no range limit to widen")
        range_limit += 100.0
    # guard: the running sums at every leg's last row are ref_fan's arrivals-only TTIME / ATTEN (another order of the same additions: the difference is recorded)
    _, rec, _, _ = R.fan(cfg, th, ph)
    diff = 0.0
    for r, legs in enumerate(paths):
        assert len(legs) == int((rec[r, :, H.REC["STEPS"]] > 0).sum())
        for j, (k, rows, sums) in enumerate(legs):
            assert abs(k) == rec[r, j, H.REC["STEPS"]] and (k < 0) == (rec[r, j, H.REC["BROKE"]] > 0), (name, r, j)
            for q, f in enumerate(("TTIME", "ATTEN")):
                diff = max(diff, abs(sums[-1, q] / rec[r, j, H.REC[f]] - 1.0))
    assert diff <= 1e-12, (name, diff)
    # guard: leg 0 is ref_trace_leg0's, bit for bit
    cfg0 = H.make_cfg(eq, **dict(kw, bounces=0)) if rngdep else H.make_cfg(eq, range_limit=range_limit, **dict(kw, bounces=0))
    for legs, t, p in zip(paths, th, ph):
        k0, rows0 = R.trace_leg0(cfg0, float(t), float(p))
        assert k0 == legs[0][0] and np.array_equal(rows0, legs[0][1]), (name, t, p)
    out.update({f"{name}_theta": th, f"{name}_phi": ph, f"{name}_sum_diff": np.float64(diff), f"{name}_turn": turn,
                f"{name}_k": np.array([[legs[j][0] if j < len(legs) else 0 for j in range(3)] for legs in paths], dtype=np.int64)})
    if rngdep:
        out[f"{name}_src"] = np.array(kw["src"]); out[f"{name}_z_grnd"] = np.float64(kw["z_grnd"])
    else:
        out[f"{name}_range_limit"] = np.float64(range_limit)
    line = (f"{name}: levels {levels}, {len(leg)} crossings, {int((leg == 1).sum())} on leg 1, {int((leg == 2).sum())} on leg 2, cap needed {int(out[f'{name}_cap_needed'])}, "
            f"sums against ref_fan's within {diff:.1e}" + ("" if rngdep else f", range limit {range_limit:g} km"))
    if name == "3d":
        # two levels exactly on a row of ray 2's first leg, one row going up and one going down; for the oracle, whose rows are these bit for bit
        opaths = [O.trace_path(cfg, t, p) for t, p in zip(th, ph)]
        for legs, olegs in zip(paths, opaths):
            assert len(legs) == len(olegs) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(legs, olegs))
        z = paths[2][0][1][:, 2]
        top = int(np.argmax(z))
        ok = lambda v: (np.abs(turn - v) > 0.1).all() and min(abs(v - l) for l in levels) > 0.5      # noqa: E731
        i_up = next(i for i in range(1, top) if z[i] > 27.0 and ok(z[i]))
        i_dn = next(i for i in range(top + 1, len(z) - 1) if z[i] < 13.0 and ok(z[i]))
        on = sorted(levels + [float(z[i_up]), float(z[i_dn])])
        extra = _crossing_arrays(eq, "3d_onrow", paths, on)
        hit = (extra["3d_onrow_ray"] == 2) & (extra["3d_onrow_leg"] == 0) & np.isin(extra["3d_onrow_frac"], (0.0, 1.0))
        assert hit.sum() == 2 and sorted(extra["3d_onrow_seg"][hit]) == sorted([i_up - 1, i_dn]), (i_up, i_dn, extra["3d_onrow_seg"][hit])
        extra.update({"3d_onrow_theta": th, "3d_onrow_phi": ph, "3d_onrow_range_limit": np.float64(range_limit), "3d_onrow_rows": np.array([i_up, i_dn])})
        out.update(extra)
        line += f"; 3d_onrow: levels {on}"
    return out, line


def main_legs():
    out = {}
    with ProcessPoolExecutor(len(LR.LEGS_SETS)) as pool:           # (a process per set: the reference keeps its state in globals, and the grid sets take minutes)
        for part, line in pool.map(_legs_set, list(LR.LEGS_SETS)):
            out.update(part)
            print(line)
    path = os.path.join(OUT, "levels_legs.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
    main_legs()
