"""Generates tests/golden/levels_small.npz: level crossings of the COMPILED, UNMODIFIED reference's own rows (oracle/_ref/libref_*.so).

    make -C oracle all && python tests/golden/make_golden_levels.py

For the 3-D and the Global set on ToyAtmo: the six rays of tests/levels_reference.py, every row of leg 0 from the reference's ref_trace_leg0, the
crossing rule of tests/levels_reference.py applied to them at 20, 35 and 110 km, and - from a ref_fan run with mode = 1 (WriteRays) - the travel
times of the two reference sample rows (every 25th step) that bracket each crossing.

Conditioning is a condition here, not a measurement: no ray's turning height on the leg may lie within 0.1 km of a level (the level is moved up by
whole kilometres until that holds, and the levels chosen are part of the fixture), and every segment that crosses must have
|h_{i+1} - h_i| > 1e-6 km.  Counts can then be compared exactly, without exemptions.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import harness as H  # noqa: E402
import levels_reference as LR  # noqa: E402

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


if __name__ == "__main__":
    main()
