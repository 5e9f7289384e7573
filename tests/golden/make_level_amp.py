"""Generates tests/golden/level_amp.npz: ray-tube amplitudes at receiver altitudes from the COMPILED, UNMODIFIED reference's own rows
(oracle/_ref/libref_*.so), beside the reference's own Jacobian amplitude at the same crossings.

    make -C oracle all && python tests/golden/make_level_amp.py

Per set a few rays; per ray the fan of include/geoac_level_amp.h - the ray, its theta probe and its phi probe - at h = 0.02 and h = 0.04 degrees, every
row of every leg from ref_trace_path, the crossings by the rule of tests/levels_reference.py, the medium from ref_atmo_probe /
ref_grid_probe, and the header's arithmetic from tests/level_amp_reference.py.  Every passage of a base ray through a level is a fixture crossing, named by
(ray, level, leg, dir, ord).  Beside the tube's DET, TZ, D, AMP:
  amp_jac      GeoAc_Amplitude of the calc_amp = 1 state row interpolated at the crossing's FRAC, as the reference computes it (its own D, quirk Q3 on the
               spherical sets: dp_ds over r sin(lat))
  amp_jac_cos  spherical sets only: the same with Q3's sin replaced by cos, the metric's factor.  THIS is the one the tube is compared with: the term
               drops out of a fixed-level determinant, so the tube cannot reproduce Q3 (include/geoac_level_amp.h)
  fd_sens      |AMP' / AMP - 1| of the tube at h = 0.02 with theta (1 + 1e-12) on all three rays: what a rounding of the launch angle does to it

Cap (a condition, not a measurement): every fixture crossing has |AMP_tube / AMP_jacobian - 1| <= 2e-2 at h = 0.02.  Crossings the reference itself puts
beyond it - a caustic between the probes - are left out BY NAME in LEFT_OUT below, at most 10 % of a set's; the maker fails on a crossing beyond the cap
that is not named, on a name that is within it, and on a set that leaves out more than 10 %.  The plain-C oracle's paths are asserted equal to the reference's
bit for bit, and the numpy amplitude used for amp_jac is held to the reference's own GEOAC_REC_AMP at every ground arrival of the base rays (1e-9).

GEOAC_EQ_GLOBAL_RNGDEP is not in the fixture: the library refuses the set (include/geoac_level_amp.h).  `--scan 3drd` / `--scan globalrd` run the same arithmetic
over ALL rays of table a_amp1 on the ragged grid at h = 0.02 and 0.04 and write profiles/level_amp_scan_<set>.txt: the figures DESIGN 8p quotes for the two media.
"""
import os
import sys
import tempfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import harness as H  # noqa: E402
import level_amp_reference as LA  # noqa: E402
import levels_reference as LV  # noqa: E402
import rngdep_data as RD  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LEVELS = [20.0, 35.0]
STEPS = (0.02, 0.04)
CAP = 2e-2
CAP_LVL = 16
SETS = {"3d": H.EQ_3D, "global": H.EQ_GLOBAL, "3drd": H.EQ_3D_RNGDEP}
SCAN_SETS = {"3drd": H.EQ_3D_RNGDEP, "globalrd": H.EQ_GLOBAL_RNGDEP}
# crossings beyond the cap in the reference itself: (theta, phi, level [km], leg, dir, ord)
LEFT_OUT = {
    "3d": [],
    "global": [],
    "3drd": [(15.0, 35.0, 20.0, 0, -1, 0)],          # gap 3.0e-2: 1 of 16
}
LEFT_OUT_SHARE = 0.1


def _inputs(name, whole_table=False):
    """(reference, oracle, theta, phi, cfg keywords, src3, z_grnd) of a set.  The grid sets: three rays of table a_amp1 - its first, its middle and its last
    (a rule that does not look at what the rays give; the first turns below 20 km on the Cartesian grid and adds no crossing) - or the whole table"""
    eq = SCAN_SETS.get(name, SETS.get(name))
    if eq == H.EQ_3D:
        th, ph = np.tile([16.0, 24.0, 30.0, 38.0], 2), np.repeat([-90.0, 37.0], 4)
        return H.RefShim(eq), H.Oracle(eq), th, ph, dict(bounces=1, calc_amp=True), (0.0, 0.0, 0.0), 0.0
    if eq == H.EQ_GLOBAL:
        th, ph = np.tile([5.0, 12.0, 20.0, 30.0], 2), np.repeat([-90.0, 37.0], 4)
        return H.RefShim(eq), H.Oracle(eq), th, ph, dict(bounces=1, calc_amp=True, src=(0.0, 30.0, 0.0)), (0.0, 30.0, 0.0), 0.0
    glob = eq == H.EQ_GLOBAL_RNGDEP
    grid = RD.write_grid_ragged(os.path.join(tempfile.gettempdir(), "ag" if glob else "ac"), glob)
    zl = RD.ragged_load_z_grnd(glob)
    R = H.RefShim(eq, grid=grid, z_grnd=zl)
    O = H.Oracle(eq, met=None); O.load_grid(*grid, z_grnd=zl)
    th, ph, params, _, _, _ = RD.ragged_table(RD.ragged_fixture(glob), "a_amp1")
    pick = np.arange(len(th)) if whole_table else np.array([0, len(th) // 2, len(th) - 1])
    return R, O, th[pick], ph[pick], dict(bounces=1, calc_amp=True, src=params["src"], z_grnd=params["z_grnd"]), tuple(params["src"]), float(params["z_grnd"])


def _jacobian_D(eq, y, m, cos_metric):
    """GeoAc_Jacobian of full state rows y [n][E] (3DStratified.cpp:410-451, 3DRngDep.cpp:547-592, Global.cpp:594-607) with the medium m at the row;
    the stratified Cartesian set's group velocity needs nu_x, nu_y of the ray: they come in as y's last two columns"""
    c, u, v, _ = m
    if eq == H.EQ_3D:
        nx, ny, nz = y[:, -2], y[:, -1], y[:, 3]
        nu = y[:, -3]
        g = np.stack([c * nx / nu + u, c * ny / nu + v, c * nz / nu], axis=1)
        t = g / np.linalg.norm(g, axis=1, keepdims=True)
        return t[:, 0] * (y[:, 5] * y[:, 10] - y[:, 9] * y[:, 6]) - y[:, 4] * (t[:, 1] * y[:, 10] - t[:, 2] * y[:, 9]) + y[:, 8] * (t[:, 1] * y[:, 6] - t[:, 2] * y[:, 5])
    n = y[:, 3:6]
    nm = np.linalg.norm(n, axis=1)
    if eq == H.EQ_3D_RNGDEP:
        g = np.stack([c * n[:, 0] / nm + u, c * n[:, 1] / nm + v, c * n[:, 2] / nm], axis=1)
        t = g / np.linalg.norm(g, axis=1, keepdims=True)
        return t[:, 0] * (y[:, 7] * y[:, 14] - y[:, 13] * y[:, 8]) - y[:, 6] * (t[:, 1] * y[:, 14] - t[:, 2] * y[:, 13]) + y[:, 12] * (t[:, 1] * y[:, 8] - t[:, 2] * y[:, 7])
    r, lat = y[:, 0], y[:, 1]
    g = np.stack([c * n[:, 0] / nm, c * n[:, 1] / nm + v, c * n[:, 2] / nm + u], axis=1)
    gm = np.linalg.norm(g, axis=1)
    dr, dt = g[:, 0] / gm, g[:, 1] / gm / r
    dp = g[:, 2] / gm / (r * (np.cos(lat) if cos_metric else np.sin(lat)))
    return r * r * np.cos(lat) * (dr * (y[:, 7] * y[:, 14] - y[:, 13] * y[:, 8]) - y[:, 6] * (dt * y[:, 14] - dp * y[:, 13]) + y[:, 12] * (dt * y[:, 8] - dp * y[:, 7]))


def _base_crossings(eq, legs):
    """every passage of one ray through the levels: (level, leg, dir, ord, full interpolated state row) in path order"""
    out = []
    for j, (k, rows, sums) in enumerate(legs):
        seen = {}
        for c in LV.crossings(eq, rows, LEVELS):
            key = (c["level"], c["dir"])
            o = seen.get(key, 0)
            seen[key] = o + 1
            i, f = c["seg"], c["frac"]
            out.append((c["level"], j, c["dir"], o, rows[i] + f * (rows[i + 1] - rows[i])))
    return out


def _ray_constants(eq, y, th, ph, m, s):
    """the stratified Cartesian set's nu, nu_x, nu_y of each ray appended to its state rows (constants of the ray, as amp_jac forms them)"""
    if eq != H.EQ_3D:
        return y
    cth = np.cos(np.radians(th))
    e0, e1 = cth * np.sin(np.radians(ph)), cth * np.cos(np.radians(ph))
    MS = 1.0 + (e0 * s[1] / s[0] + e1 * s[2] / s[0])
    nx, ny = e0 / MS, e1 / MS
    nu = (s[0] - nx * m[1] - ny * m[2]) / m[0]
    return np.concatenate([y, nu[:, None], nx[:, None], ny[:, None]], axis=1)


def arrival_amp_check(eq, F, cfg, th, ph, paths, med, src3, z_grnd):
    """the numpy amplitude - the restatement's num / den with GeoAc_Jacobian's D (the reference's own form, Q3 included) - at the last row of every leg that
    landed, against GEOAC_REC_AMP of the fan F (the reference or the oracle) at the same rays: worst relative difference.  This holds the factor
    rho nu c^3 Q cos(theta) / (rho_s nu_s c_s^3 G), winds and quirk Q4 included, to the reference's GeoAc_Amplitude itself."""
    _, rec, _, _ = F.fan(cfg, th, ph)
    ys, ti, want = [], [], []
    for i, legs in enumerate(paths):
        for j, (k, rows, sums) in enumerate(legs):
            if k > 0 and rec[i, j, H.REC["VALID"]] > 0:
                ys.append(rows[-1]); ti.append(i); want.append(rec[i, j, H.REC["AMP"]])
    y, ti, want = np.stack(ys), np.array(ti), np.array(want)
    r = np.zeros((len(y), 12))
    r[:, LA.P0:LA.P0 + min(6, y.shape[1])] = y[:, :6] if eq != H.EQ_3D else np.concatenate([y[:, :4], np.zeros((len(y), 2))], axis=1)
    m = med(*LA.crossing_abscissae(eq, r))
    s = tuple(np.repeat(v, len(y)) for v in med(*LA.source_points(eq, [src3], z_grnd)))
    with np.errstate(all="ignore"):
        num, den0 = LA.tube(eq, r, r, r, th[ti], ph[ti], 1.0, np.full(len(y), 6370.0), m, s, parts=True)[4:]
        amp = 1.0 / (4.0 * np.pi) * np.sqrt(np.abs(num / (den0 * _jacobian_D(eq, _ray_constants(eq, y, th[ti], ph[ti], m, s), m, False))))
    return float(np.abs(amp / want - 1.0).max()), len(y)


def _gaps(eq, R, cfg, th, ph, src3, z_grnd, h):
    """the tube at step h against the Jacobian amplitude (the cos form on the spherical sets) at every passage of the rays: names, statuses, gaps"""
    med = LA.medium_of_oracle(R)
    n = len(th)
    T, P = LA.fan_angles(th, ph, h)
    paths = [R.trace_path(cfg, t, p) for t, p in zip(T, P)]
    count, lrec = LV.restate_fan(eq, paths, LEVELS, CAP_LVL)
    rows_of = [(i,) + c for i in range(n) for c in _base_crossings(eq, paths[i])]
    idx = np.array([r[0] for r in rows_of]); lv = np.array([r[1] for r in rows_of]); leg = np.array([r[2] for r in rows_of])
    dr = np.array([r[3] for r in rows_of]); od = np.array([r[4] for r in rows_of]); full = np.stack([r[5] for r in rows_of])
    m0 = np.zeros(len(idx), dtype=int)
    rows = LA.reference_rows(eq, count[None], lrec[None], th, ph, h, m0, idx, lv, leg, dr, od, LEVELS, med, [src3], z_grnd=z_grnd)
    rec = LA.branch_records(count[None], lrec[None], m0, lv, leg, dr.astype(float), od, idx, n, 0)[0]
    m = med(*LA.crossing_abscissae(eq, rec))
    s = tuple(np.repeat(v, len(idx)) for v in med(*LA.source_points(eq, [src3], z_grnd)))
    Dj = _jacobian_D(eq, _ray_constants(eq, full, th[idx], ph[idx], m, s), m, True)
    with np.errstate(all="ignore"):
        gap = np.abs(np.sqrt(np.abs(Dj) / rows[:, LA.LAMP["D"]]) - 1.0)
    names = [(float(th[i]), float(ph[i]), float(LEVELS[l]), int(g), int(d), int(o)) for i, l, g, d, o in zip(idx, lv, leg, dr, od)]
    return names, rows[:, LA.LAMP["STATUS"]].astype(int), gap


def scan(name):
    """all rays of table a_amp1 on the ragged grid: per crossing the gap at h = 0.02 and 0.04; writes profiles/level_amp_scan_<name>.txt"""
    eq = SCAN_SETS[name]
    R, _, th, ph, kw, src3, z_grnd = _inputs(name, whole_table=True)
    cfg = H.make_cfg(eq, **kw)
    n2, s2, g2 = _gaps(eq, R, cfg, th, ph, src3, z_grnd, STEPS[0])
    n4, s4, g4 = _gaps(eq, R, cfg, th, ph, src3, z_grnd, STEPS[1])
    assert n2 == n4
    bad2 = ~((s2 == LA.OK) & (g2 <= CAP))
    first_up = np.array([nm[3] == 0 and nm[4] == 1 for nm in n2])
    lines = [f"# tests/golden/make_level_amp.py --scan {name}: table a_amp1 ({len(th)} rays) on the ragged 7 x 4 grid, one bounce, levels {LEVELS} km; the forward tube of the",
             "# compiled reference's own rays against the Jacobian amplitude of the reference's calc_amp = 1 state row interpolated at the crossing" + (" (cos form)" if LA.spherical(eq) else ""),
             f"# crossings {len(n2)}; beyond {CAP:g} at h = 0.02 (or tube not OK): {int(bad2.sum())}; worst gap at h = 0.02 {np.nanmax(g2):.3e}, at h = 0.04 {np.nanmax(g4):.3e};",
             f"# upward passages of leg 0 alone: {int(first_up.sum())} crossings, {int((bad2 & first_up).sum())} beyond, worst {np.nanmax(g2[first_up]):.3e}",
             "# theta phi level_km leg dir ord  status  gap(h=0.02)  gap(h=0.04)"]
    for nm, st, a, b in zip(n2, s2, g2, g4):
        lines.append(f"{nm[0]:g} {nm[1]:g} {nm[2]:g} {nm[3]} {nm[4]:+d} {nm[5]}  {LA.STATUS_NAMES[st]}  {a:.3e}  {b:.3e}")
    path = os.path.join(os.path.dirname(os.path.dirname(OUT)), "profiles", f"level_amp_scan_{name}.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]))
    print("->", path)


def _set(name):
    eq = SETS[name]
    R, O, th, ph, kw, src3, z_grnd = _inputs(name)
    cfg = H.make_cfg(eq, **kw)
    n = len(th)
    med = LA.medium_of_oracle(R)

    def tables(theta, h):
        T, P = LA.fan_angles(theta, ph, h)
        paths = [R.trace_path(cfg, t, p) for t, p in zip(T, P)]
        count, lrec = LV.restate_fan(eq, paths, LEVELS, CAP_LVL)
        assert count.max() <= CAP_LVL
        return paths, count[None], lrec[None]

    paths, count, lrec = tables(th, STEPS[0])
    for i in range(n):                                                              # the oracle's paths are the reference's, bit for bit
        ol = O.trace_path(cfg, th[i], ph[i])
        assert len(ol) == len(paths[i]) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(paths[i], ol)), (name, i)
    arr_err, arr_n = arrival_amp_check(eq, R, cfg, th, ph, paths[:n], med, src3, z_grnd)
    assert arr_n >= 2 and arr_err <= 1e-9, (name, "numpy amplitude against GEOAC_REC_AMP at the ground arrivals", arr_err, arr_n)
    rows_of = [(i,) + c for i in range(n) for c in _base_crossings(eq, paths[i])]
    idx = np.array([r[0] for r in rows_of]); lv = np.array([r[1] for r in rows_of]); leg = np.array([r[2] for r in rows_of])
    dr = np.array([r[3] for r in rows_of]); od = np.array([r[4] for r in rows_of])
    full = np.stack([r[5] for r in rows_of])
    args = (np.zeros(len(idx), dtype=int), idx, lv, leg, dr, od, LEVELS, med, [src3])
    t02 = LA.reference_rows(eq, count, lrec, th, ph, STEPS[0], *args, z_grnd=z_grnd)
    _, count4, lrec4 = tables(th, STEPS[1])
    t04 = LA.reference_rows(eq, count4, lrec4, th, ph, STEPS[1], *args, z_grnd=z_grnd)
    th_e = th * (1.0 + 1e-12)
    _, count_e, lrec_e = tables(th_e, STEPS[0])
    t_e = LA.reference_rows(eq, count_e, lrec_e, th_e, ph, STEPS[0], *args, z_grnd=z_grnd)
    A = LA.LAMP
    # the three crossing points and the medium, as the restatement took them
    member0 = np.zeros(len(idx), dtype=int)
    recs = [LA.branch_records(count, lrec, member0, lv, leg, dr.astype(float), od, idx, n, j)[0] for j in range(3)]
    recs4 = [LA.branch_records(count4, lrec4, member0, lv, leg, dr.astype(float), od, idx, n, j)[0] for j in range(3)]
    pts = np.stack([np.stack(LA.LS.crossing_points(eq, r), axis=1) for r in recs + recs4[1:]], axis=1)          # [n][5][2]: base, theta / phi probe at 0.02, at 0.04
    m = med(*LA.crossing_abscissae(eq, recs[0]))
    s = tuple(np.repeat(v, len(idx)) for v in med(*LA.source_points(eq, [src3], z_grnd)))
    r_level = 6370.0 + np.asarray(LEVELS)[lv]
    det, tz, D, amp, num, den0 = LA.tube(eq, recs[0], recs[1], recs[2], th[idx], ph[idx], STEPS[0], r_level, m, s, parts=True)
    ok = t02[:, A["STATUS"]] == LA.OK
    assert np.array_equal(LA.bits(amp[ok]), LA.bits(t02[ok, A["AMP"]]))
    # the Jacobian amplitude of the interpolated state row: the tube's num / den with the reference's own D in the tube's place
    y = _ray_constants(eq, full, th[idx], ph[idx], m, s)
    out = {}
    with np.errstate(all="ignore"):
        amp_jac = 1.0 / (4.0 * np.pi) * np.sqrt(np.abs(num / (den0 * _jacobian_D(eq, y, m, False))))
        want = amp_jac
        if LA.spherical(eq):
            want = 1.0 / (4.0 * np.pi) * np.sqrt(np.abs(num / (den0 * _jacobian_D(eq, y, m, True))))
            out[f"{name}_amp_jac_cos"] = want
        gap = np.abs(t02[:, A["AMP"]] / want - 1.0)
        sens = np.abs(t_e[:, A["AMP"]] / t02[:, A["AMP"]] - 1.0)
    names = [(float(th[i]), float(ph[i]), float(LEVELS[l]), int(g), int(d), int(o)) for i, l, g, d, o in zip(idx, lv, leg, dr, od)]
    # beyond the cap; a crossing whose tube is not OK at both steps, or whose fd_sens is not finite, has no place in the fixture either
    beyond = ~ok | ~(gap <= CAP) | ~np.isfinite(sens) | (t04[:, A["STATUS"]] != LA.OK)
    for k in np.flatnonzero(beyond):
        print(f"  {name}: beyond the cap {names[k]},   # status {LA.STATUS_NAMES[int(t02[k, A['STATUS']])]}, gap {gap[k]:.3e}")
    listed = np.array([nm in LEFT_OUT[name] for nm in names])
    assert np.array_equal(beyond, listed), (name, "LEFT_OUT must name exactly these", [names[k] for k in np.flatnonzero(beyond != listed)])
    assert listed.sum() <= LEFT_OUT_SHARE * len(names), (name, int(listed.sum()), len(names))
    keep = ~listed
    assert (t04[keep, A["STATUS"]] == LA.OK).all(), name
    out.update({f"{name}_theta": th, f"{name}_phi": ph, f"{name}_levels": np.array(LEVELS), f"{name}_src": np.array(src3), f"{name}_z_grnd": np.float64(z_grnd),
                f"{name}_ray": idx[keep].astype(np.int32), f"{name}_level": lv[keep].astype(np.int32), f"{name}_leg": leg[keep].astype(np.int32),
                f"{name}_dir": dr[keep].astype(np.int32), f"{name}_ord": od[keep].astype(np.int32), f"{name}_points": pts[keep],
                f"{name}_medium": np.stack(m, axis=1)[keep], f"{name}_medium_src": np.array([v[0] for v in s]),
                f"{name}_tube02": t02[keep][:, A["DET"]:A["AMP"] + 1], f"{name}_tube04": t04[keep][:, A["DET"]:A["AMP"] + 1],
                f"{name}_ttime": t02[keep, A["TTIME"]], f"{name}_atten": t02[keep, A["ATTEN"]],
                f"{name}_amp_jac": amp_jac[keep], f"{name}_fd_sens": sens[keep], f"{name}_gap": gap[keep], f"{name}_arrival_amp_err": np.float64(arr_err)})
    if f"{name}_amp_jac_cos" in out:
        out[f"{name}_amp_jac_cos"] = out[f"{name}_amp_jac_cos"][keep]
    g4 = np.abs(t04[keep, A["AMP"]] / want[keep] - 1.0)
    q3 = np.abs(amp_jac[keep] / want[keep] - 1.0).max() if LA.spherical(eq) else 0.0
    branches = sorted(set(zip(leg[keep].tolist(), dr[keep].tolist(), od[keep].tolist())))
    line = (f"{name}: {int(keep.sum())} crossings kept, {int(listed.sum())} left out; branches {branches}; worst gap to the Jacobian amplitude {gap[keep].max():.3e} at h = 0.02, "
            f"{g4.max():.3e} at h = 0.04; worst fd_sens {sens[keep].max():.3e}; numpy amplitude against GEOAC_REC_AMP at {arr_n} ground arrivals {arr_err:.2e}"
            + (f"; the reference's own amplitude (Q3) is off the geometric one by up to {q3:.3e}" if q3 else ""))
    return out, line


def main():
    out = {"steps": np.array(STEPS), "cap": np.float64(CAP)}
    with ProcessPoolExecutor(len(SETS)) as pool:                     # (a process per set: the reference keeps its state in globals, and the grid sets take minutes)
        for part, line in pool.map(_set, list(SETS)):
            out.update(part)
            print(line)
    path = os.path.join(OUT, "level_amp.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--scan":
        scan(sys.argv[2])
    else:
        main()
