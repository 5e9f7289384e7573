"""Generates tests/golden/*.npz from the COMPILED, UNMODIFIED reference (oracle/_ref/libref_*.so, built
by oracle/Makefile from /root/reference).  Run here only (the reference does not travel):

    make -C oracle all && python tests/golden/make_golden.py            # {global,3d,2d}_small.npz; `rngdep`, `globalrd`: the grid sets'
    python tests/golden/make_golden.py polar                            # global_polar.npz (3 minutes on one core)
    python tests/golden/make_golden.py globalrd_polar                   # globalrd_polar.npz (2 minutes)
    python tests/golden/make_golden.py jet                              # jet_small.npz: the stratified sets on tests/golden/JetAtmo.met (`zuvwTdp`; 4 minutes on three cores)
    python tests/golden/make_golden.py ragged3d                         # rngdep_ragged.npz (the columns) + rngdep_ragged_3drd.npz: the ragged 7 x 4 jet grid (3 minutes on six cores)
    python tests/golden/make_golden.py raggedglobal                     # rngdep_ragged.npz + rngdep_ragged_globalrd.npz

The fixtures are data: launch angles + configuration in, full-precision arrival records / samples /
probe values out.  tests/test_oracle_golden.py pins the plain-C oracle to them bit for bit;
the GPU parity tests compare the HIP path with the same vectors.
"""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import harness as H  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

THETAS = [0.5, 5.0, 15.0, 25.0, 35.0, 45.0]
PHIS = [-90.0, 0.0, 37.0]


def small_fan():
    th = np.array([t for p in PHIS for t in THETAS])
    ph = np.array([p for p in PHIS for t in THETAS])
    return th, ph


def cfg_dict(cfg):
    return dict(z_grnd=cfg.z_grnd, tweak_abs=cfg.tweak_abs, freq=cfg.freq, vert_limit=cfg.vert_limit,
                range_limit=cfg.range_limit, src=np.array(list(cfg.src)), bounces=cfg.bounces,
                calc_amp=cfg.calc_amp, mode=cfg.mode)


def main():
    for eq in (H.EQ_GLOBAL, H.EQ_3D, H.EQ_2D):
        name = H.EQ_NAMES[eq]
        R = H.RefShim(eq)
        th, ph = small_fan()
        out = {"theta": th, "phi": ph}
        # fan records, both CalcAmp modes, the three output modes (Q7)
        for amp in (1, 0):
            for mode in (0, 1, 3):
                cfg = H.make_cfg(eq, calc_amp=bool(amp), mode=mode)
                steps, rec, smp, nsmp = R.fan(cfg, th, ph, smp_cap=40000)
                tag = f"amp{amp}_mode{mode}"
                out[f"rec_{tag}"] = rec
                out[f"steps_{tag}"] = np.int64(steps)
                out[f"nsmp_{tag}"] = np.int64(nsmp)
                if amp == 1 and mode == 3:
                    sel = np.arange(0, len(smp), 4)          # every 4th sample row keeps the fixture small
                    out[f"smp_idx_{tag}"] = sel
                    out[f"smp_{tag}"] = smp[sel]
        # a run with non-default ground / source / absorption / limits
        if eq == H.EQ_GLOBAL:
            src = (1.0, 41.131, -112.896)
        elif eq == H.EQ_3D:
            src = (0.0, 0.0, 1.0)
        else:
            src = (1.0, 0.0, 0.0)
        cfg = H.make_cfg(eq, bounces=1, calc_amp=True, mode=0, src=src, z_grnd=0.3, tweak_abs=0.5, freq=0.5,
                         range_limit=800.0)
        steps, rec, _, _ = R.fan(cfg, th, ph)
        out["rec_alt"] = rec
        out["steps_alt"] = np.int64(steps)
        for k, v in cfg_dict(cfg).items():
            out[f"altcfg_{k}"] = np.asarray(v)
        # stepper rows of one leg (every 50th row + the last three)
        cfg = H.make_cfg(eq, calc_amp=True)
        k, rows = R.trace_leg0(cfg, 15.0, -90.0)
        sel = np.unique(np.concatenate([np.arange(0, abs(k) + 1, 50), np.arange(abs(k) - 2, abs(k) + 1)]))
        out["trace_k"] = np.int64(k)
        out["trace_idx"] = sel
        out["trace_rows"] = rows[sel]
        # atmosphere + absorption probes
        t = R.tables()
        rng = np.random.default_rng(12345)
        x = rng.uniform(t["x"][0] - 0.5, t["x"][-1] + 0.5, 1000)
        x[:8] = [t["x"][0], t["x"][-1], t["x"][1], t["x"][700], t["x"][0] - 1, t["x"][-1] + 1, t["x"][3], t["x"][4]]
        o9, rho = R.atmo_probe(x)
        out["probe_x"] = x
        out["probe_out9"] = o9
        out["probe_rho"] = rho
        xa = rng.uniform(t["x"][0], t["x"][-1], 200)
        fa = 10.0 ** rng.uniform(-2, 1, 200)
        out["abs_x"] = xa
        out["abs_f"] = fa
        out["abs_alpha"] = R.absorption_probe(xa, fa, 0.0, 0.3)
        for key in ("x", "T", "u", "v", "rho", "sT", "su", "sv", "srho"):
            out[f"tab_{key}"] = t[key]
        path = os.path.join(OUT, f"{name}_small.npz")
        np.savez_compressed(path, **out)
        print(name, "->", path, os.path.getsize(path) // 1024, "KiB")


def main_rngdep():
    """3D.RngDep: synthetic 5x5 grid (tests/rngdep_data.py), compiled reference libref_3drd.so"""
    import tempfile
    import rngdep_data as RD
    RD.save_grid_npz()
    grid = RD.write_grid(os.path.join(tempfile.gettempdir(), "gd"))
    eq = H.EQ_3D_RNGDEP
    R = H.RefShim(eq, grid=grid)
    out = {}
    rng = np.random.default_rng(2024)
    n = 400
    x = rng.uniform(-1100, 1100, n); y = rng.uniform(-900, 900, n); z = rng.uniform(-1, 141, n)
    x[:6] = [-1000, 1000, 0, 500, -500, 250]; y[:6] = [-800, 800, 0, -400, 400, 0]; z[:6] = [0, 139.6, 10, 0.4, 70, 0.0]
    o30, a8 = R.grid_probe(x, y, z)
    out.update(probe_x=x, probe_y=y, probe_z=z, probe_out30=o30, probe_api8=a8)
    th = np.array([3.0, 9.0, 16.0, 24.0, 31.0, 40.0]); ph = np.array([-90.0, -35.0, 20.0, 75.0, 130.0, -160.0])
    out.update(theta=th, phi=ph)
    for amp in (1, 0):
        for mode in (0, 3):
            cfg = H.make_cfg(eq, bounces=1, calc_amp=bool(amp), mode=mode, src=(0.0, 0.0, 0.0))
            steps, rec, smp, nsmp = R.fan(cfg, th, ph, smp_cap=40000)
            tag = f"amp{amp}_mode{mode}"
            out[f"rec_{tag}"] = rec; out[f"steps_{tag}"] = np.int64(steps); out[f"nsmp_{tag}"] = np.int64(nsmp)
            if amp == 1 and mode == 3:
                sel = np.arange(0, len(smp), 4)
                out[f"smp_idx_{tag}"] = sel; out[f"smp_{tag}"] = smp[sel]
    # off-centre elevated source, other frequency and absorption scale, tighter box.  The ground stays at 0 (this main tapers the winds around z_grnd when it LOADS:
    # a raised ground in the Cartesian grid set is main_ragged's, below)
    cfg = H.make_cfg(eq, bounces=2, calc_amp=True, mode=0, src=(120.0, -60.0, 1.0), freq=0.4, tweak_abs=0.6,
                     xy_limits=(-700.0, 900.0, -600.0, 700.0))
    steps, rec, _, _ = R.fan(cfg, th, ph)
    out["rec_alt"] = rec; out["steps_alt"] = np.int64(steps)
    path = os.path.join(OUT, "3drd_small.npz")
    np.savez_compressed(path, **out)
    print("3drd ->", path, os.path.getsize(path) // 1024, "KiB;", os.path.getsize(RD.GRID_NPZ) // 1024, "KiB grid")


def main_globalrd():
    """Global.RngDep: synthetic 5x5 lat/lon grid (tests/rngdep_data.py), compiled reference libref_globalrd.so"""
    import tempfile
    import rngdep_data as RD
    RD.save_grid_global_npz()
    grid = RD.write_grid_global(os.path.join(tempfile.gettempdir(), "gg"))
    eq = H.EQ_GLOBAL_RNGDEP
    R = H.RefShim(eq, grid=grid)
    out = {}
    rng = np.random.default_rng(2025)
    n = 400
    r = 6370.0 + rng.uniform(-1, 141, n); lat = np.radians(rng.uniform(24, 38, n)); lon = np.radians(rng.uniform(-9, 9, n))
    r[:6] = 6370.0 + np.array([0, 139.6, 10, 0.4, 70, 0.0]); lat[:6] = np.radians([25, 37, 31, 28, 34, 29.5]); lon[:6] = np.radians([-8, 8, 0, 4, -4, 0])
    o30, a8 = R.grid_probe(r, lat, lon)
    out.update(probe_r=r, probe_lat=lat, probe_lon=lon, probe_out30=o30, probe_api8=a8)
    th = np.array([3.0, 9.0, 16.0, 24.0, 31.0, 40.0]); ph = np.array([-90.0, -35.0, 20.0, 75.0, 130.0, -160.0])
    out.update(theta=th, phi=ph)
    for amp in (1, 0):
        for mode in (0, 3):
            cfg = H.make_cfg(eq, bounces=1, calc_amp=bool(amp), mode=mode, src=(0.0, 31.0, 0.0))
            steps, rec, smp, nsmp = R.fan(cfg, th, ph, smp_cap=40000)
            tag = f"amp{amp}_mode{mode}"
            out[f"rec_{tag}"] = rec; out[f"steps_{tag}"] = np.int64(steps); out[f"nsmp_{tag}"] = np.int64(nsmp)
            if amp == 1 and mode == 3:
                sel = np.arange(0, len(smp), 4)
                out[f"smp_idx_{tag}"] = sel; out[f"smp_{tag}"] = smp[sel]
    # off-centre elevated source, raised ground, other frequency, tighter lat/lon box (radians, as the break check compares them)
    cfg = H.make_cfg(eq, bounces=2, calc_amp=True, mode=0, src=(1.5, 29.0, 1.0), z_grnd=0.3, freq=0.4, tweak_abs=0.6,
                     xy_limits=tuple(np.radians([26.0, 36.5, -7.0, 6.0])))
    steps, rec, _, _ = R.fan(cfg, th, ph)
    out["rec_alt"] = rec; out["steps_alt"] = np.int64(steps)
    path = os.path.join(OUT, "globalrd_small.npz")
    np.savez_compressed(path, **out)
    print("globalrd ->", path, os.path.getsize(path) // 1024, "KiB;", os.path.getsize(RD.GRID_GLOBAL_NPZ) // 1024, "KiB grid")


# ---- stratified Global set near the poles (tests/test_gpu_polar.py) ----
# name -> source (z, lat, lon), azimuth of the poleward direction.  The azimuths of a fan are POLAR_AZ + that direction: rays that pass the pole at
# 0.004 .. 0.05 degrees on either side, and rays that leave sideways and away.  85.5 N: where a stage's 1/cos(lat) taken from the step's first stage was last quoted as harmless; -89: cos as at 89, sin and tan mirrored.
POLAR_SOURCES = {"n89": ((0.0, 89.0, 0.0), 0.0), "n855": ((0.0, 85.5, 20.0), 0.0), "s89": ((0.0, -89.0, 0.0), 180.0)}
POLAR_TH = [2.0, 8.0, 14.0, 20.0, 26.0]
POLAR_AZ = [-3.0, -2.0, -1.0, -0.25, 0.25, 1.0, 2.0, 3.0, 10.0, 45.0, 90.0, 180.0]
POLAR_SENS_EPS = 1e-12
# Azimuth 0 - the ray aimed AT the pole - was dropped from all three fans: it fails the conditioning assertion below on the compiled reference.  ToyAtmo's
# zonal wind carries it past the pole at a distance far below 0.004 degrees, and the reference's own arrival longitude then answers theta (1 + 1e-12) with
# 2.3e-9 rad where it is -1.8e-3 rad (89 N and 89 S, theta 26, leg 1: 1.3e-6 by compare_records' measure) and its launch-angle derivatives with 4.9e-7
# (85.5 N, theta 2): no arithmetic but the reference's own bit pattern follows it to 1e-6 there.  Rays over the pole stay in the tests that need no
# reference: tests/test_gpu_polar.py adds them to the bit-identity and Hamiltonian checks, the straight-ray cases of tests/test_oracle_known_answers.py hold one.


def polar_fan(poleward):
    th = np.array([t for a in POLAR_AZ for t in POLAR_TH])
    ph = np.array([poleward + a for a in POLAR_AZ for t in POLAR_TH])
    return th, ph


def main_polar():
    """global_polar.npz: per source and CalcAmp setting the compiled reference's records and step total, and `sens`: how far each compared field of each
    arrival moves IN THE REFERENCE when theta is multiplied by 1 + 1e-12 (parity.field_errors: compare_records' own measures).  4 x sens <= 1e-6 is
    asserted for every field of every arrival - the 1e-6 comparison of the HIP path needs no exemption list on these fans."""
    from parity import field_errors
    eq = H.EQ_GLOBAL
    R, O = H.RefShim(eq), H.Oracle(eq)
    out = {"names": np.array(list(POLAR_SOURCES)), "az_rel": np.array(POLAR_AZ), "sens_eps": np.float64(POLAR_SENS_EPS)}
    for name, (src, poleward) in POLAR_SOURCES.items():
        th, ph = polar_fan(poleward)
        out[f"{name}_src"] = np.array(src); out[f"{name}_theta"] = th; out[f"{name}_phi"] = ph
        for amp in (1, 0):
            cfg = H.make_cfg(eq, bounces=2, calc_amp=bool(amp), src=src)
            steps, rec, _, _ = R.fan(cfg, th, ph)
            so, ro, _, _ = O.fan(cfg, th, ph)
            assert so == steps and np.array_equal(ro, rec), f"{name} amp{amp}: the oracle's records differ from the compiled reference's"
            sp, rp, _, _ = R.fan(cfg, th * (1.0 + POLAR_SENS_EPS), ph)
            for f in ("VALID", "STEPS", "BROKE"):
                assert np.array_equal(rp[..., H.REC[f]], rec[..., H.REC[f]]), f"{name} amp{amp}: {f} moves with theta (1 + {POLAR_SENS_EPS:g})"
            E = 18 if amp else 6
            fe = field_errors(rp, rec, E)
            fields = sorted(fe)
            sens = np.stack([fe[f] for f in fields], axis=-1)
            worst = {f: float(np.nanmax(fe[f])) for f in fields}
            assert 4.0 * np.nanmax(sens) <= 1e-6, f"{name} amp{amp}: the reference itself is ill-conditioned here: {worst}"
            tag = f"{name}_amp{amp}"
            out[f"{tag}_rec"] = rec; out[f"{tag}_steps"] = np.int64(steps)
            out[f"{tag}_sens"] = sens.astype(np.float32); out[f"{tag}_sens_fields"] = np.array(fields)
            lat = rec[..., H.REC["STATE"] + 1][rec[..., H.REC["VALID"]] > 0]
            print(f"{tag}: {steps} steps, {int((rec[..., H.REC['VALID']] > 0).sum())} of {rec.shape[0] * rec.shape[1]} legs VALID, arrival latitudes "
                  f"{np.degrees(lat.min()):.2f} .. {np.degrees(lat.max()):.2f} deg; worst sensitivity " + ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    path = os.path.join(OUT, "global_polar.npz")
    np.savez_compressed(path, **out)
    print("polar ->", path, os.path.getsize(path) // 1024, "KiB")


# ---- range-dependent spherical set at high latitude (tests/test_gpu_globalrd.py, test_gpu_probes.py, test_oracle_globalrd.py) ----
# rngdep_data.POLAR_GRID: the committed columns on rows 82 .. 89.5 N, 15 degrees of longitude apart (116 km at the source, 14.6 km on the last row).  5 x 7 fan
# from 86 N: towards the pole and 3, 8 degrees beside it (arrivals at 88.9 .. 89.35 N, the steeper rays; the shallow ones leave over the last row), sideways
# (leaves through the longitude box or arrives at 84 N) and away.  Every second leg leaves the grid: BROKE, with an exact step count, is part of what is pinned.
RDPOLAR_SRC = (0.0, 86.0, 0.0)
RDPOLAR_TH = [3.0, 20.0, 24.0, 28.0, 33.0]
RDPOLAR_AZ = [-3.0, 0.0, 3.0, 8.0, 110.0, 180.0, -160.0]


def main_globalrd_polar():
    """globalrd_polar.npz: Global.RngDep on the polar grid, compiled reference libref_globalrd.so (a process of its own: the reference holds one grid), the
    oracle asserted equal bit for bit.  Records of the fan (bounces = 1, amplitudes on), the reference's own answer to theta (1 + 1e-12) per arrival and
    field (4 x that <= 1e-6 asserted: no exemptions), and Eval_Spline_AllOrder2 / the scalar API at 400 points of the grid."""
    import tempfile
    import rngdep_data as RD
    from parity import field_errors
    eq = H.EQ_GLOBAL_RNGDEP
    grid = RD.write_grid_global(os.path.join(tempfile.gettempdir(), "ggp"), **RD.POLAR_GRID)
    R = H.RefShim(eq, grid=grid)
    O = H.Oracle(eq, met=None); O.load_grid(*grid)
    lat_n, lon_n = RD.lat_nodes_global(RD.POLAR_GRID["centre_lat"], RD.POLAR_GRID["lat_step"]), RD.lon_nodes_global(RD.POLAR_GRID["lon_step"])
    out = {"lat_nodes": lat_n, "lon_nodes": lon_n, "src": np.array(RDPOLAR_SRC)}
    rng = np.random.default_rng(2026)
    n = 400
    # a third of a cell beyond the rows and columns, as the mid-latitude probes; below the pole
    r = 6370.0 + rng.uniform(-1, 141, n); lat = np.radians(rng.uniform(81.4, 89.95, n)); lon = np.radians(rng.uniform(-35, 35, n))
    r[:6] = 6370.0 + np.array([0, 139.6, 10, 0.4, 70, 0.0]); lat[:6] = np.radians([lat_n[0], lat_n[4], lat_n[2], lat_n[1], lat_n[3], 84.8]); lon[:6] = np.radians([lon_n[0], lon_n[4], 0, lon_n[3], lon_n[1], 0])
    o30, a8 = R.grid_probe(r, lat, lon)
    oo30, oa8 = O.grid_probe(r, lat, lon)
    assert np.array_equal(oo30, o30) and np.array_equal(oa8, a8), "the oracle's interpolant differs from the compiled reference's"
    out.update(probe_r=r, probe_lat=lat, probe_lon=lon, probe_out30=o30, probe_api8=a8)
    th = np.array([t for a in RDPOLAR_AZ for t in RDPOLAR_TH]); ph = np.array([a for a in RDPOLAR_AZ for t in RDPOLAR_TH])
    out.update(theta=th, phi=ph)
    cfg = H.make_cfg(eq, bounces=1, calc_amp=True, mode=0, src=RDPOLAR_SRC)
    steps, rec, _, _ = R.fan(cfg, th, ph)
    so, ro, _, _ = O.fan(cfg, th, ph)
    assert so == steps and np.array_equal(ro, rec), "the oracle's records differ from the compiled reference's"
    sp, rp, _, _ = R.fan(cfg, th * (1.0 + POLAR_SENS_EPS), ph)
    for f in ("VALID", "STEPS", "BROKE"):
        assert np.array_equal(rp[..., H.REC[f]], rec[..., H.REC[f]]), f"{f} moves with theta (1 + {POLAR_SENS_EPS:g})"
    fe = field_errors(rp, rec, 18, 0)
    fields = sorted(fe)
    sens = np.stack([fe[f] for f in fields], axis=-1)
    worst = {f: float(np.nanmax(fe[f])) for f in fields}
    assert 4.0 * np.nanmax(sens) <= 1e-6, f"the reference itself is ill-conditioned here: {worst}"
    out.update(rec_amp1=rec, steps_amp1=np.int64(steps), sens=sens.astype(np.float32), sens_fields=np.array(fields), sens_eps=np.float64(POLAR_SENS_EPS))
    valid = rec[..., H.REC["VALID"]] > 0
    lat_a = np.degrees(rec[..., H.REC["STATE"] + 1][valid])
    print(f"globalrd_polar: {steps} steps, {int(valid.sum())} arrivals at {lat_a.min():.2f} .. {lat_a.max():.2f} N, {int((rec[..., H.REC['BROKE']] > 0).sum())} legs BROKE; worst sensitivity "
          + ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    path = os.path.join(OUT, "globalrd_polar.npz")
    np.savez_compressed(path, **out)
    print("globalrd_polar ->", path, os.path.getsize(path) // 1024, "KiB")


# ---- the stratified sets on a jet profile with meridional wind, read through the second profile format (tests/test_gpu_jet.py, test_oracle_golden.py) ----
# tests/golden/JetAtmo.met (tests/jet_data.py, `zuvwTdp`): u up to 85 m/s, v = 40 / -22 / 15 m/s.  Two fans per set, azimuths all round (the v sin(phi) and
# ny v terms vanish at +-90): (a) from the ground, (b) from 12 km - wind AT the source (u = 30, v = -22 m/s: the initial slowness and the amplitude's m0.u,
# m0.v, quirk Q4) - with rays launched below the horizontal.  range_limit = JET_RANGE keeps the longest leg of the Cartesian sets near 1e5 steps (ducted
# rays in the jets run to the limit and BREAK there: an exact step count is part of what is pinned).
JET_TH_A = [2.0, 7.0, 19.0, 34.0]
JET_TH_B = [-20.0, -8.0, -2.0, 1.0, 6.0, 12.0, 18.0, 25.0, 33.0, 41.0]
JET_AZ = [-180.0, -135.0, -90.0, -45.0, 0.0, 45.0, 90.0, 135.0]
JET_RANGE = 2000.0


# Rays left out of the lattice (theta, azimuth): they fail the conditioning assertion of main_jet on the compiled reference in at least one set - the reference's
# own answer to theta (1 + 1e-12) moves a compared field by more than 2.5e-7 there, so no arithmetic but its own bit pattern follows it to 1e-6.
#   a ( 7, -135)  3D / 2D: grazes the top of the tropospheric duct; the perturbed ray's second leg changes its STEP COUNT (STATE moves by 8e-2)
#   a ( 2,    0), a (2, -180)  Global: third leg, 9.7e-7 and 8.4e-7 (launch-angle derivatives of rays that bounce three times inside the duct)
#   b (33,   45)  3D / 2D: 6.3e-6 / 4.8e-7 on the third leg (turns at the edge of the stratospheric jet)
#   b (12,  135), b (12, 90), b (1, -180)  Global: 2.9e-5, 1.4e-6 (third legs) and 5.1e-7 (the ducted ray itself, ATTEN after 42 683 steps)
JET_DROPPED = {"a": [(7.0, -135.0), (2.0, 0.0), (2.0, -180.0)], "b": [(33.0, 45.0), (12.0, 135.0), (12.0, 90.0), (1.0, -180.0)]}


def jet_fans():
    import jet_data as JD
    out = {}
    for name, ths, z in (("a", JET_TH_A, 0.0), ("b", JET_TH_B, JD.SRC_Z)):
        rays = [(t, a) for a in JET_AZ for t in ths if (t, a) not in JET_DROPPED[name]]
        out[name] = (np.array([r[0] for r in rays]), np.array([r[1] for r in rays]), z)
    return out


def _jet_set(eq):
    """one set's share of jet_small.npz (runs in a process of its own): (record tables, atmosphere probes, printed lines, failures)"""
    import jet_data as JD
    from parity import field_errors
    sname = H.EQ_NAMES[eq]
    fans = jet_fans()
    out, lines, failures = {}, [], []
    R, O = H.RefShim(eq, met=JD.JET, fmt=JD.FMT), H.Oracle(eq, met=JD.JET, fmt=JD.FMT)
    for tag, (fan, kw) in JD.TABLES.items():
        th, ph, z = fans[fan]
        cfg = H.make_cfg(eq, src=JD.src(eq, z), range_limit=JET_RANGE, **kw)
        steps, rec, _, _ = R.fan(cfg, th, ph)
        so, ro, _, _ = O.fan(cfg, th, ph)
        assert so == steps and np.array_equal(ro, rec), f"{sname} {tag}: the oracle's records differ from the compiled reference's"
        sp, rp, _, _ = R.fan(cfg, th * (1.0 + POLAR_SENS_EPS), ph)
        moved = np.flatnonzero((rp[..., :3] != rec[..., :3]).any(axis=(1, 2)))
        E = JD.ESIZE[eq][1 if kw["calc_amp"] else 0]
        fe = field_errors(rp, rec, E, JD.HIDX[eq])
        fields = sorted(fe)
        sens = np.stack([fe[f] for f in fields], axis=-1)
        worst = {f: float(np.nanmax(fe[f])) for f in fields}
        per_ray = np.nanmax(np.nan_to_num(sens), axis=(1, 2))
        valid = rec[..., H.REC["VALID"]] > 0
        lines.append(f"{sname} {tag}: {steps} steps, {int(valid.sum())} arrivals ({int(valid[th < 0].sum())} of rays launched downwards), {int((rec[..., H.REC['BROKE']] > 0).sum())} legs BROKE, "
                     f"longest leg {int(rec[..., H.REC['STEPS']].max())} steps; worst sensitivity " + ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
        if len(moved):
            failures.append(f"{sname} {tag}: VALID / STEPS / BROKE move with theta (1 + {POLAR_SENS_EPS:g}) on rays {[(th[i], ph[i]) for i in moved]}")
        if not 4.0 * np.nanmax(sens) <= 1e-6:
            failures.append(f"{sname} {tag}: the reference itself is ill-conditioned on rays {[(th[i], ph[i], float(per_ray[i])) for i in np.flatnonzero(per_ray > 2.5e-7)]}: {worst}")
        key = f"{sname}_{tag}"
        if tag == "b_f001":
            # the frequency enters the absorption alone: every other column is b_amp1's, bit for bit - the fixture holds the ATTEN column (jet_data.table puts the table together)
            other = np.arange(H.REC_STRIDE) != H.REC["ATTEN"]
            assert np.array_equal(rec[..., other], out[f"{sname}_b_amp1_rec"][..., other]), f"{sname}: freq changes more than ATTEN"
            out[f"{key}_atten"] = rec[..., H.REC["ATTEN"]]
        else:
            out[f"{key}_rec"] = rec
        out[f"{key}_steps"] = np.int64(steps)
        out[f"{key}_sens"] = sens.astype(np.float32); out[f"{key}_sens_fields"] = np.array(fields)
    # atmosphere + absorption probes, as main(): nodes, both ends, beyond both ends - and points on and next to the 3 .. 10 m segments
    t = R.tables()
    rng = np.random.default_rng(12345)
    x = rng.uniform(t["x"][0] - 0.5, t["x"][-1] + 0.5, 1000)
    x[:8] = [t["x"][0], t["x"][-1], t["x"][1], t["x"][700], t["x"][0] - 1, t["x"][-1] + 1, t["x"][3], t["x"][4]]
    k = np.flatnonzero(np.diff(t["x"]) < 0.011)[:30]
    assert len(k) == 30
    x[8:128] = np.concatenate([t["x"][k], t["x"][k + 1], 0.5 * (t["x"][k] + t["x"][k + 1]), t["x"][k] - 1e-9])
    o9, rho = R.atmo_probe(x)
    oo9, orho = O.atmo_probe(x)
    assert np.array_equal(oo9, o9) and np.array_equal(orho, rho), f"{sname}: the oracle's spline accessors differ from the compiled reference's"
    xa = rng.uniform(t["x"][0], t["x"][-1], 200)
    fa = 10.0 ** rng.uniform(-2, 1, 200)
    alpha = R.absorption_probe(xa, fa, 0.0, 0.3)
    assert np.array_equal(O.absorption_probe(xa, fa, 0.0, 0.3), alpha), f"{sname}: the oracle's absorption differs from the compiled reference's"
    atmo = dict(probe_x=x, probe_out9=o9, probe_rho=rho, abs_x=xa, abs_f=fa, abs_alpha=alpha, **{f"tab_{k}": v for k, v in t.items()})
    return out, atmo, lines, failures


def main_jet():
    """jet_small.npz: per set (a process each: the reference holds one profile per set), table and field the compiled reference's records and step total - the
    oracle asserted equal bit for bit - and `sens`, as main_polar stores it: 4 x sens <= 1e-6 asserted for every field of every arrival, the counts asserted
    unchanged under theta (1 + 1e-12).  Plus the probes of test_gpu_probes.py on this profile and the reference's spline tables.  The Cartesian sets
    share G2S_Spline1D.cpp: their tables and probe values are asserted identical and stored once (`cart_`)."""
    import jet_data as JD
    from concurrent.futures import ProcessPoolExecutor
    eqs = (H.EQ_GLOBAL, H.EQ_3D, H.EQ_2D)
    out = {"range_limit": np.float64(JET_RANGE), "sens_eps": np.float64(POLAR_SENS_EPS), "src_z": np.float64(JD.SRC_Z)}
    for name, (th, ph, z) in jet_fans().items():
        out[f"{name}_theta"] = th; out[f"{name}_phi"] = ph
    with ProcessPoolExecutor(max_workers=3) as pool:
        res = dict(zip(eqs, pool.map(_jet_set, eqs)))
    failures = []
    for eq in eqs:
        out.update(res[eq][0])
        print("\n".join(res[eq][2]))
        failures += res[eq][3]
    assert not failures, "\n".join(failures)
    for k, v in res[H.EQ_3D][1].items():
        assert np.array_equal(v, res[H.EQ_2D][1][k]), f"{k}: the 2-D set's value differs from the 3-D set's"
        out[f"cart_{k}"] = v
    for k, v in res[H.EQ_GLOBAL][1].items():
        if k in ("tab_T", "tab_rho"):                 # (no set changes T or rho on loading: stored once)
            assert np.array_equal(v, out[f"cart_{k}"]), f"{k}: the Global set's value differs from the Cartesian sets'"
        else:
            out[f"global_{k}"] = v
    path = os.path.join(OUT, "jet_small.npz")
    np.savez_compressed(path, **out)
    print("jet ->", path, os.path.getsize(path) // 1024, "KiB")


# ---- both range-dependent sets on the ragged 7 x 4 jet grid (rngdep_data.write_grid_ragged; tests/test_gpu_rngdep.py, test_gpu_globalrd.py, test_gpu_probes.py,
#      test_host_grid.py, test_oracle_rngdep.py, test_oracle_globalrd.py) ----
# nx != ny, unequal node spacing on both horizontal axes (neighbouring cells 350 | 180 km, 1.5 | 3.5 degrees), irregular heights with six 3.3 m segments
# next to segments of 71 .. 379 m (rngdep_data.ragged_heights), winds of +-50 m/s with a meridional part that changes sign, a raised ground (z_grnd = 0.3: the Cartesian main tapers the winds around
# it when it LOADS, the spherical -prop loads with 0 and raises the ground afterwards).  Fan a: from the ground, off every node.  Fan b: from 12 km - wind at the source -
# with rays launched below the horizontal, freq = 10 and tweak_abs = 0.6; b_f001 the same at 0.01 Hz.  Two bounces: about every second leg leaves the grid (BROKE, with
# an exact step count).
RAGGED_SRC = {H.EQ_3D_RNGDEP: {"a": (60.0, -40.0, 0.0), "b": (-100.0, 50.0, 12.0)}, H.EQ_GLOBAL_RNGDEP: {"a": (0.0, 30.7, 2.2), "b": (12.0, 30.0, -1.0)}}
RAGGED_TH = {"a": [4.0, 9.0, 15.0, 21.0, 27.0], "b": [-12.0, -3.0, 8.0, 22.0, 38.0]}
RAGGED_AZ = {"a": [-70.0, 35.0, 150.0], "b": [-100.0, -25.0, 40.0, 115.0, 170.0]}
RAGGED_ZG = 0.3
# Rays left out of a fan (theta, azimuth): they fail the conditioning assertion of main_ragged on the compiled reference (at most one ray in ten of a fan).
#   globalrd a (15, -70): theta (1 + 1e-12) moves the launch-angle derivatives of its second arrival by 9.3e-6 in the reference itself (STATE, amplitudes on; every
#   other field and the amplitude-less run stay below 2e-8) - the ray turns inside one of the 3.3 m segments, where quirk Q12a multiplies the slopes
RAGGED_DROPPED = {H.EQ_3D_RNGDEP: {"a": [], "b": []}, H.EQ_GLOBAL_RNGDEP: {"a": [(15.0, -70.0)], "b": []}}


def ragged_fan(eq, name):
    rays = [(t, a) for a in RAGGED_AZ[name] for t in RAGGED_TH[name] if (t, a) not in RAGGED_DROPPED[eq][name]]
    assert len(rays) <= 30 and 10 * (len(RAGGED_AZ[name]) * len(RAGGED_TH[name]) - len(rays)) <= len(RAGGED_AZ[name]) * len(RAGGED_TH[name])
    return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


def _ragged_load(eq, grid):
    """reference and oracle with the grid loaded as the set's main loads it"""
    zl = RAGGED_ZG if eq == H.EQ_3D_RNGDEP else 0.0
    R = H.RefShim(eq, grid=grid, z_grnd=zl)
    O = H.Oracle(eq, met=None); O.load_grid(*grid, z_grnd=zl)
    return R, O


def _ragged_probe_points(eq):
    """400 points in the set's own coordinates (a, b: the horizontal axes, z: height above the first node).  The first NODE points sit on nodes of all three axes:
    first and last node of each axis, the nodes on either side of the widest-to-narrowest pair of neighbouring cells, the nodes of a 3 m segment; then 60 points in and
    on the 3 m segments, 40 a third of a cell beyond every edge, and random ones"""
    import rngdep_data as RD
    glob = eq == H.EQ_GLOBAL_RNGDEP
    na, nb = RD.ragged_nodes(glob)
    zn = np.load(RD.RAGGED_NPZ)["z"]
    short = np.flatnonzero(np.diff(zn) < RD.RAGGED_SHORT)
    rng = np.random.default_rng(2027 + int(glob))
    n = 400
    a = rng.uniform(na[0], na[-1], n); b = rng.uniform(nb[0], nb[-1], n); z = rng.uniform(-1.0, zn[-1] + 1.0, n)
    ia = [0, 6, 1, 2, 3, 2, 5, 4, 0, 6, 3, 1]           # (cells 350 | 180 km and 1.5 | 3.5 degrees: nodes 1, 2, 3)
    ib = [0, 3, 1, 2, 1, 2, 0, 3, 3, 0, 2, 1]
    iz = [0, len(zn) - 1, 7, 1, short[0], short[0] + 1, short[-1], short[-1] + 1, 100, len(zn) - 2, 200, short[len(short) // 2]]
    a[:12] = na[ia]; b[:12] = nb[ib]; z[:12] = zn[iz]
    k = short[np.arange(20) % len(short)]
    z[12:72] = np.concatenate([zn[k[:20]], zn[k[:20] + 1], zn[k[:20]] + np.diff(zn)[k[:20]] * rng.uniform(0.05, 0.95, 20)])
    da, db = np.diff(na), np.diff(nb)
    a[72:82] = na[0] - da[0] / 3.0; a[82:92] = na[-1] + da[-1] / 3.0; b[92:102] = nb[0] - db[0] / 3.0; b[102:112] = nb[-1] + db[-1] / 3.0
    a[92:97] = na[0] - da[0] / 3.0; a[102:107] = na[-1] + da[-1] / 3.0          # (corners: beyond two edges at once)
    return a, b, z


RAGGED_NODE_POINTS = 12


def _ragged_probe(R, O, eq):
    a, b, z = _ragged_probe_points(eq)
    if eq == H.EQ_GLOBAL_RNGDEP:
        args = (6370.0 + z, np.radians(a), np.radians(b))
        names = ("probe_r", "probe_lat", "probe_lon")
    else:
        args = (a, b, z)
        names = ("probe_x", "probe_y", "probe_z")
    o30, a8 = R.grid_probe(*args)
    oo30, oa8 = O.grid_probe(*args)
    assert np.array_equal(oo30, o30) and np.array_equal(oa8, a8), "the oracle's interpolant differs from the compiled reference's"
    assert np.isfinite(o30).all() and np.isfinite(a8).all()
    out = dict(zip(names, args))
    out.update(probe_out30=o30, probe_api8=a8, probe_node_points=np.int64(RAGGED_NODE_POINTS))
    return out


def _ragged_table(job):
    """one table's share of a ragged fixture (a process of its own: the reference takes 25 .. 45 s per 20 rays): (tag, arrays, printed line, failures)"""
    from parity import field_errors
    eq, grid, tag = job
    if tag == "probe":
        R, O = _ragged_load(eq, grid)
        return tag, _ragged_probe(R, O, eq), "", []
    import rngdep_data as RD
    fan, kw = RD.RAGGED_TABLES[tag]
    th, ph = ragged_fan(eq, fan)
    R, O = _ragged_load(eq, grid)
    cfg = H.make_cfg(eq, src=RAGGED_SRC[eq][fan], z_grnd=RAGGED_ZG, **kw)
    steps, rec, _, _ = R.fan(cfg, th, ph)
    so, ro, _, _ = O.fan(cfg, th, ph)
    assert so == steps and np.array_equal(ro, rec), f"{tag}: the oracle's records differ from the compiled reference's"
    sp, rp, _, _ = R.fan(cfg, th * (1.0 + POLAR_SENS_EPS), ph)
    failures = []
    moved = np.flatnonzero((rp[..., :3] != rec[..., :3]).any(axis=(1, 2)))
    E = (18 if kw["calc_amp"] else 6)
    hidx = 2 if eq == H.EQ_3D_RNGDEP else 0
    fe = field_errors(rp, rec, E, hidx)
    fields = sorted(fe)
    sens = np.stack([fe[f] for f in fields], axis=-1)
    worst = {f: float(np.nanmax(fe[f])) for f in fields}
    per_ray = np.nanmax(np.nan_to_num(sens), axis=(1, 2))
    if len(moved):
        failures.append(f"{tag}: VALID / STEPS / BROKE move with theta (1 + {POLAR_SENS_EPS:g}) on rays {[(th[i], ph[i]) for i in moved]}")
    if not 4.0 * np.nanmax(sens) <= 1e-6:
        failures.append(f"{tag}: the reference itself is ill-conditioned on rays {[(th[i], ph[i], float(per_ray[i])) for i in np.flatnonzero(per_ray > 2.5e-7)]}: {worst}")
    valid = rec[..., H.REC["VALID"]] > 0
    line = (f"{H.EQ_NAMES[eq]} {tag}: {steps} steps, {int(valid.sum())} of {valid.size} legs VALID ({int(valid[th < 0].sum())} of rays launched downwards), "
            f"{int((rec[..., H.REC['BROKE']] > 0).sum())} BROKE, longest leg {int(rec[..., H.REC['STEPS']].max())} steps; worst sensitivity " + ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    out = {f"{tag}_rec": rec, f"{tag}_steps": np.int64(steps), f"{tag}_sens": sens.astype(np.float32), f"{tag}_sens_fields": np.array(fields)}
    return tag, out, line, failures


def ragged_cells(eq, rec):
    """the grid cells (ia, ib) the arrivals of a record table land in"""
    import rngdep_data as RD
    glob = eq == H.EQ_GLOBAL_RNGDEP
    na, nb = RD.ragged_nodes(glob)
    st = rec[..., H.REC["STATE"]:H.REC["STATE"] + 3][rec[..., H.REC["VALID"]] > 0]
    pa, pb = (np.degrees(st[:, 1]), np.degrees(st[:, 2])) if glob else (st[:, 0], st[:, 1])
    return set(zip(np.searchsorted(na, pa).tolist(), np.searchsorted(nb, pb).tolist()))


def main_ragged(eq):
    """rngdep_ragged_<set>.npz: per table the compiled reference's records, step total and `sens` (as main_polar stores it: 4 x sens <= 1e-6 asserted for every field of
    every arrival, VALID / STEPS / BROKE asserted unchanged under theta (1 + 1e-12)), the oracle asserted equal bit for bit; Eval_Spline_AllOrder2 and the scalar API at
    400 points; node arrays and sources.  b_f001 is stored as its ATTEN column: every other column is asserted equal to b_amp1's."""
    import tempfile
    import rngdep_data as RD
    from concurrent.futures import ProcessPoolExecutor
    glob = eq == H.EQ_GLOBAL_RNGDEP
    sname = H.EQ_NAMES[eq]
    RD.save_grid_ragged_npz()
    grid = RD.write_grid_ragged(os.path.join(tempfile.gettempdir(), "rg" if glob else "rc"), glob)
    na, nb = RD.ragged_nodes(glob)
    out = {"nodes_a": na, "nodes_b": nb, "z_grnd": np.float64(RAGGED_ZG), "sens_eps": np.float64(POLAR_SENS_EPS)}
    for fan in ("a", "b"):
        th, ph = ragged_fan(eq, fan)
        out[f"{fan}_theta"] = th; out[f"{fan}_phi"] = ph; out[f"{fan}_src"] = np.array(RAGGED_SRC[eq][fan])
    jobs = [(eq, grid, tag) for tag in list(RD.RAGGED_TABLES) + ["probe"]]
    with ProcessPoolExecutor(max_workers=len(jobs)) as pool:
        res = list(pool.map(_ragged_table, jobs))
    failures = []
    for tag, arrays, line, fails in res:
        out.update(arrays)
        failures += fails
        if line:
            print(line)
    assert not failures, "\n".join(failures)
    other = np.arange(H.REC_STRIDE) != H.REC["ATTEN"]
    assert np.array_equal(out["b_f001_rec"][..., other], out["b_amp1_rec"][..., other]), "freq changes more than ATTEN"
    assert not np.array_equal(out["b_f001_rec"][..., H.REC["ATTEN"]], out["b_amp1_rec"][..., H.REC["ATTEN"]])
    out["b_f001_atten"] = out.pop("b_f001_rec")[..., H.REC["ATTEN"]]
    # what the fans must reach
    rec = np.concatenate([out["a_amp1_rec"], out["b_amp1_rec"]])
    n_valid = int((rec[..., H.REC["VALID"]] > 0).sum()); n_broke = int((rec[..., H.REC["BROKE"]] > 0).sum())
    longest = int(rec[..., H.REC["STEPS"]].max()); cells = ragged_cells(eq, rec)
    print(f"{sname}: fans a + b (amplitudes on): {n_valid} VALID legs, {n_broke} BROKE, longest leg {longest} steps, arrivals in {len(cells)} cells {sorted(cells)}")
    assert n_valid >= 15 and n_broke >= 10 and longest > 15000 and len(cells) >= 6
    path = os.path.join(OUT, f"rngdep_ragged_{sname}.npz")
    np.savez_compressed(path, **out)
    print(f"ragged {sname} ->", path, os.path.getsize(path) // 1024, "KiB;", os.path.getsize(RD.RAGGED_NPZ) // 1024, "KiB grid")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ragged3d":
        main_ragged(H.EQ_3D_RNGDEP)
    elif len(sys.argv) > 1 and sys.argv[1] == "raggedglobal":
        main_ragged(H.EQ_GLOBAL_RNGDEP)
    elif len(sys.argv) > 1 and sys.argv[1] == "jet":
        main_jet()
    elif len(sys.argv) > 1 and sys.argv[1] == "polar":
        main_polar()
    elif len(sys.argv) > 1 and sys.argv[1] == "globalrd_polar":
        main_globalrd_polar()
    elif len(sys.argv) > 1 and sys.argv[1] == "globalrd":
        main_globalrd()
    elif len(sys.argv) > 1 and sys.argv[1] == "rngdep":
        main_rngdep()
    else:
        main()
