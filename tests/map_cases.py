"""The parity cases of the arrival-map tests: launch set-up and grid literals, shared by tests/test_maps_host.py (which proves on the CPU oracle's
records that every grid meets the non-vacuity conditions) and tests/test_gpu_maps.py (which runs them on the device).  Grid extents and detect_db
were chosen from the oracle's arrivals; they are literals, not derived from the code under test."""
import numpy as np

import harness as H
import map_reference as MR
import rngdep_data as RD
from test_gpu_ensemble import _angles, _raw_members
from test_gpu_freqs import FREQS
from test_gpu_sources import SOURCES

# grids per equation set: every arrival of the 97-ray fan of _angles() through ToyAtmo and its perturbed members, three legs
GRID_2D = dict(origin=200.0, step=25.0, n=64)                                        # range 200 .. 1800 km
GRID_3D = dict(origin=(-1850.0, -950.0), step=(50.0, 50.0), n=(58, 47))             # x -1850 .. 1050, y -950 .. 1400 km
GRID_GLOBAL = dict(origin=(21.0, -16.0), step=(0.5, 0.5), n=(44, 54))               # lat 21 .. 43, lon -16 .. 11 deg
GRID_3D_SOURCES = dict(origin=(-2000.0, -1100.0), step=(50.0, 50.0), n=(61, 51))    # the four sources of test_gpu_sources.SOURCES
GRID_GLOBAL_2SRC = dict(origin=(20.0, -120.0), step=(1.0, 1.0), n=(26, 132))        # sources (30, 0) and (45, -100)
GRID_3DRD = dict(origin=(-1000.0, -800.0), step=(500.0, 400.0), n=(4, 4))           # the cells of the synthetic grid of profiles
GRID_GLOBALRD = dict(origin=(25.0, -8.0), step=(3.0, 4.0), n=(4, 4))
GRIDS = {H.EQ_2D: GRID_2D, H.EQ_3D: GRID_3D, H.EQ_GLOBAL: GRID_GLOBAL}
# detection thresholds [dB]: with amplitudes the level is 20 log10(AMP) - ATTEN, without them -ATTEN
DETECT_AMP, DETECT_NOAMP = -70.0, -1.0

CASES = {}
for _eq in (H.EQ_2D, H.EQ_3D, H.EQ_GLOBAL):
    for _amp in (0, 1):
        for _b in (0, 2):
            CASES[f"plain-{H.EQ_NAMES[_eq]}-amp{_amp}-b{_b}"] = dict(kind="plain", eq=_eq, params=dict(bounces=_b, calc_amp=_amp),
                                                                    spec=dict(GRIDS[_eq], detect_db=DETECT_AMP if _amp else DETECT_NOAMP))
CASES["ensemble3-global"] = dict(kind="ensemble", eq=H.EQ_GLOBAL, params=dict(bounces=2, calc_amp=1), spec=dict(GRID_GLOBAL, detect_db=DETECT_AMP))
CASES["sources4-3d"] = dict(kind="sources", eq=H.EQ_3D, n_src=4, n_prof=1, params=dict(bounces=2, calc_amp=1), spec=dict(GRID_3D_SOURCES, detect_db=DETECT_AMP))
CASES["sources2x3-global"] = dict(kind="sources", eq=H.EQ_GLOBAL, n_src=2, n_prof=3, params=dict(bounces=2, calc_amp=1), spec=dict(GRID_GLOBAL_2SRC, detect_db=DETECT_AMP))
CASES["freqs4-global"] = dict(kind="freqs", eq=H.EQ_GLOBAL, freqs=FREQS[:4], params=dict(bounces=2, calc_amp=1), spec=dict(GRID_GLOBAL, detect_db=-80.0))
CASES["3drd"] = dict(kind="3drd", eq=H.EQ_3D_RNGDEP, params=dict(bounces=1, calc_amp=1, mode=0, src=(0.0, 0.0, 0.0)), spec=dict(GRID_3DRD, detect_db=DETECT_AMP))
CASES["globalrd"] = dict(kind="globalrd", eq=H.EQ_GLOBAL_RNGDEP, params=dict(bounces=1, calc_amp=1, mode=0, src=(0.0, 31.0, 0.0)), spec=dict(GRID_GLOBALRD, detect_db=DETECT_AMP))

# longitude wrap: a fan from lon 179.5 whose eastbound rays cross the date line (the state's longitude is continuous: they arrive at 180 .. 190 deg)
WRAP_SRC = (0.0, 30.0, 179.5)
WRAP_GRID_0 = dict(origin=(21.0, 0.0), step=(0.5, 0.5), n=(44, 720))                # origin[1] = 0: lon 0 .. 360, the wrap leaves 164 .. 190 where it is
WRAP_GRID_180 = dict(origin=(21.0, -180.0), step=(0.5, 0.5), n=(44, 720))           # lon -180 .. 180: arrivals beyond 180 are inside only when wrapped


def gold_angles(kind):
    g = np.load(f"{H.GOLDEN_DIR}/{'3drd' if kind == '3drd' else 'globalrd'}_small.npz")
    return g["theta"], g["phi"]


def write_grid(kind, dirpath):
    return RD.write_grid(dirpath, short_paths=False) if kind == "3drd" else RD.write_grid_global(dirpath, short_paths=False)


def case_angles(case):
    return gold_angles(case["kind"]) if case["kind"] in ("3drd", "globalrd") else _angles()


def oracle_tables(case, tmpdir):
    """the case's launch on the CPU oracle: rec [M][n_rays][legs][32], atten [F][n_rays][legs]"""
    eq, kind, prm = case["eq"], case["kind"], case["params"]
    th, ph = case_angles(case)
    cfg = dict(bounces=prm["bounces"], calc_amp=bool(prm["calc_amp"]))
    if "src" in prm:
        cfg["src"] = prm["src"]
    recs, atten = [], None
    if kind == "plain":
        recs.append(H.Oracle(eq, H.TOYATMO).fan(H.make_cfg(eq, **cfg), th, ph)[1])
    elif kind == "ensemble":
        for raw in _raw_members():
            O = H.Oracle(eq, met=None)
            O.load_arrays(*raw)
            recs.append(O.fan(H.make_cfg(eq, **cfg), th, ph)[1])
    elif kind == "sources":
        for src in SOURCES[eq][:case["n_src"]]:
            for raw in (_raw_members() if case["n_prof"] > 1 else [None]):
                O = H.Oracle(eq, H.TOYATMO if raw is None else None)
                if raw is not None:
                    O.load_arrays(*raw)
                recs.append(O.fan(H.make_cfg(eq, src=tuple(src), **cfg), th, ph)[1])
    elif kind == "freqs":
        O = H.Oracle(eq, H.TOYATMO)
        per_f = [O.fan(H.make_cfg(eq, freq=f, **cfg), th, ph)[1] for f in case["freqs"]]
        recs.append(per_f[0])
        atten = np.stack([r[:, :, H.REC["ATTEN"]] for r in per_f])
    else:
        O = H.Oracle(eq, met=None)
        O.load_grid(*write_grid(kind, str(tmpdir)))
        recs.append(O.fan(H.make_cfg(eq, **cfg), th, ph)[1])
    rec = np.stack(recs)
    if atten is None:
        atten = rec[0, :, :, H.REC["ATTEN"]][None]
    return rec, atten


def reference_of(case, rec, atten, level=None, **spec_overrides):
    """reference map of a case's tables; level defaults to the numpy level table (host tests)"""
    sp = MR.spec(**dict(case["spec"], **spec_overrides))
    if level is None:
        level = MR.level_numpy(rec, atten, case["params"]["calc_amp"])
    return sp, MR.reference_map(case["eq"], rec, level, sp)
