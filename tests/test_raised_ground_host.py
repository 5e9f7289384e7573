"""The raised-ground closed forms (tests/raised_ground.py) without a GPU: the plain-C oracle's records of the four fans, and the numpy restatements
of every post-launch product run on them, held to the forms that tests/test_gpu_raised_ground.py holds the device to.  This proves that the forms
are right, that the inputs meet every condition the GPU tests rely on (hit counts, shares of cells left out, margins from cell borders, the
r_earth-versus-rg separation) and that every tolerance is one the reference itself stays within.  The measured figures are printed
(profiles/raised_ground_known_answers.txt keeps them beside the device's)."""
import numpy as np
import pytest

import harness as H
import raised_ground as RGD
import refine_reference as RR
import station_reference as SR

SETS = RGD.ALL_SETS


class _Twin:
    """the oracle's lattice launch of one set and everything the restatements make of it"""

    def __init__(self, eq, tmpdir):
        self.eq = eq
        self.O = RGD.oracle(eq, tmpdir)
        self.th, self.ph, self.nt, self.nph = RGD.lattice()
        self.cfg = RGD.cfg(eq)
        self.rec = self.launch(self.th, self.ph)
        self.sta, self.t_star, self.delta = RGD.ground_stations(eq, self.launch)
        self.level = np.zeros((1, 1) + self.rec.shape[:2])
        self.sp = SR.spec(self.nt, self.nph, phi_periodic=True, cap=4)
        self.hits, self.rows, _ = SR.reference_stations(eq, self.rec[None], self.th, self.ph, self.level, self.sp, self.sta)
        self.mem = RR.members(eq, [RGD.SRC[eq]], (0.0, 0.0) if eq == H.EQ_3D else None)          # windless: u / c = v / c = 0 at the source

    def launch(self, th, ph):
        return self.O.fan(self.cfg, th, ph)[1]

    def refine(self, **kw):
        return RR.reference_refine(self.eq, self.hits, self.rows, self.sta, RR.spec(**kw), lambda a, b: self.launch(a, b)[None], self.mem,
                                   r_earth=RGD.R_EARTH, z_grnd=RGD.Z_GRND)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    made = {}

    def get(eq):
        if eq not in made:
            made[eq] = _Twin(eq, tmp_path_factory.mktemp(f"rg{eq}"))
        return made[eq]
    return get


def _show(eq, part, figures):
    print(f"raised ground, oracle, {H.EQ_NAMES[eq]}, {part}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))


@pytest.mark.parametrize("eq", SETS)
def test_launch_records(twins, eq):
    _show(eq, "launch", RGD.check_launch(eq, twins(eq).rec))


@pytest.mark.parametrize("eq", SETS)
def test_stations(twins, eq):
    t = twins(eq)
    _show(eq, "stations (not gated)", RGD.check_station_lists(t.hits[0], t.rows[0], t.t_star))


@pytest.mark.parametrize("eq", SETS)
def test_refinement(twins, eq):
    t = twins(eq)
    rows, _, stats, _ = t.refine(**RGD.GROUND_SPEC)
    lattice_delta = RGD.check_axial_symmetry(eq, t.rec)[0] if eq in RGD.SPHERICAL else None
    print(stats, "rounds", rows[:, RR.RFN["ITER"]].astype(int).tolist())
    _show(eq, "refinement", RGD.check_refined(eq, rows, t.sta, t.t_star, t.delta, lattice_delta))
    _show(eq, "miss, converged rows", RGD.check_miss(eq, rows, t.sta, t.launch, separated=False))
    first, _, stats1, _ = t.refine(**dict(RGD.GROUND_SPEC, max_iter=1, tol=1e-9))
    assert stats1["launches"] == 1 and (first[:, RR.RFN["STATUS"]] == RR.ITER_LIMIT).all()
    _show(eq, "miss, first round", RGD.check_miss(eq, first, t.sta, t.launch, separated=True))


@pytest.mark.parametrize("eq", SETS)
def test_tube_map_and_arrival_map(twins, eq):
    import map_reference as MR
    import tubemap_reference as TR
    t = twins(eq)
    sp = RGD.tube_spec(eq)
    layers = TR.reference_tubemap(eq, t.rec[None], t.th, t.ph, t.level, sp)
    _show(eq, "tube map", RGD.check_tubemap(eq, layers["count"][0], t.rec, sp))
    half = RGD.tube_spec(eq, east_half=True)
    _show(eq, "tube map, eastern half", RGD.check_tubemap(eq, TR.reference_tubemap(eq, t.rec[None], t.th, t.ph, t.level, half)["count"][0], t.rec, half))
    flat = RGD.station_cells(eq, sp, t.sta, layers["count"][0])
    hits, rows, _ = SR.reference_stations(eq, t.rec[None], t.th, t.ph, t.level, dict(t.sp, edge_max=sp["edge_max"]), TR.centres(sp)[flat])
    RGD.check_ttime_min_at_centres(layers["ttime_min"][0], flat, hits[0], rows[0])
    msp = RGD.map_spec(eq)
    _show(eq, "arrival map", RGD.check_arrival_map(eq, MR.reference_map(eq, t.rec[None], t.level, msp), t.rec, msp))


# ---- levels: the oracle's paths through the restatement of k_levels ----
class _LevelTwin:
    """the lattice launch with one bounce as the oracle's paths (without amplitudes: crossings take positions and times only), its crossing tables by
    the restatement of k_levels, and the two columns of the arrival records that check_levels reads, taken from the paths' own leg ends"""

    def __init__(self, eq, O):
        import levels_reference as LV
        self.eq, self.O, self.LV = eq, O, LV
        self.cfg = H.make_cfg(eq, calc_amp=False, src=RGD.SRC[eq], z_grnd=RGD.Z_GRND, **RGD.LEVEL_PARAMS)
        self.th, self.ph, self.nt, self.nph = RGD.lattice()
        paths = [O.trace_path(self.cfg, t, p) for t, p in zip(self.th, self.ph)]
        self.count, self.lrec = LV.restate_fan(eq, paths, RGD.LEVELS, 8)
        self.rec = np.zeros((len(paths), 2, H.REC_STRIDE))
        for r, legs in enumerate(paths):
            assert len(legs) == 2
            for leg, (k, rows, _) in enumerate(legs):
                self.rec[r, leg, H.REC["VALID"]] = 1.0 if k > 0 else 0.0            # (k < 0: the leg ended by the break check)
                self.rec[r, leg, RGD.S0:RGD.S0 + 3] = rows[-1, :3]

    def integrate(self, th, ph):
        count, lrec = self.LV.restate_fan(self.eq, [self.O.trace_path(self.cfg, t, p) for t, p in zip(th, ph)], RGD.LEVELS, 8)
        return count[None], lrec[None]


@pytest.mark.parametrize("eq", [H.EQ_3D, H.EQ_3D_RNGDEP])
def test_levels_level_stations_and_level_refinement(twins, eq):
    import level_refine_reference as LR
    import lstation_reference as LS
    t = _LevelTwin(eq, twins(eq).O)
    _show(eq, "levels", RGD.check_levels(eq, t.rec, t.count, t.lrec))
    for br in RGD.BRANCHES:
        sta, lv = RGD.level_stations_of(eq, br)
        sp = LS.spec(t.nt, t.nph, phi_periodic=True, ord_max=2, cap=4, **br["lsta"])
        hits, rows = LS.reference_level_stations(eq, t.count[None], t.lrec[None], t.th, t.ph, 2, sp, sta, lv)
        RGD.check_level_station_lists(br, hits[0], rows[0])
        out, stats, _ = LR.reference_level_refine(eq, hits, rows, sta, lv, RGD.LEVELS, LR.spec(**RGD.LEVEL_SPEC), t.integrate, LR.sources(eq, [RGD.SRC[eq]]))
        print(stats)
        _show(eq, f"level refinement, leg {br['leg']}", RGD.check_level_refined(eq, br, out, sta))


def test_miss_check_refuses_the_sphere_radius(twins):
    """the restatement run with z_grnd = 0 measures its misses on r_earth, as a kernel would that took the sphere radius for the ground radius:
    check_miss refuses its first-round rows (and accepts those measured at rg: test_refinement)"""
    t = twins(H.EQ_GLOBAL)
    first, _, _, _ = RR.reference_refine(t.eq, t.hits, t.rows, t.sta, RR.spec(**dict(RGD.GROUND_SPEC, max_iter=1, tol=1e-9)), lambda a, b: t.launch(a, b)[None], t.mem,
                                         r_earth=RGD.R_EARTH, z_grnd=0.0)
    with pytest.raises(AssertionError):
        RGD.check_miss(t.eq, first, t.sta, t.launch, separated=True)
