"""ctypes mirror of include/geoac_hip.h + include/geoac_host.h (libgeoac_hip.so, built in-tree by
geoac_amd/csrc/Makefile or __graft_entry__.build()).  Names follow the reference's vocabulary:
rays, legs (bounces), launch angles theta/phi, arrivals."""
import ctypes
import os

import numpy as np

EQ_2D, EQ_3D, EQ_GLOBAL, EQ_3D_RNGDEP, EQ_GLOBAL_RNGDEP = 0, 1, 2, 3, 4
REC_STRIDE = 32
REC = dict(VALID=0, STEPS=1, BROKE=2, TTIME=3, ATTEN=4, TURN=5, INCL=6, BACKAZ=7, AMP=8, RANGE=9, JACOB=10, STATE=12)
MODE_WRITE_RAYS, MODE_WRITE_CAUSTICS, MODE_INTERACTIVE = 1, 2, 4
FAN_STEP_LIMIT, FAN_SUB_FALLBACK, FAN_ABS_FALLBACK = 1, 0x100, 0x200          # geoac_fan_status (include/geoac_hip.h)

_dp = ctypes.POINTER(ctypes.c_double)


class GeoAcError(RuntimeError):
    pass


class Params(ctypes.Structure):
    """geoac_params (include/geoac_hip.h): the reference's globals + *_RunProp locals."""
    _fields_ = [("ds_min", ctypes.c_double), ("ds_max", ctypes.c_double), ("ray_limit", ctypes.c_double),
                ("vert_limit", ctypes.c_double), ("range_limit", ctypes.c_double), ("z_grnd", ctypes.c_double),
                ("r_earth", ctypes.c_double), ("tweak_abs", ctypes.c_double), ("freq", ctypes.c_double),
                ("src", ctypes.c_double * 3), ("bounces", ctypes.c_int), ("calc_amp", ctypes.c_int),
                ("mode", ctypes.c_int), ("sample_stride", ctypes.c_int), ("xy_limits", ctypes.c_double * 4)]


class MapSpec(ctypes.Structure):
    """geoac_map_spec (include/geoac_map.h): grid, filters and detection threshold of an arrival map"""
    _fields_ = [("origin", ctypes.c_double * 2), ("step", ctypes.c_double * 2), ("n", ctypes.c_int * 2), ("wrap_lon", ctypes.c_int),
                ("leg_min", ctypes.c_int), ("leg_max", ctypes.c_int), ("turn_min", ctypes.c_double), ("turn_max", ctypes.c_double),
                ("detect_db", ctypes.c_double)]


MAP_COUNT, MAP_TTIME_MIN, MAP_CEL_MAX, MAP_LEVEL_MAX, MAP_BEST = 0, 1, 2, 3, 4
_MAP_LAYERS = (("count", MAP_COUNT, np.uint64), ("ttime_min", MAP_TTIME_MIN, np.float64), ("cel_max", MAP_CEL_MAX, np.float64),
               ("level_max", MAP_LEVEL_MAX, np.float64), ("best", MAP_BEST, np.int64))


def map_spec(origin, step, n, wrap_lon=False, leg_min=0, leg_max=2**31 - 1, turn_min=-np.inf, turn_max=np.inf, detect_db=np.nan):
    """a MapSpec from plain values; one-axis grids (the 2-D set) may give scalars: axis 1 then is a single cell"""
    origin, step, n = (list(np.atleast_1d(a)) for a in (origin, step, n))
    if len(origin) == 1:
        origin, step, n = origin + [0.0], step + [1.0], n + [1]
    return MapSpec((ctypes.c_double * 2)(*[float(v) for v in origin]), (ctypes.c_double * 2)(*[float(v) for v in step]), (ctypes.c_int * 2)(*[int(v) for v in n]),
                   1 if wrap_lon else 0, int(leg_min), int(leg_max), float(turn_min), float(turn_max), float(detect_db))


def map_check(eqset, spec):
    """geoac_map_check: host-only validation (no GPU needed); returns the cell count or raises GeoAcError"""
    cells = ctypes.c_int64(0)
    rc = load_library().geoac_map_check(int(eqset), ctypes.byref(spec), ctypes.byref(cells))
    if rc:
        raise GeoAcError(f"geoac_map_check: {load_library().geoac_strerror(rc).decode()}")
    return int(cells.value)


MAX_LEVELS, LVL_STRIDE = 8, 12
LVL = dict(LEG=0, DIR=1, FRAC=2, TTIME=3, ATTEN=4, P0=5)      # a crossing record (include/geoac_levels.h)


def levels_check(eqset, params, z_km, cap=8):
    """geoac_levels_check: host-only validation of a level list against `params` (no GPU needed); raises GeoAcError with the status and the fault"""
    lib = load_library()
    z = _arr(z_km).reshape(-1)
    fault = ctypes.c_char_p()
    rc = lib.geoac_levels_check(int(eqset), ctypes.byref(params), len(z), _p(z) if len(z) else None, int(cap), ctypes.byref(fault))
    if rc:
        raise GeoAcError(f"geoac_levels_check: {lib.geoac_strerror(rc).decode()}: {fault.value.decode() if fault.value else ''}")


class StationSpec(ctypes.Structure):
    """geoac_station_spec (include/geoac_stations.h): lattice of the launch angles, filters and list length of a station search"""
    _fields_ = [("n_theta", ctypes.c_int), ("n_phi", ctypes.c_int), ("phi_periodic", ctypes.c_int), ("leg_min", ctypes.c_int), ("leg_max", ctypes.c_int),
                ("turn_tol", ctypes.c_double), ("edge_max", ctypes.c_double), ("cap", ctypes.c_int)]


STA_STRIDE = 16
STA = dict(LEG=0, TRI=1, RAY0=2, ORIENT=3, W0=4, W1=5, W2=6, THETA=7, PHI=8, TTIME=9, CELERITY=10, TURN=11, INCL=12, BACKAZ=13)


def station_spec(n_theta, n_phi, phi_periodic=False, leg_min=0, leg_max=2**31 - 1, turn_tol=np.inf, edge_max=np.inf, cap=16):
    """a StationSpec from plain values"""
    return StationSpec(int(n_theta), int(n_phi), 1 if phi_periodic else 0, int(leg_min), int(leg_max), float(turn_tol), float(edge_max), int(cap))


def station_check(eqset, spec, n_rays, n_sta):
    """geoac_station_check: host-only validation (no GPU needed); raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_station_fault.restype = ctypes.c_char_p
    rc = lib.geoac_station_check(int(eqset), ctypes.byref(spec), int(n_rays), int(n_sta))
    if rc:
        fault = lib.geoac_station_fault(int(eqset), ctypes.byref(spec), int(n_rays), int(n_sta))
        raise GeoAcError(f"geoac_station_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")


class LStationSpec(ctypes.Structure):
    """geoac_lstation_spec (include/geoac_lstations.h): lattice of the launch angles, legs and ordinals that take part, edge filter and list length
    of a level-station search"""
    _fields_ = [("n_theta", ctypes.c_int), ("n_phi", ctypes.c_int), ("phi_periodic", ctypes.c_int), ("leg_min", ctypes.c_int), ("leg_max", ctypes.c_int),
                ("ord_max", ctypes.c_int), ("edge_max", ctypes.c_double), ("cap", ctypes.c_int)]


LSTA_STRIDE = 16
LSTA = dict(LEG=0, DIR=1, ORD=2, TRI=3, RAY0=4, ORIENT=5, W0=6, W1=7, W2=8, THETA=9, PHI=10, TTIME=11, ATTEN=12, N0=13)


def lstation_spec(n_theta, n_phi, phi_periodic=False, leg_min=0, leg_max=2**31 - 1, ord_max=1, edge_max=np.inf, cap=16):
    """an LStationSpec from plain values"""
    return LStationSpec(int(n_theta), int(n_phi), 1 if phi_periodic else 0, int(leg_min), int(leg_max), int(ord_max), float(edge_max), int(cap))


def _level_of(level_of):
    return np.ascontiguousarray(level_of, dtype=np.int32).reshape(-1)


def lstation_check(eqset, spec, n_rays, n_levels, level_of):
    """geoac_lstation_check: host-only validation (no GPU needed) of a spec and the stations' level indices; raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_lstation_fault.restype = ctypes.c_char_p
    lv = _level_of(level_of)
    args = (int(eqset), ctypes.byref(spec), int(n_rays), int(n_levels), len(lv), lv.ctypes.data_as(ctypes.c_void_p))
    rc = lib.geoac_lstation_check(*args)
    if rc:
        raise GeoAcError(f"geoac_lstation_check: {lib.geoac_strerror(rc).decode()}: {lib.geoac_lstation_fault(*args).decode()}")


class RefineSpec(ctypes.Structure):
    """geoac_refine_spec (include/geoac_refine.h): round limit, shrink limit, tolerance [km] and step cut [deg] of a station refinement"""
    _fields_ = [("max_iter", ctypes.c_int), ("max_shrink", ctypes.c_int), ("tol", ctypes.c_double), ("step_max_deg", ctypes.c_double)]


RFN_STRIDE = 16
RFN = dict(MEMBER=0, STATION=1, LEG=2, TRI=3, STATUS=4, ITER=5, THETA=6, PHI=7, MISS=8, TTIME=9, CELERITY=10, TURN=11, INCL=12, BACKAZ=13, AMP=14, JACOB=15)
RFN_STATUS = dict(CONVERGED=1, ITER_LIMIT=2, STALLED=3, LOST=4, SINGULAR=5)
RFN_MAX_RAY_MEMBERS = 1 << 20


def refine_spec(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2):
    """a RefineSpec from plain values"""
    return RefineSpec(int(max_iter), int(max_shrink), float(tol), float(step_max_deg))


def refine_check(eqset, spec):
    """geoac_refine_check: host-only validation (no GPU needed); raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_refine_fault.restype = ctypes.c_char_p
    rc = lib.geoac_refine_check(int(eqset), ctypes.byref(spec))
    if rc:
        fault = lib.geoac_refine_fault(int(eqset), ctypes.byref(spec))
        raise GeoAcError(f"geoac_refine_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")


class LevelRefineSpec(ctypes.Structure):
    """geoac_level_refine_spec (include/geoac_level_refine.h): round limit, shrink limit, tolerance [km], step cut [deg] and finite-difference
    step [deg] of a level refinement"""
    _fields_ = [("max_iter", ctypes.c_int), ("max_shrink", ctypes.c_int), ("tol", ctypes.c_double), ("step_max_deg", ctypes.c_double), ("probe_deg", ctypes.c_double)]


LRF_STRIDE = 16
LRF = dict(MEMBER=0, STATION=1, LEG=2, DIR=3, ORD=4, STATUS=5, ITER=6, THETA=7, PHI=8, MISS=9, TTIME=10, CELERITY=11, ATTEN=12, N0=13)
LRF_STATUS = RFN_STATUS


def level_refine_spec(max_iter=8, max_shrink=4, tol=0.1, step_max_deg=0.2, probe_deg=0.02):
    """a LevelRefineSpec from plain values"""
    return LevelRefineSpec(int(max_iter), int(max_shrink), float(tol), float(step_max_deg), float(probe_deg))


def level_refine_check(eqset, spec):
    """geoac_level_refine_check: host-only validation (no GPU needed); raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_level_refine_fault.restype = ctypes.c_char_p
    rc = lib.geoac_level_refine_check(int(eqset), ctypes.byref(spec))
    if rc:
        fault = lib.geoac_level_refine_fault(int(eqset), ctypes.byref(spec))
        raise GeoAcError(f"geoac_level_refine_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")


LAMP_STRIDE = 16
LAMP = dict(MEMBER=0, INDEX=1, LEG=2, DIR=3, ORD=4, STATUS=5, THETA=6, PHI=7, DET=8, TZ=9, D=10, AMP=11, C=12, RHO=13, TTIME=14, ATTEN=15)
LAMP_STATUS = dict(OK=1, ABSENT=2, NO_PROBE=3, SINGULAR=4, SKIPPED=5)


def level_amp_check(eqset, probe_deg):
    """geoac_level_amp_check: host-only validation (no GPU needed); raises GeoAcError naming the fault"""
    lib = load_library()
    fault = ctypes.c_char_p()
    rc = lib.geoac_level_amp_check(int(eqset), ctypes.c_double(float(probe_deg)), ctypes.byref(fault))
    if rc:
        raise GeoAcError(f"geoac_level_amp_check: {lib.geoac_strerror(rc).decode()}: {fault.value.decode()}")


class TubeSpec(ctypes.Structure):
    """geoac_tube_spec (include/geoac_tubemap.h): the grid of a MapSpec, the lattice and triangle filters of a StationSpec, the band on a hit's
    interpolated turning height and the detection threshold of a tube map"""
    _fields_ = [("origin", ctypes.c_double * 2), ("step", ctypes.c_double * 2), ("n", ctypes.c_int * 2), ("wrap_lon", ctypes.c_int),
                ("n_theta", ctypes.c_int), ("n_phi", ctypes.c_int), ("phi_periodic", ctypes.c_int), ("leg_min", ctypes.c_int), ("leg_max", ctypes.c_int),
                ("turn_tol", ctypes.c_double), ("edge_max", ctypes.c_double), ("turn_min", ctypes.c_double), ("turn_max", ctypes.c_double),
                ("detect_db", ctypes.c_double)]


TUBE = dict(COUNT=0, TTIME_MIN=1, CEL_MAX=2, LEVEL_MAX=3, BEST=4)
TUBE_MAX_SPAN, TUBE_COOP_MIN = 1 << 20, 32
_TUBE_LAYERS = (("count", TUBE["COUNT"], np.uint64), ("ttime_min", TUBE["TTIME_MIN"], np.float64), ("cel_max", TUBE["CEL_MAX"], np.float64),
                ("level_max", TUBE["LEVEL_MAX"], np.float64), ("best", TUBE["BEST"], np.int64))


def tube_spec(origin, step, n, n_theta, n_phi, edge_max, wrap_lon=False, phi_periodic=False, leg_min=0, leg_max=2**31 - 1, turn_tol=np.inf,
              turn_min=-np.inf, turn_max=np.inf, detect_db=np.nan):
    """a TubeSpec from plain values (edge_max has no default: it must be finite, it bounds the cells a landing triangle can cover)"""
    return TubeSpec((ctypes.c_double * 2)(*[float(v) for v in origin]), (ctypes.c_double * 2)(*[float(v) for v in step]), (ctypes.c_int * 2)(*[int(v) for v in n]),
                    1 if wrap_lon else 0, int(n_theta), int(n_phi), 1 if phi_periodic else 0, int(leg_min), int(leg_max), float(turn_tol), float(edge_max),
                    float(turn_min), float(turn_max), float(detect_db))


def tube_check(eqset, spec, n_rays):
    """geoac_tube_check: host-only validation (no GPU needed); returns the cell count or raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_tube_fault.restype = ctypes.c_char_p
    cells = ctypes.c_int64(0)
    rc = lib.geoac_tube_check(int(eqset), ctypes.byref(spec), int(n_rays), ctypes.byref(cells))
    if rc:
        fault = lib.geoac_tube_fault(int(eqset), ctypes.byref(spec), int(n_rays))
        raise GeoAcError(f"geoac_tube_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")
    return int(cells.value)


class LTubeSpec(ctypes.Structure):
    """geoac_ltube_spec (include/geoac_ltubemap.h): the grid of a MapSpec, the lattice, legs, ordinals and edge filter of an LStationSpec, and the
    directions and levels of a level tube map"""
    _fields_ = [("origin", ctypes.c_double * 2), ("step", ctypes.c_double * 2), ("n", ctypes.c_int * 2), ("wrap_lon", ctypes.c_int),
                ("n_theta", ctypes.c_int), ("n_phi", ctypes.c_int), ("phi_periodic", ctypes.c_int), ("leg_min", ctypes.c_int), ("leg_max", ctypes.c_int),
                ("ord_max", ctypes.c_int), ("edge_max", ctypes.c_double), ("dir_mask", ctypes.c_int), ("level_mask", ctypes.c_int)]


LTUBE = dict(COUNT=0, TTIME_MIN=1, ATTEN_MIN=2, FIRST=3)
_LTUBE_LAYERS = (("count", LTUBE["COUNT"], np.uint64), ("ttime_min", LTUBE["TTIME_MIN"], np.float64), ("atten_min", LTUBE["ATTEN_MIN"], np.float64),
                 ("first", LTUBE["FIRST"], np.int64))


def ltube_spec(origin, step, n, n_theta, n_phi, edge_max, level_mask, wrap_lon=False, phi_periodic=False, leg_min=0, leg_max=2**31 - 1, ord_max=1,
               dir_mask=3):
    """an LTubeSpec from plain values (edge_max has no default: it must be finite, it bounds the cells a crossing triangle can cover; level_mask
    has none either: bit l selects level l of the launch's list)"""
    return LTubeSpec((ctypes.c_double * 2)(*[float(v) for v in origin]), (ctypes.c_double * 2)(*[float(v) for v in step]), (ctypes.c_int * 2)(*[int(v) for v in n]),
                     1 if wrap_lon else 0, int(n_theta), int(n_phi), 1 if phi_periodic else 0, int(leg_min), int(leg_max), int(ord_max), float(edge_max),
                     int(dir_mask), int(level_mask))


def ltube_check(eqset, spec, n_rays, n_levels):
    """geoac_ltube_check: host-only validation (no GPU needed) against a launch of n_rays rays and n_levels levels; returns the cell count and the
    number of selected levels, or raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_ltube_fault.restype = ctypes.c_char_p
    cells, n_sel = ctypes.c_int64(0), ctypes.c_int(0)
    rc = lib.geoac_ltube_check(int(eqset), ctypes.byref(spec), int(n_rays), int(n_levels), ctypes.byref(cells), ctypes.byref(n_sel))
    if rc:
        fault = lib.geoac_ltube_fault(int(eqset), ctypes.byref(spec), int(n_rays), int(n_levels))
        raise GeoAcError(f"geoac_ltube_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")
    return int(cells.value), int(n_sel.value)


class LAmpMapSpec(ctypes.Structure):
    """geoac_lampmap_spec (include/geoac_lampmap.h): the fields of an LTubeSpec, then det_floor and detect_amp"""
    _fields_ = LTubeSpec._fields_ + [("det_floor", ctypes.c_double), ("detect_amp", ctypes.c_double)]


LAMPMAP = dict(COUNT=0, WEAK=1, AMP_MAX=2, RAMP_MAX=3, LOUDEST=4)
_LAMPMAP_LAYERS = (("count", LAMPMAP["COUNT"], np.uint64), ("weak", LAMPMAP["WEAK"], np.uint64), ("amp_max", LAMPMAP["AMP_MAX"], np.float64),
                   ("ramp_max", LAMPMAP["RAMP_MAX"], np.float64), ("loudest", LAMPMAP["LOUDEST"], np.int64))


def lampmap_spec(origin, step, n, n_theta, n_phi, edge_max, level_mask, wrap_lon=False, phi_periodic=False, leg_min=0, leg_max=2**31 - 1, ord_max=1,
                 dir_mask=3, det_floor=0.0, detect_amp=float("nan")):
    """an LAmpMapSpec from plain values: the arguments of ltube_spec(), the smallest |DET| a hit may have to carry an amplitude, and the received
    amplitude from which a member counts in the DETECT layer (NaN: no such layer)"""
    return LAmpMapSpec((ctypes.c_double * 2)(*[float(v) for v in origin]), (ctypes.c_double * 2)(*[float(v) for v in step]), (ctypes.c_int * 2)(*[int(v) for v in n]),
                       1 if wrap_lon else 0, int(n_theta), int(n_phi), 1 if phi_periodic else 0, int(leg_min), int(leg_max), int(ord_max), float(edge_max),
                       int(dir_mask), int(level_mask), float(det_floor), float(detect_amp))


def lampmap_check(eqset, spec, n_rays, n_levels):
    """geoac_lampmap_check: host-only validation (no GPU needed) against a launch of n_rays rays and n_levels levels; returns the cell count and the
    number of selected levels, or raises GeoAcError naming the first fault"""
    lib = load_library()
    lib.geoac_lampmap_fault.restype = ctypes.c_char_p
    cells, n_sel = ctypes.c_int64(0), ctypes.c_int(0)
    rc = lib.geoac_lampmap_check(int(eqset), ctypes.byref(spec), int(n_rays), int(n_levels), ctypes.byref(cells), ctypes.byref(n_sel))
    if rc:
        fault = lib.geoac_lampmap_fault(int(eqset), ctypes.byref(spec), int(n_rays), int(n_levels))
        raise GeoAcError(f"geoac_lampmap_check: {lib.geoac_strerror(rc).decode()}: {fault.decode()}")
    return int(cells.value), int(n_sel.value)


EIG_STRIDE = 16
EIG = dict(RCVR=0, INDEX=1, BOUNCES=2, THETA=3, PHI=4, TTIME=5, CELERITY=6, AMP_DB=7, ATTEN_DB=8, INCL=9, BEARING=10, BACKAZ=11,
           AZDEV=12, NSMP=13, SMP0=14)


class EigParams(ctypes.Structure):
    """geoac_eig_params (include/geoac_eig.h)"""
    _fields_ = [("theta_min", ctypes.c_double), ("theta_max", ctypes.c_double), ("bnc_min", ctypes.c_int), ("bnc_max", ctypes.c_int),
                ("iterations", ctypes.c_int), ("azimuth_err_lim", ctypes.c_double), ("verbose", ctypes.c_int)]


def library_path():
    """the in-tree build; GEOAC_LIB names another build of the same library (A/B and diagnostic builds: tools/ab_metric.py, -DGEOAC_KSTAT)"""
    return os.environ.get("GEOAC_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgeoac_hip.so")


_lib = None


def load_library():
    """dlopen libgeoac_hip.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise GeoAcError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"or `make -C geoac_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(path)
    lib.geoac_strerror.restype = ctypes.c_char_p
    lib.geoac_last_error.restype = ctypes.c_char_p
    lib.geoac_last_error.argtypes = [ctypes.c_void_p]
    lib.geoac_version.restype = ctypes.c_char_p
    lib.geoac_grid_load.argtypes = None
    lib.geoac_grid_load_eq.argtypes = None
    lib.geoac_fan_enumerate.restype = ctypes.c_long
    lib.geoac_fan_enumerate.argtypes = [ctypes.c_double] * 6 + [ctypes.c_long, _dp, _dp]
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(_dp)


def _arr(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---------------- host set-up helpers (include/geoac_host.h) ----------------
def met_load(path, eqset, fmt="zTuvdp"):
    """read a .met profile the way Spline_Single_G2S does; returns dict x,T,u,v,rho (x = radius for Global)."""
    lib = load_library()
    rows = lib.geoac_met_rows(path.encode())
    if rows < 3:
        raise GeoAcError(f"cannot read profile {path} (rows={rows})")
    a = [np.zeros(rows) for _ in range(5)]
    n = lib.geoac_met_load(path.encode(), fmt.encode(), eqset, rows, *[_p(t) for t in a])
    if n != rows:
        raise GeoAcError(f"geoac_met_load({path}) -> {n}")
    return dict(zip(("x", "T", "u", "v", "rho"), a))


def natural_spline_slopes(x, f):
    lib = load_library()
    x, f = _arr(x), _arr(f)
    s = np.zeros(len(x))
    lib.geoac_natural_spline_slopes(len(x), _p(x), _p(f), _p(s))
    return s


def fan_enumerate(theta_min=0.5, theta_max=45.0, theta_step=0.5, phi_min=-90.0, phi_max=-90.0, phi_step=1.0):
    """launch angles of the reference's double loop (repeated addition; phi outer, theta inner)."""
    lib = load_library()
    n = lib.geoac_fan_enumerate(theta_min, theta_max, theta_step, phi_min, phi_max, phi_step, 0, None, None)
    if n < 0:
        raise GeoAcError("fan_enumerate: bad step")
    th, ph = np.zeros(n), np.zeros(n)
    lib.geoac_fan_enumerate(theta_min, theta_max, theta_step, phi_min, phi_max, phi_step, n, _p(th), _p(ph))
    return th, ph


def default_params(eqset):
    p = Params()
    rc = load_library().geoac_default_params(eqset, ctypes.byref(p))
    if rc:
        raise GeoAcError("geoac_default_params failed")
    return p


# ---------------- launch-plan options (geoac_set_option) ----------------
# Options every new FanContext / FanPool gets (key without the GEOAC_ prefix -> value); tests and A/B tools set them through options() or
# directly.  The library itself reads no environment variable (unless GEOAC_DEBUG_ENV=1).
DEFAULT_OPTIONS = {}


class options:
    """with options(S_ROWS=4096, COMPACT=0): ...  -  contexts created inside carry these launch-plan options"""

    def __init__(self, **kw):
        self.kw = {str(k): str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = dict(DEFAULT_OPTIONS)
        DEFAULT_OPTIONS.update(self.kw)
        return self

    def __exit__(self, *exc):
        DEFAULT_OPTIONS.clear()
        DEFAULT_OPTIONS.update(self.old)
        return False


def build_id(path=None):
    """geoac_build_id of the loaded library (or of the library at `path`): the hash of the sources and flags it was compiled from"""
    lib = load_library() if path is None else ctypes.CDLL(path)
    lib.geoac_build_id.restype = ctypes.c_char_p
    return lib.geoac_build_id().decode()


def has_ab_kernels():
    """True for an A/B build of the library (`make AB=1`): it also holds the diagnostic kernels the launch plan never selects (DUO, GRID_LANES=2)"""
    lib = load_library()
    return bool(lib.geoac_build_has_ab())


def option_names():
    lib = load_library()
    lib.geoac_option_names.restype = ctypes.POINTER(ctypes.c_char_p)
    p, out, i = lib.geoac_option_names(), [], 0
    while p[i]:
        out.append(p[i].decode()); i += 1
    return out


def _apply_options(lib, h, opts):
    lib.geoac_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    for k, v in opts.items():
        k = str(k)
        if k.startswith("GEOAC_"):
            k = k[6:]
        rc = lib.geoac_set_option(h, k.encode(), str(v).encode())
        if rc:
            msg = lib.geoac_last_error(h)
            raise GeoAcError(f"geoac_set_option({k}={v}): {lib.geoac_strerror(rc).decode()}: {msg.decode() if msg else ''}")


# ---------------- the GPU fan context ----------------
class FanContext:
    """One geoac_ctx: a GPU, a stream, an atmosphere, a parameter set; runs fans of launch angles."""

    def __init__(self, eqset, device=0, stream=None, options=None):
        self.lib = load_library()
        self.eqset = eqset
        self._h = ctypes.c_void_p()
        rc = self.lib.geoac_create(ctypes.byref(self._h), eqset, device)
        if rc:
            raise GeoAcError(f"geoac_create: {self.lib.geoac_strerror(rc).decode()}")
        _apply_options(self.lib, self._h, dict(DEFAULT_OPTIONS, **(options or {})))
        if stream is not None:
            self._chk(self.lib.geoac_set_stream(self._h, ctypes.c_void_p(stream)))
        self.params = default_params(eqset)
        self.n_rays = 0
        self.n_members = 1
        self.n_sources = 1
        self._n_freq = 1

    def _chk(self, rc):
        if rc:
            msg = self.lib.geoac_last_error(self._h)
            raise GeoAcError(f"{self.lib.geoac_strerror(rc).decode()}: {msg.decode() if msg else ''}")

    def close(self):
        if self._h:
            self.lib.geoac_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self):
        """geoac_clone: a second context on the same device sharing this one's atmosphere tables (several fans at once); valid until this context uploads another
        atmosphere or is closed - after that the clone's launches fail"""
        c = object.__new__(FanContext)
        c.lib, c.eqset, c._h = self.lib, self.eqset, ctypes.c_void_p()
        self._chk(self.lib.geoac_clone(self._h, ctypes.byref(c._h)))
        c.params = Params.from_buffer_copy(bytes(self.params))
        c.n_rays = 0
        c.n_members = 1
        c.n_sources = 1
        c._n_freq = 1
        if hasattr(self, "_grid_dims"):
            c._grid_dims = self._grid_dims
        return c

    def upload_atmo_1d(self, x, T, u, v, rho, slopes4=None):
        x, T, u, v, rho = (_arr(a) for a in (x, T, u, v, rho))
        if slopes4 is None:
            slopes4 = np.concatenate([natural_spline_slopes(x, f) for f in (T, u, v, rho)])
        slopes4 = _arr(slopes4)
        self._chk(self.lib.geoac_upload_atmo_1d(self._h, len(x), _p(x), _p(T), _p(u), _p(v), _p(rho), _p(slopes4)))
        self.n_members = 1

    def upload_atmo_1d_ensemble(self, x, T, u, v, rho, slopes4=None):
        """K profiles on the shared nodes x (geoac_upload_atmo_1d_ensemble): T, u, v, rho [K][n]; slopes4 [K][4 n] (default: natural-spline
        slopes per member and field, as upload_atmo_1d).  fetch() / run() then return records of shape (K, n_rays, legs, 32)."""
        x = _arr(x)
        T, u, v, rho = (np.atleast_2d(_arr(a)) for a in (T, u, v, rho))
        K, n = T.shape
        if any(a.shape != (K, n) for a in (u, v, rho)) or x.shape != (n,):
            raise GeoAcError(f"upload_atmo_1d_ensemble: T, u, v, rho must be [K][n] arrays with n = len(x) (got x {x.shape}, T {T.shape}, u {u.shape}, v {v.shape}, rho {rho.shape})")
        if slopes4 is None:
            slopes4 = np.stack([np.concatenate([natural_spline_slopes(x, f[m]) for f in (T, u, v, rho)]) for m in range(K)])
        slopes4 = _arr(slopes4)
        if slopes4.size != K * 4 * n:
            raise GeoAcError(f"upload_atmo_1d_ensemble: slopes4 must hold [K][4 n] = {K * 4 * n} values (got {slopes4.size})")
        self._chk(self.lib.geoac_upload_atmo_1d_ensemble(self._h, K, n, _p(x), _p(T), _p(u), _p(v), _p(rho), _p(slopes4)))
        self.n_members = K

    def load_met_ensemble(self, paths, fmt="zTuvdp"):
        """one .met profile per member; the files must share their altitude column"""
        prof = [met_load(pth, self.eqset, fmt) for pth in paths]
        if not prof:
            raise GeoAcError("load_met_ensemble: no profiles")
        for pth, a in zip(paths[1:], prof[1:]):
            if a["x"].shape != prof[0]["x"].shape or not np.array_equal(a["x"], prof[0]["x"]):
                raise GeoAcError(f"load_met_ensemble: {pth} has other altitude nodes than {paths[0]} (an ensemble's members share their nodes)")
        self.upload_atmo_1d_ensemble(prof[0]["x"], *[np.stack([a[k] for a in prof]) for k in ("T", "u", "v", "rho")])
        return prof

    def upload_atmo_3d(self, x, y, z, T, u, v, rho):
        """grid of profiles: fields [nx][ny][nz] (winds already tapered, km/s)"""
        x, y, z, T, u, v, rho = (_arr(a) for a in (x, y, z, T, u, v, rho))
        self._chk(self.lib.geoac_upload_atmo_3d(self._h, len(x), len(y), len(z), _p(x), _p(y), _p(z), _p(T), _p(u), _p(v), _p(rho)))
        self._grid_dims = (len(x), len(y), len(z))
        self.n_members = 1

    def upload_atmo_3d_ensemble(self, x, y, z, T, u, v, rho):
        """K grids of profiles on the shared nodes x, y, z (geoac_upload_atmo_3d_ensemble): T, u, v, rho [K][nx][ny][nz], each member as upload_atmo_3d
        takes it.  fetch() / run() then return records of shape (K, n_rays, legs, 32)."""
        x, y, z = (_arr(a) for a in (x, y, z))
        T, u, v, rho = (_arr(a) for a in (T, u, v, rho))
        if T.ndim == 3:
            T, u, v, rho = (a[None] if a.ndim == 3 else a for a in (T, u, v, rho))
        if T.ndim != 4 or x.ndim != 1 or y.ndim != 1 or z.ndim != 1 or T.shape[1:] != (len(x), len(y), len(z)) or any(a.shape != T.shape for a in (u, v, rho)):
            raise GeoAcError(f"upload_atmo_3d_ensemble: T, u, v, rho must be [K][nx][ny][nz] arrays with nx, ny, nz = len(x), len(y), len(z) "
                             f"(got x {x.shape}, y {y.shape}, z {z.shape}, T {T.shape}, u {u.shape}, v {v.shape}, rho {rho.shape})")
        T, u, v, rho = (_arr(a) for a in (T, u, v, rho))
        K = T.shape[0]
        self._chk(self.lib.geoac_upload_atmo_3d_ensemble(self._h, K, len(x), len(y), len(z), _p(x), _p(y), _p(z), _p(T), _p(u), _p(v), _p(rho)))
        self._grid_dims = (len(x), len(y), len(z))
        self.n_members = K

    def grid_table(self):
        """the evaluation table the last upload_atmo_3d built on the device (layout of geoac_grid_table_eq)"""
        self.lib.geoac_grid_table_size.restype = ctypes.c_size_t
        n = self.lib.geoac_grid_table_size(*self._grid_dims)
        tab = np.zeros(n)
        self._chk(self.lib.geoac_grid_table_fetch(self._h, _p(tab), ctypes.c_size_t(n)))
        return tab

    def load_grid(self, prefix, locx, locy, fmt="zTuvdp", z_grnd=0.0):
        """Spline_Multi_G2S equivalent: <prefix><n>.met files + loc_x / loc_y node files"""
        g = self._read_grid(prefix, locx, locy, fmt, z_grnd)
        self.upload_atmo_3d(g["x"], g["y"], g["z"], g["T"], g["u"], g["v"], g["rho"])
        return g

    def load_grid_ensemble(self, grids, fmt="zTuvdp", z_grnd=0.0):
        """one grid specification (prefix, locx, locy) per member, each read as load_grid reads it; the members must share their x, y and z nodes"""
        grids = [tuple(g) for g in grids]
        if not grids:
            raise GeoAcError("load_grid_ensemble: no grids")
        mem = [self._read_grid(*g, fmt, z_grnd) for g in grids]
        for g, a in zip(grids[1:], mem[1:]):
            for k in ("x", "y", "z"):
                if a[k].shape != mem[0][k].shape or not np.array_equal(a[k], mem[0][k]):
                    raise GeoAcError(f"load_grid_ensemble: {g} has other {k} nodes than {grids[0]} (an ensemble's members share their nodes)")
        self.upload_atmo_3d_ensemble(mem[0]["x"], mem[0]["y"], mem[0]["z"], *[np.stack([a[k] for a in mem]) for k in ("T", "u", "v", "rho")])
        return mem

    def _read_grid(self, prefix, locx, locy, fmt, z_grnd):
        nx, ny, nz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if self.lib.geoac_grid_dims(prefix.encode(), locx.encode(), locy.encode(), ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(nz)):
            raise GeoAcError(f"cannot read grid {prefix}")
        nx, ny, nz = nx.value, ny.value, nz.value
        x, y, z = np.zeros(nx), np.zeros(ny), np.zeros(nz)
        F = [np.zeros((nx, ny, nz)) for _ in range(4)]
        rc = self.lib.geoac_grid_load_eq(self.eqset, prefix.encode(), locx.encode(), locy.encode(), fmt.encode(), ctypes.c_double(z_grnd),
                                      nx, ny, nz, _p(x), _p(y), _p(z), *[_p(f) for f in F])
        if rc:
            raise GeoAcError(f"geoac_grid_load_eq -> {rc}")
        return dict(x=x, y=y, z=z, T=F[0], u=F[1], v=F[2], rho=F[3])

    def load_met(self, path, fmt="zTuvdp"):
        a = met_load(path, self.eqset, fmt)
        self.upload_atmo_1d(a["x"], a["T"], a["u"], a["v"], a["rho"])
        return a

    def set_params(self, **kw):
        for k, val in kw.items():
            if k == "src":
                self.params.src = (ctypes.c_double * 3)(*val)
            elif k == "xy_limits":
                self.params.xy_limits = (ctypes.c_double * 4)(*val)
            else:
                setattr(self.params, k, val)
        self._chk(self.lib.geoac_set_params(self._h, ctypes.byref(self.params)))

    def set_sources(self, src):
        """source set (geoac_set_sources): src [n_src][3], each row in the layout of Params.src.  One launch then integrates the fan's angles from
        every source (and through every profile of an ensemble): fetch() / run() return (n_src, n_rays, legs, 32), or (n_src, K, n_rays, legs, 32)
        with an ensemble of K; rec[s] is bit-identical to a run with set_params(src=src[s]).  One row sets Params.src and leaves the mode."""
        src = _arr(src)
        if src.ndim != 2 or src.shape[1] != 3 or src.shape[0] < 1:
            raise GeoAcError(f"set_sources: src must be an array of shape [n_src][3] with n_src >= 1 (got {src.shape})")
        self._chk(self.lib.geoac_set_sources(self._h, src.shape[0], _p(src)))
        self.n_sources = src.shape[0]
        self.params.src = (ctypes.c_double * 3)(*src[0])

    def set_frequencies(self, freqs):
        """frequency set (geoac_set_frequencies): one launch then gives every arrival's attenuation at each of the frequencies [Hz] (at most 16); run() and
        fetch() are unchanged - the records are those of freq = freqs[0] - and fetch_atten() returns the table [F][n_rays][legs], atten[f] bit-identical
        to the ATTEN column of a run with set_params(freq=freqs[f]).  One frequency sets Params.freq and leaves the mode."""
        fr = _arr(freqs)
        if fr.ndim != 1:
            raise GeoAcError(f"set_frequencies: freqs must be a one-dimensional array (got shape {fr.shape})")
        self._chk(self.lib.geoac_set_frequencies(self._h, len(fr), _p(fr)))
        self._n_freq = len(fr)
        self.params.freq = float(fr[0])

    @property
    def n_frequencies(self):
        """frequencies of the active set (1: none)"""
        n = ctypes.c_int(0)
        self._chk(self.lib.geoac_get_frequencies(self._h, ctypes.byref(n)))
        return n.value

    def fetch_atten(self, out=None):
        """cumulative attenuation [dB] of the last launch per (frequency, ray, leg): [F][n_rays][legs] (F = 1 without a frequency set: the records' ATTEN
        column); `out`: a caller-owned C-contiguous float64 array of that shape"""
        shape = (self._n_freq, self.n_rays, self.params.bounces + 1)
        if out is None:
            att = np.empty(shape)
        else:
            att = out
            if not (isinstance(att, np.ndarray) and att.dtype == np.float64 and att.flags.c_contiguous and att.shape == shape):
                raise GeoAcError(f"fetch_atten(out=): need a C-contiguous float64 array of shape {shape}")
        self._chk(self.lib.geoac_fan_fetch_atten(self._h, _p(att)))
        return att

    # ---- level crossings (include/geoac_levels.h): found on the device behind the per-ray sums of every epoch; nothing is computed here ----
    def set_levels(self, z_km, cap=8):
        """geoac_set_levels: up to 8 altitudes [km above sea level], strictly ascending, above z_grnd and below the vertical limit; every later launch then
        keeps, per (ray, level), a count of the passages through the altitude and the first `cap` of them (1 .. 64).  An empty list leaves the mode."""
        z = _arr(z_km).reshape(-1)
        self._chk(self.lib.geoac_set_levels(self._h, len(z), _p(z) if len(z) else None, int(cap)))

    @property
    def levels(self):
        """(z_km, cap) of the current level list (an empty array: none)"""
        n, cap = ctypes.c_int(0), ctypes.c_int(0)
        z = np.zeros(MAX_LEVELS)
        self._chk(self.lib.geoac_get_levels(self._h, ctypes.byref(n), _p(z), ctypes.byref(cap)))
        return z[:n.value].copy(), cap.value

    def fetch_levels(self):
        """crossings of the last launch: (count, rec) - count int32 [M][n_rays][L], it keeps running past cap; rec float64 [M][n_rays][L][cap][12] in the
        LVL layout, the first `cap` crossings in path order, zero past the count.  M = n_sources * n_members, the axis dropped when M == 1 as fetch() drops it."""
        z, cap = self.levels
        shape = (self._launch_members(), self.n_rays, len(z))
        count = np.zeros(shape, dtype=np.int32)
        rec = np.zeros(shape + (cap, LVL_STRIDE))
        self._chk(self.lib.geoac_fan_fetch_levels(self._h, _p(rec), count.ctypes.data_as(ctypes.c_void_p)))
        if shape[0] == 1:
            count, rec = count[0], rec[0]
        return count, rec

    def levels_dev(self):
        """device buffers of the last launch's crossings: ((rec_ptr, rec_bytes), (count_ptr, count_bytes)), valid until the next launch or set_levels"""
        rp, rb, cp, cb = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
        self._chk(self.lib.geoac_fan_levels_dev(self._h, ctypes.byref(rp), ctypes.byref(rb), ctypes.byref(cp), ctypes.byref(cb)))
        return (rp.value, rb.value), (cp.value, cb.value)

    # ---- arrival maps (include/geoac_map.h): the binning runs on the device; nothing is computed here ----
    def _launch_members(self):
        return self.n_sources * self.n_members

    def fetch_level(self):
        """level [dB] of every arrival of the last launch, (calc_amp ? 20 log10(AMP) : 0) - ATTEN per frequency: [M][F][n_rays][legs], NaN where the leg
        wrote no row (M = n_sources * n_members, F = frequencies of the set)"""
        lv = np.empty((self._launch_members(), self._n_freq, self.n_rays, self.params.bounces + 1))
        self._chk(self.lib.geoac_fan_fetch_level(self._h, _p(lv)))
        return lv

    def map(self, spec=None, **kw):
        """geoac_fan_map of the last launch: `spec` a MapSpec, or the arguments of map_spec().  Returns a dict of numpy arrays: count, ttime_min, cel_max
        [M][n0][n1], level_max, best [M][F][n0][n1], outside [M], and detect [F][n0][n1] when detect_db is given.  May be called again with another
        spec without a new launch."""
        if spec is None:
            spec = map_spec(**kw)
        self._chk(self.lib.geoac_fan_map(self._h, ctypes.byref(spec)))
        out = self._fetch_layers("geoac_fan_map", _MAP_LAYERS, MAP_LEVEL_MAX, spec)
        out["outside"] = np.empty(out["count"].shape[0], dtype=np.uint64)
        self._chk(self.lib.geoac_fan_map_outside(self._h, out["outside"].ctypes.data_as(ctypes.c_void_p)))
        return out

    def _fetch_layers(self, fn, layers, first_mf, spec):
        """the layers of the current map made by `fn` (geoac_fan_map / geoac_fan_tubemap: <fn>_shape, <fn>_fetch, <fn>_fetch_detect) as a dict of
        numpy arrays; the layers from `first_mf` on are per frequency; detect when the spec has a detect_db"""
        M, F, n0, n1 = (ctypes.c_int(0) for _ in range(4))
        self._chk(getattr(self.lib, fn + "_shape")(self._h, *[ctypes.byref(v) for v in (M, F, n0, n1)]))
        M, F, n0, n1 = M.value, F.value, n0.value, n1.value
        out = {}
        for name, layer, dtype in layers:
            a = np.empty((M, n0, n1) if layer < first_mf else (M, F, n0, n1), dtype=dtype)
            self._chk(getattr(self.lib, fn + "_fetch")(self._h, layer, a.ctypes.data_as(ctypes.c_void_p)))
            out[name] = a
        if spec.detect_db == spec.detect_db:
            out["detect"] = np.empty((F, n0, n1), dtype=np.uint32)
            self._chk(getattr(self.lib, fn + "_fetch_detect")(self._h, out["detect"].ctypes.data_as(ctypes.c_void_p)))
        return out

    def map_timing(self):
        """HIP-event time of the last map() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_map_timing(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- station arrivals (include/geoac_stations.h): search and interpolation run on the device; nothing is computed here ----
    def stations(self, spec=None, sta=None, **kw):
        """geoac_fan_stations of the last launch: `spec` a StationSpec, or the arguments of station_spec(); sta [n_sta][2] in the map's axes (lat, lon
        [deg] / x, y [km]).  Returns hits [M][n_sta] u32 (the true count, may exceed cap), rows [M][n_sta][cap][STA_STRIDE] (columns STA) and level
        [M][n_sta][cap][F].  May be called again with another spec or other stations without a new launch."""
        if spec is None:
            spec = station_spec(**kw)
        sta = _arr(sta)
        if sta.ndim != 2 or sta.shape[1] != 2:
            raise GeoAcError(f"stations: sta must have shape [n_sta][2] (got {sta.shape})")
        self._chk(self.lib.geoac_fan_stations(self._h, ctypes.byref(spec), len(sta), _p(sta)))
        M, F, R, cap = (ctypes.c_int(0) for _ in range(4))
        self._chk(self.lib.geoac_fan_stations_shape(self._h, *[ctypes.byref(v) for v in (M, F, R, cap)]))
        M, F, R, cap = M.value, F.value, R.value, cap.value
        hits, rows, level = np.empty((M, R), dtype=np.uint32), np.empty((M, R, cap, STA_STRIDE)), np.empty((M, R, cap, F))
        self._chk(self.lib.geoac_fan_stations_fetch(self._h, hits.ctypes.data_as(ctypes.c_void_p), _p(rows), _p(level)))
        return hits, rows, level

    def stations_timing(self):
        """HIP-event time of the last stations() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_stations_timing(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- level stations (include/geoac_lstations.h): branch table, search and interpolation run on the device; nothing is computed here ----
    def level_stations(self, spec=None, sta=None, level_of=None, **kw):
        """geoac_fan_level_stations of the last launch (one with set_levels): `spec` an LStationSpec, or the arguments of lstation_spec(); sta [n_sta][2]
        in the map's axes (lat, lon [deg] / x, y [km]); level_of [n_sta] indices into the launch's level list.  Returns hits [M][n_sta] u32 (the true
        count, may exceed cap) and rows [M][n_sta][cap][LSTA_STRIDE] (columns LSTA).  May be called again with another spec or other stations
        without a new launch."""
        if spec is None:
            spec = lstation_spec(**kw)
        sta = _arr(sta)
        if sta.ndim != 2 or sta.shape[1] != 2:
            raise GeoAcError(f"level_stations: sta must have shape [n_sta][2] (got {sta.shape})")
        lv = _level_of(level_of)
        if len(lv) != len(sta):
            raise GeoAcError(f"level_stations: level_of must hold one level index per station (got {len(lv)} for {len(sta)} stations)")
        self._chk(self.lib.geoac_fan_level_stations(self._h, ctypes.byref(spec), len(sta), _p(sta), lv.ctypes.data_as(ctypes.c_void_p)))
        M, R, cap = (ctypes.c_int(0) for _ in range(3))
        self._chk(self.lib.geoac_fan_level_stations_shape(self._h, *[ctypes.byref(v) for v in (M, R, cap)]))
        M, R, cap = M.value, R.value, cap.value
        hits, rows = np.empty((M, R), dtype=np.uint32), np.empty((M, R, cap, LSTA_STRIDE))
        self._chk(self.lib.geoac_fan_level_stations_fetch(self._h, hits.ctypes.data_as(ctypes.c_void_p), _p(rows)))
        return hits, rows

    def level_stations_timing(self):
        """HIP-event time of the last level_stations() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_level_stations_timing(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- what the two refinements' wrappers do alike: the six counters of a *_stats call as a dict, the two times of a *_timing call ----
    def _rounds_stats(self, fn):
        st = np.zeros(6, dtype=np.uint64)
        self._chk(fn(self._h, st.ctypes.data_as(ctypes.c_void_p)))
        return dict(zip(("launches", "ray_members", "seeds", "converged", "stalled_or_limit", "lost_or_singular"), (int(v) for v in st)))

    def _rounds_timing(self, fn):
        ms = (ctypes.c_double * 2)(0.0, 0.0)
        self._chk(fn(self._h, ms))
        return dict(launch_ms=ms[0], kernel_ms=ms[1])

    # ---- station refinement (include/geoac_refine.h): rounds, step rule and rows run on the device; nothing is computed here ----
    def refine(self, spec=None, **kw):
        """geoac_fan_refine of the current station lists (stations() after a calc_amp = 1 lattice launch): `spec` a RefineSpec, or the arguments of
        refine_spec().  Returns rows [n_seeds][RFN_STRIDE] (columns RFN, status values RFN_STATUS), level [n_seeds][F] and a dict of counters.  The
        call replaces the context's launch angles and last launch by its own last round (n_rays becomes n_seeds when there are any)."""
        if spec is None:
            spec = refine_spec(**kw)
        self._chk(self.lib.geoac_fan_refine(self._h, ctypes.byref(spec)))
        n, F, it = (ctypes.c_int(0) for _ in range(3))
        self._chk(self.lib.geoac_fan_refine_shape(self._h, *[ctypes.byref(v) for v in (n, F, it)]))
        n, F = n.value, F.value
        rows, level = np.empty((n, RFN_STRIDE)), np.empty((n, F))
        self._chk(self.lib.geoac_fan_refine_fetch(self._h, _p(rows), _p(level)))
        if n:
            self.n_rays = n
        return rows, level, self._rounds_stats(self.lib.geoac_fan_refine_stats)

    def refine_timing(self):
        """HIP-event times of the last refine() [ms]: its launches, its own kernels"""
        return self._rounds_timing(self.lib.geoac_fan_refine_timing)

    # ---- level refinement (include/geoac_level_refine.h): rounds, probes, step rule and rows run on the device; nothing is computed here ----
    def level_refine(self, spec=None, **kw):
        """geoac_fan_level_refine of the current level-station lists (level_stations() after a lattice launch with levels): `spec` a LevelRefineSpec, or
        the arguments of level_refine_spec().  Returns rows [n_seeds][LRF_STRIDE] (columns LRF, status values LRF_STATUS) and a dict of counters.  The
        call replaces the context's launch angles and last launch by its own last round (n_rays becomes 3 * n_seeds when there are any)."""
        if spec is None:
            spec = level_refine_spec(**kw)
        self._chk(self.lib.geoac_fan_level_refine(self._h, ctypes.byref(spec)))
        n, it = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.geoac_fan_level_refine_shape(self._h, ctypes.byref(n), ctypes.byref(it)))
        n = n.value
        rows = np.empty((n, LRF_STRIDE))
        self._chk(self.lib.geoac_fan_level_refine_fetch(self._h, _p(rows)))
        if n:
            self.n_rays = 3 * n
        return rows, self._rounds_stats(self.lib.geoac_fan_level_refine_stats)

    def level_refine_timing(self):
        """HIP-event times of the last level_refine() [ms]: its launches, its own kernels"""
        return self._rounds_timing(self.lib.geoac_fan_level_refine_timing)

    # ---- level amplitudes (include/geoac_level_amp.h): the ray-tube amplitude at a level runs on the device; nothing is computed here ----
    def _level_amp_rows(self):
        n, M = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.geoac_fan_level_amp_shape(self._h, ctypes.byref(n), ctypes.byref(M)))
        rows = np.empty((n.value, LAMP_STRIDE))
        self._chk(self.lib.geoac_fan_level_amp_fetch(self._h, _p(rows)))
        return rows, M.value

    def level_amp_at(self, theta_deg, phi_deg, level_of, leg, dir, ord, probe_deg=0.02):
        """geoac_fan_level_amp_at: the tube amplitude of ray i at launch angles (theta_deg[i], phi_deg[i]) on level level_of[i] of the level list, branch
        (leg[i], dir[i] = +1 up / -1 down, ord[i]); scalars serve every ray.  Launches one fan of 3 n rays (the rays and their two probes at + probe_deg)
        with the level list still set, so the context's launch angles and last launch become that fan (n_rays = 3 n).  Returns rows [M][n][LAMP_STRIDE]
        (columns LAMP, status values LAMP_STATUS), M = n_sources * n_members."""
        th, ph = _arr(theta_deg).reshape(-1), _arr(phi_deg).reshape(-1)
        n = len(th)
        if len(ph) != n:
            raise GeoAcError("level_amp_at: theta_deg and phi_deg differ in length")
        ints = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32).reshape(-1), (n,))) for v in (level_of, leg, dir, ord)]
        self._chk(self.lib.geoac_fan_level_amp_at(self._h, n, _p(th), _p(ph), *[v.ctypes.data_as(ctypes.c_void_p) for v in ints], ctypes.c_double(float(probe_deg))))
        self.n_rays = 3 * n
        rows, M = self._level_amp_rows()
        return rows.reshape(M, n, LAMP_STRIDE)

    def level_amp(self):
        """geoac_fan_level_amp: the tube amplitude of every seed of the current level_refine() result, read from its final launch's crossing tables at its
        probe_deg - no launch is made.  Returns rows [n_seeds][LAMP_STRIDE]; seeds that did not converge are SKIPPED."""
        self._chk(self.lib.geoac_fan_level_amp(self._h))
        return self._level_amp_rows()[0]

    def level_amp_timing(self):
        """HIP-event times of the last level_amp_at() / level_amp() [ms]: its launch (0 for level_amp()), its own kernels with the medium probe"""
        return self._rounds_timing(self.lib.geoac_fan_level_amp_timing)

    # ---- tube maps (include/geoac_tubemap.h): the rasteriser runs on the device; nothing is computed here ----
    def tubemap(self, spec=None, **kw):
        """geoac_fan_tubemap of the last launch: `spec` a TubeSpec, or the arguments of tube_spec().  Returns a dict of numpy arrays: count, ttime_min,
        cel_max [M][n0][n1], level_max, best [M][F][n0][n1], and detect [F][n0][n1] when detect_db is given.  May be called again with another spec
        without a new launch."""
        if spec is None:
            spec = tube_spec(**kw)
        self._chk(self.lib.geoac_fan_tubemap(self._h, ctypes.byref(spec)))
        return self._fetch_layers("geoac_fan_tubemap", _TUBE_LAYERS, TUBE["LEVEL_MAX"], spec)

    def tubemap_timing(self):
        """HIP-event time of the last tubemap() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_tubemap_timing(self._h, ctypes.byref(ms)))
        return ms.value

    def tubemap_stats(self):
        """work counters of the last tubemap(): triangles that proposed cell centres, those walked cooperatively by a wave, centres tested"""
        st = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.geoac_fan_tubemap_stats(self._h, st.ctypes.data_as(ctypes.c_void_p)))
        return dict(triangles=int(st[0]), cooperative=int(st[1]), candidates=int(st[2]))

    # ---- level tube maps (include/geoac_ltubemap.h): the rasteriser runs on the device; nothing is computed here ----
    def level_tubemap(self, spec=None, **kw):
        """geoac_fan_level_tubemap of the last launch (one with set_levels): `spec` an LTubeSpec, or the arguments of ltube_spec().  Returns a dict of
        numpy arrays: count, ttime_min, atten_min, first [M][Ls][n0][n1] and reach [Ls][n0][n1] (Ls: the levels level_mask selects, in ascending
        level index).  May be called again with another spec without a new launch."""
        if spec is None:
            spec = ltube_spec(**kw)
        self._chk(self.lib.geoac_fan_level_tubemap(self._h, ctypes.byref(spec)))
        M, Ls, n0, n1 = (ctypes.c_int(0) for _ in range(4))
        self._chk(self.lib.geoac_fan_level_tubemap_shape(self._h, *[ctypes.byref(v) for v in (M, Ls, n0, n1)]))
        M, Ls, n0, n1 = M.value, Ls.value, n0.value, n1.value
        out = {}
        for name, layer, dtype in _LTUBE_LAYERS:
            out[name] = np.empty((M, Ls, n0, n1), dtype=dtype)
            self._chk(self.lib.geoac_fan_level_tubemap_fetch(self._h, layer, out[name].ctypes.data_as(ctypes.c_void_p)))
        out["reach"] = np.empty((Ls, n0, n1), dtype=np.uint32)
        self._chk(self.lib.geoac_fan_level_tubemap_fetch_reach(self._h, out["reach"].ctypes.data_as(ctypes.c_void_p)))
        return out

    def level_tubemap_timing(self):
        """HIP-event time of the last level_tubemap() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_level_tubemap_timing(self._h, ctypes.byref(ms)))
        return ms.value

    def level_tubemap_stats(self):
        """work counters of the last level_tubemap(): triangles that proposed cell centres, those walked cooperatively by a wave, centres tested,
        and whether the call formed the branch table (False: it found the one a former call or level_stations() had formed)"""
        st = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.geoac_fan_level_tubemap_stats(self._h, st.ctypes.data_as(ctypes.c_void_p)))
        return dict(triangles=int(st[0]), cooperative=int(st[1]), candidates=int(st[2]), table_formed=bool(st[3]))

    # ---- level loudness maps (include/geoac_lampmap.h): the rasteriser and the amplitude chain run on the device; nothing is computed here ----
    def level_ampmap(self, spec=None, **kw):
        """geoac_fan_level_ampmap of the last launch (one with set_levels): `spec` an LAmpMapSpec, or the arguments of lampmap_spec().  Returns a dict
        of numpy arrays: count, weak, amp_max, ramp_max, loudest [M][Ls][n0][n1] and detect [Ls][n0][n1] (None when detect_amp is NaN).  May be
        called again with another spec without a new launch."""
        if spec is None:
            spec = lampmap_spec(**kw)
        self._chk(self.lib.geoac_fan_level_ampmap(self._h, ctypes.byref(spec)))
        M, Ls, n0, n1, det = (ctypes.c_int(0) for _ in range(5))
        self._chk(self.lib.geoac_fan_level_ampmap_shape(self._h, *[ctypes.byref(v) for v in (M, Ls, n0, n1, det)]))
        M, Ls, n0, n1 = M.value, Ls.value, n0.value, n1.value
        out = {}
        for name, layer, dtype in _LAMPMAP_LAYERS:
            out[name] = np.empty((M, Ls, n0, n1), dtype=dtype)
            self._chk(self.lib.geoac_fan_level_ampmap_fetch(self._h, layer, out[name].ctypes.data_as(ctypes.c_void_p)))
        out["detect"] = None
        if det.value:
            out["detect"] = np.empty((Ls, n0, n1), dtype=np.uint32)
            self._chk(self.lib.geoac_fan_level_ampmap_fetch_detect(self._h, out["detect"].ctypes.data_as(ctypes.c_void_p)))
        return out

    def level_ampmap_timing(self):
        """HIP-event time of the last level_ampmap() on the context's stream [ms]"""
        ms = ctypes.c_double(0)
        self._chk(self.lib.geoac_fan_level_ampmap_timing(self._h, ctypes.byref(ms)))
        return ms.value

    def level_ampmap_stats(self):
        """work counters of the last level_ampmap(), as level_tubemap_stats() gives them"""
        st = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.geoac_fan_level_ampmap_stats(self._h, st.ctypes.data_as(ctypes.c_void_p)))
        return dict(triangles=int(st[0]), cooperative=int(st[1]), candidates=int(st[2]), table_formed=bool(st[3]))

    def set_angles(self, theta_deg, phi_deg):
        th, ph = _arr(theta_deg), _arr(phi_deg)
        if th.ndim != 1 or th.shape != ph.shape:
            raise GeoAcError(f"set_angles: theta and phi must be one-dimensional arrays of one length (got shapes {th.shape} and {ph.shape})")
        self.n_rays = len(th)
        self._chk(self.lib.geoac_fan_set_angles(self._h, len(th), _p(th), _p(ph)))

    def launch(self):
        self._chk(self.lib.geoac_fan_launch(self._h))

    def fetch(self, out=None):
        """records of the last launch; `out`: caller-owned C-contiguous float64 array [n_rays][legs][32] (e.g. the numpy view of a pinned
        torch tensor) to copy into instead of a fresh array.  Ensembles (n_members > 1): [K][n_rays][legs][32]; source sets (n_sources > 1):
        [n_src][n_rays][legs][32], with an ensemble [n_src][K][n_rays][legs][32]"""
        legs = self.params.bounces + 1
        shape = (self.n_rays, legs, REC_STRIDE)
        if self.n_members > 1:
            shape = (self.n_members,) + shape
        if self.n_sources > 1:
            shape = (self.n_sources,) + shape
        if out is None:
            rec = np.empty(shape)
        else:
            rec = out
            if not (isinstance(rec, np.ndarray) and rec.dtype == np.float64 and rec.flags.c_contiguous and rec.shape == shape):
                raise GeoAcError(f"fetch(out=): need a C-contiguous float64 array of shape {shape}")
        steps = ctypes.c_uint64(0)
        self._chk(self.lib.geoac_fan_fetch(self._h, _p(rec), ctypes.byref(steps)))
        return rec, int(steps.value)

    def fetch_samples(self):
        """WriteRays / WriteCaustics rows, ordered by (ray, leg, m): [n][10] (GEOAC_SMP_* layout)"""
        n = ctypes.c_int64(0)
        self._chk(self.lib.geoac_fan_sample_count(self._h, ctypes.byref(n)))
        smp = np.zeros((max(n.value, 1), 10))
        if n.value:
            self._chk(self.lib.geoac_fan_fetch_samples(self._h, _p(smp), ctypes.c_int64(n.value)))
        return smp[:n.value]

    def records_dev(self):
        ptr = ctypes.c_void_p(); nbytes = ctypes.c_size_t()
        self._chk(self.lib.geoac_fan_records_dev(self._h, ctypes.byref(ptr), ctypes.byref(nbytes)))
        return ptr.value, nbytes.value

    def copy_records_to(self, dev_ptr):
        """async D2D copy of the record table into a caller-owned device buffer (ordered on the context's stream)"""
        self._chk(self.lib.geoac_fan_copy_records_dev(self._h, ctypes.c_void_p(dev_ptr)))

    # ---- device-function probes (include/geoac_probe.h): need one completed launch ----
    def probe_atmo_1d(self, x):
        x = _arr(x); n = len(x)
        o9 = np.zeros((n, 9)); rho = np.zeros(n)
        self._chk(self.lib.geoac_probe_atmo_1d(self._h, n, _p(x), _p(o9), _p(rho)))
        return o9, rho

    def probe_absorption(self, x, freq):
        x = _arr(x); f = _arr(freq); n = len(x)
        out = np.zeros(n)
        self._chk(self.lib.geoac_probe_absorption(self._h, n, _p(x), _p(f), _p(out)))
        return out

    def probe_absorption_table(self, x):
        """alpha from the absorption table the post-pass of the stratified sets reads (-1 where the table does not serve the point)"""
        x = _arr(x); n = len(x)
        out = np.zeros(n)
        self._chk(self.lib.geoac_probe_absorption_table(self._h, n, _p(x), _p(out)))
        return out

    def abs_table_info(self):
        """of the last launch: table entries (0 = exact evaluation everywhere), entries flagged at build time, path segments evaluated exactly"""
        e, f, n, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_double(0)
        self._chk(self.lib.geoac_abs_table_info(self._h, ctypes.byref(e), ctypes.byref(f), ctypes.byref(n), ctypes.byref(w)))
        return dict(entries=e.value, flagged=f.value, fixup_segments=int(n.value), worst_rel_err=w.value)

    def fan_status(self):
        """condition flags of the last launch: FAN_STEP_LIMIT, and what the context has withdrawn from its plan (FAN_SUB_FALLBACK, FAN_ABS_FALLBACK)"""
        fl = ctypes.c_uint64(0)
        self._chk(self.lib.geoac_fan_status(self._h, ctypes.byref(fl)))
        return int(fl.value)

    def probe_grid(self, a0, a1, a2, coop=False):
        a0, a1, a2 = _arr(a0), _arr(a1), _arr(a2); n = len(a0)
        o30 = np.zeros((n, 30)); a7 = np.zeros((n, 7))
        self._chk(self.lib.geoac_probe_grid(self._h, n, _p(a0), _p(a1), _p(a2), 1 if coop else 0, _p(o30), _p(a7)))
        return o30, a7

    def total_steps(self):
        steps = ctypes.c_uint64(0)
        self._chk(self.lib.geoac_fan_fetch(self._h, None, ctypes.byref(steps)))
        return int(steps.value)

    def run(self, theta_deg, phi_deg, out=None):
        self.set_angles(theta_deg, phi_deg)
        self.launch()
        return self.fetch(out)

    def timing(self):
        ms = (ctypes.c_double * 3)(); st = (ctypes.c_uint64 * 3)()
        self._chk(self.lib.geoac_last_timing(self._h, ms, st))
        t = dict(ms_total=ms[0], ms_rk4=ms[1], ms_post=ms[2], epochs=int(st[0]), path_bytes_w=int(st[1]), path_bytes_r=int(st[2]))
        # ms_wait: between the RK4 epochs (geoac_last_wait).  A library named by GEOAC_LIB that was built before the export existed has no such key
        if hasattr(self.lib, "geoac_last_wait"):
            w = ctypes.c_double(0.0)
            self._chk(self.lib.geoac_last_wait(self._h, ctypes.byref(w)))
            t["ms_wait"] = w.value
        return t

    # ---- eigenray searches (include/geoac_eig.h), spherical sets ----
    def _eig_collect(self, res):
        L = self.lib
        L.geoac_eig_count.restype = ctypes.c_int64
        L.geoac_eig_sample_count.restype = ctypes.c_int64
        L.geoac_eig_log.restype = ctypes.c_char_p
        L.geoac_eig_log.argtypes = [ctypes.c_void_p, ctypes.c_int]
        ne, ns = L.geoac_eig_count(res), L.geoac_eig_sample_count(res)
        eig = np.zeros((max(ne, 1), EIG_STRIDE)); smp = np.zeros((max(ns, 1), 10))
        if ne:
            self._chk(L.geoac_eig_fetch(res, _p(eig)))
        if ns:
            self._chk(L.geoac_eig_fetch_samples(res, _p(smp)))
        st = (ctypes.c_uint64 * 8)()
        L.geoac_eig_stats_ex(res, st)
        return dict(eig=eig[:ne], smp=smp[:ns], stats=dict(launches=int(st[0]), rays=int(st[1]), steps=int(st[2]), rounds=int(st[3]),
                                                              critical_steps=int(st[4]), amp_launches=int(st[5])))

    def eig_search(self, receivers, theta_min=0.5, theta_max=45.0, bnc_min=0, bnc_max=0, iterations=25, azimuth_err_lim=2.0, verbose=False):
        """GeoAc's -eig_search for every receiver [lat, lon] (degrees) around the context's source, decision rounds of all receivers
        batched into fan launches.  Returns dict(eig [n][EIG_STRIDE], smp raypath rows, stats, logs)."""
        rc_arr = _arr(receivers).reshape(-1, 2)
        ep = EigParams(theta_min, theta_max, bnc_min, bnc_max, iterations, azimuth_err_lim, 1 if verbose else 0)
        res = ctypes.c_void_p()
        self._chk(self.lib.geoac_eig_search(self._h, ctypes.byref(ep), len(rc_arr), _p(rc_arr), ctypes.byref(res)))
        out = self._eig_collect(res)
        out["logs"] = [self.lib.geoac_eig_log(res, i).decode() for i in range(len(rc_arr))]
        self.lib.geoac_eig_free.argtypes = [ctypes.c_void_p]
        self.lib.geoac_eig_free(res)
        return out

    def eig_direct(self, receivers, theta_est, phi_est, bounces=0, iterations=25, verbose=False):
        """-eig_direct: refinement from given inclination / azimuth-from-north estimates, one per receiver"""
        rc_arr = _arr(receivers).reshape(-1, 2); th = _arr(theta_est); ph = _arr(phi_est)
        ep = EigParams(0.5, 45.0, bounces, bounces, iterations, 2.0, 1 if verbose else 0)
        res = ctypes.c_void_p()
        self._chk(self.lib.geoac_eig_direct(self._h, ctypes.byref(ep), len(rc_arr), _p(rc_arr), _p(th), _p(ph), int(bounces), ctypes.byref(res)))
        out = self._eig_collect(res)
        out["logs"] = [self.lib.geoac_eig_log(res, i).decode() for i in range(len(rc_arr))]
        self.lib.geoac_eig_free.argtypes = [ctypes.c_void_p]
        self.lib.geoac_eig_free(res)
        return out


# ---------------- several GPUs from one process (include/geoac_multi.h) ----------------
class FanPool:
    """geoac_pool: one context per listed device, azimuth groups from a shared queue, records gathered into the caller's table."""

    def __init__(self, eqset, devices, options=None):
        self.lib = load_library()
        self.eqset = eqset
        self.devices = [int(d) for d in devices]
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        rc = self.lib.geoac_pool_create(ctypes.byref(self._h), eqset, len(self.devices), arr)
        if rc:
            raise GeoAcError(f"geoac_pool_create: {self.lib.geoac_strerror(rc).decode()}")
        self.lib.geoac_pool_last_error.restype = ctypes.c_char_p
        self.lib.geoac_pool_ctx.restype = ctypes.c_void_p
        self.lib.geoac_pool_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int]
        for i in range(len(self.devices)):
            _apply_options(self.lib, ctypes.c_void_p(self.lib.geoac_pool_ctx(self._h, i)), dict(DEFAULT_OPTIONS, **(options or {})))
        self.params = default_params(eqset)
        self._chk(self.lib.geoac_pool_set_params(self._h, ctypes.byref(self.params)))

    def _chk(self, rc):
        if rc:
            msg = self.lib.geoac_pool_last_error(self._h)
            raise GeoAcError(f"{self.lib.geoac_strerror(rc).decode()}: {msg.decode() if msg else ''}")

    def close(self):
        if self._h:
            self.lib.geoac_pool_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_met(self, path, fmt="zTuvdp"):
        a = met_load(path, self.eqset, fmt)
        x, T, u, v, rho = (_arr(a[k]) for k in ("x", "T", "u", "v", "rho"))
        sl = _arr(np.concatenate([natural_spline_slopes(x, f) for f in (T, u, v, rho)]))
        self._chk(self.lib.geoac_pool_upload_atmo_1d(self._h, len(x), _p(x), _p(T), _p(u), _p(v), _p(rho), _p(sl)))

    def load_grid(self, prefix, locx, locy, fmt="zTuvdp", z_grnd=0.0):
        nx, ny, nz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if self.lib.geoac_grid_dims(prefix.encode(), locx.encode(), locy.encode(), ctypes.byref(nx), ctypes.byref(ny), ctypes.byref(nz)):
            raise GeoAcError(f"cannot read grid {prefix}")
        nx, ny, nz = nx.value, ny.value, nz.value
        x, y, z = np.zeros(nx), np.zeros(ny), np.zeros(nz)
        F = [np.zeros((nx, ny, nz)) for _ in range(4)]
        rc = self.lib.geoac_grid_load_eq(self.eqset, prefix.encode(), locx.encode(), locy.encode(), fmt.encode(), ctypes.c_double(z_grnd),
                                      nx, ny, nz, _p(x), _p(y), _p(z), *[_p(f) for f in F])
        if rc:
            raise GeoAcError(f"geoac_grid_load_eq -> {rc}")
        self._chk(self.lib.geoac_pool_upload_atmo_3d(self._h, nx, ny, nz, _p(x), _p(y), _p(z), *[_p(f) for f in F]))

    def set_params(self, **kw):
        for k, val in kw.items():
            if k == "src":
                self.params.src = (ctypes.c_double * 3)(*val)
            elif k == "xy_limits":
                self.params.xy_limits = (ctypes.c_double * 4)(*val)
            else:
                setattr(self.params, k, val)
        self._chk(self.lib.geoac_pool_set_params(self._h, ctypes.byref(self.params)))

    def run(self, theta_deg, phi_deg, rays_per_group=0):
        th, ph = _arr(theta_deg), _arr(phi_deg)
        rec = np.zeros((len(th), self.params.bounces + 1, REC_STRIDE))
        steps = ctypes.c_uint64(0)
        self._chk(self.lib.geoac_pool_fan_run(self._h, len(th), _p(th), _p(ph), int(rays_per_group), _p(rec), ctypes.byref(steps)))
        return rec, int(steps.value)

    def shares(self):
        n = len(self.devices)
        r, s, g = ((ctypes.c_uint64 * n)() for _ in range(3))
        self._chk(self.lib.geoac_pool_last_shares(self._h, r, s, g))
        return dict(rays=list(r), steps=list(s), groups=list(g))

