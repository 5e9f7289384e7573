"""Parity rule between the HIP path and the checker (oracle / golden vectors), per BASELINE.json:
bit-exact on counts (legs, arrivals, steps), <= 1e-6 relative on floating-point fields."""
import numpy as np

from harness import REC

RTOL = 1e-6       # BASELINE.json north_star: "within 1e-6 relative on travel-time/range/amplitude"


def _rel(a, b, floor):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


HEIGHT_COMP = {18: None, 6: None, 12: 2, 4: 2, 3: 1}       # E -> index of the height component (Cartesian sets); 2D amp-on E=6 handled by caller


def _state_scale(st_w, want, valid, hidx):
    """per-component scale of the end state over the fan.  The arrival height of the Cartesian sets is the first
    sub-ground sample, a residual of order 1e-4 km of a trajectory that spans ~100 km: its error is judged against
    the turning height, not against itself."""
    scale = np.maximum(np.abs(st_w).max(axis=0, keepdims=True), 1e-30)
    if hidx is not None:
        scale[0, hidx] = max(scale[0, hidx], np.abs(want[..., REC["TURN"]][valid]).max())
    return scale


def _state_floor(E, hidx):
    """floor of the denominator, as a fraction of the component's scale over the fan.  1e-6 relative is asked of every component;
    a component that passes through zero (launch-angle derivatives change sign along a fan) is judged against 1e-6 of its
    column scale there (absolute slack 1e-12 x scale).  Only the height component of the Cartesian sets - the first sub-ground
    sample, a residual of a ~100 km trajectory - gets the wider 1e-3 floor, against the turning height (see _state_scale)."""
    f = np.full((1, E), 1e-6)
    if hidx is not None:
        f[0, hidx] = 1e-3
    return f


def compare_compact(got_rec, gold, idx=None, rtol=RTOL, check_amp=True, collect_loose=False):
    """HIP record table [n][legs][32] against a compact full-size fixture (tests/golden/make_golden_full.py): steps and flags of
    every (ray, leg) exact; TTIME, ATTEN, TURN, INCL, BACKAZ, AMP, RANGE within rtol (rules of compare_records) for the rays the
    fixture keeps values for.  idx: ray indices of the fan the fixture's rows correspond to (None: all rays in order).
    collect_loose: only list the amplitudes beyond rtol (out["AMP_exempt"]) instead of judging them - make_golden_full.py `exempt`."""
    rec = got_rec if idx is None else got_rec[idx]
    steps = rec[..., REC["STEPS"]].astype(np.int64)
    flags = (rec[..., REC["VALID"]] > 0).astype(np.int8) | ((rec[..., REC["BROKE"]] > 0).astype(np.int8) << 1)
    bad = np.flatnonzero((steps != gold["steps"]).any(axis=1))
    assert bad.size == 0, f"STEPS differ on {bad.size} rays, first {bad[:5]}: {steps[bad[:3]]} vs {gold['steps'][bad[:3]]}"
    assert np.array_equal(flags, gold["flags"]), "VALID / BROKE flags differ"
    vidx = gold["vals_idx"] if "vals_idx" in gold else np.arange(len(rec))
    r = rec[vidx]; want = gold["vals"]
    fields = [str(f) for f in gold["val_fields"]]
    fl = gold["flags"][vidx]
    valid = (fl & 1) > 0; ran = gold["steps"][vidx] > 0
    out = {}
    for k, f in enumerate(fields):
        g, w = r[..., REC[f]], want[..., k]
        if f in ("TTIME", "ATTEN"):
            m = ran; e = _rel(g[m], w[m], 1e-3 if f == "TTIME" else 1e-12)
        elif f in ("INCL", "BACKAZ"):
            m = valid; e = np.abs(g[m] - w[m]) / 180.0
        elif f in ("AMP",):
            if not check_amp:
                continue
            m = valid; e = _rel(g[m], w[m], 1e-300)
            if "amp_sens" in gold:
                # Conditioning of the reference's own amplitude (make_golden_full.py, `sens` pass): a handful of arrivals (rays trapped in a
                # duct, Jacobian 1e3-1e4 x the typical one) answer a 1e-14 change of the launch inclination with a 1e-6 change of amplitude IN
                # THE COMPILED REFERENCE - no arithmetic but its own bit pattern matches those to 1e-6.  The rule: AMP within 1e-6, except for
                # the arrivals NAMED in the fixture (`amp_exempt`: row of the fixture's value table, leg - written by make_golden_full.py
                # `exempt`, which admits an arrival only if the reference's own sensitivity bound covers it, and at most max(3, 1e-4 N) of
                # them); a named arrival is held to 4 x its sensitivity (the running maximum over the legs of the ray so far: a later leg
                # inherits the conditioning of the legs before it).  A loose arrival that is not named fails.
                sens = np.maximum.accumulate(np.asarray(gold["amp_sens"], dtype=np.float64), axis=1)[m]
                # a perturbation that changed a step count leaves no bound (inf): such an arrival is held to rtol like any other
                sens = np.where(np.isinf(sens), 0.0, sens)
                rows, legs = np.nonzero(m)
                loose = e > rtol
                named = np.zeros(e.size, dtype=bool)
                ex = np.asarray(gold["amp_exempt"]).reshape(-1, 2) if "amp_exempt" in gold else np.zeros((0, 2), dtype=np.int64)
                assert len(ex) <= max(3, 1e-4 * e.size), f"AMP: the fixture names {len(ex)} exempt arrivals, more than max(3, 1e-4 x {e.size})"
                if len(ex):
                    named = np.isin(rows.astype(np.int64) * 64 + legs, ex[:, 0].astype(np.int64) * 64 + ex[:, 1])
                out["AMP_beyond_rtol"] = int(loose.sum())
                out["AMP_beyond_rtol_max"] = float(e[loose].max()) if loose.any() else 0.0
                out["AMP_exempt"] = [[int(rows[i]), int(legs[i]), float(e[i]), float(4.0 * sens[i])] for i in np.flatnonzero(loose)]     # row, leg, error, bound
                if not collect_loose:
                    unnamed = loose & ~named
                    assert not unnamed.any(), (f"AMP: {int(unnamed.sum())} arrivals beyond {rtol:g} that the fixture does not name as ill-conditioned in the "
                                               f"reference; first (row, leg, err): {[(int(rows[i]), int(legs[i]), float(e[i])) for i in np.flatnonzero(unnamed)[:5]]}")
                    assert (e[loose] <= 4.0 * sens[loose]).all(), f"AMP: a named arrival is beyond 4 x the reference's own sensitivity; worst {e.max():.3e}"
                out[f] = float(e[~loose].max()) if (~loose).any() else 0.0
                continue
        else:
            m = valid; e = _rel(g[m], w[m], 1e-3)
        out[f] = float(e.max()) if e.size else 0.0
        assert out[f] <= rtol, f"{f}: max rel err {out[f]:.3e}"
    return out


def compare_records(got, want, E, rtol=RTOL, check_amp=True, hidx="auto"):
    """got/want: [n_rays][legs][32] record tables."""
    if hidx == "auto":
        hidx = HEIGHT_COMP.get(E)
    assert got.shape == want.shape
    # ---- integer-valued fields: exact ----
    for f in ("VALID", "STEPS", "BROKE"):
        assert np.array_equal(got[..., REC[f]], want[..., REC[f]]), f"{f} differs"
    ran = want[..., REC["STEPS"]] > 0
    valid = want[..., REC["VALID"]] > 0
    # ---- cumulative sums exist for every leg that ran ----
    for f, floor in (("TTIME", 1e-3), ("ATTEN", 1e-12)):
        r = _rel(got[..., REC[f]][ran], want[..., REC[f]][ran], floor)
        assert r.size == 0 or r.max() <= rtol, f"{f}: max rel err {r.max():.3e}"
    # ---- arrival fields ----
    for f, floor in (("TURN", 1e-3), ("RANGE", 1e-3)):
        r = _rel(got[..., REC[f]][valid], want[..., REC[f]][valid], floor)
        assert r.size == 0 or r.max() <= rtol, f"{f}: max rel err {r.max():.3e}"
    for f in ("INCL", "BACKAZ"):          # degrees: absolute 1e-6 * 180
        d = np.abs(got[..., REC[f]][valid] - want[..., REC[f]][valid])
        assert d.size == 0 or d.max() <= rtol * 180.0, f"{f}: max abs err {d.max():.3e}"
    st_g = got[..., REC["STATE"]:REC["STATE"] + E][valid]
    st_w = want[..., REC["STATE"]:REC["STATE"] + E][valid]
    if st_w.size:
        scale = _state_scale(st_w, want, valid, hidx)                          # per-component scale over the fan
        r = np.abs(st_g - st_w) / np.maximum(np.abs(st_w), _state_floor(E, hidx) * scale)
        assert r.max() <= rtol, f"end state: max rel err {r.max():.3e} at comp {np.unravel_index(r.argmax(), r.shape)}"
    if check_amp and E > 6:
        for f in ("AMP", "JACOB"):
            r = _rel(got[..., REC[f]][valid], want[..., REC[f]][valid], 1e-300)
            assert r.size == 0 or r.max() <= rtol, f"{f}: max rel err {r.max():.3e}"


def max_rel_errors(got, want, E, hidx="auto"):
    """diagnostic: dict of max relative errors per field (no asserts)."""
    if hidx == "auto":
        hidx = HEIGHT_COMP.get(E)
    out = {}
    ran = want[..., REC["STEPS"]] > 0
    valid = want[..., REC["VALID"]] > 0
    for f in ("VALID", "STEPS", "BROKE"):
        out[f] = int(np.sum(got[..., REC[f]] != want[..., REC[f]]))
    for f in ("TTIME", "ATTEN"):
        out[f] = float(_rel(got[..., REC[f]][ran], want[..., REC[f]][ran], 1e-300).max()) if ran.any() else 0.0
    for f in ("TURN", "RANGE", "INCL", "BACKAZ", "AMP", "JACOB"):
        out[f] = float(_rel(got[..., REC[f]][valid], want[..., REC[f]][valid], 1e-300).max()) if valid.any() else 0.0
    st_g = got[..., REC["STATE"]:REC["STATE"] + E][valid]
    st_w = want[..., REC["STATE"]:REC["STATE"] + E][valid]
    if st_w.size:
        scale = _state_scale(st_w, want, valid, hidx)
        out["STATE"] = float((np.abs(st_g - st_w) / np.maximum(np.abs(st_w), _state_floor(E, hidx) * scale)).max())
    return out


def field_errors(got, want, E, hidx="auto"):
    """diagnostic: the error of every (ray, leg) in every field compare_records judges, by compare_records' own measures (floors, degrees
    against 180, the end state against its column scale over the fan: the worst component) - dict field -> [n_rays][legs], NaN where the
    field is not judged.  No asserts; got and want must have the same counts for the figures to mean anything."""
    if hidx == "auto":
        hidx = HEIGHT_COMP.get(E)
    ran = want[..., REC["STEPS"]] > 0
    valid = want[..., REC["VALID"]] > 0
    out = {}

    def put(f, m, e):
        a = np.full(want.shape[:2], np.nan)
        a[m] = e
        out[f] = a
    for f, floor in (("TTIME", 1e-3), ("ATTEN", 1e-12)):
        put(f, ran, _rel(got[..., REC[f]][ran], want[..., REC[f]][ran], floor))
    for f in ("TURN", "RANGE"):
        put(f, valid, _rel(got[..., REC[f]][valid], want[..., REC[f]][valid], 1e-3))
    for f in ("INCL", "BACKAZ"):
        put(f, valid, np.abs(got[..., REC[f]][valid] - want[..., REC[f]][valid]) / 180.0)
    st_g = got[..., REC["STATE"]:REC["STATE"] + E][valid]
    st_w = want[..., REC["STATE"]:REC["STATE"] + E][valid]
    if st_w.size:
        scale = _state_scale(st_w, want, valid, hidx)
        put("STATE", valid, (np.abs(st_g - st_w) / np.maximum(np.abs(st_w), _state_floor(E, hidx) * scale)).max(axis=1))
    if E > 6:
        for f in ("AMP", "JACOB"):
            put(f, valid, _rel(got[..., REC[f]][valid], want[..., REC[f]][valid], 1e-300))
    return out


def fan_properties(rec, steps, E, nu_slice, c_ratio, eik_tol=1e-4):
    """size-independent properties of a fan's record table (no reference needed): count bookkeeping - the legs' step counts add up to the
    device counter, a leg that broke has no later legs, legs run in order, a row is written exactly for the legs that ran and did not
    break -, cumulative travel time / attenuation non-decreasing over a ray's legs, and the eikonal (Hamiltonian) residual at EVERY
    arrival: |nu| = c0 / c(arrival point) (winds are tapered to 0 at the ground); c_ratio: that quotient, a scalar or one value per
    arrival in record order; eik_tol: bound of that residual.  Returns the number of arrivals."""
    valid = rec[..., REC["VALID"]] > 0
    ran = rec[..., REC["STEPS"]] > 0
    broke = rec[..., REC["BROKE"]] > 0
    assert int(rec[..., REC["STEPS"]].sum()) == steps, f"step counts of the records add up to {int(rec[..., REC['STEPS']].sum())}, the device counted {steps}"
    assert not (broke[:, :-1] & ran[:, 1:]).any(), "a leg ran after a broken one"
    assert (ran[:, 1:] <= ran[:, :-1]).all(), "legs out of order"
    assert (valid == (ran & ~broke)).all(), "a result row without a completed leg (or the reverse)"
    tt = rec[..., REC["TTIME"]]; at = rec[..., REC["ATTEN"]]
    assert ((tt[:, 1:] >= tt[:, :-1]) | ~ran[:, 1:]).all(), "travel time decreases over the legs of a ray"
    assert ((at[:, 1:] >= at[:, :-1]) | ~ran[:, 1:]).all(), "attenuation decreases over the legs of a ray"
    st = rec[..., REC["STATE"]:REC["STATE"] + E][valid]
    numag = np.sqrt((st[:, nu_slice] ** 2).sum(axis=1))
    eik = np.abs(numag / c_ratio - 1.0)
    # stratified sets: the RK4 truncation error of the reference scheme itself (~1e-6).  Grid sets: the reference's interpolant takes the derivatives of c from splines of
    # finite differences of the node values (Q11 / Q12), not from the interpolated c itself, so its own rays conserve the Hamiltonian to ~1e-3 only (measured: median 7e-5,
    # maximum 1.1e-3 over the 1.5 M arrivals of config 4; the same rays agree with the compiled reference to 1e-9) - callers pass eik_tol = 5e-3 there.  Not a parity bound.
    assert eik.max() < eik_tol, f"eikonal residual {eik.max():.3e} at an arrival"
    return int(valid.sum())


# ---------------- eigenray searches (config 5): the reference binary's logs and result files ----------------
def ring_receivers(n=64, lat0=31.0, lon0=0.0, radius_deg=2.5):
    """config 5: n receivers [lat, lon] on a ring of 2.5 degrees of arc around the source, by ring position"""
    az = np.arange(n) * (2.0 * np.pi / n)
    return np.stack([lat0 + radius_deg * np.cos(az), lon0 + radius_deg * np.sin(az) / np.cos(np.radians(lat0))], axis=1)


def ring_golden_name(p):
    """fixture directory (tests/golden/cli/) of ring position p of the 64-ring: the rank-0 receivers of the 8-GPU run were made first
    (cfg5_r0..r7 = positions 0, 8, ..., 56), then one receiver of each other rank (cfg5_r8..r14 = positions 1..7), then the rest by position"""
    if p % 8 == 0:
        return f"cfg5_r{p // 8}"
    if p < 8:
        return f"cfg5_r{7 + p}"
    return f"cfg5_p{p}"


def parse_eig_results(path):
    """[{bounces, theta, phi, ...}] from a reference <title>_results.dat of an eigenray search"""
    import re
    out = []
    for block in open(path).read().split("Eigenray-")[1:]:
        nums = lambda key: [float(x) for x in re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?", block.split(key)[1].split("\n")[0])]      # noqa: E731
        out.append(dict(bounces=int(re.search(r"(\d+) bounce", block).group(1)),
                        theta=nums("theta, phi =")[0], phi=nums("theta, phi =")[1], ttime=nums("Travel Time =")[0], celerity=nums("Celerity =")[0],
                        amp=nums("Amplitude (geometric) =")[0], atten=nums("Atmospheric attenuation =")[0], incl=nums("Arrival inclination =")[0],
                        bearing=nums("Bearing to source =")[0], backaz=nums("Back azimuth of arrival =")[0], azdev=nums("Azimuth deviation =")[0]))
    return out


EIG_COLS = dict(RCVR=0, INDEX=1, BOUNCES=2, THETA=3, PHI=4, TTIME=5, CELERITY=6, AMP_DB=7, ATTEN_DB=8, INCL=9, BEARING=10, BACKAZ=11, AZDEV=12)
EIG_FIELDS = (("theta", "THETA"), ("phi", "PHI"), ("ttime", "TTIME"), ("celerity", "CELERITY"), ("amp", "AMP_DB"), ("atten", "ATTEN_DB"),
              ("incl", "INCL"), ("bearing", "BEARING"), ("backaz", "BACKAZ"), ("azdev", "AZDEV"))


def compare_eig_rows(got, want, where=""):
    """eigenray rows of ONE receiver (geoac_eig_fetch layout) against the parsed blocks of the reference's result file: same number of
    eigenrays, same bounce counts, every printed field to its 8 printed digits"""
    E = EIG_COLS
    assert len(got) == len(want), f"{where}: {len(got)} eigenrays vs the reference's {len(want)}"
    for g, w in zip(got, want):
        assert int(g[E["BOUNCES"]]) == w["bounces"], f"{where}: bounce count {int(g[E['BOUNCES']])} vs {w['bounces']}"
        for f, col in EIG_FIELDS:
            x, y = float(g[E[col]]), w[f]
            # 8 printed digits; the deviation is a difference of nearly equal bearings: absolute on the scale of a degree
            assert abs(x - y) <= 2e-7 * max(abs(x), abs(y)) + (2e-6 if f in ("azdev", "phi", "backaz", "bearing") else 1e-12), (where, f, x, y)
    return len(want)


def compare_eig_ring(eig, positions, cli_gold):
    """a gathered eigenray table (column 0 = ring position) against the reference binary's result files of those ring positions
    (tests/golden/cli/<ring_golden_name(p)>/g_results.dat).  Returns counts for the bench line; raises on a mismatch."""
    import os
    n_ref, checked, missing = 0, 0, []
    for p in positions:
        gold = os.path.join(cli_gold, ring_golden_name(int(p)), "g_results.dat")
        if not os.path.exists(gold):
            missing.append(int(p))
            continue
        n_ref += compare_eig_rows(eig[eig[:, EIG_COLS["RCVR"]] == p], parse_eig_results(gold), where=f"ring position {int(p)}")
        checked += 1
    return dict(receivers_checked=checked, eigenrays_matched=n_ref, receivers_without_fixture=missing)


def compare_logs(got, want):
    """an eigenray search's verbose text against the reference binary's, line by line, token by token (numbers to the printed digits)"""
    gl = [l for l in got.split("\n")]
    wl = [l for l in want.split("\n")]
    assert len(gl) == len(wl), f"log: {len(gl)} lines vs {len(wl)}"
    for i, (g, w) in enumerate(zip(gl, wl)):
        gt, wt = g.replace("\t", " ").split(" "), w.replace("\t", " ").split(" ")
        assert len(gt) == len(wt), f"log line {i + 1}: {g!r} vs {w!r}"
        for a, b in zip(gt, wt):
            a2, b2 = a.rstrip(",.)").lstrip("(["), b.rstrip(",.)").lstrip("([")
            if a2 == b2:
                continue
            try:
                x, y = float(a2), float(b2)
            except ValueError:
                raise AssertionError(f"log line {i + 1}: {a!r} vs {b!r}")
            # deviations are differences of nearly equal bearings: compare those on the scale of a degree
            assert abs(x - y) <= 1.2e-5 * max(abs(x), abs(y)) + 2e-6, f"log line {i + 1}: {a!r} vs {b!r}\n{g}\n{w}"
