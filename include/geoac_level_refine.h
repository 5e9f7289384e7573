/* geoac_level_refine.h - level refinement: Newton eigenrays for every estimate of the level-station lists, on the device.
 *
 * geoac_fan_level_stations (geoac_lstations.h) leaves first-order estimates: launch angles interpolated inside the crossing triangle that
 * encloses a receiver at altitude.  geoac_fan_level_refine takes every kept row of every (member, station) list as a seed and iterates its launch
 * angles until the ray passes through the station on the seed's branch.  A path row carries no Jacobian, so the 2 x 2 derivative of the crossing
 * point by the launch angles is taken by finite differences: a round integrates three rays per seed - the trial and two probes, one launch angle
 * each moved by probe_deg - as one small fan through the existing launch path (geoac_fan_set_angles, geoac_fan_launch, unchanged, the level list
 * still set), and one kernel then takes a damped Newton step per seed from the three crossing records.  The result is one row per seed - the
 * eigenray's launch angles, its miss, and its own travel time, celerity, attenuation and slowness at the station - for every member of an
 * ensemble, a grid ensemble, a source set or a frequency set.
 *
 * How this differs from geoac_fan_refine (geoac_refine.h): that call works on the ground lists and steers by the landing Jacobian of a
 * calc_amp = 1 record; this one works on the level-station lists, reads crossing records (geoac_levels.h) and nothing of a landing record, so
 * calc_amp may be 0 or 1 and no per-member medium at the source is needed - which is why grid ensembles are served here.  The step rule and
 * the statuses are the same, word for word.
 *
 * Cost.  A round is one fan of 3 * n_seeds rays through all M members of the context (M = n_src * K).  A seed belongs to one member and reads
 * that member's crossings alone, so M - 1 of every M integrated ray-members are discarded, as in geoac_refine.h.  3 * n_seeds * M may not exceed
 * GEOAC_RFN_MAX_RAY_MEMBERS (GEOAC_E_CAPACITY, before anything is launched).  Because every member's crossing records are bit-identical to
 * those of a context that holds that member alone, so are its rows.
 *
 * Preconditions (GEOAC_E_INVALID with geoac_last_error otherwise): the context holds current level-station lists (geoac_fan_level_stations
 * after a completed launch with levels, nothing invalidating since); the level list has not changed since that launch; no sample capture
 * (GEOAC_MODE_WRITE_RAYS / _CAUSTICS) is set.  GEOAC_EQ_2D: GEOAC_E_UNSUPPORTED.
 *
 * Seeds.  Every kept row (the first min(hits, cap)) of every list, in the lists' own order: member, station, key (b * n_tri + tri).
 * n_seeds = sum of min(hits, cap); zero seeds is a valid, empty result (no launch is made, the lists stay current).  A seed carries its member
 * m, its station s, the level l = level_of[s] and its branch (GEOAC_LSTA_LEG, _DIR, _ORD).  Round 0's trial angles are the row's
 * GEOAC_LSTA_THETA, GEOAC_LSTA_PHI.  The stations, level_of and the seeds' columns are copied into the call's own device block before the first
 * launch, which invalidates the lists.
 *
 * A round.  With N = n_seeds, ray j * N + i of the round's fan is seed i: j = 0 at the trial (th, ph), j = 1 at (th + h, ph), j = 2 at
 * (th, ph + h), h = probe_deg.
 *
 * BRANCH(ray): walk the kept crossings (the first min(count, cap_levels)) of (m, ray, l) in path order with two ordinal counters, upward and
 * downward, that reset when GEOAC_LVL_LEG changes (the rule of geoac_lstations.h); BRANCH is the first crossing whose (leg, direction, ordinal)
 * is the seed's, or "absent".  Its crossing point (c0, c1) is taken in the stations' axes exactly as geoac_lstations.h defines it: GEOAC_LVL_P0,
 * P0 + 1 for the Cartesian sets, (P0 + 1) * 180.0 / Pi, (P0 + 2) * 180.0 / Pi for the spherical sets.
 *
 * Arithmetic: IEEE double, no fused multiply-adds, every operation in the order written, so that a host restatement gives the same bits
 * (tests/level_refine_reference.py).  SIN, COS, ASIN, WRAP, DIST and Pi are those geoac_refine.h defines.  (s0, s1) is the station, (c0, c1) the
 * crossing point of the base ray (j = 0), (ct0, ct1) that of the theta probe (j = 1), (cp0, cp1) that of the phi probe (j = 2).
 *   miss:  +inf when the base ray's branch is absent, else
 *          spherical sets: DIST(c0, c1, s0, s1; r_earth + z_km[l]) [km];  Cartesian sets: dx = s0 - c0, dy = s1 - c1, sqrt(dx * dx + dy * dy) [km];
 *          a miss that is NaN counts as +inf.
 *   Newton step:
 *     Cartesian:  e0 = s0 - c0,  e1 = s1 - c1,
 *                 a00 = (ct0 - c0) / h,  a10 = (ct1 - c1) / h,  a01 = (cp0 - c0) / h,  a11 = (cp1 - c1) / h
 *     spherical:  the same with every longitude difference through WRAP:  e1 = WRAP(s1 - c1),  a10 = WRAP(ct1 - c1) / h,  a11 = WRAP(cp1 - c1) / h
 *     det = a00 * a11 - a01 * a10;  d_th = (a11 * e0 - a01 * e1) / det;  d_ph = (a00 * e1 - a10 * e0) / det;
 *     both are degrees of launch angle in the launch convention already (the probes moved the launch angles themselves): no unit change, no
 *     sign flip.  A probe whose branch is absent, det == 0, or det, d_th or d_ph not finite: the seed is SINGULAR.  Each of d_th, d_ph is cut
 *     to +- step_max_deg.
 *
 * The step rule is that of geoac_refine.h with the miss and the Newton step above.  Per seed: the trial (th, ph); the best point (b_th, b_ph)
 * and its miss b_miss; the step (d_th, d_ph); a shrink counter n; the rounds used.  Round r = 1, 2, .. is: launch all trials and their probes,
 * then for every seed still active
 *   1. miss of the trial; rounds used = r.
 *   2. miss <= tol: CONVERGED, best = trial, b_miss = miss.  The seed is frozen: it is integrated again at the same angles in every later round,
 *      so its crossing record is in the final tables.
 *   3. else if r == 1 and miss == +inf: LOST (there is no point to step from).
 *   4. else if r == 1 or miss < b_miss: the trial is accepted: best = trial, b_miss = miss, n = 0, (d_th, d_ph) = the Newton step of this round
 *      (SINGULAR ends the seed here).
 *   5. else the trial is rejected: d_th = d_th / 2.0, d_ph = d_ph / 2.0, n = n + 1; n > max_shrink: STALLED.
 *   6. a seed still active gets the next trial th = b_th + d_th, ph = b_ph + d_ph; a seed that ended without converging gets trial = best.
 * The loop ends when no seed is active or after max_iter launches; seeds still active then are ITER_LIMIT.
 *
 * Rows: GEOAC_LRF_STRIDE doubles, columns below.  A CONVERGED row carries GEOAC_LVL_TTIME, GEOAC_LVL_ATTEN and GEOAC_LVL_P0 + 3 .. + 5 of the
 * base ray's crossing record in the final launch, bit for bit (with a frequency set ATTEN is that of frequency 0, as in the crossing records),
 * and CELERITY = range / TTIME.  The range is horizontal and MEASURED FROM THE MEMBER'S OWN SOURCE POINT to the station: spherical
 * DIST(lat_src, lon_src, s0, s1; r_earth); Cartesian dx = s0 - x_src, dy = s1 - y_src, sqrt(dx * dx + dy * dy).  (GEOAC_RFN_CELERITY of
 * geoac_refine.h follows GEOAC_REC_RANGE instead, which the Cartesian sets take from the origin.)  Any other row carries MEMBER .. MISS (best
 * angles, best miss; a LOST row has MISS = -1) and zeros after it.
 *
 * Effect on the context.  The call replaces the context's launch angles and its last launch (n_rays becomes 3 * n_seeds); records, crossing
 * records, maps, station lists, level-station lists and tube maps of the lattice launch are invalid afterwards, as after any launch.  The
 * refinement's own results stay valid until the next geoac_fan_launch, geoac_fan_set_angles, atmosphere upload, geoac_set_sources,
 * geoac_set_frequencies or geoac_set_levels.  Parameters are not touched.
 *
 * Not covered: the 2-D set; the pool (geoac_multi.h); the command-line drivers; the amplitude at altitude (path rows carry no Jacobian); two
 * eigenrays inside one lattice cell (a fold there gives one seed or none); raypath samples of the eigenrays.  All device work goes to the
 * context's stream.  A context that never calls an entry point of this header allocates nothing and launches nothing for it.
 */
#ifndef GEOAC_LEVEL_REFINE_H_
#define GEOAC_LEVEL_REFINE_H_

#include "geoac_lstations.h"
#include "geoac_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_LRF_STRIDE 16
enum {
    GEOAC_LRF_MEMBER   = 0,    /* member of the launch, m = source * K + profile                              */
    GEOAC_LRF_STATION  = 1,    /* station index of geoac_fan_level_stations                                   */
    GEOAC_LRF_LEG      = 2,    /* the seed's branch: GEOAC_LSTA_LEG,                                          */
    GEOAC_LRF_DIR      = 3,    /*   GEOAC_LSTA_DIR (+1 upward, -1 downward)                                   */
    GEOAC_LRF_ORD      = 4,    /*   and GEOAC_LSTA_ORD                                                        */
    GEOAC_LRF_STATUS   = 5,    /* GEOAC_RFN_CONVERGED .. (geoac_refine.h)                                     */
    GEOAC_LRF_ITER     = 6,    /* rounds the seed took part in                                                */
    GEOAC_LRF_THETA    = 7,    /* launch inclination of the best point [deg]                                  */
    GEOAC_LRF_PHI      = 8,    /* launch azimuth [deg], launch convention                                     */
    GEOAC_LRF_MISS     = 9,    /* horizontal distance of the crossing point from the station [km]             */
    GEOAC_LRF_TTIME    = 10,   /* from here on: CONVERGED rows only.  Travel time to the station [s]          */
    GEOAC_LRF_CELERITY = 11,   /* range from the member's own source point / TTIME [km/s]                     */
    GEOAC_LRF_ATTEN    = 12,   /* attenuation [dB] at geoac_params.freq                                       */
    GEOAC_LRF_N0       = 13    /* N0 .. N2 = P3 .. P5 of the crossing record (columns 13 .. 15)               */
};

typedef struct {
    int    max_iter;      /* refinement launches at most, 1 .. GEOAC_RFN_MAX_ITER                                                      */
    int    max_shrink;    /* consecutive rejected trials before a seed is STALLED, 0 .. GEOAC_RFN_MAX_SHRINK                           */
    double tol;           /* miss <= tol ends a seed [km] (spherical: great-circle distance on r_earth + z_km[l]; Cartesian: Euclidean); finite, > 0 */
    double step_max_deg;  /* each component of a Newton step is cut to +- this; finite, > 0                                            */
    double probe_deg;     /* the finite-difference step h of both probes [deg of launch angle]; finite, 0 < h <= 1                     */
} geoac_level_refine_spec;

/* host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D, GEOAC_E_INVALID for a field out of range;
 * geoac_level_refine_fault names the first fault (NULL: none; a string literal) */
int         geoac_level_refine_check(int eqset, const geoac_level_refine_spec* spec);
const char* geoac_level_refine_fault(int eqset, const geoac_level_refine_spec* spec);

/* refine every estimate of the current level-station lists (see above).  Returns after the last round. */
int  geoac_fan_level_refine(geoac_ctx* ctx, const geoac_level_refine_spec* spec);
/* shape of the current result: seeds, launches made */
int  geoac_fan_level_refine_shape(geoac_ctx* ctx, int* n_seeds, int* launches);
/* rows [n_seeds][GEOAC_LRF_STRIDE] f64 to the host */
int  geoac_fan_level_refine_fetch(geoac_ctx* ctx, double* rows);
/* device pointer of the rows (NULL when there are no seeds), valid until the next geoac_fan_level_refine, ordered on the context's stream */
int  geoac_fan_level_refine_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes);
/* HIP-event times of the last geoac_fan_level_refine [ms]: [0] the sum of its launches (geoac_last_timing of each), [1] its own kernels */
int  geoac_fan_level_refine_timing(geoac_ctx* ctx, double ms[2]);
/* launches, ray-members integrated (3 * n_seeds * M per launch), seeds, CONVERGED, STALLED + ITER_LIMIT, LOST + SINGULAR */
int  geoac_fan_level_refine_stats(geoac_ctx* ctx, uint64_t stats[6]);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_LEVEL_REFINE_H_ */
