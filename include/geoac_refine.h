/* geoac_refine.h - station refinement: Newton eigenrays for every estimate of the station lists, on the device.
 *
 * geoac_fan_stations (geoac_stations.h) leaves first-order estimates: launch angles interpolated inside the landing triangle that encloses a
 * station.  geoac_fan_refine takes every kept row of every (member, station) list as a seed and iterates its launch angles until the ray lands
 * on the station: a round integrates all seeds as one small fan through the existing launch path (geoac_fan_set_angles, geoac_fan_launch,
 * unchanged), and one kernel then takes a damped Newton step per seed from the 2 x 2 landing Jacobian that a calc_amp = 1 record holds.  The
 * result is one row per seed - the eigenray's launch angles, its miss, and its own travel time, celerity, turning height, arrival angles,
 * amplitude and level - for every member of an ensemble, a source set or a frequency set.
 *
 * How this differs from geoac_eig_direct (geoac_eig.h): that entry point replays the reference's per-receiver routine, its long double solve,
 * its step-size rule and its log, one profile, one source, one frequency per context.  This one has its own step rule (below), solves in double,
 * writes no log and no raypath samples, and serves the sets.  The two agree as two converged solutions of the same equation do, not bit for bit.
 *
 * Cost.  A round is one fan of n_seeds rays through all M members of the context (M = n_src * K).  A seed belongs to one member and reads that
 * member's record alone, so M - 1 of every M integrated ray-members are discarded.  That is the price of leaving the launch plan untouched; the
 * rounds are small and bound by the latency of their longest ray either way.  n_seeds * M may not exceed GEOAC_RFN_MAX_RAY_MEMBERS
 * (GEOAC_E_CAPACITY).  Because every member's records are bit-identical to those of a context that holds that member alone, so are its rows.
 *
 * Preconditions (GEOAC_E_INVALID with geoac_last_error otherwise): the context holds current station lists (geoac_fan_stations after a completed
 * launch, nothing invalidating since); that launch ran with calc_amp = 1, the parameters still say calc_amp = 1, and no sample capture
 * (GEOAC_MODE_WRITE_RAYS / _CAUSTICS) is set.  GEOAC_EQ_2D: GEOAC_E_UNSUPPORTED.
 *
 * Seeds.  Every kept row (the first min(hits, cap)) of every list, in the lists' own order: member, station, key (leg * n_tri + tri).
 * n_seeds = sum of min(hits, cap); zero seeds is a valid, empty result (no launch is made).  A seed of leg l reads leg l of its ray's record.
 * Round 0's trial angles are the seed's GEOAC_STA_THETA, GEOAC_STA_PHI.
 *
 * Effect on the context.  The call replaces the context's launch angles and its last launch (n_rays becomes n_seeds); maps, station lists and
 * tube maps of the lattice launch are invalid afterwards, as after any launch.  The refinement's own results stay valid until the next
 * geoac_fan_launch, geoac_fan_set_angles, atmosphere upload, geoac_set_sources or geoac_set_frequencies.  Parameters are not touched.
 *
 * Arithmetic: IEEE double, no fused multiply-adds, every operation in the order written, so that a host restatement gives the same bits
 * (tests/refine_reference.py).  Pi = 3.141592653589793238462643.  The elementary functions are defined here by their operations, not taken from a
 * maths library (two libraries differ in the last bit):
 *   SIN(x), COS(x), |x| <= Pi/2:  x2 = x * x;  SIN: t = x, s = x, for k = 1 .. 14: t = -(t * x2) / ((2k) * (2k + 1)), s = s + t;
 *                                              COS: t = 1, s = 1, for k = 1 .. 14: t = -(t * x2) / ((2k - 1) * (2k)),  s = s + t
 *       (the divisors are exact small integers in double)
 *   SINCOSD(a) of an angle in degrees: q = floor(a / 90.0 + 0.5), r = (a - 90.0 * q) * Pi / 180.0, n = q - 4.0 * floor(q / 4.0);
 *       n = 0: (SIN r, COS r); 1: (COS r, -SIN r); 2: (-SIN r, -COS r); 3: (-COS r, SIN r)
 *   ASIN(s), 0 <= s <= 1:  s <= 0.5: u = s; else u = sqrt((1.0 - s) / 2.0).  x2 = u * u, t = u, a = u,
 *       for k = 1 .. 30: t = ((t * x2) * ((2k - 1) * (2k - 1))) / ((2k) * (2k + 1)), a = a + t.   s <= 0.5: a; else Pi / 2.0 - 2.0 * a
 *   WRAP(d) = d - 360.0 * floor((d + 180.0) / 360.0)
 *   DIST(lat1, lon1, lat2, lon2; R) [deg]: a = SIN(((lat2 - lat1) * Pi / 180.0) / 2.0), b = SIN((WRAP(lon2 - lon1) * Pi / 180.0) / 2.0),
 *       h = a * a + (COS(lat1 * Pi / 180.0) * COS(lat2 * Pi / 180.0)) * (b * b), h > 1: h = 1;  DIST = (2.0 * R) * ASIN(sqrt(h))     (the haversine form)
 *
 * The record.  R is the record of the seed's ray in its own member on its leg, S = R + GEOAC_REC_STATE, (s0, s1) the station, (th, ph) the
 * trial angles that produced R [deg, launch convention], rg = r_earth + z_grnd.
 *   miss:  +inf when R[GEOAC_REC_VALID] == 0, else
 *          spherical sets: DIST(S[1] * 180.0 / Pi, S[2] * 180.0 / Pi, s0, s1; rg) [km];  Cartesian sets: dx = s0 - S[0], dy = s1 - S[1], sqrt(dx * dx + dy * dy) [km];
 *          a miss that is NaN counts as +inf.
 *   Newton step (the ground-intercept-corrected landing derivatives of the reference's GeoAc_3DEigenray_LM, in the routine's azimuth lp = 90 - ph):
 *     spherical:  e0 = s0 * Pi / 180.0 - S[1],  e1 = WRAP(s1 - S[2] * 180.0 / Pi) * Pi / 180.0,  q = 1.0 / rg,  qc = 1.0 / (rg * COS(S[1])),
 *                 a00 = S[7] - ((q * S[4]) / S[3]) * S[6],    a01 = S[13] - ((q * S[4]) / S[3]) * S[12],
 *                 a10 = S[8] - ((qc * S[5]) / S[3]) * S[6],   a11 = S[14] - ((qc * S[5]) / S[3]) * S[12]
 *     GEOAC_EQ_3D:  e0 = s0 - S[0], e1 = s1 - S[1];  (st, ct) = SINCOSD(th), (sp, cp) = SINCOSD(90.0 - ph),  n0 = ct * cp, n1 = ct * sp,
 *                 m = 1.0 + (n0 * mach0 + n1 * mach1)   (mach: u / c, v / c of the member's profile at max(z_src, z_grnd), as geoac_eig_direct takes them),
 *                 g0 = (n0 / m) / S[3], g1 = (n1 / m) / S[3],
 *                 a00 = S[4] - g0 * S[6],  a01 = S[8] - g0 * S[10],  a10 = S[5] - g1 * S[6],  a11 = S[9] - g1 * S[10]
 *     GEOAC_EQ_3D_RNGDEP:  e0, e1 as above;  g0 = S[3] / S[5], g1 = S[4] / S[5],
 *                 a00 = S[6] - g0 * S[8],  a01 = S[12] - g0 * S[14],  a10 = S[7] - g1 * S[8],  a11 = S[13] - g1 * S[14]
 *     det = a00 * a11 - a01 * a10;  dlt = (((a11 * e0 - a01 * e1) / det) * 180.0) / Pi;  dlp = (((a00 * e1 - a10 * e0) / det) * 180.0) / Pi;
 *     det == 0, or det, dlt or dlp not finite: the seed is SINGULAR.  Each of dlt, dlp is cut to +- step_max_deg.  The step in launch angles is
 *     (d_th, d_ph) = (dlt, -dlp).
 *
 * The step rule.  Per seed: the trial (th, ph); the best point (b_th, b_ph) and its miss b_miss; the step (d_th, d_ph); a shrink counter n; the
 * rounds used.  Round r = 1, 2, .. is: launch all trials, then for every seed still active
 *   1. miss of the trial's record; rounds used = r.
 *   2. miss <= tol: CONVERGED, best = trial, b_miss = miss.  The seed is frozen: it is integrated again at the same angles in every later round,
 *      so its record is in the final table.
 *   3. else if r == 1 and miss == +inf: LOST (there is no point to step from).
 *   4. else if r == 1 or miss < b_miss: the trial is accepted: best = trial, b_miss = miss, n = 0, (d_th, d_ph) = the Newton step of this record
 *      (SINGULAR ends the seed here).
 *   5. else the trial is rejected: d_th = d_th / 2.0, d_ph = d_ph / 2.0, n = n + 1; n > max_shrink: STALLED.
 *   6. a seed still active gets the next trial th = b_th + d_th, ph = b_ph + d_ph; a seed that ended without converging gets trial = best.
 * The loop ends when no seed is active or after max_iter launches; seeds still active then are ITER_LIMIT.
 *
 * Rows: GEOAC_RFN_STRIDE doubles, columns below.  A CONVERGED row carries its record's fields (of the final launch, bit for bit) and
 * CELERITY = station range / TTIME, the range as GEOAC_REC_RANGE defines it for the set: spherical DIST(lat_src, lon_src, s0, s1; r_earth), Cartesian
 * sqrt(s0 * s0 + s1 * s1).  Any other row carries MEMBER .. MISS (best angles, best miss; a LOST row has MISS = -1) and zeros after it.
 * level[seed][f] = level[m][f][ray = seed][leg] of the final launch's level table (geoac_map.h) for CONVERGED rows, 0 otherwise.
 *
 * Not covered: the 2-D set; the pool (geoac_multi.h); the command-line drivers; two eigenrays inside one lattice cell (a fold there gives one
 * seed or none); raypath samples of the eigenrays.  All device work goes to the context's stream.  A context that never calls an entry point of
 * this header allocates nothing and launches nothing for it.
 */
#ifndef GEOAC_REFINE_H_
#define GEOAC_REFINE_H_

#include "geoac_stations.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_RFN_STRIDE 16
enum {
    GEOAC_RFN_MEMBER   = 0,    /* member of the launch, m = source * K + profile                              */
    GEOAC_RFN_STATION  = 1,    /* station index of geoac_fan_stations                                         */
    GEOAC_RFN_LEG      = 2,    /* leg of the seed (GEOAC_STA_LEG)                                             */
    GEOAC_RFN_TRI      = 3,    /* triangle of the seed (GEOAC_STA_TRI)                                        */
    GEOAC_RFN_STATUS   = 4,    /* GEOAC_RFN_CONVERGED ..                                                      */
    GEOAC_RFN_ITER     = 5,    /* rounds the seed took part in                                                */
    GEOAC_RFN_THETA    = 6,    /* launch inclination of the best point [deg]                                  */
    GEOAC_RFN_PHI      = 7,    /* launch azimuth [deg], launch convention                                     */
    GEOAC_RFN_MISS     = 8,    /* distance of the landing point from the station [km]                         */
    GEOAC_RFN_TTIME    = 9,    /* from here on: CONVERGED rows only                                           */
    GEOAC_RFN_CELERITY = 10,
    GEOAC_RFN_TURN     = 11,
    GEOAC_RFN_INCL     = 12,
    GEOAC_RFN_BACKAZ   = 13,
    GEOAC_RFN_AMP      = 14,
    GEOAC_RFN_JACOB    = 15
};
enum {
    GEOAC_RFN_CONVERGED  = 1,  /* miss <= tol                                                                 */
    GEOAC_RFN_ITER_LIMIT = 2,  /* still active after max_iter launches                                        */
    GEOAC_RFN_STALLED    = 3,  /* more than max_shrink rejected trials in a row                               */
    GEOAC_RFN_LOST       = 4,  /* the seed's own ray was not VALID on the leg                                 */
    GEOAC_RFN_SINGULAR   = 5   /* zero or non-finite determinant or step                                      */
};

#define GEOAC_RFN_MAX_ITER        32
#define GEOAC_RFN_MAX_SHRINK      16
#define GEOAC_RFN_MAX_RAY_MEMBERS (1 << 20)     /* n_seeds * M of one round */

typedef struct {
    int    max_iter;      /* refinement launches at most, 1 .. GEOAC_RFN_MAX_ITER                                                      */
    int    max_shrink;    /* consecutive rejected trials before a seed is STALLED, 0 .. GEOAC_RFN_MAX_SHRINK                           */
    double tol;           /* miss <= tol ends a seed [km] (spherical: great-circle distance on r_earth + z_grnd; Cartesian: Euclidean); finite, > 0 */
    double step_max_deg;  /* each component of a Newton step is cut to +- this (the reference uses 0.2); finite, > 0                   */
} geoac_refine_spec;

/* host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D, GEOAC_E_INVALID for a field out of range;
 * geoac_refine_fault names the first fault (NULL: none; a string literal) */
int         geoac_refine_check(int eqset, const geoac_refine_spec* spec);
const char* geoac_refine_fault(int eqset, const geoac_refine_spec* spec);

/* refine every estimate of the current station lists (see above).  Returns after the last round. */
int  geoac_fan_refine(geoac_ctx* ctx, const geoac_refine_spec* spec);
/* shape of the current result: seeds, F, launches made */
int  geoac_fan_refine_shape(geoac_ctx* ctx, int* n_seeds, int* n_freq, int* iterations);
/* rows [n_seeds][GEOAC_RFN_STRIDE] f64, level [n_seeds][F] f64 to the host (either may be NULL) */
int  geoac_fan_refine_fetch(geoac_ctx* ctx, double* rows, double* level);
/* device pointer of one of them (which: 0 rows, 1 level), valid until the next geoac_fan_refine, ordered on the context's stream */
int  geoac_fan_refine_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes);
/* HIP-event times of the last geoac_fan_refine [ms]: [0] the sum of its launches (geoac_last_timing of each), [1] its own kernels */
int  geoac_fan_refine_timing(geoac_ctx* ctx, double ms[2]);
/* launches, ray-members integrated (n_seeds * M per launch), seeds, CONVERGED, STALLED + ITER_LIMIT, LOST + SINGULAR */
int  geoac_fan_refine_stats(geoac_ctx* ctx, uint64_t stats[6]);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_REFINE_H_ */
