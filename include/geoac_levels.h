/* geoac_levels.h - level crossings: every passage of every ray of a launch through up to 8 receiver altitudes.
 *
 * The other products of a launch lie on the ground (records, maps, station lists, tube maps, refined eigenrays: all of them describe the leg-end
 * row of a ray).  A receiver above the ground - a balloon, an aircraft, a mountain array, a thermospheric probe level - needs the rows in
 * between, which the launch has on the device anyway: the path rows of an epoch and, beside them, each segment's travel-time and attenuation
 * contribution.  With levels set, one more kernel (k_levels, geoac_levels.hip) walks them in row order behind the per-ray sums and keeps, per
 * (ray, level), a count of the crossings and the first `cap` of them in path order.
 *
 * Crossing rule, per path segment (rows i, i+1 of one leg; h the height coordinate: z for the Cartesian sets, the geocentric radius r for the
 * spherical sets, where the level is r_earth + z_km, added once on the host):
 *     upward    h_i <  lev <= h_{i+1}           downward   h_i >= lev >  h_{i+1}
 * half-open, so that a row lying exactly on a level counts once.  On a crossing
 *     FRAC  = (lev - h_i) / (h_{i+1} - h_i)
 *     TTIME = (travel time of the legs before + this leg's sum before the segment) + FRAC * (the segment's contribution)
 *     ATTEN   the same with the attenuation contributions
 *     Pq    = p_i + FRAC * (p_{i+1} - p_i)   for every component q of the path row
 * with every multiply and add rounded on its own (no fused multiply-add), so the bits do not depend on the compiler.  The running sums are
 * k_accum's, formed in k_accum's order: at a leg end they are GEOAC_REC_TTIME / GEOAC_REC_ATTEN bit for bit.
 *
 * Shapes (M = n_src * K members of the launch, ordered as geoac_fan_fetch orders them; L levels; rays in the caller's order):
 *     count  int32  [M][n_rays][L]                          crossings seen - it keeps running past `cap`, so an overflow is visible
 *     rec    double [M][n_rays][L][cap][GEOAC_LVL_STRIDE]   the first `cap` crossings in path order, slots past the count all zero
 * Both are the same bits on every run and under every launch plan: a thread owns its ray's slots, there are no atomics and no sorting.
 *
 * Frequency sets: ATTEN is the attenuation at frequency 0 (geoac_params.freq) only.
 * Not covered: the amplitude at altitude - path rows do not carry the Jacobian components an amplitude needs.  The 2-D set (its sums always
 * take the sample-capture form) is refused, as are sample capture (WriteRays / WriteCaustics) on a context with levels, and geoac_clone, the
 * eigenray searches and the pool on such a context.
 *
 * A context that never calls geoac_set_levels, or has set 0 levels, launches none of this and holds none of its buffers.
 */
#ifndef GEOAC_LEVELS_H_
#define GEOAC_LEVELS_H_

#include "geoac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_MAX_LEVELS   8
#define GEOAC_LVL_MAX_CAP  64
#define GEOAC_LVL_DEF_CAP  8

/* ---- a crossing record: GEOAC_LVL_STRIDE doubles ---- */
enum {
    GEOAC_LVL_LEG    = 0,    /* leg of the ray the crossing lies in (0: before the first bounce)                                   */
    GEOAC_LVL_DIR    = 1,    /* +1 upward, -1 downward                                                                             */
    GEOAC_LVL_FRAC   = 2,    /* position within the path segment, in [0, 1]                                                        */
    GEOAC_LVL_TTIME  = 3,    /* travel time from the source [s], cumulative over legs as GEOAC_REC_TTIME is                        */
    GEOAC_LVL_ATTEN  = 4,    /* attenuation [dB] at geoac_params.freq, cumulative as GEOAC_REC_ATTEN is                            */
    GEOAC_LVL_P0     = 5,    /* P0 .. P5: the components of the path row, interpolated at FRAC, in the stored units -              */
                             /*   GEOAC_EQ_3D: x, y, z [km], then nu_z, the one slowness component the row carries (P4, P5 = 0)    */
                             /*   GEOAC_EQ_3D_RNGDEP: x, y, z [km], then the three slowness components                             */
                             /*   spherical sets: r [km], lat, lon [rad], then the three slowness components                       */
    GEOAC_LVL_RSVD   = 11,   /* reserved, written as 0                                                                             */
    GEOAC_LVL_STRIDE = 12
};

/* Host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D, or GEOAC_E_INVALID unless
 *   0 <= n_levels <= GEOAC_MAX_LEVELS, cap is 0 (= GEOAC_LVL_DEF_CAP) or in 1 .. GEOAC_LVL_MAX_CAP,
 *   every z_km is finite, strictly ascending, strictly above params->z_grnd and below the vertical limit (spherical sets:
 *   below vert_limit - r_earth; a vert_limit of NaN - "the top node of the atmosphere", not known yet - bounds nothing).
 * fault (may be NULL) receives a static string naming the first thing wrong, or NULL. */
int geoac_levels_check(int eqset, const geoac_params* params, int n_levels, const double* z_km, int cap, const char** fault);

/* Sets the level list [km above sea level] and the crossings kept per (ray, level); n_levels = 0 leaves the mode and frees its buffers.
 * Checked as geoac_levels_check does against the context's parameters now, and again by geoac_fan_launch against those then in force. */
int geoac_set_levels(geoac_ctx* ctx, int n_levels, const double* z_km, int cap);

/* the current list: z_km (may be NULL) receives n_levels doubles (room for GEOAC_MAX_LEVELS) */
int geoac_get_levels(geoac_ctx* ctx, int* n_levels, double* z_km, int* cap);

/* After geoac_fan_launch: the crossings of that launch (shapes above; either pointer may be NULL).  Waits for the launch as geoac_fan_fetch
 * does.  GEOAC_E_INVALID when the last completed launch had no levels, or the level list has changed since. */
int geoac_fan_fetch_levels(geoac_ctx* ctx, double* rec_out, int32_t* count_out);

/* ... and the device buffers themselves (valid until the next launch or geoac_set_levels), for callers that work on the device */
int geoac_fan_levels_dev(geoac_ctx* ctx, void** rec_dev, size_t* rec_bytes, void** count_dev, size_t* count_bytes);

#ifdef __cplusplus
}
#endif

#endif
