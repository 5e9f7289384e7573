/* geoac_map.h - arrival maps: the record table of a launch reduced, on the device, to a few small 2-D fields.
 *
 * A launch leaves up to [n_src][K][n_rays][legs][GEOAC_REC_STRIDE] doubles on the device (geoac_hip.h).  What an analyst asks of them - where
 * does the sound reach the ground, how early, how loud, and for an ensemble in how many members - is a binning of the arrivals on a regular
 * grid.  geoac_fan_map does that binning beside the record table and hands back layers of 8 bytes per cell instead of 256 bytes per arrival.
 *
 * Grid axes are the arrival coordinates a `_results.dat` row prints:
 *   spherical sets (GEOAC_EQ_GLOBAL, GEOAC_EQ_GLOBAL_RNGDEP):  axis 0 = latitude, axis 1 = longitude [deg], STATE+1 and STATE+2 `* 180.0 / Pi`
 *   Cartesian 3-D sets (GEOAC_EQ_3D, GEOAC_EQ_3D_RNGDEP):      axis 0 = x, axis 1 = y [km], STATE+0 and STATE+1
 *   GEOAC_EQ_2D:                                               axis 0 = range [km], STATE+0; n[1] must be 1 and axis 1 is not read
 * Every record with GEOAC_REC_VALID != 0 whose leg lies in [leg_min, leg_max] and whose GEOAC_REC_TURN lies in [turn_min, turn_max) is an
 * arrival of the map; it falls into cell floor((c - origin) / step) per axis, or is counted as `outside` when that leaves the grid.
 *
 * Members and frequencies: M = n_src * K members, ordered as geoac_fan_fetch orders them; F = n_freq (M > 1 and F > 1 exclude each other).
 * The level of an arrival is the sum of the two dB columns of its row: (calc_amp ? 20 log10(AMP) : 0) - ATTEN, with a frequency set
 * 20 log10(AMP) - atten[f].  It is formed once per arrival into level[M][F][n_rays][legs] (NaN where the leg is not VALID).
 *
 * Every reduction is an integer atomic (counts; minima and maxima on the order-preserving 64-bit key of the double), so a map is the same
 * bits on every run.  Arrivals whose level is not finite count in COUNT, TTIME_MIN and CEL_MAX and are left out of LEVEL_MAX, BEST and DETECT.
 *
 * Call order: geoac_fan_launch, then geoac_fan_map any number of times (another grid, another turning-height band: the fan is not integrated
 * again).  A new launch, geoac_fan_set_angles, an atmosphere upload, geoac_set_sources and geoac_set_frequencies invalidate map and level
 * table: the fetches then return GEOAC_E_INVALID.  All device work goes to the context's stream.  A context that never calls an entry point
 * of this header allocates nothing and launches nothing for it.  The pool (geoac_multi.h) has no map call.
 */
#ifndef GEOAC_MAP_H_
#define GEOAC_MAP_H_

#include "geoac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- layers: 8 bytes per cell, row-major, axis 1 fastest ---- */
enum {
    GEOAC_MAP_COUNT     = 0,   /* [M][n0][n1]    u64  arrivals in the cell                                          empty: 0    */
    GEOAC_MAP_TTIME_MIN = 1,   /* [M][n0][n1]    f64  smallest GEOAC_REC_TTIME [s]                                  empty: +inf */
    GEOAC_MAP_CEL_MAX   = 2,   /* [M][n0][n1]    f64  largest GEOAC_REC_RANGE / GEOAC_REC_TTIME (one IEEE division) empty: -inf */
    GEOAC_MAP_LEVEL_MAX = 3,   /* [M][F][n0][n1] f64  largest finite level [dB]                                     empty: -inf */
    GEOAC_MAP_BEST      = 4,   /* [M][F][n0][n1] i64  ray * legs + leg of the arrival holding LEVEL_MAX, the smallest on a tie; empty: -1 */
    GEOAC_MAP_LAYERS    = 5
};

#define GEOAC_MAP_MAX_CELLS (1 << 24)

typedef struct {
    double origin[2];     /* coordinate of the low edge of cell 0 per axis (finite)                                             */
    double step[2];       /* cell size per axis (finite, > 0)                                                                   */
    int    n[2];          /* cells per axis (>= 1, n[0] * n[1] <= GEOAC_MAP_MAX_CELLS; GEOAC_EQ_2D: n[1] == 1)                   */
    int    wrap_lon;      /* spherical sets only: lon -= 360 floor((lon - origin[1]) / 360) before binning                      */
    int    leg_min;       /* legs leg_min .. leg_max take part, both inclusive (0 <= leg_min <= leg_max; leg_max may exceed the  */
    int    leg_max;       /*   launch's last leg)                                                                               */
    double turn_min;      /* arrivals with turn_min <= GEOAC_REC_TURN < turn_max take part (-inf / +inf: no bound; not NaN,      */
    double turn_max;      /*   turn_min < turn_max)                                                                             */
    double detect_db;     /* NaN: no detection map; otherwise DETECT counts the members whose LEVEL_MAX >= detect_db            */
} geoac_map_spec;

/* host-only validation of a spec for an equation set (no device needed): GEOAC_OK and the cell count n[0] * n[1], or GEOAC_E_INVALID */
int  geoac_map_check(int eqset, const geoac_map_spec* spec, int64_t* cells);

/* bin the arrivals of the last completed launch.  GEOAC_E_INVALID (with geoac_last_error): no completed launch, or one invalidated since;
 * a spec geoac_map_check refuses.  GEOAC_E_NOMEM: the layers could not be allocated on the device. */
int  geoac_fan_map(geoac_ctx* ctx, const geoac_map_spec* spec);
/* shape of the current map: M, F, n0, n1 */
int  geoac_fan_map_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1);
/* one layer (GEOAC_MAP_*) to the host / its device pointer (valid until the next geoac_fan_map, ordered on the context's stream) */
int  geoac_fan_map_fetch(geoac_ctx* ctx, int layer, void* host);
int  geoac_fan_map_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes);
/* DETECT [F][n0][n1] u32; GEOAC_E_INVALID when the map was made with detect_db = NaN */
int  geoac_fan_map_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host);
/* outside[M]: arrivals that passed the filters and fell off the grid */
int  geoac_fan_map_outside(geoac_ctx* ctx, uint64_t* outside_host);
/* HIP-event time of the last geoac_fan_map on the context's stream [ms] (waits for it) */
int  geoac_fan_map_timing(geoac_ctx* ctx, double* ms);

/* level[M][F][n_rays][legs] f64 of the last completed launch (formed on first use after a launch): to the host / its device pointer */
int  geoac_fan_fetch_level(geoac_ctx* ctx, double* level_host);
int  geoac_fan_level_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_MAP_H_ */
