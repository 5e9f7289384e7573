/* geoac_tubemap.h - tube maps: the landing triangles of one launch rasterised on the grid of an arrival map, on the device.
 *
 * geoac_fan_map (geoac_map.h) bins arrival points, so its result depends on the grid: finer than the landing spacing of the rays it has holes,
 * coarser it counts rays per cell.  The physical object is the ray tube: a lattice triangle's landing triangle covers an area of ground and every
 * point inside it has one first-order eigenray (geoac_stations.h).  geoac_fan_tubemap goes triangle by triangle over the grid cells a landing
 * triangle can cover, runs the station header's inside test at each cell centre and reduces the hits into layers.  The map has no holes inside
 * an insonified region, its COUNT is the multipath count (eigenrays reaching the cell centre), and it is by construction what geoac_fan_stations
 * returns at every cell centre.
 *
 * Definition (normative).  The grid is that of geoac_map_spec (same axes: spherical sets latitude, longitude [deg]; Cartesian 3-D sets x, y [km]),
 * the lattice and the triangle filters are those of geoac_station_spec.  The centre of cell (i0, i1) is
 *   s_a = origin[a] + (i_a + 0.5) * step[a]          (the product is rounded before the sum)
 * A hit of cell (i0, i1), member m, is a (leg, triangle) pair that geoac_stations.h reports for a station at (s_0, s_1): the same triangulation
 * (triangle 2 * cell = (a, b, c), 2 * cell + 1 = (a, c, d), n_tri = 2 * cells), the same VALID / turn_tol / edge_max filters, the same longitude
 * wrap relative to the station on the spherical sets, the same cross products, sign rule and weights Wk = wk / s - and one filter more: the
 * hit's interpolated GEOAC_STA_TURN, ((W0 * t0) + (W1 * t1)) + (W2 * t2) of the corners' GEOAC_REC_TURN, must lie in [turn_min, turn_max).
 * Every interpolated value of a hit is the station row's value, operation for operation: GEOAC_STA_TTIME, GEOAC_STA_CELERITY (interpolated range /
 * interpolated travel time) and level[f] of the station lists.  All of it is IEEE double without fused multiply-adds; a host restatement gives the
 * same bits (tests/tubemap_reference.py, built on tests/station_reference.py).
 *
 * The station rule always takes a corner's longitude relative to the station modulo 360, so on the spherical sets a cell's hits do not depend
 * on wrap_lon: the field is validated as geoac_map_check validates it and is otherwise not read.
 *
 * Layers, 8 bytes per cell, row-major, axis 1 fastest (M members, F frequencies and their order as in geoac_map.h):
 *   GEOAC_TUBE_COUNT     [M][n0][n1]    u64  hits: the multipath count                                              empty: 0
 *   GEOAC_TUBE_TTIME_MIN [M][n0][n1]    f64  smallest interpolated travel time [s]                                  empty: +inf
 *   GEOAC_TUBE_CEL_MAX   [M][n0][n1]    f64  largest GEOAC_STA_CELERITY [km/s]                                      empty: -inf
 *   GEOAC_TUBE_LEVEL_MAX [M][F][n0][n1] f64  largest finite interpolated level [dB]                                 empty: -inf
 *   GEOAC_TUBE_BEST      [M][F][n0][n1] i64  leg * n_tri + tri of the hit holding LEVEL_MAX, the smallest on a tie  empty: -1
 *   DETECT               [F][n0][n1]    u32  members whose LEVEL_MAX >= detect_db                                   absent when detect_db is NaN
 * Hits whose level is not finite count in COUNT, TTIME_MIN and CEL_MAX and are left out of LEVEL_MAX, BEST and DETECT.  Minima and maxima are
 * taken on the order-preserving 64-bit key of the double (geoac_map.h), and every reduction is an integer atomic: a tube map is the same bits
 * on every run.
 *
 * Refusals (geoac_tube_fault names the first).  GEOAC_EQ_2D: GEOAC_E_UNSUPPORTED.  GEOAC_E_INVALID: everything geoac_map_check refuses for
 * origin, step, n, wrap_lon, the leg band, the turning band, and everything geoac_station_check refuses for n_theta, n_phi, phi_periodic, turn_tol,
 * edge_max; edge_max that is not finite (without it a triangle's candidate cells are unbounded, and on the spherical sets a triangle stretched
 * across a station's antimeridian would cover the grid); on the spherical sets edge_max >= 180 or n[1] * step[1] > 360; a per-triangle candidate
 * span (2 edge_max / step[0] + 3) * (2 edge_max / step[1] + 3) above GEOAC_TUBE_MAX_SPAN; launch angles that are not the lattice the spec names
 * (the bit-for-bit host check of geoac_fan_stations).
 *
 * Call order and invalidation are those of geoac_map.h (the map's generation counter is used): geoac_fan_launch, then geoac_fan_tubemap any
 * number of times; a new launch, geoac_fan_set_angles, an atmosphere upload, geoac_set_sources and geoac_set_frequencies invalidate the layers
 * (the fetches return GEOAC_E_INVALID).  All device work goes to the context's stream.  A context that never calls an entry point of this header
 * allocates nothing and launches nothing for it.  The pool (geoac_multi.h) has no tube-map call.
 */
#ifndef GEOAC_TUBEMAP_H_
#define GEOAC_TUBEMAP_H_

#include "geoac_stations.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GEOAC_TUBE_COUNT     = 0,
    GEOAC_TUBE_TTIME_MIN = 1,
    GEOAC_TUBE_CEL_MAX   = 2,
    GEOAC_TUBE_LEVEL_MAX = 3,
    GEOAC_TUBE_BEST      = 4,
    GEOAC_TUBE_LAYERS    = 5
};

/* largest per-triangle candidate span (2 edge_max / step[0] + 3) * (2 edge_max / step[1] + 3) a spec may ask for: a box of 1 024 x 1 024 cell
 * centres for one landing triangle, 16 384 trips of a wave.  A larger span means a grid far finer than the fan it rasterises. */
#define GEOAC_TUBE_MAX_SPAN (1 << 20)
/* a triangle proposing more candidate centres than this is walked by its whole wave, 64 centres per trip, instead of by its own lane */
#define GEOAC_TUBE_COOP_MIN 32

typedef struct {
    double origin[2];        /* the grid of geoac_map_spec: low edge of cell 0 per axis (finite)                                          */
    double step[2];          /*   cell size per axis (finite, > 0)                                                                        */
    int    n[2];             /*   cells per axis (>= 1, n[0] * n[1] <= GEOAC_MAP_MAX_CELLS)                                                */
    int    wrap_lon;         /*   0 or 1, spherical sets only; does not change the layers (see above)                                     */
    int    n_theta, n_phi;   /* the lattice of geoac_station_spec: ray = j * n_theta + i, n_theta * n_phi == n_rays, both >= 2             */
    int    phi_periodic;     /*   1: azimuth column n_phi - 1 neighbours column 0                                                         */
    int    leg_min, leg_max; /* legs leg_min .. leg_max take part, both inclusive (0 <= leg_min <= leg_max)                               */
    double turn_tol;         /* max - min of the corners' GEOAC_REC_TURN <= turn_tol (+inf: no bound; not NaN, >= 0)                      */
    double edge_max;         /* longest side of the landing triangle, in axis units, <= edge_max (finite, > 0; spherical sets: < 180)     */
    double turn_min;         /* hits with turn_min <= interpolated GEOAC_STA_TURN < turn_max take part (-inf / +inf: no bound; not NaN,    */
    double turn_max;         /*   turn_min < turn_max)                                                                                    */
    double detect_db;        /* NaN: no detection map; otherwise DETECT counts the members whose LEVEL_MAX >= detect_db                   */
} geoac_tube_spec;

/* host-only validation (no device needed): GEOAC_OK and the cell count n[0] * n[1]; GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D; GEOAC_E_INVALID for
 * anything else that is wrong.  geoac_tube_fault names the first fault (NULL: none; a string literal, valid for ever). */
int         geoac_tube_check(int eqset, const geoac_tube_spec* spec, int n_rays, int64_t* cells);
const char* geoac_tube_fault(int eqset, const geoac_tube_spec* spec, int n_rays);

/* rasterise the landing triangles of the last completed launch.  GEOAC_E_INVALID (with geoac_last_error): no completed launch, or one
 * invalidated since; a spec geoac_tube_check refuses; launch angles that are not the lattice the spec names.  GEOAC_E_UNSUPPORTED: the 2-D set.
 * GEOAC_E_NOMEM: the layers could not be allocated on the device. */
int  geoac_fan_tubemap(geoac_ctx* ctx, const geoac_tube_spec* spec);
/* shape of the current tube map: M, F, n0, n1 */
int  geoac_fan_tubemap_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1);
/* one layer (GEOAC_TUBE_*) to the host / its device pointer (valid until the next geoac_fan_tubemap, ordered on the context's stream) */
int  geoac_fan_tubemap_fetch(geoac_ctx* ctx, int layer, void* host);
int  geoac_fan_tubemap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes);
/* DETECT [F][n0][n1] u32; GEOAC_E_INVALID when the map was made with detect_db = NaN */
int  geoac_fan_tubemap_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host);
/* HIP-event time of the last geoac_fan_tubemap on the context's stream [ms] (waits for it) */
int  geoac_fan_tubemap_timing(geoac_ctx* ctx, double* ms);
/* work counters of the last geoac_fan_tubemap, four u64: triangles that passed the station-independent filters and proposed at least one
 * centre, triangles among them walked cooperatively by a wave, candidate centres tested, 0 (spare).  They describe the walk, not the result. */
int  geoac_fan_tubemap_stats(geoac_ctx* ctx, uint64_t* stats4);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_TUBEMAP_H_ */
