/* geoac_lstations.h - level stations: first-order eigenray estimates at R receivers above the ground, from the level crossings of one launch, on
 * the device.
 *
 * geoac_fan_stations (geoac_stations.h) answers "what arrives at my receiver, launched at which angles, and when?" for a receiver on the ground:
 * it searches the landing triangles of a lattice fan.  A receiver at altitude - a balloon, an aircraft, a mountain array - needs the same search
 * over the points where the rays pass through its altitude.  A launch with levels (geoac_levels.h) leaves those points on the device: per
 * (member, ray, level) the first cap_levels passages in path order.  geoac_fan_level_stations joins the two: a station names a horizontal
 * position and one of the launch's levels, and the crossing triangles of that level that enclose the position give the estimates.
 *
 * Stations.  sta [n_sta][2] holds the horizontal position in the axes of geoac_stations.h: latitude, longitude [deg] for the spherical sets
 * (GEOAC_EQ_GLOBAL, GEOAC_EQ_GLOBAL_RNGDEP), x, y [km] for the Cartesian 3-D sets.  level_of[s] in 0 .. L-1 is the index of the station's altitude
 * in the level list of the launch that produced the crossings; any number of stations may share a level.  GEOAC_EQ_2D returns GEOAC_E_UNSUPPORTED
 * (it has neither level crossings nor a lattice).
 *
 * Branches.  The crossings kept for one (ray, level) are in path order: only the first min(count, cap_levels) exist here.  Crossing k gets the
 * ordinal o = the number of earlier kept crossings of that (ray, level) with the same GEOAC_LVL_LEG and the same GEOAC_LVL_DIR.  Its branch is
 * (leg, d, o), d = 0 for an upward and 1 for a downward passage, and the branch index is
 *     b = ((leg - leg0) * 2 + d) * ord_max + o        leg0 = leg_min,  0 <= o < ord_max,  B = n_legs * 2 * ord_max branches
 * with n_legs the legs leg_min .. min(leg_max, legs - 1) of the launch.  The ordinals of the kept crossings are exact because they are the first
 * in path order, so a ray whose count ran past cap_levels still serves the branches it holds.  Corners are matched by branch and not by record
 * slot k: a ray whose leg 0 turns below a level and its neighbour whose leg 0 passes it twice still pair their leg-1 crossings.
 *
 * Triangles and the hit rule.  Lattice cells, the triangles 2 * cell and 2 * cell + 1, phi_periodic and the corner order are those of
 * geoac_stations.h, word for word.  A triangle takes part on branch b at level l when all three corner rays hold branch b at level l and when
 * the longest side of its crossing triangle is <= edge_max (compared as squares).  A corner's crossing point is GEOAC_LVL_P0, P0 + 1 for the
 * Cartesian sets and (P0 + 1) * 180.0 / Pi, (P0 + 2) * 180.0 / Pi for the spherical sets; it is taken relative to the station, x = c0 - s0,
 * y = c1 - s1, and for the spherical sets y = y - 360.0 * floor((y + 180.0) / 360.0).  The cross products w0, w1, w2, their sum s and the sign rule
 * are those of geoac_stations.h: a hit when s != 0 and all three w are >= 0 or all three are <= 0; Wk = wk / s.  A station exactly on an edge
 * shared by two triangles is a hit of both, a station exactly on a crossing point a hit of every triangle around it.  There is no VALID test on
 * the leg's record - a ray that later leaves the medium has still crossed - and no turn_tol: a triangle that spans a stratospheric and a
 * thermospheric return is stretched, and edge_max removes it.
 *
 * Row of a hit: GEOAC_LSTA_STRIDE doubles.  Every interpolated column is ((W0 * v0) + (W1 * v1)) + (W2 * v2), in IEEE double without fused
 * multiply-adds, so that a host restatement gives the same bits (tests/lstation_reference.py).  THETA and PHI interpolate the lattice axes;
 * under phi_periodic corners 1 and 2 of PHI are first brought within 180 degrees of corner 0 (d = vk - v0, d = d - 360.0 * floor((d + 180.0) /
 * 360.0), vk = v0 + d).  TTIME, ATTEN and N0 .. N2 interpolate GEOAC_LVL_TTIME, GEOAC_LVL_ATTEN and GEOAC_LVL_P0 + 3 .. + 5 of the corners'
 * crossing records (the slowness components the path row carries; GEOAC_EQ_3D carries one, its N1 and N2 are 0).  With a frequency set ATTEN is
 * that of frequency 0, as in the crossing records.
 *
 * Order and overflow.  The rows of a (member, station) list are sorted by the key b * n_tri + tri, ascending.  hits[m][s] is the true number of
 * hits and may exceed cap; the cap smallest keys are the rows kept; unused rows are zero.  No floating-point value is reduced across threads and
 * nothing is ordered by an atomic: the result is the same bits on every run.
 *
 * Validity.  The lists are current while the context's invalidation counter is unchanged, as for geoac_fan_stations.  The call itself also needs
 * geoac_fan_levels_dev to succeed: the last completed launch had levels and the level list has not changed since; otherwise GEOAC_E_INVALID, and
 * geoac_last_error names which of the two failed.  All device work goes to the context's stream.  A context that never calls an entry point of
 * this header allocates nothing and launches nothing for it.
 *
 * Not covered: the amplitude at altitude (path rows carry no Jacobian), the pool (geoac_multi.h) and the command-line drivers.  A tube map at
 * altitude - these hits at every cell centre of a grid, reduced - is geoac_fan_level_tubemap (geoac_ltubemap.h), which shares the branch table
 * this call forms.  The estimates are refined by a call of their own: geoac_fan_level_refine (geoac_level_refine.h) takes every kept row of these lists
 * as a seed and iterates it to the ray that passes the station (geoac_fan_refine works on the ground lists).
 */
#ifndef GEOAC_LSTATIONS_H_
#define GEOAC_LSTATIONS_H_

#include "geoac_levels.h"
#include "geoac_stations.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_LSTA_STRIDE 16
enum {
    GEOAC_LSTA_LEG    = 0,    /* leg of the passage                                                          */
    GEOAC_LSTA_DIR    = 1,    /* +1 upward, -1 downward                                                      */
    GEOAC_LSTA_ORD    = 2,    /* ordinal of the passage among those of its leg and direction                 */
    GEOAC_LSTA_TRI    = 3,    /* triangle index, 2 * cell + (0 | 1)                                          */
    GEOAC_LSTA_RAY0   = 4,    /* ray index of corner 0 (= corner a of the cell, j * n_theta + i)             */
    GEOAC_LSTA_ORIENT = 5,    /* sign of s, +1 or -1                                                         */
    GEOAC_LSTA_W0     = 6,    /* barycentric weights of corners 0, 1, 2                                      */
    GEOAC_LSTA_W1     = 7,
    GEOAC_LSTA_W2     = 8,
    GEOAC_LSTA_THETA  = 9,    /* launch inclination of the estimate [deg]                                    */
    GEOAC_LSTA_PHI    = 10,   /* launch azimuth [deg]                                                        */
    GEOAC_LSTA_TTIME  = 11,   /* travel time to the station [s]                                              */
    GEOAC_LSTA_ATTEN  = 12,   /* attenuation [dB] at geoac_params.freq                                       */
    GEOAC_LSTA_N0     = 13    /* N0 .. N2 = interpolated P3 .. P5 of the crossing records (columns 13 .. 15) */
};

typedef struct {
    int    n_theta, n_phi, phi_periodic;   /* the lattice, exactly as in geoac_station_spec                                                     */
    int    leg_min, leg_max;               /* legs that take part, both inclusive (0 <= leg_min <= leg_max; leg_max may exceed the last leg)    */
    int    ord_max;                        /* ordinals 0 .. ord_max - 1 take part; 1 .. GEOAC_LVL_MAX_CAP                                       */
    double edge_max;                       /* longest side of the crossing triangle, in axis units, <= edge_max (+inf: no bound; not NaN, > 0)  */
    int    cap;                            /* rows kept per (member, station), 1 .. GEOAC_STA_MAX_CAP                                           */
} geoac_lstation_spec;

/* host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D, GEOAC_E_INVALID for anything else that is wrong
 * (n_theta * n_phi != n_rays, a bad field, n_levels outside 1 .. GEOAC_MAX_LEVELS, n_sta outside 1 .. GEOAC_STA_MAX_STATIONS, a level_of entry
 * outside 0 .. n_levels - 1); geoac_lstation_fault names the first fault (NULL: none; a string literal, valid for ever) */
int         geoac_lstation_check(int eqset, const geoac_lstation_spec* spec, int n_rays, int n_levels, int n_sta, const int32_t* level_of);
const char* geoac_lstation_fault(int eqset, const geoac_lstation_spec* spec, int n_rays, int n_levels, int n_sta, const int32_t* level_of);

/* the level-station lists of the last completed launch.  sta: [n_sta][2] host doubles in the axes above; level_of: [n_sta] host indices into the
 * launch's level list.  GEOAC_E_INVALID (with geoac_last_error): no completed launch, or one invalidated since; a launch without levels, or a
 * level list changed since; a spec or a level_of entry geoac_lstation_check refuses; launch angles that are not the lattice the spec names.
 * GEOAC_E_UNSUPPORTED: the 2-D set.  GEOAC_E_NOMEM: the branch table or the lists could not be allocated on the device. */
int  geoac_fan_level_stations(geoac_ctx* ctx, const geoac_lstation_spec* spec, int n_sta, const double* sta, const int32_t* level_of);
/* shape of the current lists: M, n_sta, cap */
int  geoac_fan_level_stations_shape(geoac_ctx* ctx, int* n_members, int* n_sta, int* cap);
/* hits [M][n_sta] u32, rows [M][n_sta][cap][GEOAC_LSTA_STRIDE] f64 to the host (either may be NULL) */
int  geoac_fan_level_stations_fetch(geoac_ctx* ctx, uint32_t* hits, double* rows);
/* device pointer of one of them (which: 0 hits, 1 rows), valid until the next geoac_fan_level_stations, ordered on the context's stream */
int  geoac_fan_level_stations_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes);
/* HIP-event time of the last geoac_fan_level_stations on the context's stream [ms] (waits for it) */
int  geoac_fan_level_stations_timing(geoac_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_LSTATIONS_H_ */
