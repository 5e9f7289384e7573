/* geoac_stations.h - station arrivals: first-order eigenray estimates at R receivers from the record table of one launch, on the device.
 *
 * A launched fan whose angles form a lattice (n_theta inclinations x n_phi azimuths, ray = j * n_theta + i, the order of geoac_fan_enumerate)
 * maps every lattice triangle to a landing triangle per leg.  A landing triangle that encloses a station contains an eigenray to first order,
 * and barycentric interpolation inside it gives that eigenray's launch angles, travel time, celerity, turning height, arrival angles and level.
 * This is the classical first stage of an eigenray search (the reference's GeoAc_EstimateEigenray does it one scan at a time); the estimates
 * are the natural seeds of a refinement (-eig_direct; geoac_fan_refine, geoac_refine.h).  Nothing is refined here.
 *
 * geoac_fan_stations reads only the record table, the launch angles and the level table (geoac_map.h), so it serves the four 3-D equation
 * sets alike and every member of an ensemble, a source set or a frequency set: M = n_src * K members, F = n_freq, as in geoac_map.h.
 *
 * Station coordinates are the axes of the map: spherical sets (GEOAC_EQ_GLOBAL, GEOAC_EQ_GLOBAL_RNGDEP) latitude, longitude [deg]; Cartesian 3-D
 * sets (GEOAC_EQ_3D, GEOAC_EQ_3D_RNGDEP) x, y [km].  GEOAC_EQ_2D returns GEOAC_E_UNSUPPORTED: on one axis the search is for the interval between
 * two neighbouring rays that holds the station's range, a different (1-D) routine that this header does not provide.
 *
 * Triangles.  Lattice cell (i, j), cell = j * (n_theta - 1) + i, has the corners a = (i, j), b = (i + 1, j), c = (i + 1, j + 1), d = (i, j + 1);
 * with phi_periodic the column after n_phi - 1 is column 0 (n_phi columns of cells instead of n_phi - 1).  Triangle 2 * cell = (a, b, c),
 * triangle 2 * cell + 1 = (a, c, d); n_tri = 2 * cells.  A triangle takes part on leg l when all three corner records are VALID on l, when
 * max - min of their GEOAC_REC_TURN is <= turn_tol, and when the longest side of its landing triangle is <= edge_max (compared as squares:
 * dx * dx + dy * dy <= edge_max * edge_max).
 *
 * Geometry, all in IEEE double without fused multiply-adds, so that a host restatement gives the same bits (tests/station_reference.py).
 * A corner's landing point is taken in the map's coordinates (spherical: STATE+1, STATE+2 `* 180.0 / Pi`) relative to the station: x = c0 - s0,
 * y = c1 - s1, and for the spherical sets y = y - 360.0 * floor((y + 180.0) / 360.0).  (A triangle whose corners lie on both sides of the
 * station's antimeridian is therefore stretched around the globe; edge_max removes it.)  With the corner offsets p0, p1, p2:
 *   w0 = p1 x p2, w1 = p2 x p0, w2 = p0 x p1   (a x b = ax * by - ay * bx),   s = (w0 + w1) + w2
 * The triangle is a hit when s != 0 and all three w are >= 0 or all three are <= 0; the weights are Wk = wk / s.  A station exactly on an edge
 * shared by two triangles is a hit of both (one weight is 0 in each), a station exactly on a landing point a hit of every triangle around it.
 *
 * Row of a hit: GEOAC_STA_STRIDE doubles.  Every interpolated column is ((W0 * v0) + (W1 * v1)) + (W2 * v2) of the corners' values.  Before
 * interpolating PHI (under phi_periodic only) and BACKAZ (always) corners 1 and 2 are brought within 180 degrees of corner 0:
 * d = vk - v0, d = d - 360.0 * floor((d + 180.0) / 360.0), vk = v0 + d; the result is not wrapped again (it is continuous with corner 0).
 * level[.., f] interpolates level[m][f][ray][leg] of geoac_map.h the same way (NaN when a corner's level is NaN).
 *
 * Order and overflow.  The rows of a (member, station) list are sorted by the key leg * n_tri + tri, ascending.  hits[m][s] is the true number
 * of hits and may exceed cap; the cap smallest keys are the rows kept; unused rows (and their levels) are zero.  No floating-point value is
 * reduced across threads and nothing is ordered by an atomic: the result is the same bits on every run.
 *
 * Call order and invalidation are those of geoac_map.h: geoac_fan_launch, then geoac_fan_stations any number of times; a new launch,
 * geoac_fan_set_angles, an atmosphere upload, geoac_set_sources and geoac_set_frequencies invalidate the lists (the fetches return
 * GEOAC_E_INVALID).  All device work goes to the context's stream.  A context that never calls an entry point of this header allocates nothing
 * and launches nothing for it.  The pool (geoac_multi.h) has no station call.
 */
#ifndef GEOAC_STATIONS_H_
#define GEOAC_STATIONS_H_

#include "geoac_map.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_STA_STRIDE 16
enum {
    GEOAC_STA_LEG      = 0,    /* leg of the arrival                                                          */
    GEOAC_STA_TRI      = 1,    /* triangle index, 2 * cell + (0 | 1)                                          */
    GEOAC_STA_RAY0     = 2,    /* ray index of corner 0 (= corner a of the cell, j * n_theta + i)             */
    GEOAC_STA_ORIENT   = 3,    /* sign of s, +1 or -1: it flips across a caustic                              */
    GEOAC_STA_W0       = 4,    /* barycentric weights of corners 0, 1, 2                                      */
    GEOAC_STA_W1       = 5,
    GEOAC_STA_W2       = 6,
    GEOAC_STA_THETA    = 7,    /* launch inclination of the estimate [deg]                                    */
    GEOAC_STA_PHI      = 8,    /* launch azimuth [deg]                                                        */
    GEOAC_STA_TTIME    = 9,    /* travel time [s]                                                             */
    GEOAC_STA_CELERITY = 10,   /* interpolated GEOAC_REC_RANGE / interpolated GEOAC_REC_TTIME [km/s]          */
    GEOAC_STA_TURN     = 11,   /* turning height [km]                                                         */
    GEOAC_STA_INCL     = 12,   /* arrival inclination [deg]                                                   */
    GEOAC_STA_BACKAZ   = 13    /* back azimuth [deg], continuous with corner 0                                */
                               /* columns 14, 15: spare, zero                                                 */
};

#define GEOAC_STA_MAX_CAP      256
#define GEOAC_STA_MAX_STATIONS (1 << 24)

typedef struct {
    int    n_theta, n_phi;   /* the launch angles are a lattice: ray = j * n_theta + i, i = inclination index (fast), j = azimuth index;
                                n_theta * n_phi == n_rays, both >= 2; every ray of row i carries the same theta, every ray of column j the
                                same phi, bit for bit (checked on the host copy of the angles: GEOAC_E_INVALID otherwise)                 */
    int    phi_periodic;     /* 1: azimuth column n_phi - 1 neighbours column 0 (a -180 .. 179 fan); 0 or 1                               */
    int    leg_min, leg_max; /* legs leg_min .. leg_max take part, both inclusive (0 <= leg_min <= leg_max; leg_max may exceed the
                                launch's last leg)                                                                                        */
    double turn_tol;         /* max - min of the corners' GEOAC_REC_TURN <= turn_tol (+inf: no bound; not NaN, >= 0)                      */
    double edge_max;         /* longest side of the landing triangle, in axis units, <= edge_max (+inf: no bound; not NaN, > 0)           */
    int    cap;              /* rows kept per (member, station), 1 .. GEOAC_STA_MAX_CAP                                                   */
} geoac_station_spec;

/* host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D, GEOAC_E_INVALID for anything else that is wrong
 * (n_theta * n_phi != n_rays, a bad field, n_sta outside 1 .. GEOAC_STA_MAX_STATIONS); geoac_station_fault names the first fault (NULL: none;
 * a string literal, valid for ever) */
int         geoac_station_check(int eqset, const geoac_station_spec* spec, int n_rays, int n_sta);
const char* geoac_station_fault(int eqset, const geoac_station_spec* spec, int n_rays, int n_sta);

/* the station lists of the last completed launch.  sta: [n_sta][2] host doubles in the axes above.  GEOAC_E_INVALID (with geoac_last_error):
 * no completed launch, or one invalidated since; a spec geoac_station_check refuses; launch angles that are not the lattice the spec names.
 * GEOAC_E_UNSUPPORTED: the 2-D set.  GEOAC_E_NOMEM: the lists could not be allocated on the device. */
int  geoac_fan_stations(geoac_ctx* ctx, const geoac_station_spec* spec, int n_sta, const double* sta);
/* shape of the current lists: M, F, n_sta, cap */
int  geoac_fan_stations_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n_sta, int* cap);
/* hits [M][n_sta] u32, rows [M][n_sta][cap][GEOAC_STA_STRIDE] f64, level [M][n_sta][cap][F] f64 to the host (any of them may be NULL) */
int  geoac_fan_stations_fetch(geoac_ctx* ctx, uint32_t* hits, double* rows, double* level);
/* device pointer of one of them (which: 0 hits, 1 rows, 2 level), valid until the next geoac_fan_stations, ordered on the context's stream */
int  geoac_fan_stations_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes);
/* HIP-event time of the last geoac_fan_stations on the context's stream [ms] (waits for it) */
int  geoac_fan_stations_timing(geoac_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_STATIONS_H_ */
