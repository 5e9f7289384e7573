/* geoac_ltubemap.h - level tube maps: the crossing triangles of one launch rasterised per level on the grid of an arrival map, on the device.
 *
 * geoac_fan_tubemap (geoac_tubemap.h) answers on the ground "where is this source heard, over how many paths, and when does the first arrive?".
 * A launch with levels (geoac_levels.h) leaves every ray's passages through L altitudes on the device, and geoac_fan_level_stations
 * (geoac_lstations.h) searches their crossing triangles at given receivers.  geoac_fan_level_tubemap asks the ground map's question at those
 * altitudes: it goes branch plane by branch plane, triangle by triangle over the grid cells a crossing triangle can cover, runs the level-station
 * header's inside test at each cell centre and reduces the hits into layers.  It is by construction what geoac_fan_level_stations returns with one
 * station per cell centre, reduced - without the walk of every lattice cell against every centre.  A map cell names a branch and a triangle,
 * which is what geoac_fan_level_stations and after it geoac_fan_level_refine (geoac_level_refine.h) take on from.
 *
 * Definition (normative).  The grid is that of geoac_map_spec (origin, step, n, wrap_lon; spherical sets latitude, longitude [deg]; Cartesian
 * 3-D sets x, y [km]); the lattice, the legs, ord_max and edge_max are those of geoac_lstation_spec.  level_mask selects levels of the launch's
 * list: bit l selects level l, Ls is the number of bits set, and layer index ls counts the selected levels in ascending level index.  The centre
 * of cell (i0, i1) is
 *   s_a = origin[a] + (i_a + 0.5) * step[a]          (the product is rounded before the sum)
 * A hit of cell (m, l, i0, i1) is a row that geoac_fan_level_stations reports for a station at (s_0, s_1) with level_of = l under the same
 * lattice, legs, ord_max and edge_max, whose direction is in dir_mask (bit 0: upward rows, GEOAC_LSTA_DIR = +1; bit 1: downward rows).
 * Everything else is geoac_lstations.h's, operation for operation: the branch rule, corner matching by branch and not by record slot, no VALID
 * test and no turn_tol, the longitude wrap relative to the station on the spherical sets, the cross products and the sign rule, Wk = wk / s.
 * A hit's travel time and attenuation are the row's GEOAC_LSTA_TTIME and GEOAC_LSTA_ATTEN, ((W0 * v0) + (W1 * v1)) + (W2 * v2) of the corners'
 * crossing records; with a frequency set that is frequency 0, as in the records.  calc_amp may be 0 or 1.  All of it is IEEE double without
 * fused multiply-adds; a host restatement gives the same bits (tests/ltubemap_reference.py, built on tests/lstation_reference.py).
 *
 * The rule always takes a corner's longitude relative to the centre modulo 360, so on the spherical sets a cell's hits do not depend on
 * wrap_lon: the field is validated as geoac_map_check validates it and is otherwise not read.
 *
 * Layers, 8 bytes per cell, row-major, axis 1 fastest (M members as in geoac_map.h):
 *   GEOAC_LTUBE_COUNT     [M][Ls][n0][n1] u64  hits: the multipath count at that altitude                               empty: 0
 *   GEOAC_LTUBE_TTIME_MIN [M][Ls][n0][n1] f64  smallest interpolated travel time [s]                                    empty: +inf
 *   GEOAC_LTUBE_ATTEN_MIN [M][Ls][n0][n1] f64  smallest interpolated attenuation [dB] (positive, as GEOAC_LVL_ATTEN)     empty: +inf
 *   GEOAC_LTUBE_FIRST     [M][Ls][n0][n1] i64  b * n_tri + tri of the hit holding TTIME_MIN, the smallest on a tie      empty: -1
 *   REACH                 [Ls][n0][n1]    u32  members with COUNT > 0
 * b is the branch index of geoac_lstations.h, ((leg - leg_min) * 2 + d) * ord_max + o, and n_tri = 2 * lattice cells.  A hit whose TTIME or ATTEN
 * is not finite counts in COUNT (and so in REACH) only: a cell all of whose hits are such has COUNT > 0 beside the empty markers.  Minima are taken
 * on the order-preserving 64-bit key of the double (geoac_map.h), and every reduction is an integer atomic: a map is the same bits on every run.
 *
 * There is no celerity layer.  A celerity at altitude is a range over a time, and the range needs each member's source point and the range
 * series of geoac_level_refine.h; a caller has both the cell centre and TTIME_MIN and forms it with its own source.  There is no amplitude
 * layer here: path rows carry no Jacobian (geoac_levels.h).  geoac_fan_level_ampmap (geoac_lampmap.h) forms one from the crossing triangles themselves.
 *
 * Refusals (geoac_ltube_fault names the first).  GEOAC_EQ_2D: GEOAC_E_UNSUPPORTED.  GEOAC_E_INVALID: everything geoac_map_check refuses for
 * origin, step, n and wrap_lon, everything geoac_lstation_check refuses for n_theta, n_phi, phi_periodic, leg_min, leg_max,
 * ord_max and edge_max; edge_max that is not finite; on the spherical sets edge_max >= 180 or n[1] * step[1] > 360; a per-triangle candidate span
 * (2 edge_max / step[0] + 3) * (2 edge_max / step[1] + 3) above GEOAC_TUBE_MAX_SPAN; dir_mask outside 1 .. 3; level_mask of 0 or with a bit at or
 * above the launch's level count.  At call time also what geoac_fan_level_stations refuses: no completed launch, or one invalidated since; a
 * launch without levels, or a level list changed since (the message of geoac_fan_levels_dev is passed on); launch angles that are not the
 * lattice the spec names.  GEOAC_E_NOMEM names the size it asked for.
 *
 * Call order and invalidation: geoac_fan_launch with levels, then geoac_fan_level_tubemap any number of times.  The layers are current while
 * the context's invalidation counter is unchanged (a new launch, geoac_fan_set_angles, an atmosphere upload, geoac_set_sources and
 * geoac_set_frequencies end them; the fetches then return GEOAC_E_INVALID), and the call and every fetch need geoac_fan_levels_dev to succeed, as
 * in geoac_lstations.h: geoac_set_levels ends the map too.  The branch table is the one geoac_fan_level_stations forms: a context that calls both with the same leg_min, leg_max and
 * ord_max forms it once per launch.  All device work goes to the context's stream.  A context that never calls an entry point of this header
 * allocates nothing and launches nothing for it.  The pool (geoac_multi.h) has no level-tube-map call.
 */
#ifndef GEOAC_LTUBEMAP_H_
#define GEOAC_LTUBEMAP_H_

#include "geoac_lstations.h"
#include "geoac_tubemap.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GEOAC_LTUBE_COUNT     = 0,
    GEOAC_LTUBE_TTIME_MIN = 1,
    GEOAC_LTUBE_ATTEN_MIN = 2,
    GEOAC_LTUBE_FIRST     = 3,
    GEOAC_LTUBE_LAYERS    = 4
};

typedef struct {
    double origin[2];        /* the grid of geoac_map_spec: low edge of cell 0 per axis (finite)                                          */
    double step[2];          /*   cell size per axis (finite, > 0)                                                                        */
    int    n[2];             /*   cells per axis (>= 1, n[0] * n[1] <= GEOAC_MAP_MAX_CELLS)                                                */
    int    wrap_lon;         /*   0 or 1, spherical sets only; does not change the layers (see above)                                     */
    int    n_theta, n_phi;   /* the lattice of geoac_lstation_spec: ray = j * n_theta + i, n_theta * n_phi == n_rays, both >= 2            */
    int    phi_periodic;     /*   1: azimuth column n_phi - 1 neighbours column 0                                                         */
    int    leg_min, leg_max; /* legs leg_min .. leg_max take part, both inclusive (0 <= leg_min <= leg_max; leg_max may exceed the last)  */
    int    ord_max;          /* ordinals 0 .. ord_max - 1 take part; 1 .. GEOAC_LVL_MAX_CAP                                               */
    double edge_max;         /* longest side of the crossing triangle, in axis units, <= edge_max (finite, > 0; spherical sets: < 180)    */
    int    dir_mask;         /* 1: upward passages, 2: downward passages, 3: both                                                         */
    int    level_mask;       /* bit l selects level l of the launch's list; not 0, no bit at or above the launch's level count            */
} geoac_ltube_spec;

/* host-only validation (no device needed) against a launch of n_rays rays and n_levels levels: GEOAC_OK and the cell count n[0] * n[1] and the
 * number of selected levels Ls (either pointer may be NULL); GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D; GEOAC_E_INVALID for anything else that is
 * wrong.  geoac_ltube_fault names the first fault (NULL: none; a string literal, valid for ever). */
int         geoac_ltube_check(int eqset, const geoac_ltube_spec* spec, int n_rays, int n_levels, int64_t* cells, int* n_selected);
const char* geoac_ltube_fault(int eqset, const geoac_ltube_spec* spec, int n_rays, int n_levels);

/* rasterise the crossing triangles of the last completed launch.  Statuses as listed under Refusals. */
int  geoac_fan_level_tubemap(geoac_ctx* ctx, const geoac_ltube_spec* spec);
/* shape of the current map: M, Ls, n0, n1 */
int  geoac_fan_level_tubemap_shape(geoac_ctx* ctx, int* n_members, int* n_selected, int* n0, int* n1);
/* one layer (GEOAC_LTUBE_*) to the host / its device pointer (valid until the next geoac_fan_level_tubemap, ordered on the context's stream) */
int  geoac_fan_level_tubemap_fetch(geoac_ctx* ctx, int layer, void* host);
int  geoac_fan_level_tubemap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes);
/* REACH [Ls][n0][n1] u32 */
int  geoac_fan_level_tubemap_fetch_reach(geoac_ctx* ctx, uint32_t* reach_host);
/* HIP-event time of the last geoac_fan_level_tubemap on the context's stream [ms] (waits for it; a branch table formed by the call is inside) */
int  geoac_fan_level_tubemap_timing(geoac_ctx* ctx, double* ms);
/* work counters of the last geoac_fan_level_tubemap, four u64: triangles that held their branch, passed the pre-test and proposed at least one
 * centre; triangles among them walked cooperatively by a wave; candidate centres tested; 1 when the call formed the branch table, 0 when it
 * found the one a former call of this header or of geoac_lstations.h had formed.  They describe the walk, not the result. */
int  geoac_fan_level_tubemap_stats(geoac_ctx* ctx, uint64_t* stats4);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_LTUBEMAP_H_ */
