// geoac_lstations_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_lstations.hip (level stations,
// include/geoac_lstations.h).  The file sees a context through the launch view of geoac_map_int.h with a slot of its own (GEOAC_SLOT_LSTA), and the crossing records
// through the public geoac_fan_levels_dev / geoac_get_levels; the lattice proof and extent are those of geoac_stations_int.h, the list walk is
// geoac_lattice_list.h, shared with geoac_stations.hip.
#ifndef GEOAC_LSTATIONS_INT_H_
#define GEOAC_LSTATIONS_INT_H_

#include "geoac_stations_int.h"

extern "C" void geoac_lsta_release(void* state);                                 // geoac_destroy: frees the level-station state (device current, stream idle)

// device copies of the stations [n_sta][2] and of level_of [n_sta] of the current lists (GEOAC_E_INVALID without current lists)
extern "C" int  geoac_lsta_coords_dev(geoac_ctx* ctx, const double** sta_dev, const int** level_of_dev, int* n_sta);
// the branch table of the last completed launch, xland[M][L][B][n_rays] of double4 (c0, c1, slot k, present) in the map's coordinates, under
// the legs leg_min .. leg_max and the ordinals 0 .. ord_max - 1: formed on first use after a launch, or when (leg0, n_legs, ord_max) differ from
// what it was formed with, and kept until then (the level-station state is created if the context has none).  B = n_legs * 2 * ord_max,
// b = ((leg - leg0) * 2 + d) * ord_max + o.  *formed: 1 when this call formed the table.  Every out pointer may be NULL.  `what` names the
// caller in messages; a launch without levels, or a level list changed since, is refused with the message of geoac_fan_levels_dev.
// geoac_fan_level_stations and geoac_fan_level_tubemap (geoac_ltubemap.hip) both read the table through this call.
extern "C" int  geoac_lsta_xland_dev(geoac_ctx* ctx, const char* what, int leg_min, int leg_max, int ord_max, const void** xland_dev, int* n_branches, int* leg0,
                                     int* n_legs, int* formed);

#endif
