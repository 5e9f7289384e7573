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

#endif
