// geoac_stations_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_stations.hip (station arrivals,
// include/geoac_stations.h), and what geoac_stations.hip owns for the other post-launch files: the landing table of a launch, the proof that
// the launch angles are a lattice, and the stations of the current lists.  (The list walk itself, which geoac_lstations.hip runs too, is
// geoac_lattice_list.h.)
#ifndef GEOAC_STATIONS_INT_H_
#define GEOAC_STATIONS_INT_H_

#include <string>

#include "geoac_map_int.h"

extern "C" void geoac_sta_release(void* state);                                  // geoac_destroy: frees the station state (device current, stream idle)

// device copy of the stations [n_sta][2] of the current lists (GEOAC_E_INVALID without current lists)
extern "C" int  geoac_sta_coords_dev(geoac_ctx* ctx, const double** sta_dev, int* n_sta);
// the landing table of the last completed launch, land[M][legs][n_rays] of double4 (c0, c1, turn, valid) in the map's coordinates: formed on
// first use after a launch (the station state is created if the context has none) and kept until the next.  `what` names the caller in messages.
extern "C" int  geoac_sta_land_dev(geoac_ctx* ctx, const char* what, const void** land_dev);

// why the launch angles of the view are not an n_theta x n_phi lattice bit for bit (ray = j * n_theta + i), or an empty string
std::string geoac_lattice_fault(const GeoacLaunchView& v, int n_theta, int n_phi);
// what of a lattice takes part: legs leg0 .. leg0 + n_legs - 1 of the launch's `legs`, and the number of lattice cells
void geoac_lattice_extent(int leg_min, int leg_max, int legs, int n_theta, int n_phi, int phi_periodic, int* leg0, int* n_legs, int* n_cells);

#endif
